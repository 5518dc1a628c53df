"""Reference code of tests/test_gpu_large_offsets.py: the case table, the size rule, the read lengths of the ragged shape, the placement of
the windows and the closed forms of the stages that have one.  Nothing here touches the engine; tests/test_large_offsets_cpu.py pins every
piece against the oracle on small batches, so that the GPU test does not trust this code on its own word."""
import numpy as np

from oracle import fxoracle_py as fo

MARKS = (31, 32, 33)                     # the byte offsets 2^31 (a signed int), 2^32 (a u32), 2^33 (an int count of dwords)
TARGET = (1 << 33) + (1 << 28)           # what the input array and the packed output of the fixed shape must both reach
SEED = 7
PREFIX = 100_000                         # reads of the oracle prefix that the size rule is computed on
ROUND = 1_000_000                        # N is rounded up to a multiple of this
KI = 3000                                # reads per window: eleven tiles of the largest tile size (256), so >= five whole tiles on each side of a mark
SLAB = 16_000_000                        # reads per slab of the whole-array checks
RANDOM_WINDOWS = 8
QTF = dict(qt_threshold=20, qt_min_len=30, qf_min_quality=20, qf_min_percent=80)
AD72 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCACATCTCGATCTCGTATGCCGTCTTCTGCTTGAAAAAAAA"
assert len(AD72) == 72

# the two families that tests/test_gpu_geometry.py::FAM does not hold: the two-lanes-per-read rows kernel of 38 words (rows of 209..304 bytes
# under FXG_ROWS=2) and the long clip form that runs in ONE pass without checkpoint scratch (clip_one_pass() below)
EXTRA = {
    "rows38x2": dict(stride=304, pd=dict(stages=6, **QTF), kernel="fxg_kernel_rows<38,2>", T=32, env=dict(FXG_ROWS="2"), rows=True),
    "clip72": dict(stride=100, pd=dict(stages=1, adapter=AD72, clip_min_len=15, clip_flags=0), kernel="fxg_kernel_tiles<-72,0> clip(packed)", clip=True),
}
PADDED = ("rows26", "rows38", "rows26x2", "rows38x2", "multi4", "multi3", "multi2", "tiles00", "clip13", "clip13gl", "clip40k", "clip72", "cfg5")
PAD = 3                                  # padded shape: fixed_len = stride - PAD

# family -> N (reads) and, per shape, the marks (exponents of two) that the input array and the packed output must cross.  N follows from the
# oracle alone (size_rule(): the smallest multiple of ROUND at which N * kept-bytes-per-read of the fixed shape, measured by the oracle on the
# first PREFIX reads of seed SEED, reaches TARGET; the input array is never the smaller of the two).  Conditions, not measurements: every fixed
# case crosses all three marks on both sides, every ragged / padded case all three on the input side and at least 2^31 and 2^32 on the output
# side (test_large_offsets_cpu.py recomputes N and the oracle's prediction of every ragged / padded output from the same prefix: the declared
# sets follow from it, with >= 1.5 GiB over 2^32 and >= 0.4 % to either side of 2^33).
A3, A2 = (31, 32, 33), (31, 32)
CASES = {     # (input marks, output marks) per shape; arrays of N * stride bytes: 8.4 GiB (mask) .. 25.7 GiB (cfg5)
    "rows26":    dict(N=190_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "rows38":    dict(N=125_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "rows26x2":  dict(N=94_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "rows38x2":  dict(N=62_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "multi4":    dict(N=507_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A2)),
    "multi3":    dict(N=373_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "multi2":    dict(N=259_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "tiles00":   dict(N=125_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "clip13":    dict(N=137_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "clip13gl":  dict(N=137_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "clip40k":   dict(N=171_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "clip72":    dict(N=207_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "cfg5":      dict(N=184_000_000, fixed=(A3, A3), ragged=(A3, A2), padded=(A3, A3)),
    "ftrim":     dict(N=91_000_000, fixed=(A3, A3), ragged=(A3, A2)),
    "rev2":      dict(N=63_000_000, fixed=(A3, A3), ragged=(A3, A2)),
    "rev5":      dict(N=57_000_000, fixed=(A3, A3), ragged=(A3, A2)),
    "mask":      dict(N=60_000_000, fixed=(A3, A3), ragged=(A3, A2)),
    "artifacts": dict(N=89_000_000, fixed=(A3, A3), ragged=(A3, A2)),
    "nfilter":   dict(N=146_000_000, fixed=(A3, A3), ragged=(A3, A2)),
}
STATS = dict(N=60_000_000, stride=150)          # the statistics kernel: 60 M x 150 = 8.38 GiB per array


def families():
    from test_gpu_geometry import FAM
    d = dict(FAM)
    d.update(EXTRA)
    return d


def clip_one_pass(alen, stride):
    """The tests' own statement of which long clip form (adapters of 17..99 bases) a fixed-length batch runs: one pass without scratch while
    the second pass' rows (the span of a path, the rows between checkpoints, a tenth of the read as margin) would not be fewer than the read's."""
    assert 16 < alen < 100
    span, ck = alen + (alen + 1) // 5, max(4, (stride + 7) // 8)
    return stride <= 255 and span + ck + stride // 10 > stride


def shapes(fam):
    return ("fixed", "ragged") + (("padded",) if fam in PADDED else ())


# ---- size rule ----
def prefix_kept_bytes(f, shape="fixed", n=PREFIX):
    """(kept reads, kept bytes) of the oracle on the first n reads of the family's input in the given shape."""
    st = f["stride"]
    b, q = fo.synth_batch(SEED, 0, n, st, bool(f.get("clip")), st)
    o = oracle_window(f, b, q, 0, shape)
    return int(o["counters"][fo.C_KEPT]), int(o["counters"][fo.C_KEPT_BASES])


def size_rule(kept_bytes, n=PREFIX):
    per_read = kept_bytes / n
    need = int(np.ceil(TARGET / per_read))
    return -(-need // ROUND) * ROUND


def crossed(nbytes):
    return tuple(m for m in MARKS if nbytes > (1 << m))


# ---- the ragged shape: lens[r] is a pure function of the read index ----
_C1, _C2 = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93


def _signed(c):
    return c - (1 << 64) if c >= 1 << 63 else c


def needs_one(pd):
    """Reads of length 0 reach a filter without a trimmer in front of it: the oracle drops them, the kernels' verdict keeps them (the note in
    tests/test_gpu_rows_sparse_fetch.py); such stages get lengths of at least 1."""
    return bool(pd["stages"] & 4) and not pd["stages"] & 2


def lens_numpy(r0, k, stride, pd=None):
    """uint16 lengths of reads r0 .. r0 + k: with h a 64-bit multiplicative hash of r, one read in sixteen gets a length uniform in [0, stride],
    the others one uniform in [stride // 2, stride]."""
    r = np.arange(r0, r0 + k, dtype=np.uint64)
    h = r * np.uint64(_C1)
    h ^= h >> np.uint64(32)
    h *= np.uint64(_C2)
    wide = (h >> np.uint64(60)) == 0
    u = (h >> np.uint64(24)) & np.uint64(0xFFFFFFFF)
    lo = np.where(wide, np.uint64(0), np.uint64(stride // 2))
    ln = lo + ((u * (np.uint64(stride + 1) - lo)) >> np.uint64(32))
    if pd is not None and needs_one(pd):
        ln = np.maximum(ln, np.uint64(1))
    return ln.astype(np.uint16)


def lens_torch(torch, r0, k, stride, pd=None, device="cpu"):
    """The same formula in torch's int64 (wrapping multiplies, arithmetic shifts masked to logical ones): int16 tensor, as Engine.run() takes it."""
    out = torch.empty(k, dtype=torch.int16, device=device)
    for s in range(0, k, SLAB):
        e = min(k, s + SLAB)
        r = torch.arange(r0 + s, r0 + e, dtype=torch.int64, device=device)
        h = r * _signed(_C1)
        h = h ^ ((h >> 32) & 0xFFFFFFFF)
        h = h * _signed(_C2)
        wide = ((h >> 60) & 15) == 0
        u = (h >> 24) & 0xFFFFFFFF
        lo = torch.where(wide, 0, stride // 2)
        ln = lo + ((u * (stride + 1 - lo)) >> 32)
        if pd is not None and needs_one(pd):
            ln = torch.clamp(ln, min=1)
        out[s:e] = ln.to(torch.int16)
    return out


# ---- the oracle on a window ----
def shape_args(f, shape, r0, k):
    """(lens or None, fixed_len or None) of reads r0 .. r0 + k in a shape."""
    st = f["stride"]
    if shape == "ragged":
        return lens_numpy(r0, k, st, f["pd"]), None
    return None, st - PAD if shape == "padded" else st


def oracle_window(f, b, q, r0, shape):
    """The oracle's answer for reads r0 .. r0 + len(b) of a family's input, every read on its own.  The reference clipper aligns a read together with
    the stale tail that longer reads before it left behind (one aligner per call); the engine without clip history aligns each read alone.
    The two agree while all reads of a call have one length, so a ragged clip window goes through the oracle one length at a time and is put
    together again in read order."""
    from helpers import oracle_params
    lens, fl = shape_args(f, shape, r0, len(b))
    p = oracle_params(f["pd"])
    if lens is None or not f["pd"]["stages"] & 1:
        return fo.run_pipeline(b, q, lens, p, fixed_len=fl)
    n = len(b)
    res = np.zeros(n, np.uint32)
    pieces_b, pieces_q = [None] * n, [None] * n
    counters = np.zeros(0, np.uint64)
    for L in np.unique(lens):
        idx = np.nonzero(lens == L)[0]
        o = fo.run_pipeline(np.ascontiguousarray(b[idx]), np.ascontiguousarray(q[idx]), lens[idx], p)
        counters = o["counters"].copy() if not len(counters) else counters + o["counters"]
        res[idx] = o["res"]
        ends = np.cumsum(o["out_len"].astype(np.int64))
        for j, (ki, e, ol) in enumerate(zip(o["kept_index"], ends, o["out_len"])):
            pieces_b[idx[ki]] = o["out_bases"][e - ol:e]
            pieces_q[idx[ki]] = o["out_qual"][e - ol:e]
    kept = [i for i in range(n) if pieces_b[i] is not None]
    cat = lambda ps: np.concatenate([ps[i] for i in kept]) if kept else np.zeros(0, np.uint8)
    return dict(res=res, out_bases=cat(pieces_b), out_qual=cat(pieces_q), out_len=np.array([len(pieces_b[i]) for i in kept], np.uint16),
                kept_index=np.array(kept, np.uint32), counters=counters)


# ---- window placement ----
def window_start(centre, n, k=KI):
    """First read of the window of k reads centred on read `centre`, kept inside [0, n)."""
    return int(max(0, min(n - k, centre - k // 2)))


def input_mark_read(mark, stride):
    """The read whose row holds byte `mark` of the input arrays."""
    return mark // stride


def output_mark_read(out_off, kept_index, mark):
    """The read whose kept bytes hold byte `mark` of the packed stream (or, where `mark` is the stream's end or lies behind reads kept with no
    bytes, the last kept read that starts at or before it): out_off is the exclusive scan of the kept lengths (torch tensor or numpy array)."""
    if isinstance(out_off, np.ndarray):
        k = int(np.searchsorted(out_off, mark, side="right")) - 1
    else:
        import torch
        k = int(torch.searchsorted(out_off, torch.tensor([mark], dtype=out_off.dtype, device=out_off.device), right=True)[0]) - 1
    return int(kept_index[k]) & 0xFFFFFFFF


def windows(n, stride, in_marks, out_marks, out_off, kept_index, seed):
    """[(label, first read, side, byte)] of every window of one run, by first read: prefix, suffix, one per crossed mark of the input ("in", the
    mark's byte offset) and of the output ("out"), RANDOM_WINDOWS seeded ones (side and byte None).  In read order, so that the first failure
    of a run is the lowest broken offset: a mark's window, not the suffix."""
    k = min(KI, n)
    w = [("prefix", 0, None, None), ("suffix", n - k, None, None)]
    for m in in_marks:
        w.append(("input 2^%d" % m, window_start(input_mark_read(1 << m, stride), n, k), "in", 1 << m))
    for m in out_marks:
        w.append(("output 2^%d" % m, window_start(output_mark_read(out_off, kept_index, 1 << m), n, k), "out", 1 << m))
    rng = np.random.default_rng(1000 + seed)
    if n > 3 * k:
        w += [("random", int(x), None, None) for x in rng.integers(k, n - 2 * k, size=RANDOM_WINDOWS)]
    return sorted(w, key=lambda x: x[1])


# ---- closed forms (torch, no engine): what the whole packed stream of a fixed-length slab must be ----
def closed_form(torch, fam, f, b, q):
    """(expected bases [n, L'], expected qualities [n, L']) of the rows b, q (uint8 [n, stride]) where every read is kept at one length, or None."""
    pd = f["pd"]
    st = pd["stages"]
    if st == 16:
        lo, hi = pd["ft_first"] - 1, pd["ft_last"]
        return b[:, lo:hi], q[:, lo:hi]
    if st in (8, 24):
        comp = torch.arange(256, dtype=torch.uint8, device=b.device)
        for x, y in (b"AT", b"TA", b"CG", b"GC", b"at", b"ta", b"cg", b"gc"):
            comp[x] = y
        rb, rq = comp[b.flip(1).long()], q.flip(1)
        if st == 24:
            lo, hi = pd["ft_first"] - 1, pd["ft_last"]
            rb, rq = rb[:, lo:hi], rq[:, lo:hi]
        return rb, rq
    if st == 64:
        low = (q.to(torch.int16) - pd.get("qoffset", 33)) < pd["mask_min_quality"]
        return torch.where(low, torch.tensor(ord(pd.get("mask_char", "N")), dtype=torch.uint8, device=b.device), b), q
    if fam == "artifacts":
        return b, q
    return None
