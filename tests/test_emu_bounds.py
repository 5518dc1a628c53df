"""CPU tier, guard pages: every array a kernel body is handed ends (or starts) exactly at a PROT_NONE page.

The parity tests check WHAT a kernel computes; this tier checks WHERE it reads and writes.  Every input and output array of the emulated
run sits at exactly its contracted size (include/fxg.h, "Memory contract": the array's bytes rounded up to the 16-byte granule) with an
unmapped page right behind it (guard "after") or right in front of it (guard "before", for reads below a row's start).  A body that touches a
byte outside the contract on that side takes a SIGSEGV.  Each case runs in a child process of its own (`python tests/test_emu_bounds.py
<case>`), so a fault fails one named test, with the case in its message, instead of pytest; the child also compares its arrays with the oracle,
so a guarded run is a parity run as well.  The emulator is built once, by the parent; the children only load it.

A contracted end is a page boundary only where the array's size is a multiple of 16 (n = 64 and 16 below, or strides of 16); elsewhere the
rest of the last granule lies between the two.  Shapes: len == stride and len < stride, strides of every residue mod 4 and multiples of 16, n = 1 and n off the tile, ragged lengths, reads of
1 base and long ones, a last read that ends in an adapter prefix of 1 .. A - 1 bases or is all adapter, N and bytes outside ACGTN at the very
last byte, outputs where every read is kept (out_bases filled to its capacity), text without a final newline at at_eof 0 and 1.

Known limit: emu_rows_piece and the statistics emulator (tests/emu/fxg_emu.cpp) do their own global loads instead of the kernels'
fxg_rows_fetch / fxg_kernel_quality_stats outer loops, and the staged clip tile is a host buffer.  The guard pages prove the shared
per-thread bodies, not those GPU-only loops; tests/test_gpu_bounds.py covers those with poison and canaries on the device.
"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]         # (the children run this file as a script)
from helpers import CLIP_BUCKETS  # noqa: E402
FULL = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCACATCACGATCTCGTATGCCGTCTTCTGCTTGAAAAAAAAAAGGGGGGGGGGCCCCCCCCCCTTTTTTTTT"
CHILD_TIMEOUT = 120


def _cases():
    cs = []

    def add(name, **kw):
        kw.setdefault("guard", "after")
        kw.setdefault("env", {})
        kw.setdefault("seed", len(cs) + 1)
        cs.append(dict(name=name, **kw))

    # ---- quality trim / filter: the row kernel's every rows_nw (10 14 20 26 38), one and two lanes per read, and the tile kernel around it ----
    q6 = dict(stages=6, qt_threshold=20, qt_min_len=5, qf_min_quality=20, qf_min_percent=60)
    keep_all = dict(stages=2, qt_threshold=0, qt_min_len=1)          # every base kept: out_bases / out_qual fill to n * stride
    for stride, env in ((1, {}), (20, {}), (28, {}), (39, {}), (45, {}), (62, {}), (80, {}), (96, {}), (101, {}), (150, {}), (151, {}), (200, {}),
                        (257, {"FXG_ROWS": "2"}), (304, {"FXG_ROWS": "2"}), (303, {}), (1000, {})):
        for n in (1, 64, 67):
            add("qual.s%d.n%d.fixed" % (stride, n), stride=stride, n=n, lens="fixed", params=q6, env=env)
            add("qual.s%d.n%d.keepall" % (stride, n), stride=stride, n=n, lens="fixed", params=keep_all, env=env)
        add("qual.s%d.ragged" % stride, stride=stride, n=131, lens="ragged", params=q6, env=env)
        add("qual.s%d.short" % stride, stride=stride, n=131, lens="short", params=q6, env=env)
        add("qual.s%d.before" % stride, stride=stride, n=67, lens="ragged", params=keep_all, env=env, guard="before")
    # ---- fixed trim, reverse complement, both (fxg_kernel_tiles MODE 0 / 1, the <0,5> instance), -t/-m ----
    for stride in (1, 7, 36, 100, 101, 150, 151, 254, 1000):
        for pd in (dict(stages=8), dict(stages=24, ft_first=2, ft_last=max(1, stride - 3)), dict(stages=16, ft_first=1, ft_last=0),
                   dict(stages=40, ft_trim_end=1, ft_min_len=0), dict(stages=32, ft_trim_end=3, ft_min_len=2)):
            tag = "ftrim.s%d.st%d" % (stride, pd["stages"])
            add(tag + ".fixed", stride=stride, n=64, lens="fixed", params=pd)
            add(tag + ".ragged", stride=stride, n=1 if stride == 1000 else 131, lens="ragged", params=pd, tail="N")
            if pd["stages"] & 8:
                add(tag + ".before", stride=stride, n=37, lens="fixed", params=pd, guard="before")
    # ---- mask, artifacts census, N filter ----
    for stride in (1, 31, 36, 100, 150, 151, 253, 1000):
        for pd, tails in ((dict(stages=64, mask_min_quality=20), ("N", "odd")), (dict(stages=128), ("N", "odd")),
                          (dict(stages=256), ("N", "odd")), (dict(stages=256, nf_keep_n=1), ("N",))):
            for tail in tails:
                tag = "census.s%d.st%d.k%d.%s" % (stride, pd["stages"], pd.get("nf_keep_n", 0), tail)
                add(tag, stride=stride, n=64, lens="fixed", params=pd, tail=tail)
            add("census.s%d.st%d.k%d.ragged" % (stride, pd["stages"], pd.get("nf_keep_n", 0)), stride=stride, n=131, lens="short", params=pd,
                guard="before" if stride % 2 else "after")
    # ---- the clipper: every bucket, staged and over the batch, the last read ending in adapter prefixes and all adapter ----
    for A in CLIP_BUCKETS:
        A = min(A, 99)
        ad = FULL[:A].decode()
        strides = (200, 180, 101) if A <= 16 else (256, 252, 150)
        for stride in strides:
            for gl in ("0", "1"):
                for K in sorted({1, 2, 3, A - 1} - {0}):
                    add("clip.a%d.s%d.gl%s.K%d" % (A, stride, gl, K), stride=stride, n=64, lens="fixed", adapter=ad, tail="ad%d" % K,
                        params=dict(stages=1, adapter=ad, clip_min_len=15, clip_flags=0 if K % 2 else 4), env={"FXG_CLIP_GLOBAL": gl})
                add("clip.a%d.s%d.gl%s.all" % (A, stride, gl), stride=stride, n=37, lens="fixed", adapter=ad, tail="adall",
                    params=dict(stages=7, adapter=ad, clip_min_len=5, clip_flags=8, qt_threshold=20, qt_min_len=5, qf_min_quality=10, qf_min_percent=20),
                    env={"FXG_CLIP_GLOBAL": gl})
        add("clip.a%d.ragged.before" % A, stride=strides[0], n=67, lens="ragged", adapter=ad, tail="ad2", guard="before",
            params=dict(stages=1, adapter=ad, clip_min_len=10, clip_flags=0))
    for A, stride in ((34, 50), (99, 120), (20, 25)):                  # the one-pass forms of the 17..99 buckets (short rows)
        ad = FULL[:A].decode()
        add("clip.onepass.a%d.s%d" % (A, stride), stride=stride, n=37, lens="fixed", adapter=ad, tail="ad3", params=dict(stages=1, adapter=ad, clip_min_len=5))
    for A in (4, 13, 16, 34, 99):                                      # FXG_NO_PACKED_CLIP: the general two-word form
        ad = FULL[:A].decode()
        add("clip.general.a%d" % A, stride=101, n=37, lens="fixed", adapter=ad, tail="ad2", params=dict(stages=1, adapter=ad, clip_min_len=5),
            env={"FXG_NO_PACKED_CLIP": "1"})
    for A, stride in ((13, 300), (34, 300), (99, 421)):                # reads beyond 255 bases: the 16-column k form, checkpoints in scratch
        ad = FULL[:A].decode()
        for gl in ("0", "1"):
            add("clip.long.a%d.s%d.gl%s" % (A, stride, gl), stride=stride, n=16, lens="fixed", adapter=ad, tail="ad3",
                params=dict(stages=1, adapter=ad, clip_min_len=15), env={"FXG_CLIP_GLOBAL": gl})
    for A in (8, 13, 34):                                              # N at the last byte, -n rule on and off
        ad = FULL[:A].decode()
        for fl in (0, 4):
            add("clip.nlast.a%d.f%d" % (A, fl), stride=200, n=64, lens="fixed", adapter=ad, tail="N", params=dict(stages=1, adapter=ad, clip_min_len=5, clip_flags=fl),
                env={"FXG_CLIP_GLOBAL": "1"})
    for A, stride in ((13, 200), (34, 252), (8, 64)):                 # history across batches (the staged form over the rebuilt rows)
        ad = FULL[:A].decode()
        add("clip.hist.a%d.s%d" % (A, stride), stride=stride, n=41, lens="ragged", adapter=ad, tail="ad2", batches=3,
            params=dict(stages=1, adapter=ad, clip_min_len=5, clip_flags=4))
    # ---- quality statistics: piece form and row-strip form ----
    for stride in (1, 16, 17, 36, 100, 151, 160, 200, 1000):
        for form in ("piece", "rows"):
            env = {"FXG_EMU_QS_ROWS": "1"} if form == "rows" else {}
            add("qstats.s%d.%s.fixed" % (stride, form), kind="qstats", stride=stride, n=64, lens="fixed", env=env)
            add("qstats.s%d.%s.ragged" % (stride, form), kind="qstats", stride=stride, n=131, lens="ragged", env=env,
                guard="before" if stride % 2 else "after")
    add("qstats.s150.piece.n1000", kind="qstats", stride=150, n=1000, lens="fixed")
    # ---- the text path: index, pack, format, weights ----
    for lpr in (4, 2):
        for n, maxlen in ((1, 1), (1, 37), (9, 150), (131, 100), (50, 300)):
            for final_nl in (True, False):
                for at_eof in (0, 1):
                    add("text.l%d.n%d.m%d.nl%d.eof%d" % (lpr, n, maxlen, final_nl, at_eof), kind="text", lpr=lpr, n=n, maxlen=maxlen, final_nl=final_nl,
                        at_eof=at_eof, guard="after" if (n + at_eof) % 2 else "before")
    # ---- the formatter's output modes (fxg_fastq_format_opts): every source kind x mode x last record, both guard sides ----
    import format_opts_cases as F
    for source in F.BOUNDS_SOURCES:
        for mode in F.BOUNDS_MODES:
            for last in F.BOUNDS_LAST:
                for guard in ("after", "before"):
                    add("fmtopts.%s.%s.%s.%s" % (source, mode, last, guard), kind="fmtopts", source=source, mode=mode, last=last, guard=guard)
    return cs


CASES = _cases()


# ---------------------------------------------------------------------------------------------------------------------------------
# the child: one case
# ---------------------------------------------------------------------------------------------------------------------------------
def _batch(c, rng, adapter):
    from helpers import random_batch
    n, stride = c["n"], c["stride"]
    ad = adapter.encode() if adapter else None
    b, q, lens = random_batch(rng, n, stride, 1, stride, c["lens"] == "fixed", adapter=ad)
    if c["lens"] == "short":                                    # every read shorter than the row
        lens = np.minimum(lens, max(stride - 1, 1)).astype(np.uint16) if stride > 1 else lens
    if c["lens"] in ("ragged", "short") and n > 1:
        lens[0] = 1
    if c["lens"] == "ragged":
        lens[-1] = stride                                       # the last read ends at the end of the array
    last = stride if lens is None else int(lens[-1])
    tail = c.get("tail")
    if tail and tail.startswith("ad"):
        b[-1, :] = ord("T")
        if tail == "adall":
            b[-1, :] = np.frombuffer((ad * (stride // len(ad) + 1))[:stride], dtype=np.uint8)
        else:
            k = min(int(tail[2:]), last)
            b[-1, last - k:last] = np.frombuffer(ad[:k], dtype=np.uint8)
    elif tail == "N":
        b[-1, last - 1] = ord("N")
    elif tail == "odd":
        b[-1, last - 1] = ord("x")
    return b, q, lens


def _run_pipe(c):
    import emu_py as emu
    from helpers import assert_same, oracle_params
    from oracle import fxoracle_py as fo
    rng = np.random.default_rng(c["seed"])
    p = oracle_params(c["params"])
    shared = c.get("batches") or (c["params"]["stages"] & 1 and c["lens"] != "fixed")      # ragged clipper input: the aligner's history (N3)
    hist = emu.hist_new() if shared else None
    al = fo.aligner_new() if shared else None
    for k in range(c.get("batches") or 1):
        b, q, lens = _batch(c, rng, c.get("adapter"))
        e = emu.run_pipeline(b, q, lens, p, hist=hist, guard=c["guard"])
        if c.get("tail") == "odd" and c["params"]["stages"] & (8 | 128 | 256):
            assert int(e["counters"][15]) & 2, "a byte outside ACGTN raises FXG_DEV_ERR_BAD_BASE"
            continue
        o = fo.run_pipeline(b, q, lens, p, aligner=al)
        assert_same(o, e, "%s.b%d" % (c["name"], k))


def _run_qstats(c):
    import emu_py as emu
    from oracle import fxoracle_py as fo
    rng = np.random.default_rng(c["seed"])
    b, q, lens = _batch(c, rng, None)
    cols = c["stride"]
    h = emu.run_quality_stats(b, q, lens, cols=cols, guard=c["guard"])
    qs = fo.QStats()
    qs.add(b, q, lens, qoffset=33)
    assert np.array_equal(h, qs.device_layout(cols, 33)), c["name"]
    qs.close()


def _run_text(c):
    import emu_py as emu
    from oracle import fxoracle_py as fo
    rng = np.random.default_rng(c["seed"])
    lpr, n, guard = c["lpr"], c["n"], c["guard"]
    recs, lens = [], rng.integers(1, c["maxlen"] + 1, size=n)
    lens[-1] = c["maxlen"]
    for i, L in enumerate(lens):
        s = bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=int(L)))
        if lpr == 4:
            qv = bytes(rng.integers(33, 75, size=int(L), dtype=np.uint8))
            recs.append(b"@r%d\n%s\n+\n%s\n" % (i, s, qv))
        else:
            recs.append(b">r%d\n%s\n" % (i, s))
    text = b"".join(recs)
    if not c["final_nl"]:
        text = text[:-1]
    at_eof = bool(c["at_eof"])
    ix = emu.fastq_index(text + b"\n" if (at_eof and not c["final_nl"]) else text, at_eof=at_eof, lpr=lpr, guard=guard)
    info = ix["info"]
    full = n if (c["final_nl"] or at_eof) else n - 1            # a last record without its newline is not complete until the end of input
    assert info.records == full and info.irregular == 0, (info.records, full, info.irregular)
    if full == 0:
        return
    assert np.array_equal(ix["lens"][:full], lens[:full]), "record lengths"
    stride = int(lens[:full].max())
    b, q, irr = emu.fastq_pack(ix, full, stride, guard=guard)
    assert irr == 0
    if lpr == 4:
        p = fo.parse_fastq(b"".join(recs[:full]), stride=stride)
        for r in range(full):
            L = int(lens[r])
            assert np.array_equal(b[r, :L], p["bases"][r, :L]) and np.array_equal(q[r, :L], p["qual"][r, :L]), "packed row %d" % r
    else:
        for r in range(full):
            L = int(lens[r])
            assert bytes(b[r, :L]) == recs[r].split(b"\n")[1], "packed row %d" % r
    res = np.full(full, 1 << 16, dtype=np.uint32) | lens[:full].astype(np.uint32)      # every record kept whole: the output is the input
    out = emu.fastq_format(ix, full, res, rows_qual=q, stride=stride if q is not None else 0, guard=guard)
    assert out == b"".join(recs[:full]), "formatted text"
    if lpr == 2:
        w = emu.fasta_weights(ix, full, res, guard=guard)
        assert w[0] == full and w[1] == full, w


def _run_fmtopts(c):
    """d_len as u16[n] (res null), the size pass's quality window of every source kind, pk_qual / pk_bases in whole 16-byte chunks and a byte tail,
    the bases read again for sequence ids, 20-digit ordinals, the numeric writer's LF: every array at exactly its size against the guard page,
    d_out at exactly out_bytes -- learnt from a first run into a roomy d_out (the inputs guarded there too), which is also compared with the model"""
    import emu_py as emu
    import format_opts_cases as F
    kw, numeric = F.BOUNDS_MODES[c["mode"]]
    data = F.bounds_block(F.BOUNDS_LAST[c["last"]], numeric)
    q = F.bounds_request(data, c["source"])
    want = F.expected(data, 4, 33, **q["ekw"], **kw)
    rc, out, nb = emu.format_opts(q, c["guard"], len(data) * 8, **kw)
    assert rc == 0 and nb == len(want) and out == want, ("a roomy d_out", rc, nb, len(want))
    rc, out, nb = emu.format_opts(q, c["guard"], nb, **kw)
    assert rc == 0 and nb == len(want) and out == want, ("d_out of exactly out_bytes", rc, nb, len(want))


def run_case(c):
    os.environ.update(c["env"])
    sys.path[:0] = [ROOT, HERE]
    {"pipe": _run_pipe, "qstats": _run_qstats, "text": _run_text, "fmtopts": _run_fmtopts}[c.get("kind", "pipe")](c)


# ---------------------------------------------------------------------------------------------------------------------------------
# the parent
# ---------------------------------------------------------------------------------------------------------------------------------
def _child(c):
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), json.dumps(c)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=CHILD_TIMEOUT, cwd=ROOT)
        return p.returncode, p.stdout.decode(errors="replace")[-3000:]
    except subprocess.TimeoutExpired:
        return "timeout", ""


@pytest.fixture(scope="module")
def outcomes():
    sys.path[:0] = [HERE]
    import emu_py as emu
    from oracle import fxoracle_py as fo
    emu.build()                     # once, here: the children only load the library
    emu.build_fmtopts()
    fo.lib()
    try:
        cpus = len(os.sched_getaffinity(0))
    except AttributeError:
        cpus = os.cpu_count() or 1
    with ThreadPoolExecutor(max(1, min(8, cpus))) as ex:
        return dict(zip((c["name"] for c in CASES), ex.map(_child, CASES)))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_guarded(outcomes, case):
    rc, out = outcomes[case["name"]]
    sig = {-11: "SIGSEGV", -7: "SIGBUS", -6: "SIGABRT"}.get(rc if isinstance(rc, int) else 0)
    assert rc == 0, "%s: child %s%s\ncase: %s\n%s" % (case["name"], rc, " (%s: an access outside the contracted range)" % sig if sig else "",
                                                     json.dumps(case), out)


def test_case_names_unique():
    assert len({c["name"] for c in CASES}) == len(CASES)


if __name__ == "__main__":
    run_case(json.loads(sys.argv[1]))
