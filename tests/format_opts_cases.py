"""Output modes of the device formatter (fxg_fastq_format_opts: ids and quality encoding): the model, the inputs and the checks that both tiers run.

tests/test_gpu_format_opts.py runs every check here on the real engine, tests/test_format_opts_cpu.py on the emulation stub with the formatter's entry
behind it (tests/emu/fmtopts_stub.cpp) -- through the same Engine methods: `StubEngine` is the Engine over that library, with its "device" tensors in
host memory.  Every comparison is exact bytes plus out_bytes; every formatted block sits between two 4 KiB canaries that must come back untouched.

The model (`expected`, and `model_rename` / `model_convert` on top of it for the two tools) works on well-formed records only: split, rename or
re-encode, join.  tests/test_format_opts_cpu.py pins it against the reference's own fastx_renamer.c and fastq_quality_converter.c.
"""
import ctypes as C
import os

import numpy as np

import fxref_replay
from fastx_toolkit_amd import engine as E
from helpers import REPLAY, ref_driver, run_ref

CANARY, GUARD = 0xA5, 4096
ORDINAL_BASES = [0, 8, 98, 999998, 2 ** 32 - 3, 10 ** 19 - 2]
RECORD_COUNTS = [1, 15, 16, 17, 255, 256, 257, 5000]
QUAL_LENGTHS = [1, 2, 15, 16, 17, 31, 33, 150, 1000]


# ---- the reference driver ---------------------------------------------------------------------------------------------------------------
OWN_ANSWERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "format_opts", "fxref_answers.xz")
_own = None


def reference(argv, data):
    """(exit code, stdout, stderr) of `fxref argv` (oracle/_ref/fxref, the real libfastx) with data on stdin.  Where the driver is not built the
    answer comes from the recorded ones, as everywhere in the suite (tests/fxref_replay.py); the requests of these tests are recorded in a store of
    their own beside the suite's, same format, made the same way (FXREF_RECORD, then fxref_replay.pack into OWN_ANSWERS)."""
    global _own
    drv = ref_driver()
    if drv != REPLAY or os.environ.get("FXREF_RECORD"):
        return run_ref([drv] + argv, data)
    if _own is None:
        suite, fxref_replay.STORE = fxref_replay.STORE, OWN_ANSWERS
        try:
            _own = fxref_replay._load()
        finally:
            fxref_replay.STORE = suite
    key = fxref_replay._key(argv, data)
    assert key in _own, "no recorded reference answer for %r with %d bytes on stdin in %s" % (argv, len(data), OWN_ANSWERS)
    return fxref_replay._decode(_own[key])[:3]


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def records(data, lpr):
    """[[line, ...], ...]: lines cut at their first CR (chomp.c:36-41), lpr of them per record"""
    lines = [l.split(b"\r")[0] for l in data.split(b"\n")]
    if lines and lines[-1] == b"":
        lines.pop()
    return [lines[i:i + lpr] for i in range(0, len(lines), lpr)]


def qual_values(rec, qoffset):
    """the quality values of a FASTQ record: one character per base, else numbers (fastx.c:382-390)"""
    return [c - qoffset for c in rec[3]] if len(rec[3]) == len(rec[1]) else [int(t) for t in rec[3].split()]


def expected(data, lpr, qoffset=33, res=None, fwd_start=0, out_fasta=False, id_mode=0, id_both=False, base=0, qual_mode=0, packed=None, count32=False):
    """What the formatter writes.  res: per record (keep, length) or None = every record whole; packed: per KEPT record (bases, values) in place of
    the input's slice [fwd_start, fwd_start + length) (reverse-complemented / masked output)."""
    out, rank = [], 0
    for k, rec in enumerate(records(data, lpr)):
        keep, ln = (1, len(rec[1])) if res is None else res[k]
        if not keep:
            continue
        vals = qual_values(rec, qoffset)[fwd_start:fwd_start + ln] if lpr == 4 else None
        seq = rec[1][fwd_start:fwd_start + ln]
        if packed is not None:
            seq, vals = packed[rank]
        num = base + rank + 1
        name = [rec[0][1:], b"%d" % (num % 2 ** 32 if count32 else num), seq][id_mode]
        rank += 1
        if lpr == 2 or out_fasta:
            out.append(b">" + name + b"\n" + seq + b"\n")
            continue
        name2 = name if (id_mode and id_both) else rec[2][1:]
        numeric = [len(rec[3]) != len(rec[1]), False, True][qual_mode]
        q = b" ".join(b"%d" % v for v in vals) if numeric else bytes(v + qoffset for v in vals)
        out.append(b"@" + name + b"\n" + seq + b"\n+" + name2 + b"\n" + q + b"\n")
    return b"".join(out)


def model_rename(data, how, fasta=False, qoffset=33):
    """fastx_renamer -n SEQ | COUNT (fastx_renamer.c:87-105): the id on both name lines, an unsigned int counter"""
    return expected(data, 2 if fasta else 4, qoffset, id_mode=E.ID_SEQUENCE if how == "SEQ" else E.ID_ORDINAL, id_both=True, count32=True)


def model_convert(data, numeric, qoffset=33):
    """fastq_quality_converter -a | -n (fastq_quality_converter.c:62-84)"""
    return expected(data, 4, qoffset, qual_mode=E.QUAL_NUMERIC if numeric else E.QUAL_ASCII)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def qual_line(vals, qoffset, numeric):
    """a quality line of the values; a numeric line is never as long as the bases (one value: two characters at least), so it reads back as numbers.
    A character line holds bytes up to 127 (the reference's chars are signed): at offset 64 the values above 63 only come in as numbers."""
    if numeric and not (len(vals) == 1 and 0 <= vals[0] < 10):
        return b" ".join(b"%d" % v for v in vals)
    return bytes((v if v + qoffset < 128 else v - 79) + qoffset for v in vals)


def make_block(rng, n, lmin=1, lmax=60, fasta=False, qoffset=33, numeric="none", crlf=False, collapsed=False, p_n=0.05):
    """n records: names of 0..40 bytes (the empty name among them), third line empty or not, ragged lengths; numeric: none | all | alternating"""
    lo = -15 if qoffset == 64 else 0
    eol = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(n):
        L = int(rng.integers(lmin, lmax + 1))
        s = rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=L, p=[(1 - p_n) / 4] * 4 + [p_n]).tobytes()
        nl = int(rng.integers(0, 41)) if i % 7 else 0
        name = (b"r%d-%d" % (i, 1 + i % 5) if collapsed else (b"r%d %s" % (i, b"x" * 40))[:nl])
        if fasta:
            out.append(b">" + name + eol + s + eol)
            continue
        vals = [int(v) for v in rng.integers(lo, 94, size=L)]
        num = numeric == "all" or (numeric == "alternating" and i % 2 == 1)
        out.append(b"@" + name + eol + s + eol + (b"+" + name if i % 3 == 0 else b"+" if i % 3 == 1 else b"") + eol + qual_line(vals, qoffset, num) + eol)
    return b"".join(out)


def quality_range_block(qoffset, numeric):
    """every quality value of the offset (-15..93 at 64, 0..93 at 33) at every per-lane share of the 16-lane writer: lengths QUAL_LENGTHS"""
    lo = -15 if qoffset == 64 else 0
    span, out, at = list(range(lo, 94)), [], 0
    for rep in range(2):
        for L in QUAL_LENGTHS:
            vals = [span[(at + j * (1 + rep)) % len(span)] for j in range(L)]
            at += 7
            num = numeric == "all" or (numeric == "alternating" and len(out) % 2 == 1)
            out.append(b"@q%d\n%s\n+%s\n%s\n" % (len(out), b"ACGTN"[len(out) % 5:][:1] * L, b"x" if rep else b"", qual_line(vals, qoffset, num)))
    return b"".join(out)


# ---- the two backends -----------------------------------------------------------------------------------------------------------------
class StubEngine(E.Engine):
    """The Engine over a look-alike libfxg.so of the CPU tier: same methods, the "device" tensors in host memory, no stream to order against."""

    def __init__(self, path):
        import torch
        self.torch, self.lib, self.device_id, self.device, self._side = torch, E.load_library(path), 0, torch.device("cpu"), None
        self.ctx = C.c_void_p()
        assert self.lib.fxg_ctx_create(0, C.byref(self.ctx)) == 0


class Block:
    """a block of text indexed and packed on the engine"""

    def __init__(self, eng, data, fasta=False, qoffset=33, irregular=0):
        self.data, self.lpr, self.qoffset = data, 2 if fasta else 4, qoffset
        self.d_text, self.text_len = eng.text_upload(data)
        self.ix, self.lens, info = eng.fastq_index(self.d_text, self.text_len, fasta=fasta)
        assert info.irregular == irregular and info.consumed == self.text_len, (info.irregular, info.consumed)
        self.n, self.stride, self.fixed = info.records, info.max_len, info.min_len == info.max_len
        if irregular:                              # (the extrema leave a flagged record out)
            self.stride, self.fixed = int(self.lens[:self.n].cpu().numpy().view(np.uint16).max()), False
        self.bases, self.qual, irr = eng.fastq_pack(self.d_text, self.text_len, self.ix, self.n, self.stride, qoffset)
        assert irr == 0


def run(eng, b, compact=False, **pd):
    """the block through the pipeline: (Result, res as [(keep, length)])"""
    r = eng.run(b.bases, b.qual, E.make_params(**dict(pd, qoffset=33)), lens=None if b.fixed else b.lens[:b.n], fixed_len=b.stride, compact=compact, meta=compact)
    eng.sync()
    w = r.res.cpu().numpy().view(np.uint32)
    return r, [(int(x >> 16) & 1, int(x) & 0xFFFF) for x in w]


def fmt(eng, b, res=None, fwd_start=0, packed=None, reverse=False, out_fasta=False, id_mode=0, id_both=False, base=0, qual_mode=0, cap=None, plain_entry=False):
    """fxg_fastq_format_opts (plain_entry: fxg_fastq_format) into `cap` bytes (default: the bound of the modes) between two canaries.
    Returns (rc, the bytes written, out_bytes); asserts that no byte outside [0, cap) changed, and none at all when the request is refused."""
    T = eng.torch
    cap = E.format_bound(b.text_len, b.n, id_mode, qual_mode) if cap is None else cap
    buf = T.full((cap + 2 * GUARD,), CANARY, dtype=T.uint8, device=eng.device)
    nb = C.c_uint64(12345)
    pb, pq, po = (packed[0].data_ptr(), packed[1].data_ptr() if packed[1] is not None else None, packed[2].data_ptr()) if packed else (None, None, None)
    args = (eng.ctx, b.d_text.data_ptr(), b.lpr, b.ix.line.data_ptr(), b.ix.cap_lines, b.ix.flags.data_ptr(), b.n, res.data_ptr() if res is not None else None,
            fwd_start, int(reverse), pb, pq, po, b.qual.data_ptr() if b.qual is not None else None, b.stride, b.qoffset, int(out_fasta), buf.data_ptr() + GUARD, C.byref(nb))
    eng._after_torch()
    if plain_entry:
        rc = eng.lib.fxg_fastq_format(*args)
    else:
        o = E.FxgFormatOpts(id_mode, int(bool(id_both)), base, qual_mode, cap, b.lens.data_ptr())
        rc = eng.lib.fxg_fastq_format_opts(*args, C.byref(o))
    eng._before_torch()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == CANARY).all() and (host[GUARD + cap:] == CANARY).all(), "a byte outside d_out changed"
    if rc != 0:
        assert (host == CANARY).all() and nb.value == 0, "a refused request wrote"
        return rc, b"", 0
    assert nb.value <= cap
    assert (host[GUARD + nb.value:] == CANARY).all(), "a byte behind out_bytes changed"
    return rc, host[GUARD:GUARD + nb.value].tobytes(), nb.value


def same(got, want, what):
    rc, out, nb = got
    assert rc == 0 and nb == len(want) and out == want, (what, rc, nb, len(want), next((i for i, (x, y) in enumerate(zip(out, want)) if x != y), None))


# ---- the checks -----------------------------------------------------------------------------------------------------------------------
def check_ordinals(eng, n):
    """1. ordinal ids: FASTQ -> FASTQ with id_both, FASTQ -> FASTA, FASTA -> FASTA; res of a quality filter that keeps about half, and res=None"""
    rng = np.random.default_rng(100 + n)
    fq = Block(eng, make_block(rng, n))
    fa = Block(eng, make_block(rng, n, fasta=True, p_n=0.02), fasta=True)
    rq, res_q = run(eng, fq, stages=4, qf_min_quality=45, qf_min_percent=50)
    ra, res_a = run(eng, fa, stages=0x100)          # fastq_to_fasta's N-discard: the FASTA block's filter
    if n >= 255:
        assert 0.2 * n < sum(k for k, _ in res_q) < 0.8 * n and 0 < sum(k for k, _ in res_a) < n
    for base in ORDINAL_BASES:
        for b, r, res, fasta_out, both in ((fq, rq, res_q, False, True), (fq, rq, res_q, True, False), (fa, ra, res_a, False, False), (fq, rq, res_q, False, False)):
            for use_res in (True, False):
                want = expected(b.data, b.lpr, res=res if use_res else None, out_fasta=fasta_out, id_mode=E.ID_ORDINAL, id_both=both, base=base)
                got = fmt(eng, b, res=r.res if use_res else None, out_fasta=fasta_out, id_mode=E.ID_ORDINAL, id_both=both, base=base)
                same(got, want, ("ordinal", n, base, b.lpr, fasta_out, both, use_res))


def check_ordinals_packed_reversed(eng):
    """2. ordinal ids on reverse-complemented output: the rank feeds both pk_off and the id"""
    rng = np.random.default_rng(7)
    b = Block(eng, make_block(rng, 700, numeric="alternating"))
    r, res = run(eng, b, compact=True, stages=8)
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")
    packed = [(rec[1][::-1].translate(comp), qual_values(rec, 33)[::-1]) for rec in records(b.data, 4)]
    for both in (True, False):
        want = expected(b.data, 4, res=res, id_mode=E.ID_ORDINAL, id_both=both, base=98, packed=packed)
        same(fmt(eng, b, res=r.res, packed=(r.out_bases, r.out_qual, r.out_off), reverse=True, id_mode=E.ID_ORDINAL, id_both=both, base=98), want, ("revcomp", both))


def check_sequence_ids(eng):
    """3. sequence ids: ragged lengths, the OUTPUT slice under a fixed trim, one 24 999-base read (the index flags its length for the host reader;
    the formatter takes it as it is), id_both on and off, FASTA in"""
    rng = np.random.default_rng(11)
    T = eng.torch
    fq = Block(eng, make_block(rng, 300, lmin=1, lmax=120, numeric="alternating"))
    fa = Block(eng, make_block(rng, 300, lmin=1, lmax=120, fasta=True), fasta=True)
    long_read = Block(eng, make_block(rng, 3, lmin=5, lmax=9) + make_block(rng, 1, lmin=24999, lmax=24999) + make_block(rng, 2, lmin=5, lmax=9), irregular=0x04)
    trim = Block(eng, make_block(rng, 300, lmin=4, lmax=120))
    res_t = [(1, len(rec[1]) - 3) for rec in records(trim.data, 4)]          # fastx_trimmer -f 4: every record from its fourth base on
    d_res = T.tensor([(1 << 16) | ln for _, ln in res_t], dtype=T.int32, device=eng.device)
    for both in (True, False):
        for b in (fq, fa, long_read):
            same(fmt(eng, b, id_mode=E.ID_SEQUENCE, id_both=both), expected(b.data, b.lpr, id_mode=E.ID_SEQUENCE, id_both=both), ("seq", b.lpr, b.n, both))
        same(fmt(eng, fq, out_fasta=True, id_mode=E.ID_SEQUENCE, id_both=both), expected(fq.data, 4, out_fasta=True, id_mode=E.ID_SEQUENCE, id_both=both), ("seq fasta out", both))
        same(fmt(eng, trim, res=d_res, fwd_start=3, id_mode=E.ID_SEQUENCE, id_both=both),
             expected(trim.data, 4, res=res_t, fwd_start=3, id_mode=E.ID_SEQUENCE, id_both=both), ("seq of the slice", both))


def check_quality_modes(eng, qoffset):
    """4. every quality value of the offset, lengths around the per-lane shares, records ASCII / numeric / alternating, the three modes, forward and
    packed (masker) sources; as-input on the alternating block is the old entry's output byte for byte"""
    for numeric in ("none", "all", "alternating"):
        b = Block(eng, quality_range_block(qoffset, numeric), qoffset=qoffset)
        r, res = run(eng, b, compact=True, stages=0x40, mask_min_quality=20, mask_char="N")
        recs = records(b.data, 4)
        packed = [(bytes(c if v >= 20 else 78 for c, v in zip(rec[1], qual_values(rec, qoffset))), qual_values(rec, qoffset)) for rec in recs]
        for mode in (E.QUAL_AS_INPUT, E.QUAL_ASCII, E.QUAL_NUMERIC):
            same(fmt(eng, b, qual_mode=mode), expected(b.data, 4, qoffset, qual_mode=mode), ("forward", qoffset, numeric, mode))
            same(fmt(eng, b, res=r.res, packed=(r.out_bases, r.out_qual, r.out_off), qual_mode=mode),
                 expected(b.data, 4, qoffset, res=res, qual_mode=mode, packed=packed), ("masked", qoffset, numeric, mode))
        whole = eng.torch.tensor([(1 << 16) | len(rec[1]) for rec in recs], dtype=eng.torch.int32, device=eng.device)
        old = fmt(eng, b, res=whole, plain_entry=True, cap=b.text_len + b.n + 16)
        same(old, expected(b.data, 4, qoffset), ("old entry", qoffset, numeric))
        assert fmt(eng, b, res=whole)[1] == old[1] and fmt(eng, b, res=r.res, packed=(r.out_bases, r.out_qual, r.out_off))[1] == \
            fmt(eng, b, res=r.res, packed=(r.out_bases, r.out_qual, r.out_off), plain_entry=True, cap=b.text_len + b.n + 16)[1]


def check_engine_method(eng):
    """Engine.fastq_format with the new arguments sizes its output itself"""
    rng = np.random.default_rng(5)
    b = Block(eng, make_block(rng, 40, numeric="alternating"))
    out = eng.fastq_format(b.d_text, b.text_len, b.ix, b.n, rows_qual=b.qual, id_mode=E.ID_ORDINAL, id_both=True, ordinal_base=999998, qual_mode=E.QUAL_NUMERIC, lens=b.lens)
    assert bytes(out.cpu().numpy()) == expected(b.data, 4, id_mode=E.ID_ORDINAL, id_both=True, base=999998, qual_mode=E.QUAL_NUMERIC)
    _, res = run(eng, b, stages=4, qf_min_quality=45, qf_min_percent=50)
    r, _ = run(eng, b, stages=4, qf_min_quality=45, qf_min_percent=50)
    assert bytes(eng.fastq_format(b.d_text, b.text_len, b.ix, b.n, r.res, rows_qual=b.qual).cpu().numpy()) == expected(b.data, 4, res=res)


# ---- refused requests (in the way of tests/request_cases.py: the code and the fxg_last_error text of each, literal) ----------------------
REFUSALS = [
    # name, keyword arguments of fmt(), fxg_last_error (None: a bare FXG_E_INVALID)
    ("unknown_id_mode", dict(id_mode=3), "unknown id mode 3"),
    ("unknown_id_mode_high_bit", dict(id_mode=0x80000001), "unknown id mode 2147483649"),
    ("unknown_qual_mode", dict(qual_mode=3), "unknown quality mode 3"),
    ("no_res_with_first_base", dict(fwd_start=2), "without res every record is kept whole: no packed output and no first base"),
    ("ordinals_past_u64", dict(id_mode=1, base=2 ** 64 - 2), "ordinal ids from 18446744073709551615 on pass 2^64 - 1"),
]


def check_requests(eng):
    """5. the total is known before the format kernel: total + 0 is accepted, total - 1 refused with the output untouched; unknown modes are refused"""
    rng = np.random.default_rng(3)
    b = Block(eng, make_block(rng, 300, numeric="alternating"))
    for kw in (dict(), dict(id_mode=E.ID_ORDINAL, id_both=True, base=98), dict(id_mode=E.ID_SEQUENCE, id_both=True), dict(qual_mode=E.QUAL_NUMERIC)):
        want = expected(b.data, 4, **kw)
        same(fmt(eng, b, cap=len(want), **kw), want, ("exact capacity", kw))
        rc, _, _ = fmt(eng, b, cap=len(want) - 1, **kw)
        assert rc == -1 and eng.lib.fxg_last_error(eng.ctx).decode() == "the formatted block needs %d bytes, d_out takes %d" % (len(want), len(want) - 1), kw
    for name, kw, text in REFUSALS:
        rc, _, _ = fmt(eng, b, cap=1 << 16, **kw)
        assert rc == -1 and (text is None or eng.lib.fxg_last_error(eng.ctx).decode() == text), (name, rc, eng.lib.fxg_last_error(eng.ctx))
    nb, o = C.c_uint64(), E.FxgFormatOpts(0, 0, 0, 0, 1 << 20, None)          # neither res nor lengths; no opts at all
    args = (eng.ctx, b.d_text.data_ptr(), 4, b.ix.line.data_ptr(), b.ix.cap_lines, b.ix.flags.data_ptr(), b.n, None, 0, 0, None, None, None, b.qual.data_ptr(), b.stride, 33, 0,
            b.d_text.data_ptr(), C.byref(nb))
    assert eng.lib.fxg_fastq_format_opts(*args, C.byref(o)) == -1 and eng.lib.fxg_fastq_format_opts(*args, None) == -1
