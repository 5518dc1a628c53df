"""GPU tier: poison and canaries around every array the C-ABI is handed (include/fxg.h, "Memory contract").

Nothing here is placed at an unmapped boundary: every array is a view in the middle of a larger allocation, with 4 KiB on either side.
Around an input the bytes are poison that would change the answer if a kernel used them -- adapter continuations and bytes outside ACGTN
for the bases, qualities below and above every threshold, lengths of 65535 -- and the run is compared with the oracle.  Around an output
they are a sentinel that must be unchanged after the run (res, out_bases / out_qual at exactly n * stride bytes, the meta arrays, the
counters, the statistics histogram, the text path's line / length / flag arrays, packed rows and formatted output).  Poison catches reads whose
values reach a result, canaries every stray write; the CPU tier's guard pages (test_emu_bounds.py) catch the reads whose values are thrown away.
The shapes are that tier's cases, run on the kernels the GPU really launches (fxg_kernel_rows / _rows_multi, every clip form with
FXG_CLIP_GLOBAL forced both ways, the statistics kernel's piece form, the <0,5> reverse complement, the text kernels).
"""
import ctypes as C

import numpy as np
import pytest

import test_emu_bounds as eb
from helpers import assert_same, oracle_params
from oracle import fxoracle_py as fo

pytestmark = pytest.mark.gpu
PAD = 4096
SENTINEL = b"\xa5\x5a\xc3\x3c"
QPOISON = bytes([33, 126, 34, 125])            # qualities below and above every threshold the cases use


class Framed:
    """`nbytes` of device memory in the middle of PAD + nbytes + PAD, the frame filled with `outside` (tiled), the middle with `inside`."""

    def __init__(self, engine, nbytes, outside, inside=None):
        import torch
        self.nbytes = nbytes
        host = np.resize(np.frombuffer(outside, dtype=np.uint8), PAD + nbytes + PAD).copy()
        if inside is not None:
            host[PAD:PAD + nbytes] = np.ascontiguousarray(inside).view(np.uint8).reshape(-1)
        self.host = host
        self.whole = torch.from_numpy(host).to(engine.device)
        self.view = self.whole[PAD:PAD + nbytes]
        assert self.view.data_ptr() % 16 == 0

    def typed(self, dtype, shape=None):
        v = self.view.view(dtype)
        return v.view(*shape) if shape else v

    def check(self, what):
        w = self.whole.cpu().numpy()
        for side, lo, hi in (("before", 0, PAD), ("after", PAD + self.nbytes, 2 * PAD + self.nbytes)):
            bad = np.nonzero(w[lo:hi] != self.host[lo:hi])[0]
            assert len(bad) == 0, "%s: %d bytes %s the array changed, first at offset %d" % (
                what, len(bad), side, (lo + int(bad[0]) - PAD - (self.nbytes if side == "after" else 0)))


def _base_poison(c):
    ad = c.get("adapter")
    return (ad.encode() * 2) if ad else b"NxnAC@"


PIPE = [c for c in eb.CASES if c.get("kind", "pipe") == "pipe" and c["guard"] == "after"]
QSTATS = [c for c in eb.CASES if c.get("kind") == "qstats"]
TEXT = [c for c in eb.CASES if c.get("kind") == "text" and c["at_eof"] == 1]
FMTOPTS = [c for c in eb.CASES if c.get("kind") == "fmtopts" and c["guard"] == "after"]


@pytest.mark.parametrize("case", PIPE, ids=[c["name"] for c in PIPE])
def test_pipeline_poison_and_canaries(engine, monkeypatch, case):
    import torch
    from fastx_toolkit_amd import FxgError, make_params
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(case["seed"])
    shared = case.get("batches") or (case["params"]["stages"] & 1 and case["lens"] != "fixed")
    al = fo.aligner_new() if shared else None
    engine.set_clip_history(bool(shared))
    try:
        for k in range(case.get("batches") or 1):
            b, q, lens = eb._batch(case, rng, case.get("adapter"))
            n, stride = b.shape
            fb = Framed(engine, n * stride, _base_poison(case), b)
            fq = Framed(engine, n * stride, QPOISON, q)
            fl = Framed(engine, 2 * n, b"\xff\xff", lens) if lens is not None else None
            outs = dict(res=Framed(engine, 4 * n, SENTINEL), out_bases=Framed(engine, n * stride, SENTINEL), out_qual=Framed(engine, n * stride, SENTINEL),
                        out_len=Framed(engine, 2 * n, SENTINEL), kept_index=Framed(engine, 4 * n, SENTINEL), out_off=Framed(engine, 8 * n, SENTINEL),
                        counters=Framed(engine, 8 * 24, SENTINEL))
            types = dict(res=torch.int32, out_bases=torch.uint8, out_qual=torch.uint8, out_len=torch.int16, kept_index=torch.int32, out_off=torch.int64,
                         counters=torch.int64)
            o = {name: f.typed(types[name]) for name, f in outs.items()}
            r = engine.run(fb.typed(torch.uint8, (n, stride)), fq.typed(torch.uint8, (n, stride)), make_params(**case["params"]),
                           lens=fl.typed(torch.int16) if fl else None, outputs=o)
            what = "%s.b%d" % (case["name"], k)
            if case.get("tail") == "odd" and case["params"]["stages"] & (8 | 128 | 256):
                with pytest.raises(FxgError):
                    r.counters
            else:
                assert_same(fo.run_pipeline(b, q, lens, oracle_params(case["params"]), aligner=al), r.to_host(), what)
            engine.sync()
            for name, f in list(outs.items()) + [("bases", fb), ("qual", fq)] + ([("len", fl)] if fl else []):
                f.check("%s: %s" % (what, name))
    finally:
        engine.set_clip_history(False)
        if al:
            fo.aligner_free(al)


@pytest.mark.parametrize("case", QSTATS, ids=[c["name"] for c in QSTATS])
def test_quality_stats_poison_and_canaries(engine, case):
    import torch
    rng = np.random.default_rng(case["seed"])
    b, q, lens = eb._batch(case, rng, None)
    n, stride = b.shape
    fb, fq = Framed(engine, n * stride, b"NxACGT", b), Framed(engine, n * stride, QPOISON, q)
    fl = Framed(engine, 2 * n, b"\xff\xff", lens) if lens is not None else None
    cols = stride
    fh = Framed(engine, cols * 5 * 128 * 8, SENTINEL, np.zeros(cols * 5 * 128, dtype=np.uint64))
    h = engine.quality_stats(fb.typed(torch.uint8, (n, stride)), fq.typed(torch.uint8, (n, stride)), fl.typed(torch.int16) if fl else None,
                             hist=fh.typed(torch.int64, (cols, 5, 128)))
    qs = fo.QStats()
    qs.add(b, q, lens, qoffset=33)
    assert np.array_equal(h.cpu().numpy().view(np.uint64), qs.device_layout(cols, 33)), case["name"]
    qs.close()
    for name, f in (("hist", fh), ("bases", fb), ("qual", fq)) + ((("len", fl),) if fl else ()):
        f.check("%s: %s" % (case["name"], name))


@pytest.mark.parametrize("case", TEXT, ids=[c["name"] for c in TEXT])
def test_text_poison_and_canaries(engine, case):
    """fxg_fastq_index / _pack / _format / fxg_fasta_weights on arrays of exactly their contracted sizes; the text itself is followed by its
    16 readable bytes, and those hold poison too (a newline-and-record pattern that would add records if it were parsed)."""
    from fastx_toolkit_amd.engine import FxgTextInfo
    rng = np.random.default_rng(case["seed"])
    lpr, n = case["lpr"], case["n"]
    recs, lens = [], rng.integers(1, case["maxlen"] + 1, size=n)
    lens[-1] = case["maxlen"]
    for i, L in enumerate(lens):
        s = bytes(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=int(L)))
        recs.append(b"@r%d\n%s\n+\n%s\n" % (i, s, bytes(rng.integers(33, 75, size=int(L), dtype=np.uint8))) if lpr == 4 else b">r%d\n%s\n" % (i, s))
    text = b"".join(recs)                                  # (at end of input the engine appends the missing final newline)
    poison = b"\n@p\nAC\n+\nII\n>q\nGT\n"
    lib = engine.lib
    ft = Framed(engine, len(text) + 16, poison, np.frombuffer(text + poison[:16], dtype=np.uint8))
    cap_records = len(text) // (4 if lpr == 2 else 7) + 2
    cap_lines = lpr * cap_records + 1
    fline, flen, fflags = Framed(engine, 8 * cap_lines, SENTINEL), Framed(engine, 2 * cap_records, SENTINEL), Framed(engine, cap_records, SENTINEL)
    info = FxgTextInfo()
    engine._after_torch()
    engine._check(lib.fxg_fastq_index(engine.ctx, ft.view.data_ptr(), len(text), 1, lpr, fline.view.data_ptr(), cap_lines, flen.view.data_ptr(),
                                      fflags.view.data_ptr(), C.byref(info)))
    assert info.records == n and info.irregular == 0 and info.consumed == len(text), (info.records, info.irregular, info.consumed)
    assert np.array_equal(flen.view.cpu().numpy().view(np.uint16)[:n], lens)
    stride = int(lens.max())
    rows_cap = (n * stride + 15) // 16 * 16                 # packed rows are written in whole 16-byte chunks (include/fxg.h)
    fb, fq = Framed(engine, rows_cap, SENTINEL), (Framed(engine, rows_cap, SENTINEL) if lpr == 4 else None)
    irr = C.c_uint32()
    engine._check(lib.fxg_fastq_pack(engine.ctx, ft.view.data_ptr(), len(text), lpr, fline.view.data_ptr(), cap_lines, fflags.view.data_ptr(), n, stride, 33,
                                     fb.view.data_ptr(), fq.view.data_ptr() if fq else None, C.byref(irr)))
    assert irr.value == 0
    rows = fb.view.cpu().numpy()[:n * stride].reshape(n, stride)
    for r in range(n):
        assert bytes(rows[r, :int(lens[r])]) == recs[r].split(b"\n")[1], "packed row %d" % r
    res = np.full(n, 1 << 16, dtype=np.uint32) | lens.astype(np.uint32)
    fres = Framed(engine, 4 * n, SENTINEL, res)
    fout = Framed(engine, len(text) + n + 16, SENTINEL)
    nb = C.c_uint64()
    engine._check(lib.fxg_fastq_format(engine.ctx, ft.view.data_ptr(), lpr, fline.view.data_ptr(), cap_lines, fflags.view.data_ptr(), n, fres.view.data_ptr(),
                                       0, 0, None, None, None, fq.view.data_ptr() if fq else None, stride if fq else 0, 33, 0, fout.view.data_ptr(), C.byref(nb)))
    assert fout.view[:nb.value].cpu().numpy().tobytes() == text, "formatted text"
    if lpr == 2:
        w = (C.c_uint64 * 8)()
        engine._check(lib.fxg_fasta_weights(engine.ctx, ft.view.data_ptr(), fline.view.data_ptr(), cap_lines, n, fres.view.data_ptr(), C.byref(w)))
        assert w[0] == n and w[1] == n, list(w)
    engine.sync()
    for name, f in (("text", ft), ("line", fline), ("len", flen), ("flags", fflags), ("bases", fb), ("res", fres), ("out", fout)) + ((("qual", fq),) if fq else ()):
        f.check("%s: %s" % (case["name"], name))


@pytest.mark.parametrize("case", FMTOPTS, ids=[c["name"] for c in FMTOPTS])
def test_format_opts_poison_and_canaries(engine, case):
    """fxg_fastq_format_opts with every array a view of exactly its contracted size: d_len of n values, the quality rows of n * stride bytes, the
    packed arrays of the kept bytes and records, res, flags, the line index, and d_out of exactly out_bytes (learnt from a first run into a roomy
    one).  Poison around the inputs -- lengths of 65 535, quality codes of one and two digits, kept res words, numeric flags, line offsets of
    0xA55AC33C -- would change the size or the text; the sentinel around both outputs must come back unchanged."""
    import format_opts_cases as F
    from fastx_toolkit_amd.engine import FxgFormatOpts
    kw, numeric = F.BOUNDS_MODES[case["mode"]]
    data = F.bounds_block(F.BOUNDS_LAST[case["last"]], numeric)
    q = F.bounds_request(data, case["source"])
    want = F.expected(data, 4, 33, **q["ekw"], **kw)
    before = engine.scan_recoveries()
    poison = dict(text=b"\n@p\nAC\n+\nII\n>q\nGT\n", line=SENTINEL, flags=b"\x01", lens=b"\xff\xff", rows_qual=QPOISON, res=b"\x96\x00\x01\x00", pk_bases=b"NxnAC@", pk_qual=QPOISON,
                  pk_off=b"\xff" * 8)
    f = {k: Framed(engine, q[k].nbytes, poison[k], q[k]) for k in poison if q[k] is not None}
    ptr = lambda k: f[k].view.data_ptr() if k in f else None
    outs = []
    for cap in (8 * len(data), len(want)):
        fout = Framed(engine, cap, SENTINEL)
        nb = C.c_uint64()
        o = FxgFormatOpts(kw.get("id_mode", 0), int(kw.get("id_both", False)), kw.get("base", 0), kw.get("qual_mode", 0), cap, ptr("lens"))
        engine._after_torch()
        rc = engine.lib.fxg_fastq_format_opts(engine.ctx, ptr("text"), 4, ptr("line"), q["cap_lines"], ptr("flags"), q["n"], ptr("res"), q["fwd_start"], q["reverse"], ptr("pk_bases"),
                                              ptr("pk_qual"), ptr("pk_off"), ptr("rows_qual"), q["stride"], 33, 0, fout.view.data_ptr(), C.byref(nb), C.byref(o))
        engine._before_torch()
        engine._check(rc)
        engine.sync()
        assert nb.value == len(want) and fout.view[:nb.value].cpu().numpy().tobytes() == want, (case["name"], cap, nb.value, len(want))
        outs.append(fout)
    for name, fr in list(f.items()) + [("out, roomy", outs[0]), ("out, exact", outs[1])]:
        fr.check("%s: %s" % (case["name"], name))
    assert engine.scan_recoveries() == before
