"""GPU tier (-m gpu -k large_offsets): every kernel family across the 2, 4 and 8 GiB marks of its arrays.

The kernels address memory as a 64-bit, wave-uniform base per tile plus 32-bit, tile-relative lane offsets.  That is right only while every
instance forms its base, its dword / chunk counts and its output offset in 64 bits; a slip shows where a byte offset passes 2^31 (a signed
int), 2^32 (a u32) or 2^33 (an int count of dwords).  Here every family of tests/test_gpu_geometry.py::FAM, fxg_kernel_rows<38,2> and the
one-pass long clip form run on batches whose input arrays AND packed outputs pass all three marks (tests/large_offsets.py: CASES; N from the
oracle's kept bytes per read, 57 M .. 507 M reads), in three shapes: fixed (length = stride; then the meta=False call shape into the same
outputs and compact=False), ragged (lens[r] a hash of the read index, tiny and empty reads included) and padded (fixed_len = stride - 3).

Each run asserts the instance that ran, scan_recoveries() unchanged (the host's redo after a time-out gives correct output and would hide a
broken offset), the marks it declared, the offset algebra on the device, and windows of 3 000 reads against the oracle placed BY BYTE
POSITION: the prefix, the suffix, the window centred on each crossed mark of the input and of the output, and eight seeded random ones --
res[], the window's bytes, lengths and indices at their place in the packed stream, bases and qualities.  Stages with a closed form (fixed
trim, reverse complement, masker, the census where every read is kept) are compared over the WHOLE stream in slabs, which catches one
misplaced tile anywhere.  The statistics kernel (both forms) and the no-scanner fallback run past 2^33 bytes too.

Not included: the clip instance with history.  Its result for a read depends on every earlier read, so no window can be checked alone;
csrc/fxg_history.h forms its offsets in 64 bits throughout and its per-read bodies run in the CPU emulator.

A failure names the case, the shape, the window ("input 2^32", "output 2^33", "random", "prefix", "suffix"), the array and the first
differing index.
"""
import os
import time

import numpy as np
import pytest

import large_offsets as lo
from oracle import fxoracle_py as fo
from test_gpu_geometry import CALL_KNOBS

pytestmark = pytest.mark.gpu

FAMS = lo.families()


def _np_same(name, array, got, exp, at=0):
    if got.shape != exp.shape:
        raise AssertionError("%s: %s has %d elements at %d, the oracle %d" % (name, array, got.size, at, exp.size))
    if not np.array_equal(got, exp):
        i = int(np.nonzero(got != exp)[0][0])
        raise AssertionError("%s: %s differs first at index %d (= %d + %d): engine %r oracle %r" % (name, array, at + i, at, i, got[i], exp[i]))


def _dev_same(torch, name, array, got, exp, at=0):
    if got.shape != exp.shape:
        raise AssertionError("%s: %s has shape %s, expected %s" % (name, array, tuple(got.shape), tuple(exp.shape)))
    if not torch.equal(got, exp):
        i = int(torch.nonzero(got != exp).flatten()[0])
        raise AssertionError("%s: %s differs first at index %d (= %d + %d): engine %r expected %r" % (name, array, at + i, at, i, got[i].item(), exp[i].item()))


def _kernel_name(fam, f, shape, compact):
    if not compact and f.get("rows"):
        return "fxg_kernel_tiles<0,0>"                # uncompacted launches never take the rows kernels: they need no output placement
    if fam == "rev5" and shape == "ragged":
        return "fxg_kernel_tiles<0,2> revcomp"        # the dword form serves fixed-length batches only
    return f["kernel"]


def _launch(eng, monkeypatch, name, fam, f, shape, b, q, dl, compact=True, meta=True, outputs=None, recoveries=0, kernel=None):
    """One launch under the family's call knobs; the counters are read (which is where a time-out would be redone), then the instance and the
    number of recoveries are asserted."""
    from fastx_toolkit_amd import make_params
    for k in CALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in f.get("env", {}).items():
        monkeypatch.setenv(k, v)
    st = f["stride"]
    fl = None if shape == "ragged" else st - lo.PAD if shape == "padded" else st
    before = eng.scan_recoveries()
    try:
        r = eng.run(b, q, make_params(**f["pd"]), lens=dl, fixed_len=fl, compact=compact, meta=meta, outputs=outputs)
        r.counters
    finally:
        for k in f.get("env", {}):
            monkeypatch.delenv(k, raising=False)
    ll = eng.last_launch()
    assert eng.scan_recoveries() == before + recoveries, "%s: %d scan recoveries, expected %d (%r)" % (name, eng.scan_recoveries() - before, recoveries, ll)
    assert ll["kernel"].startswith(kernel or _kernel_name(fam, f, shape, compact)), "%s: ran %r" % (name, ll)
    return r, ll


def _algebra(torch, name, r, N):
    """2a: kept, kept_bytes, out_len == lens[keepmask], out_off == exclusive cumsum(out_len), kept_index == nonzero(keepmask)."""
    c = r.counters
    kept, nbytes = int(c[1]), int(c[2])
    res = r.res.view(torch.int32)
    keepmask = ((res >> 16) & 1).bool()
    kl = (res & 0xFFFF).to(torch.int64)[keepmask]
    assert int(c[0]) == N, "%s: counters[input] %d" % (name, int(c[0]))
    assert int(keepmask.sum()) == kept, "%s: %d reads kept in res[], counters say %d" % (name, int(keepmask.sum()), kept)
    assert int(kl.sum()) == nbytes, "%s: %d bytes kept in res[], counters say %d" % (name, int(kl.sum()), nbytes)
    ol = r.out_len[:kept].to(torch.int64) & 0xFFFF
    _dev_same(torch, name, "out_len (against res[] of the kept reads)", ol, kl)
    del kl
    off = torch.cumsum(ol, 0) - ol
    _dev_same(torch, name, "out_off (against the exclusive scan of out_len)", r.out_off[:kept], off)
    del off, ol
    _dev_same(torch, name, "kept_index (against nonzero(kept))", r.kept_index[:kept].to(torch.int64), torch.nonzero(keepmask).flatten())
    return keepmask, kept, nbytes


def _windows(torch, name, f, shape, r, b, q, keepmask, kept, nbytes, N, in_marks, out_marks, random=True):
    """2b: windows by byte position against the oracle."""
    st, k = f["stride"], min(lo.KI, N)
    clip = bool(f.get("clip"))
    host = lambda t: t.cpu().numpy()
    for label, r0, side, mark in lo.windows(N, st, in_marks, out_marks, r.out_off[:kept], r.kept_index, lo.SEED):
        if label == "random" and not random:
            continue
        w = "%s, window %s (reads %d..%d)" % (name, label, r0, r0 + k)
        ob, oq = fo.synth_batch(lo.SEED, r0, k, st, clip, st)
        _np_same(w, "input bases", host(b[r0:r0 + k]).reshape(-1), ob.reshape(-1), r0 * st)
        _np_same(w, "input qualities", host(q[r0:r0 + k]).reshape(-1), oq.reshape(-1), r0 * st)
        o = lo.oracle_window(f, ob, oq, r0, shape)
        kw, nw = len(o["kept_index"]), len(o["out_bases"])
        rank = int(keepmask[:r0].sum())
        o0 = int(r.out_off[rank]) if rank < kept else nbytes
        if side == "in":
            assert r0 * st <= mark < (r0 + k) * st, "%s does not hold its mark" % w
        if side == "out":
            assert o0 <= mark <= o0 + nw, "%s does not hold its mark: its packed bytes are %d..%d" % (w, o0, o0 + nw)
        _np_same(w, "res", host(r.res[r0:r0 + k]).view(np.uint32), o["res"], r0)
        _np_same(w, "out_bases", host(r.out_bases[o0:min(nbytes, o0 + nw)]), o["out_bases"], o0)
        _np_same(w, "out_qual", host(r.out_qual[o0:min(nbytes, o0 + nw)]), o["out_qual"], o0)
        _np_same(w, "kept_index", host(r.kept_index[rank:min(kept, rank + kw)]).view(np.uint32), o["kept_index"] + np.uint32(r0), rank)
        _np_same(w, "out_len", host(r.out_len[rank:min(kept, rank + kw)]).view(np.uint16), o["out_len"], rank)


def _whole_stream(torch, name, fam, f, r, b, q, N, kept, nbytes):
    """2c: the whole packed stream against the stage's closed form, in slabs; res[] constant."""
    if lo.closed_form(torch, fam, f, b[:1], q[:1]) is None:
        return False
    assert kept == N, "%s: %d of %d reads kept, the oracle keeps every read" % (name, kept, N)
    L = 0
    for s in range(0, N, lo.SLAB):
        e = min(N, s + lo.SLAB)
        eb, eq = lo.closed_form(torch, fam, f, b[s:e], q[s:e])
        L = eb.shape[1]
        _dev_same(torch, name + ", whole stream", "out_bases", r.out_bases[s * L:e * L], eb.reshape(-1), s * L)
        _dev_same(torch, name + ", whole stream", "out_qual", r.out_qual[s * L:e * L], eq.reshape(-1), s * L)
        del eb, eq
    assert nbytes == N * L, "%s: %d bytes kept, closed form %d" % (name, nbytes, N * L)
    first = r.res[:1].clone()
    for s in range(0, N, lo.SLAB * 8):
        part = r.res[s:s + lo.SLAB * 8]
        _dev_same(torch, name + ", whole stream", "res (constant)", part, first.expand_as(part), s)
    return True


def _marks(name, N, stride, nbytes, declared):
    got = (lo.crossed(N * stride), lo.crossed(nbytes))
    if declared is not None:
        assert got == tuple(declared), "%s: crossed marks (input, output) %r, declared %r (input %d bytes, output %d)" % (name, got, declared, N * stride, nbytes)
    return got


def run_case(eng, monkeypatch, fam, shape, N, declared, random=True):
    """One family in one shape on N reads.  `declared`: the (input, output) marks of the case table, asserted against the sizes that came out."""
    import torch
    f = FAMS[fam]
    st = f["stride"]
    name = "%s %s N=%d" % (fam, shape, N)
    t0 = time.time()
    try:
        b, q = eng.synth(lo.SEED, 0, N, st, bool(f.get("clip")), st)
        dl = lo.lens_torch(torch, 0, N, st, f["pd"], eng.device) if shape == "ragged" else None
        r, ll = _launch(eng, monkeypatch, name, fam, f, shape, b, q, dl)
        keepmask, kept, nbytes = _algebra(torch, name, r, N)
        in_marks, out_marks = _marks(name, N, st, nbytes, declared)
        _windows(torch, name, f, shape, r, b, q, keepmask, kept, nbytes, N, in_marks, out_marks, random)
        whole = shape == "fixed" and _whole_stream(torch, name, fam, f, r, b, q, N, kept, nbytes)
        extra = ""
        if shape == "fixed":
            cs, c13 = r.checksum(), np.array(r.counters[:13])
            res1 = r.res.clone()
            outs = dict(res=r.res, out_bases=r.out_bases, out_qual=r.out_qual, counters=torch.zeros_like(r.d_counters), out_len=None, kept_index=None, out_off=None)
            del keepmask, r
            torch.cuda.empty_cache()
            outs["res"].zero_(); outs["out_bases"][:nbytes].zero_(); outs["out_qual"][:nbytes].zero_()
            # the benchmarked call shape: no per-kept-read arrays, into the same outputs
            r2, _ = _launch(eng, monkeypatch, name + " meta=False", fam, f, shape, b, q, None, meta=False, outputs=outs)
            assert r2.out_off is None and r2.out_len is None and r2.kept_index is None
            assert np.array_equal(np.array(r2.counters[:13]), c13), "%s meta=False: counters %r, with meta %r" % (name, r2.counters[:13], c13)
            cs2 = r2.checksum()
            assert cs2 == cs, "%s meta=False: checksum %d, with meta %d" % (name, cs2, cs)
            del r2, outs
            torch.cuda.empty_cache()
            # decisions only
            r3, ll3 = _launch(eng, monkeypatch, name + " compact=False", fam, f, shape, b, q, None, compact=False)
            assert np.array_equal(np.array(r3.counters[:13]), c13), "%s compact=False: counters %r, compacting %r" % (name, r3.counters[:13], c13)
            _dev_same(torch, name + " compact=False", "res (against the compacting run)", r3.res, res1)
            extra = " checksum %d, meta=False and compact=False (%s) equal" % (cs, ll3["kernel"].split(" ")[0])
            del r3, res1
        print("large_offsets %s: %s tile %d grid %d; input %.2f GiB marks %r; kept %d, output %.2f GiB marks %r; whole stream %s;%s %.1f s, peak %.1f GB"
              % (name, ll["kernel"], ll["tile_reads"], ll["grid"], N * st / 2**30, in_marks, kept, nbytes / 2**30, out_marks, "checked" if whole else "-", extra,
                 time.time() - t0, torch.cuda.max_memory_allocated() / 1e9))
    finally:
        b = q = dl = r = keepmask = None
        torch.cuda.empty_cache()


CASE_IDS = [(fam, shape) for fam in lo.CASES for shape in lo.shapes(fam)]


@pytest.mark.parametrize("fam,shape", CASE_IDS, ids=["%s-%s" % c for c in CASE_IDS])
def test_large_offsets_family(engine, monkeypatch, fam, shape):
    if FAMS[fam].get("clip") and len(FAMS[fam]["pd"]["adapter"]) > 16:     # which long clip form the case is: the name does not say
        assert lo.clip_one_pass(len(FAMS[fam]["pd"]["adapter"]), FAMS[fam]["stride"]) == (fam == "clip72")
    run_case(engine, monkeypatch, fam, shape, lo.CASES[fam]["N"], lo.CASES[fam][shape])


def test_large_offsets_fallback_without_the_scanner(engine, monkeypatch):
    """2e: rows38 fixed at its N in the form that cannot wait (csrc/fxg_fallback.h: its own 64-bit scan and gather), forced by
    FXG_TEST_SCAN_TIMEOUT=1 on a fresh Engine: same counters and checksum as the normal run, the offset algebra, the prefix, suffix and mark
    windows.  Here, and only here, scan_recoveries() goes up by exactly one."""
    import torch
    from fastx_toolkit_amd import Engine
    fam, shape = "rows38", "fixed"
    f, N = FAMS[fam], lo.CASES[fam]["N"]
    st = f["stride"]
    name = "%s fixed N=%d, fallback" % (fam, N)
    monkeypatch.setenv("FXG_TEST_SCAN_TIMEOUT", "1")
    eng = Engine(0)
    monkeypatch.delenv("FXG_TEST_SCAN_TIMEOUT")
    t0 = time.time()
    try:
        b, q = engine.synth(lo.SEED, 0, N, st, False, st)
        r, _ = _launch(engine, monkeypatch, name + " (normal run)", fam, f, shape, b, q, None, meta=False)
        c13, cs = np.array(r.counters[:13]), r.checksum()
        del r
        torch.cuda.empty_cache()
        # (after the redo the last launch is the decision-only instance of the request: the rows kernels exist in their compacting form only)
        r, ll = _launch(eng, monkeypatch, name, fam, f, shape, b, q, None, recoveries=1, kernel=_kernel_name(fam, f, shape, False))
        assert np.array_equal(np.array(r.counters[:13]), c13), "%s: counters %r, normal run %r" % (name, r.counters[:13], c13)
        keepmask, kept, nbytes = _algebra(torch, name, r, N)
        in_marks, out_marks = _marks(name, N, st, nbytes, lo.CASES[fam][shape])
        _windows(torch, name, f, shape, r, b, q, keepmask, kept, nbytes, N, in_marks, out_marks, random=False)
        cs2 = r.checksum()
        assert cs2 == cs, "%s: checksum %d, normal run %d" % (name, cs2, cs)
        print("large_offsets %s: redone as %r, checksum %d equal; %.1f s" % (name, ll, cs, time.time() - t0))
    finally:
        eng.close()
        b = q = r = keepmask = None
        torch.cuda.empty_cache()


def stats_expected(torch, b, q, lens, fixed_len):
    """hist[col][class][quality] by torch.bincount over (class, quality) with the col < len mask, every column."""
    n, stride = b.shape
    cls = torch.zeros(256, dtype=torch.int64, device=b.device)
    for ch, k in ((65, 0), (67, 1), (71, 2), (84, 3), (78, 4)):
        cls[ch] = k
    exp = torch.zeros((stride, 5, 128), dtype=torch.int64, device=b.device)
    for col in range(stride):
        key = cls[b[:, col].long()] * 128 + q[:, col].long()
        if lens is not None:
            key = key[lens.to(torch.int64) > col]
        elif col >= fixed_len:
            continue
        exp[col] = torch.bincount(key, minlength=5 * 128).view(5, 128)
    return exp


def run_stats(eng, N, stride):
    import torch
    t0 = time.time()
    try:
        b, q = eng.synth(lo.SEED, 0, N, stride, False, stride)
        assert N * stride > 1 << 33 or N < 1_000_000, "the statistics batch no longer passes 2^33 bytes"
        for shape in ("fixed", "ragged", "padded"):
            dl = lo.lens_torch(torch, 0, N, stride, None, eng.device) if shape == "ragged" else None
            fl = None if shape == "ragged" else stride - lo.PAD if shape == "padded" else stride
            exp = stats_expected(torch, b, q, dl, fl)
            total = int(dl.to(torch.int64).sum()) if dl is not None else N * fl
            forms = (("piece form", None), ("row-strip form", "3")) if shape == "fixed" else (("row-strip form", "3"),)
            for form, rr in forms:
                name = "statistics %s %s N=%d x %d" % (shape, form, N, stride)
                if rr:
                    os.environ["FXG_QS_ROUND_ROBIN"] = rr
                try:
                    h = eng.quality_stats(b, q, lens=dl, fixed_len=fl)
                finally:
                    os.environ.pop("FXG_QS_ROUND_ROBIN", None)
                assert int(h.sum()) == total, "%s: hist.sum() %d, lens.sum() %d" % (name, int(h.sum()), total)
                for col in range(stride):
                    _dev_same(torch, name, "hist[%d]" % col, h[col].reshape(-1), exp[col].reshape(-1))
                print("large_offsets %s: every column equal, %d bases; %.1f s" % (name, total, time.time() - t0))
            del exp, dl
    finally:
        b = q = None
        torch.cuda.empty_cache()


def test_large_offsets_quality_stats(engine):
    """2d: the statistics kernel past 2^33 bytes -- piece form (dense rows), row-strip form on the same batch (FXG_QS_ROUND_ROBIN=3), row-strip
    form ragged and padded; every column against torch.bincount, hist.sum() == lens.sum()."""
    run_stats(engine, lo.STATS["N"], lo.STATS["stride"])
