"""GPU tier (-m gpu -k large_offsets): the device text path (csrc/fxg_text.h) and the barcode splitter (csrc/fxg_barcode.h) on blocks of exactly
0xFFFFFFF0 bytes, the largest text_len the C-ABI accepts.

These are the parts of the engine that address memory with plain 32-bit numbers: d_line holds u32 line starts and ends, and every offset that
reaches a load or a store is a u32 or a sum of u32s.  A line start kept in an int, a u32 sum that wraps or an off-by-16 at the cap shows only on
a block that passes 2^31 and ends at the cap.  tests/large_text.py generates three such blocks on the device (fastq_lf, fastq_mixed with CRLF
and numeric quality lines, fasta_short with more than 2^26 records) as pure functions of the record index, and states in closed form what
fxg_fastq_index, fxg_fastq_pack, fxg_fastq_format, fxg_fasta_weights and fxg_barcode_split must make of them (tests/test_large_text_cpu.py pins
that code against the oracle, the model and the reference driver).

Every comparison is exact.  Whole arrays are compared on the device in slabs wherever the closed form is a torch expression (line starts and
ends, lengths, flags, packed rows, rec_bin, the whole split output); windows of 3 000 records placed BY BYTE POSITION -- prefix, suffix, every
crossed mark of the input and of each output, the first and last bin boundary, eight seeded random ones -- go through plain host code.  The scan
depths no other test reaches run here: 2^20 segments of the index, more than 2^20 records of the format (three levels), bins * tiles > 2^30 of
a 4 096-bin split (four levels).  Each case asserts scan_recoveries() unchanged and the peak of device memory under the tier's 120 GB.

A failure names the shape, the step, the window, the array and the first differing index.
"""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import large_text as lt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "fastx_toolkit_amd", "host")
POISON, CANARY = 0x5A, 0xA5
MEMORY_LIMIT = 120e9                     # what the large-offsets tier asks for (tests/README.md)
E_INVALID = -1                           # FXG_E_INVALID
REC_SLAB = 1_000_000                     # records per slab of the whole-array checks
_CACHE = {}                              # the current shape's block, text and index (one shape at a time: 4 GiB of text and up to 1.1 GB of lines)


def _same(torch, what, got, exp, at=0):
    if got.shape != exp.shape:
        raise AssertionError("%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(exp.shape)))
    if not torch.equal(got, exp):
        i = int(torch.nonzero(got.reshape(-1) != exp.reshape(-1)).flatten()[0])
        raise AssertionError("%s differs first at index %d (= %d + %d): engine %r expected %r" % (what, at + i, at, i, got.reshape(-1)[i].item(), exp.reshape(-1)[i].item()))


def _bytes_same(what, got, exp, at=0):
    got, exp = np.frombuffer(bytes(got), np.uint8), np.frombuffer(bytes(exp), np.uint8)
    if got.shape != exp.shape:
        raise AssertionError("%s: %d bytes at %d, expected %d" % (what, got.size, at, exp.size))
    if not np.array_equal(got, exp):
        i = int(np.flatnonzero(got != exp)[0])
        raise AssertionError("%s differs first at byte %d (= %d + %d): engine %r expected %r" % (what, at + i, at, i, bytes(got[i:i + 40]), bytes(exp[i:i + 40])))


def _lo():
    return lt.MARKS[0]                   # 31: the mark the input crosses


def _hi():
    return lt.MARKS[1]                   # 32: the mark only an output that outgrows the input crosses


def _u32(t):
    """an int32 device tensor of u32 values as int64"""
    return t.long() & 0xFFFFFFFF


def block(eng, shape):
    """The shape's block on the device, indexed once: dict(b, text, ix, lens, info).  Building another shape drops the one before."""
    torch = eng.torch
    if _CACHE.get("shape") != shape:
        _CACHE.clear()
        torch.cuda.empty_cache()
        t0 = time.time()
        b = lt.Block(torch, shape, lt.BLOCKS[shape], device=eng.device)
        assert b.text_len == lt.CAP, "%s: %d records make %d bytes" % (shape, b.n, b.text_len)
        text = b.build(tail=16, poison=POISON)
        torch.cuda.synchronize()
        t1 = time.time()
        ix, lens, info = eng.fastq_index(text, b.text_len, cap_records=b.n + 2, fasta=b.fasta)
        _CACHE.update(shape=shape, b=b, text=text, ix=ix, lens=lens, info=info)
        print("large_offsets text %s: %d records, %d bytes generated in %.1f s, indexed in %.1f s" % (shape, b.n, b.text_len, t1 - t0, time.time() - t1))
    return _CACHE


def _finish(eng, name, t0, before):
    torch = eng.torch
    torch.cuda.synchronize()
    assert eng.scan_recoveries() == before, "%s: scan recoveries went from %d to %d" % (name, before, eng.scan_recoveries())
    peak = torch.cuda.max_memory_allocated()
    assert peak < MEMORY_LIMIT, "%s: peak of device memory %.1f GB" % (name, peak / 1e9)
    assert bool((_CACHE["text"][lt.CAP:] == POISON).all()), "%s: the 16 bytes behind the text changed" % name
    print("large_offsets text %s: %.1f s, peak %.1f GB" % (name, time.time() - t0, peak / 1e9))


# ---- the C-ABI with every output between canaries ------------------------------------------------------------------------------------------
GUARD = 64


def _canaried(torch, eng, nbytes, dtype=None):
    """(buffer, view): nbytes of CANARY between two guards of CANARY; the view starts 16-byte aligned"""
    buf = torch.full((GUARD + nbytes + GUARD,), CANARY, dtype=torch.uint8, device=eng.device)
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf, nbytes, written, what):
    assert bool((buf[:GUARD] == CANARY).all()), what + ": write in front of the array"
    assert bool((buf[GUARD + written:] == CANARY).all()), what + ": write behind byte %d of the array (capacity %d)" % (written, nbytes)


def abi_index(eng, text, text_len, at_eof, lpr, cap_records):
    """fxg_fastq_index into canaried arrays: (line int32 view [2 * cap_lines], cap_lines, lens, flags, info, check(lines, records))"""
    from fastx_toolkit_amd.engine import FxgTextInfo
    torch = eng.torch
    cap_lines = lpr * cap_records + 1
    lb, line = _canaried(torch, eng, 8 * cap_lines)
    nb, lens = _canaried(torch, eng, 2 * cap_records)
    fb, flags = _canaried(torch, eng, cap_records)
    info = FxgTextInfo()
    eng._after_torch()
    eng._check(eng.lib.fxg_fastq_index(eng.ctx, text.data_ptr(), text_len, int(at_eof), lpr, line.data_ptr(), cap_lines, lens.data_ptr(), flags.data_ptr(), C.byref(info)))
    torch.cuda.synchronize()

    def check(what):
        lines, n = info.lines, info.records
        _guards_intact(lb, 8 * cap_lines, 8 * cap_lines, what + ", d_line")
        li = line.view(torch.int32)
        can = int(np.array([CANARY] * 4, np.uint8).view(np.int32)[0])
        assert bool((li[lines + 1:cap_lines] == can).all()) and bool((li[cap_lines + lines:] == can).all()), what + ": d_line written behind its last line"
        _guards_intact(nb, 2 * cap_records, 2 * n, what + ", d_len")
        _guards_intact(fb, cap_records, n, what + ", d_flags")
    return line.view(torch.int32), cap_lines, lens.view(torch.int16), flags, info, check


def abi_pack(eng, c, stride):
    """fxg_fastq_pack into canaried row arrays of the contracted n * stride bytes rounded up to 16"""
    torch, b, ix = eng.torch, c["b"], c["ix"]
    nbytes = (b.n * stride + 15) // 16 * 16
    bb, bases = _canaried(torch, eng, nbytes)
    qb, qual = _canaried(torch, eng, nbytes) if not b.fasta else (None, None)
    irr = C.c_uint32()
    eng._after_torch()
    eng._check(eng.lib.fxg_fastq_pack(eng.ctx, c["text"].data_ptr(), b.text_len, b.lpr, ix.line.data_ptr(), ix.cap_lines, ix.flags.data_ptr(), b.n, stride, 33,
                                      bases.data_ptr(), qual.data_ptr() if qual is not None else None, C.byref(irr)))
    torch.cuda.synchronize()
    _guards_intact(bb, nbytes, nbytes, "%s pack, base rows" % b.shape)
    if qb is not None:
        _guards_intact(qb, nbytes, nbytes, "%s pack, quality rows" % b.shape)
    c["row_buffers"] = (bb, qb)          # (the views below live in them)
    return bases[:b.n * stride].view(b.n, stride), (qual[:b.n * stride].view(b.n, stride) if qual is not None else None), irr.value


def abi_format(eng, c, res, fwd_start=0, packed=None, reverse=False, rows_qual=None, out_fasta=False):
    """fxg_fastq_format into a canaried array of the contracted text_len + n + 16 bytes; nothing behind out_bytes may change"""
    torch, b, ix = eng.torch, c["b"], c["ix"]
    cap = b.text_len + b.n + 16
    ob, out = _canaried(torch, eng, cap)
    nb = C.c_uint64()
    pb, pq, po = (packed[0].data_ptr(), packed[1].data_ptr() if packed[1] is not None else None, packed[2].data_ptr()) if packed else (None, None, None)
    eng._after_torch()
    eng._check(eng.lib.fxg_fastq_format(eng.ctx, c["text"].data_ptr(), b.lpr, ix.line.data_ptr(), ix.cap_lines, ix.flags.data_ptr(), b.n, res.data_ptr(), fwd_start, int(reverse),
                                        pb, pq, po, rows_qual.data_ptr() if rows_qual is not None else None, rows_qual.shape[1] if rows_qual is not None else 0, 33,
                                        int(out_fasta), out.data_ptr(), C.byref(nb)))
    torch.cuda.synchronize()
    assert nb.value <= cap
    _guards_intact(ob, cap, nb.value, "%s format, d_out" % b.shape)
    return out[:nb.value]


# ---- index -------------------------------------------------------------------------------------------------------------------------------
def run_index(eng, shape):
    torch = eng.torch
    c = block(eng, shape)
    b, ix, lens, info, text = c["b"], c["ix"], c["lens"], c["info"], c["text"]
    name, n, lpr = "%s index" % shape, c["b"].n, c["b"].lpr
    mx, mn, numeric = 0, 1 << 30, 0
    for s in range(0, n, REC_SLAB):
        e = min(n, s + REC_SLAB)
        rr = b.range(s, e)
        f = b.fields(rr)
        mx, mn, numeric = max(mx, int(f["L"].max())), min(mn, int(f["L"].min())), numeric + int(f["numeric"].sum())
        cs, ce = b.line_index(rr)
        _same(torch, name + ": line starts", _u32(ix.line[lpr * s:lpr * e]), cs.reshape(-1), lpr * s)
        _same(torch, name + ": line ends", _u32(ix.line[ix.cap_lines + lpr * s:ix.cap_lines + lpr * e]), ce.reshape(-1), lpr * s)
        _same(torch, name + ": lens", lens[s:e].to(torch.int64) & 0xFFFF, f["L"], s)
        _same(torch, name + ": flags", ix.flags[s:e].to(torch.int64), f["numeric"], s)
    got = dict(lines=info.lines, records=info.records, consumed=info.consumed, max_len=info.max_len, min_len=info.min_len, irregular=info.irregular,
               first_bad=info.first_bad, numeric_records=info.numeric_records, has_cr=info.has_cr)
    want = dict(lines=lpr * n, records=n, consumed=lt.CAP, max_len=mx, min_len=mn, irregular=0, first_bad=0xFFFFFFFF, numeric_records=numeric,
                has_cr=int(shape == "fastq_mixed"))
    assert got == want, "%s: info %r, expected %r" % (name, got, want)
    short = int(b.fields(b.range(n - 1, n))["L"][0])          # fasta_short: the last record's 1..8 bases are the shortest read
    assert mx == (60 if b.fasta else 150) and mn == (short if b.fasta else 1) and short <= 150 and (numeric > n // 100) == (shape == "fastq_mixed")
    # the package's view of the same array: u32 values wherever they are read
    assert int(ix.starts[lpr * n].item()) == lt.CAP and int(ix.ends[lpr * n - 1].item()) == lt.CAP - 1 - int(shape == "fastq_mixed") and ix.record_bytes(n) == lt.CAP
    assert np.array_equal(ix.starts[lpr * n - 4:lpr * n + 1].cpu().numpy().astype(np.int64), np.concatenate([b.line_index(b.range(n - 2, n))[0].reshape(-1).cpu().numpy()[-4:], [lt.CAP]]))
    # nothing behind the last line of either half
    assert not ix.line[lpr * n + 1:ix.cap_lines].any() and not ix.line[ix.cap_lines + lpr * n:].any(), name + ": wrote behind the last line"
    # the same block cut inside its last record, more to come: one record fewer, consumed = that record's start (above 2^31)
    cut = lt.CAP - 1
    line2, cap2, lens2, flags2, info2, check2 = abi_index(eng, text, cut, False, lpr, n + 2)
    last = int(b.rec_start[n - 1])
    assert (info2.lines, info2.records, info2.consumed, info2.irregular) == (lpr * n - 1, n - 1, last, 0) and last > 1 << _lo(), \
        "%s, at_eof=False: lines %d records %d consumed %d irregular %#x; the last record starts at %d" % (name, info2.lines, info2.records, info2.consumed, info2.irregular, last)
    check2(name + ", at_eof=False")
    _same(torch, name + ", at_eof=False: line starts", line2[:lpr * n], ix.line[:lpr * n])
    _same(torch, name + ", at_eof=False: line ends of the whole records", line2[cap2:cap2 + lpr * (n - 1)], ix.line[ix.cap_lines:ix.cap_lines + lpr * (n - 1)])
    _same(torch, name + ", at_eof=False: lens", lens2[:n - 1], lens[:n - 1])
    _same(torch, name + ", at_eof=False: flags", flags2[:n - 1], ix.flags[:n - 1])


# ---- pack --------------------------------------------------------------------------------------------------------------------------------
def packed_rows(eng, c):
    if "rows" not in c:
        b, info = c["b"], c["info"]
        bases, qual, irr = abi_pack(eng, c, info.max_len)
        assert irr == 0, "%s pack: irregular %#x" % (b.shape, irr)
        c["rows"] = (bases, qual)
    return c["rows"]


def run_pack(eng, shape):
    torch = eng.torch
    c = block(eng, shape)
    b = c["b"]
    stride = c["info"].max_len
    bases, qual = packed_rows(eng, c)
    assert bases.shape == (b.n, stride) and (qual is None) == b.fasta
    for s in range(0, b.n, REC_SLAB):
        e = min(b.n, s + REC_SLAB)
        eb, eq = b.rows_of(b.range(s, e), stride)
        _same(torch, "%s pack: base rows" % shape, bases[s:e], eb, s * stride)
        if eq is not None:
            _same(torch, "%s pack: quality rows" % shape, qual[s:e], eq, s * stride)


# ---- format ------------------------------------------------------------------------------------------------------------------------------
def _res_and_offsets(torch, b, fwd, keep_all, out_fasta):
    """(res int32 [n], out_start int64 [n + 1]) of the hand-made res[] over the whole block"""
    res = torch.empty(b.n, dtype=torch.int32, device=b.device)
    sz = torch.empty(b.n + 1, dtype=torch.int64, device=b.device)
    sz[0] = 0
    for s in range(0, b.n, REC_SLAB * 4):
        e = min(b.n, s + REC_SLAB * 4)
        rr = b.range(s, e)
        r = b.res_of(rr, fwd, keep_all)
        res[s:e] = r.to(torch.int32)
        sz[s + 1:e + 1] = b.format_sizes(rr, r, out_fasta)
    return res, torch.cumsum(sz, 0)


def _newlines(torch, t, step=1 << 30):
    return sum(int((t[s:s + step] == 10).sum()) for s in range(0, t.numel(), step))


def _format_windows(eng, name, c, out, out_start, expect, extra_marks=True, extra=()):
    """windows by byte position of the input and of the output: out[out_start[r0] : out_start[r0 + k]] against expect(text of the window, r0, r1)"""
    torch, b = eng.torch, c["b"]
    seen = set()
    for label, r0 in lt.windows(torch, b.n, b.rec_start, dict(output=out_start), lt.SEED, extra=extra):
        r1 = r0 + min(lt.KI, b.n)
        w = "%s, window %s (records %d..%d)" % (name, label, r0, r1)
        a, e = int(b.rec_start[r0]), int(b.rec_start[r1])
        wtext = bytes(b.text_of(b.range(r0, r1)).cpu().numpy())
        _bytes_same(w + ": the input text", c["text"][a:e].cpu().numpy(), wtext, a)
        o0, o1 = int(out_start[r0]), int(out_start[r1])
        for m in lt.MARKS:
            if label == "output 2^%d" % m:
                assert o0 < 1 << m < o1, "%s does not hold its mark: output bytes %d..%d" % (w, o0, o1)
            if label == "input 2^%d" % m:
                assert a < 1 << m < e, "%s does not hold its mark: input bytes %d..%d" % (w, a, e)
        _bytes_same(w + ": the formatted text", out[o0:o1].cpu().numpy(), expect(wtext, r0, r1), o0)
        seen.add(label)
    return seen


def run_format_handmade(eng, shape, keep_all, out_fasta=False):
    """fxg_fastq_format of the input slices under a hand-made res[] (fwd_start 3; keep_all: every record from its first base, where the FASTQ
    output outgrows the input and passes 2^32)"""
    torch = eng.torch
    c = block(eng, shape)
    b = c["b"]
    fwd = 0 if keep_all else 3
    name = "%s format%s%s" % (shape, " of every record" if keep_all else " under a hand-made res[]", ", FASTA out" if out_fasta else "")
    res, out_start = _res_and_offsets(torch, b, fwd, keep_all, out_fasta)
    total = int(out_start[-1])
    kept = int(((res >> 16) & 1).sum())
    rows_qual = None if b.fasta else packed_rows(eng, c)[1]
    out = abi_format(eng, c, res, fwd_start=fwd, rows_qual=rows_qual, out_fasta=out_fasta)
    torch.cuda.synchronize()
    assert out.numel() == total, "%s: out_bytes %d, expected %d" % (name, out.numel(), total)
    fastq_out = not b.fasta and not out_fasta
    if keep_all and fastq_out:
        assert kept == b.n and total > 1 << _hi() and total > b.text_len, "%s: %d bytes out of %d" % (name, total, b.text_len)
    nl = _newlines(torch, out)
    assert nl == (4 if fastq_out else 2) * kept, "%s: %d newlines in the output, %d records kept" % (name, nl, kept)
    res_host = lambda r0, r1: (res[r0:r1].to(torch.int64) & 0xFFFFFFFF).cpu().numpy()
    seen = _format_windows(eng, name, c, out, out_start, lambda wtext, r0, r1: b"".join(lt.format_plain(wtext, b.lpr, res_host(r0, r1), fwd, out_fasta)))
    assert {"prefix", "suffix", "random", "input 2^%d" % _lo()} <= seen, (name, seen)
    assert ("output 2^%d" % _hi() in seen) == (total > 1 << _hi()) and ("output 2^%d" % _lo() in seen) == (total > 1 << _lo()), (name, seen, total)
    print("large_offsets text %s: %d of %d records, %d bytes (%.3f GiB), windows %s" % (name, kept, b.n, total, total / 2**30, sorted(seen)))


def run_format_revcomp(eng, shape="fastq_lf"):
    """the packed arrays of a real engine.run(stages=8) formatted with reverse=True: windows against the plain reverse complement"""
    from fastx_toolkit_amd import make_params
    torch = eng.torch
    c = block(eng, shape)
    b = c["b"]
    name = "%s reverse complement through the packed arrays" % shape
    bases, qual = packed_rows(eng, c)
    r = eng.run(bases, qual, make_params(stages=8), lens=c["lens"][:b.n], fixed_len=c["info"].max_len, compact=True, meta=True)
    out = abi_format(eng, c, r.res, packed=(r.out_bases, r.out_qual, r.out_off), reverse=True, rows_qual=qual)
    torch.cuda.synchronize()
    assert int(r.counters[1]) == b.n, "%s: %d of %d reads kept" % (name, int(r.counters[1]), b.n)
    _, out_start = _res_and_offsets(torch, b, 0, True, False)                  # every record whole: the same sizes
    total = int(out_start[-1])
    assert out.numel() == total and total > 1 << _hi(), "%s: out_bytes %d, expected %d" % (name, out.numel(), total)
    assert _newlines(torch, out) == 4 * b.n
    seen = _format_windows(eng, name, c, out, out_start, lambda wtext, r0, r1: b"".join(lt.revcomp_plain(wtext)))
    assert {"prefix", "suffix", "random", "input 2^%d" % _lo(), "output 2^%d" % _lo(), "output 2^%d" % _hi()} <= seen, (name, seen)
    print("large_offsets text %s: %d bytes (%.3f GiB), windows %s" % (name, total, total / 2**30, sorted(seen)))


MODE_OPTS = {            # id_mode, id_both, ordinal_base, qual_mode (include/fxg.h)
    "numeric-ordinal": (1, 1, 10 ** 19 - 2, 2),
    "ascii-sequence": (2, 1, 0, 1),
}


def run_format_modes(eng, shape, mode):
    """fxg_fastq_format_opts on the whole block, every record kept through d_len (res null), with the output modes on: the character quality lines
    go out as numbers under 20-digit ordinal ids on both name lines (7.8 GiB), or every line as characters under sequence ids on both
    (more than 2^32 bytes too).  d_out holds exactly the closed-form total; out_bytes, the newline and blank counts of the whole output, and windows
    by output position -- prefix, suffix, 2^31, 2^32, 2^33 where the output reaches it, eight seeded -- against the suite's model of the modes
    (format_opts_cases.expected) on the generator's records."""
    import format_opts_cases as F
    from fastx_toolkit_amd.engine import FxgFormatOpts
    torch = eng.torch
    c = block(eng, shape)
    b = c["b"]
    id_mode, both, base, qual_mode = MODE_OPTS[mode]
    name = "%s format, %s" % (shape, mode)
    sz = torch.zeros(b.n + 1, dtype=torch.int64, device=b.device)
    blanks = 0
    for s in range(0, b.n, REC_SLAB):
        e = min(b.n, s + REC_SLAB)
        rr = b.range(s, e)
        sz[s + 1:e + 1] = b.mode_sizes(rr, mode, base)
        f, (_, minus_one) = b.fields(rr), b.numeric_line(rr)
        blanks += int((f["L"] - 1).sum()) if mode == "numeric-ordinal" else int((minus_one * f["numeric"]).sum())
    out_start = torch.cumsum(sz, 0)
    del sz
    total = int(out_start[-1])
    assert total > 1 << _hi(), (name, total)
    rows_qual = packed_rows(eng, c)[1]
    ob, out = _canaried(torch, eng, total)
    nb = C.c_uint64()
    o = FxgFormatOpts(id_mode, both, base, qual_mode, total, c["lens"].data_ptr())
    eng._after_torch()
    eng._check(eng.lib.fxg_fastq_format_opts(eng.ctx, c["text"].data_ptr(), 4, c["ix"].line.data_ptr(), c["ix"].cap_lines, c["ix"].flags.data_ptr(), b.n, None, 0, 0, None, None, None,
                                             rows_qual.data_ptr(), rows_qual.shape[1], 33, 0, out.data_ptr(), C.byref(nb), C.byref(o)))
    eng._before_torch()
    torch.cuda.synchronize()
    assert nb.value == total, "%s: out_bytes %d, expected %d" % (name, nb.value, total)
    _guards_intact(ob, total, total, name)
    step = 1 << 30
    nl, sp = (sum(int((out[s:s + step] == ch).sum()) for s in range(0, total, step)) for ch in (10, 32))
    assert nl == 4 * b.n and sp == blanks, "%s: %d newlines and %d blanks in the output, expected %d and %d" % (name, nl, sp, 4 * b.n, blanks)
    extra = [("output 2^33", 1 << 33, out_start)] if total > 1 << 33 else []
    expect = lambda wtext, r0, r1: F.expected(wtext, 4, 33, id_mode=id_mode, id_both=bool(both), base=base + r0, qual_mode=qual_mode)
    seen = _format_windows(eng, name, c, out, out_start, expect, extra=extra)
    assert {"prefix", "suffix", "random", "input 2^%d" % _lo(), "output 2^%d" % _lo(), "output 2^%d" % _hi()} <= seen and ("output 2^33" in seen) == (total > 1 << 33), (name, seen)
    print("large_offsets text %s: %d bytes (%.3f GiB), windows %s" % (name, total, total / 2**30, sorted(seen)))


# ---- weights -----------------------------------------------------------------------------------------------------------------------------
def run_weights(eng, shape="fasta_short"):
    torch = eng.torch
    c = block(eng, shape)
    b = c["b"]
    res = torch.empty(b.n, dtype=torch.int32, device=b.device)
    want = [0] * 7
    for s in range(0, b.n, REC_SLAB * 4):
        e = min(b.n, s + REC_SLAB * 4)
        rr = b.range(s, e)
        r = b.res_of(rr, 3)
        res[s:e] = r.to(torch.int32)
        want = [x + y for x, y in zip(want, b.weights(rr, r))]
    got = eng.fasta_weights(c["text"], c["ix"], b.n, res)
    assert got[:7] == want and all(x > b.n for x in want[:2]), "%s weights %r, int64 sums %r" % (shape, got[:7], want)


# ---- split -------------------------------------------------------------------------------------------------------------------------------
def _expected_bins(torch, b, ents, mm, bins, eol):
    exp = torch.empty(b.n, dtype=torch.int64, device=b.device)
    for s in range(0, b.n, REC_SLAB):
        e = min(b.n, s + REC_SLAB)
        win, F = b.bc_window(b.range(s, e), eol)
        exp[s:e] = lt.classify_torch(torch, win, F, ents, mm, bins - 1)
    return exp


def run_split(eng, shape, bins, eol, partial=1, mm=1):
    torch = eng.torch
    c = block(eng, shape)
    b, text, ix = c["b"], c["text"], c["ix"]
    n, lpr = b.n, b.lpr
    name = "%s split, %d bins, %s" % (shape, bins, "--eol" if eol else "--bol")
    ents = lt.table(bins, partial, eol)
    tiles = (n + 255) // 256
    cells = bins * tiles
    if bins == 4096:
        assert cells > 1 << 30, "%s: bins * tiles = %d does not reach the scan's fourth level" % (name, cells)
    total = ix.record_bytes(n)
    assert total == lt.CAP
    words = cells + cells // 512 + 64 + 2 * bins                     # fxg_barcode_split's workspace (u64 words), which it allocates with a quarter on top
    need = int(words * 8 * 1.25) + 4096 * 8 + total + 2 * 64 + 2 * n + (3 << 30)
    free = torch.cuda.mem_get_info()[0]
    assert need < free, "%s needs %.1f GB of device memory (workspace %.1f GB), %.1f GB are free" % (name, need / 1e9, words * 8 * 1.25 / 1e9, free / 1e9)
    eng.barcode_prepare(ents, lt.BL, bins, mismatches=mm, eol=eol)
    guard = 64
    buf = torch.full((guard + total + guard,), CANARY, dtype=torch.uint8, device=eng.device)
    out = buf[guard:guard + total]
    rbuf = torch.full((n + 64,), -0x5A5B, dtype=torch.int16, device=eng.device)
    bb, br = (C.c_uint64 * (bins + 8))(*([0xC0FFEE] * (bins + 8))), (C.c_uint64 * (bins + 8))(*([0xC0FFEE] * (bins + 8)))
    eng._after_torch()
    eng._check(eng.lib.fxg_barcode_split(eng.ctx, text.data_ptr(), b.text_len, lpr, ix.line.data_ptr(), ix.cap_lines, n, rbuf.data_ptr(), out.data_ptr(), bb, br))
    torch.cuda.synchronize()
    assert bool((buf[:guard] == CANARY).all()) and bool((buf[guard + total:] == CANARY).all()), name + ": write outside d_out"
    assert bool((rbuf[n:] == -0x5A5B).all()), name + ": write outside d_rec_bin"
    assert list(bb)[bins:] == [0xC0FFEE] * 8 and list(br)[bins:] == [0xC0FFEE] * 8, name + ": write outside the totals"
    exp = _expected_bins(torch, b, ents, mm, bins, eol)
    _same(torch, name + ": rec_bin", rbuf[:n].to(torch.int64) & 0xFFFF, exp)
    sizes = b.rec_start[1:] - b.rec_start[:-1]
    want_rec = torch.bincount(exp, minlength=bins)
    order = torch.sort(exp, stable=True).indices
    ssz = sizes[order]
    ostart = torch.cat([torch.zeros(1, dtype=torch.int64, device=b.device), torch.cumsum(ssz, 0)])       # output offset of the k-th record of the output
    bin_first = torch.cat([torch.zeros(1, dtype=torch.int64, device=b.device), torch.cumsum(want_rec, 0)])  # first output record of every bin
    want_bytes = ostart[bin_first[1:]] - ostart[bin_first[:-1]]
    assert np.array_equal(np.array(list(br)[:bins], dtype=np.int64), want_rec.cpu().numpy()), name + ": bin_records"
    assert np.array_equal(np.array(list(bb)[:bins], dtype=np.int64), want_bytes.cpu().numpy()), name + ": bin_bytes"
    used = int((want_rec > 0).sum())
    assert int(want_rec[:bins - 1].sum()) > n // 2 and used >= (97 if bins == 97 else 4000), "%s: %d records matched, %d bins in use" % (name, int(want_rec[:bins - 1].sum()), used)
    # the whole output: record k of the output is input record order[k], gathered from the text on the device
    k0 = 0
    while k0 < n:
        k1 = min(n, k0 + max(1, int(n * (1 << 27) / total)))
        src = b.rec_start[order[k0:k1]]
        sz = ssz[k0:k1]
        rec = torch.repeat_interleave(torch.arange(k1 - k0, dtype=torch.int64, device=b.device), sz)
        o0, o1 = int(ostart[k0]), int(ostart[k1])
        idx = src[rec] + (torch.arange(o1 - o0, dtype=torch.int64, device=b.device) - (ostart[k0:k1] - o0)[rec])
        _same(torch, name + ": d_out (against the records gathered in bin order)", out[o0:o1], text[idx], o0)
        del rec, idx
        k0 = k1
    # windows of the output through the generator on the host: prefix, suffix, the crossed marks, the first and last bin boundary, random ones
    nonempty = torch.nonzero(want_rec > 0).flatten()
    edges = [("first bin boundary", int(ostart[bin_first[int(nonempty[0]) + 1]]), ostart), ("last bin boundary", int(ostart[bin_first[int(nonempty[-1])]]), ostart)]
    seen = set()
    for label, q0 in lt.windows(torch, n, ostart, {}, lt.SEED, extra=edges):
        q1 = q0 + lt.KI
        o0, o1 = int(ostart[q0]), int(ostart[q1])
        w = "%s, window %s (output records %d..%d, bytes %d..%d)" % (name, label, q0, q1, o0, o1)
        if label == "input 2^%d" % _lo():
            assert o0 < 1 << _lo() < o1, w + " does not hold its mark"
        _bytes_same(w, out[o0:o1].cpu().numpy(), b.text_of(order[q0:q1]).cpu().numpy(), o0)
        seen.add(label)
    assert seen == {"prefix", "suffix", "random", "input 2^%d" % _lo(), "first bin boundary", "last bin boundary"}, (name, seen)
    print("large_offsets text %s: %d entries, %d x %d cells, %d records matched in %d bins, windows %s" % (name, len(ents), bins, tiles, int(want_rec[:bins - 1].sum()), used - 1, sorted(seen)))


# ---- rejection ---------------------------------------------------------------------------------------------------------------------------
def run_rejection(eng, shape="fasta_short"):
    """text_len = 0xFFFFFFF1: index and split answer FXG_E_INVALID and touch none of their outputs"""
    from fastx_toolkit_amd.engine import FxgTextInfo
    torch = eng.torch
    c = block(eng, shape)
    b = c["b"]
    too_long = lt.CAP + 1
    cap_lines = 2 * 1000 + 1
    line = torch.full((2 * cap_lines,), 0x5A5A5A5A, dtype=torch.int32, device=eng.device)
    lens = torch.full((1000,), 0x5A5A, dtype=torch.int16, device=eng.device)
    flags = torch.full((1000,), CANARY, dtype=torch.uint8, device=eng.device)
    info = FxgTextInfo()
    eng._after_torch()
    rc = eng.lib.fxg_fastq_index(eng.ctx, c["text"].data_ptr(), too_long, 1, b.lpr, line.data_ptr(), cap_lines, lens.data_ptr(), flags.data_ptr(), C.byref(info))
    assert rc == E_INVALID and (info.lines, info.records, info.consumed) == (0, 0, 0), "index of %#x bytes: rc %d" % (too_long, rc)
    eng.barcode_prepare(lt.table(97, 0, False), lt.BL, 97, mismatches=1, eol=False)
    out = torch.full((4096,), CANARY, dtype=torch.uint8, device=eng.device)
    rb = torch.full((1000,), -0x5A5B, dtype=torch.int16, device=eng.device)
    bb, br = (C.c_uint64 * 97)(), (C.c_uint64 * 97)()
    rc = eng.lib.fxg_barcode_split(eng.ctx, c["text"].data_ptr(), too_long, b.lpr, c["ix"].line.data_ptr(), c["ix"].cap_lines, 1000, rb.data_ptr(), out.data_ptr(), bb, br)
    assert rc == E_INVALID and sum(bb) == 0 and sum(br) == 0, "split of %#x bytes: rc %d" % (too_long, rc)
    torch.cuda.synchronize()
    assert bool((line == 0x5A5A5A5A).all()) and bool((lens == 0x5A5A).all()) and bool((flags == CANARY).all()), "the refused index wrote to its outputs"
    assert bool((out == CANARY).all()) and bool((rb == -0x5A5B).all()), "the refused split wrote to its outputs"
    # the cap itself is accepted (the blocks of this file), one byte more is not
    assert lt.CAP == 0xFFFFFFF0 and c["info"].records == b.n


STEPS = {
    "index": run_index,
    "pack": run_pack,
    "format-handmade": lambda e, s: run_format_handmade(e, s, False),
    "format-every-record": lambda e, s: run_format_handmade(e, s, True),
    "format-revcomp": run_format_revcomp,
    "format-fasta-out": lambda e, s: run_format_handmade(e, s, False, out_fasta=True),
    "format-numeric-ordinal": lambda e, s: run_format_modes(e, s, "numeric-ordinal"),
    "format-ascii-sequence": lambda e, s: run_format_modes(e, s, "ascii-sequence"),
    "weights": run_weights,
    "split-97-bol": lambda e, s: run_split(e, s, 97, False),
    "split-97-eol": lambda e, s: run_split(e, s, 97, True),
    "split-4096-bol": lambda e, s: run_split(e, s, 4096, False, partial=0),
    "rejection": run_rejection,
}
# in block order: a shape's text is generated and indexed once
CASES = [("fastq_lf", "index"), ("fastq_lf", "pack"), ("fastq_lf", "format-handmade"), ("fastq_lf", "format-every-record"), ("fastq_lf", "format-revcomp"),
         ("fastq_lf", "split-97-bol"), ("fastq_lf", "split-97-eol"),
         ("fastq_mixed", "index"), ("fastq_mixed", "pack"), ("fastq_mixed", "format-numeric-ordinal"), ("fastq_mixed", "format-ascii-sequence"),
         ("fasta_short", "index"), ("fasta_short", "pack"), ("fasta_short", "format-fasta-out"), ("fasta_short", "weights"),
         ("fasta_short", "split-97-bol"), ("fasta_short", "split-97-eol"), ("fasta_short", "split-4096-bol"), ("fasta_short", "rejection")]


@pytest.mark.parametrize("shape,step", CASES, ids=["%s-%s" % c for c in CASES])
def test_large_offsets_text(engine, shape, step):
    torch = engine.torch
    torch.cuda.reset_peak_memory_stats()                     # the peak asserted below is this case's own (the cached block included)
    t0, before = time.time(), engine.scan_recoveries()
    try:
        STEPS[step](engine, shape)
        _finish(engine, "%s %s" % (shape, step), t0, before)
    finally:
        torch.cuda.empty_cache()


def test_large_offsets_text_release():
    """(drops the last block: 4 GiB of text and its index)"""
    _CACHE.clear()
    import torch
    torch.cuda.empty_cache()


# ---- the tools on an input of more than 4 GiB with the largest read buffer ---------------------------------------------------------------------
CLI_BYTES = int(4.5 * 2**30)


def _hash_file(path, count_lines=False):
    h, lines = hashlib.md5(), 0
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
            lines += chunk.count(b"\n") if count_lines else 0
    return h.hexdigest(), lines


def test_large_offsets_cli_read_buffer_above_the_block_limit(engine, tmp_path_factory):
    """FXH_READ_BUFFER_MB=8192 on 4.5 GiB of fastq_lf: the knob is clamped to 4 095 MB (below the C-ABI's block limit), so fastx_trimmer and
    fastx_barcode_splitter work in blocks of nearly 4 GiB and write byte for byte what they write in their default blocks; the record totals are
    the generator's."""
    torch = engine.torch
    _CACHE.clear()
    torch.cuda.empty_cache()
    shm = "/dev/shm"
    need = int(CLI_BYTES * 3.2)                               # the input, the splitter's files of one run, the trimmer's
    free = shutil.disk_usage(shm).free if os.path.isdir(shm) else 0
    if free < need:
        pytest.skip("tmpfs %s has %d bytes free, the input of %d bytes and its outputs need %d" % (shm, free, CLI_BYTES, need))
    subprocess.check_call(["make", "-s", "-C", HOST])
    tools = os.path.join(HOST, "bin")
    d = tmp_path_factory.mktemp("cli")
    work = os.path.join(shm, "fxg_large_text_%d" % os.getpid())
    os.makedirs(work)
    try:
        probe = lt.Block(torch, "fastq_lf", 200_000, device=engine.device, pad=0)
        n = int(CLI_BYTES / (probe.text_len / probe.n)) + 1
        b = lt.Block(torch, "fastq_lf", n, device=engine.device, pad=0)
        assert b.text_len > (1 << 32) + (1 << 28)
        inp = os.path.join(work, "in.fq")
        long3 = 0
        with open(inp, "wb") as f:
            for r0, r1 in b.slabs(1 << 27):
                rr = b.range(r0, r1)
                f.write(b.text_of(rr).cpu().numpy().tobytes())
                long3 += int((b.fields(rr)["L"] >= 3).sum())
        assert os.path.getsize(inp) == b.text_len
        del b
        torch.cuda.empty_cache()
        bc = os.path.join(str(d), "bc.txt")
        with open(bc, "w") as f:
            f.write("".join("id%d %s\n" % (j, x.decode()) for x, j in lt.table(97, 0, False)))
        results = {}
        for mode, env in (("default blocks", {}), ("FXH_READ_BUFFER_MB=8192", {"FXH_READ_BUFFER_MB": "8192", "FXH_LANES": "1"})):
            e = dict(os.environ, **env)
            t0 = time.time()
            out = os.path.join(work, "trim.fq")
            p = subprocess.run([os.path.join(tools, "fastx_trimmer"), "-f", "3", "-l", "40", "-i", inp, "-o", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=300)
            assert p.returncode == 0, (mode, p.stderr[-2000:])
            digest, lines = _hash_file(out, count_lines=True)
            os.unlink(out)
            assert lines == 4 * long3, "%s: fastx_trimmer wrote %d lines, %d records have three bases or more" % (mode, lines, long3)
            pre = os.path.join(work, "split_")
            with open(inp, "rb") as f:
                p = subprocess.run([os.path.join(tools, "fastx_barcode_splitter"), "--bcfile", bc, "--prefix", pre, "--suffix", ".fq", "--bol", "--mismatches", "1"],
                                   stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=300)
            assert p.returncode == 0, (mode, p.stderr[-2000:])
            files = sorted(x for x in os.listdir(work) if x.startswith("split_"))
            assert len(files) == 97
            hashes, nlines = {}, 0
            for x in files:
                hashes[x], k = _hash_file(os.path.join(work, x), count_lines=True)
                nlines += k
                os.unlink(os.path.join(work, x))
            table = p.stdout.decode().splitlines()
            assert table[-1] == "total\t%d" % n and nlines == 4 * n, "%s: fastx_barcode_splitter counted %r, wrote %d lines; the input has %d records" % (mode, table[-1], nlines, n)
            results[mode] = (digest, hashes, table)
            print("large_offsets text cli, %s: trimmer %s, splitter %d files, %.1f s" % (mode, digest, len(files), time.time() - t0))
        a, z = results["default blocks"], results["FXH_READ_BUFFER_MB=8192"]
        assert a[0] == z[0], "fastx_trimmer: the output differs between default blocks and FXH_READ_BUFFER_MB=8192"
        assert a[1] == z[1], "fastx_barcode_splitter: files differ: %r" % sorted(k for k in a[1] if a[1][k] != z[1].get(k))
        assert a[2] == z[2]
    finally:
        shutil.rmtree(work, ignore_errors=True)


# ---- ordinal ids over more than 2^24 kept records: the rebuilt rank in the id, in the digit offset and in the total ---------------------------
ORD_CASES = [(2, "hashed", 0), (2, "hashed", 1), (2, "hashed", 2), (2, "all", 0), (2, "all", 1), (2, "all", 2), (4, "hashed", 1), (4, "hashed", 2)]
ORD_SLAB = 1 << 20                       # kept records per slab of the whole-output comparison


@pytest.mark.parametrize("lpr,keep,base", ORD_CASES, ids=["%s-%s-base%d" % ("fasta" if c[0] == 2 else "fastq-both", c[1], c[2]) for c in ORD_CASES])
def test_large_offsets_text_ordinal_ranks(engine, lpr, keep, base):
    """fxg_fastq_format_opts with ordinal ids on lt.ORD_N = 2^24 + 2^23 + 5 four-byte records (eight as FASTQ, the id on both name lines): fifteen
    in sixteen kept by a hash, or all of them, so the kept count passes 2^24 between two of fxg_text_rank's 2^23 steps; bases 0, 10^8 - 2^24 (nine
    digits from the rank 2^24 - 1 on) and 10^19 - 2 (twenty digits).  The whole output against the closed form in slabs, out_bytes, and the
    exact-capacity pair: total - 1 refused with both numbers in the message and nothing written, total accepted.  The scan runs three levels."""
    from fastx_toolkit_amd.engine import FxgFormatOpts
    torch = engine.torch
    _CACHE.clear()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0, before, n, both, base = time.time(), engine.scan_recoveries(), lt.ORD_N, lpr == 4, lt.ORD_BASES[base]
    rec = torch.frombuffer(bytearray(lt.ORD_RECORD[lpr]), dtype=torch.uint8).to(engine.device)
    text_len = len(lt.ORD_RECORD[lpr]) * n
    text = torch.full((text_len + 16,), POISON, dtype=torch.uint8, device=engine.device)
    text[:text_len] = rec.repeat(n)
    ix, lens, info = engine.fastq_index(text, text_len, cap_records=n + 2, fasta=not both)
    assert info.records == n and info.irregular == 0 and info.consumed == text_len and info.max_len == 1, (info.records, info.irregular, info.consumed)
    rows = torch.full((n,), ord("I"), dtype=torch.uint8, device=engine.device)                       # the quality rows at stride 1
    kmask = lt.ord_keep(torch, torch.arange(n, dtype=torch.int64, device=engine.device)) if keep == "hashed" else torch.ones(n, dtype=torch.bool, device=engine.device)
    kept = int(kmask.sum())
    assert kept > (1 << 24) + (1 << 22) and (keep == "all") == (kept == n)
    res = torch.where(kmask, (1 << 16) | 1, 0).to(torch.int32)
    total = lt.ord_offset(base, kept, both)
    ob, out = _canaried(torch, engine, total)
    nb = C.c_uint64(7)

    def call(cap):
        o = FxgFormatOpts(1, int(both), base, 0, cap, None)
        engine._after_torch()
        rc = engine.lib.fxg_fastq_format_opts(engine.ctx, text.data_ptr(), lpr, ix.line.data_ptr(), ix.cap_lines, ix.flags.data_ptr(), n, res.data_ptr(), 0, 0, None, None, None,
                                              rows.data_ptr(), 1, 33, 0, out.data_ptr(), C.byref(nb), C.byref(o))
        engine._before_torch()
        torch.cuda.synchronize()
        return rc
    what = "ordinal ranks %d lines, %s, base %d" % (lpr, keep, base)
    assert call(total - 1) == E_INVALID and nb.value == 0 and bool((ob == CANARY).all()), what + ": one byte short was not refused untouched"
    assert engine.lib.fxg_last_error(engine.ctx).decode() == "the formatted block needs %d bytes, d_out takes %d" % (total, total - 1), engine.lib.fxg_last_error(engine.ctx)
    assert call(total) == 0 and nb.value == total, (what, nb.value, total, engine.lib.fxg_last_error(engine.ctx))
    _guards_intact(ob, total, total, what)
    for k0 in range(0, kept, ORD_SLAB):
        k1 = min(kept, k0 + ORD_SLAB)
        a, b = lt.ord_offset(base, k0, both), lt.ord_offset(base, k1, both)
        _same(torch, "%s, kept ranks %d..%d" % (what, k0, k1), out[a:b], lt.ord_text(torch, base, k0, k1, both, device=engine.device), a)
    torch.cuda.synchronize()
    assert engine.scan_recoveries() == before and bool((text[text_len:] == POISON).all())
    peak = torch.cuda.max_memory_allocated()
    assert peak < MEMORY_LIMIT, "%s: peak of device memory %.1f GB" % (what, peak / 1e9)
    print("large_offsets text %s: %.1f s, peak %.1f GB" % (what, time.time() - t0, peak / 1e9))
    del text, out, ob, res, rows, ix, lens
    torch.cuda.empty_cache()
