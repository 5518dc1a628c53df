"""CPU tier of the device text path and the barcode splitter on blocks of up to 0xFFFFFFF0 bytes.

1. tests/large_text.py (the reference code of tests/test_gpu_large_offsets_text.py) against trusted code on blocks of a few thousand records:
   the oracle's parser and formatter, tests/bcsplit_model.py, plain Python restatements, the reference driver where it is built; the block-size
   literals against the size rule.
2. The per-thread bodies of csrc/fxg_text.h and csrc/fxg_barcode.h at high offsets, without a GPU: a sparse anonymous mapping of CAP + 16 bytes
   holds three clusters of a block's own records at their own offsets -- from 0, around 2^31, up to the cap -- and the emulator's entry points
   run on it: the index over the whole mapping, pack / format / weights / split on line arrays that name the cluster records.  Every result is
   held against the closed forms and against the same records laid at offset 0, where nothing but the offsets may differ.
3. Engine.barcode_split's output size on an index whose offsets pass 2^31 (no device needed).
"""
import ctypes as C
import errno
import mmap
import os
import subprocess

import numpy as np
import pytest

import bcsplit_model as M
import emu_py
import large_offsets as lo
import large_text as lt
from helpers import text_through
from oracle import fxoracle_py as fo
from test_barcode_cpu import EMU_DIR, BarcodeSet, _obj

torch = pytest.importorskip("torch")
K = 1500                                 # records per cluster
NUL, SEQLEN = 0x80, 0x04                 # FXG_TEXT_IRR_NUL, FXG_TEXT_IRR_SEQLEN (include/fxg.h)


def _small(shape, n=3000, pad=37):
    b = lt.Block(torch, shape, n, pad=pad)
    rr = b.range(0, n)
    return b, rr, bytes(b.text_of(rr).numpy())


# ---- 1. the generator and its closed forms against trusted code ------------------------------------------------------------------------
def test_hash_lengths_and_codes():
    for r0 in (0, (1 << 31) - 700, (1 << 32) - 700):
        rr = torch.arange(r0, r0 + 1500, dtype=torch.int64)
        for stride, min1 in ((lt.STRIDE, True), (lt.FA_SPAN, False)):
            a = lo.lens_numpy(r0, 1500, stride, dict(stages=4) if min1 else None)
            assert np.array_equal(lt.lens_of(torch, rr, stride, min1).numpy(), a.astype(np.int64))
    v = torch.tensor([0, 9, 10, 99, 100, 12345678, 10**18 - 1, 10**18], dtype=torch.int64)
    assert lt.ndigits(torch, v).tolist() == [1, 1, 2, 2, 3, 8, 18, 19]
    codes = lt.codes_numpy()
    assert codes.shape == (lt.NCODES, lt.BL) and len({bytes(c) for c in codes}) == lt.NCODES and set(codes.reshape(-1).tolist()) == {65, 67, 71, 84}
    t = lt.table(97, 1, False)
    assert len(t) == 192 and t[0][0][1:] == t[1][0] and t[1][1] == 0 and lt.table(97, 1, True)[1][0] == t[0][0][:-1]


@pytest.mark.parametrize("shape", lt.SHAPES)
def test_text_is_what_the_shape_says(shape):
    """a plain Python reading of the generated text: prefixes, alphabets, the third line's three forms, CRLF and numeric shares, the padding"""
    b, rr, text = _small(shape, 6000)
    assert len(text) == b.text_len == int(b.rec_start[-1]) and text.endswith(b"\n")
    raw = text.split(b"\n")[:-1]
    assert len(raw) == b.lpr * b.n
    f = {k: v.numpy() for k, v in b.fields(rr).items()}
    crlf = numeric = empty3 = 0
    for r in range(b.n):
        ls = raw[b.lpr * r:b.lpr * (r + 1)]
        cr = [l.endswith(b"\r") for l in ls]
        assert all(cr) or not any(cr)
        crlf += cr[0]
        ls = [l.rstrip(b"\r") for l in ls]
        assert not any(b"\r" in l for l in ls)
        tail = b"x" * (37 if r == b.n - 1 else 0)
        if b.fasta:
            name = b">%d" % r + (b"-%d" % f["count"][r] if f["hasc"][r] else b"") + tail
            assert ls[0] == name and (20 <= len(ls[1]) <= 60 or r == b.n - 1) and set(ls[1]) <= set(b"ACGTN")
        else:
            assert ls[0] == b"@s%d" % r + tail and 1 <= len(ls[1]) <= 150 and set(ls[1]) <= set(b"ACGTN")
            assert ls[2] in (b"", b"+", b"+s%d" % r)
            empty3 += ls[2] == b""
            if len(ls[3]) == len(ls[1]):
                assert min(ls[3]) >= 33 and max(ls[3]) <= 126
            else:
                numeric += 1
                vals = [int(x) for x in ls[3].split()]
                assert len(vals) == len(ls[1]) and min(vals) >= -15 and max(vals) <= 93 and f["numeric"][r] == 1
    if b.fasta:
        assert 1 <= len(raw[-1]) <= lt.FA_LAST and f["hasc"].sum() > b.n // 3 and (f["hasc"] == 0).sum() > b.n // 3
    else:
        assert b.n // 12 < empty3 < b.n // 5
        assert (crlf > b.n // 32 and numeric > b.n // 150) if shape == "fastq_mixed" else (crlf == 0 and numeric == 0)
    if shape == "fastq_mixed":
        assert all(l.endswith(b"\r") for l in raw[-4:])          # the last record is chomped at the very end of the block
        allq = b"".join(raw[3::4])
        assert b"  " in allq and b"-" in allq and b"+" in allq and b"-15" in allq and b"93" in allq
    # any range on its own
    for a, e in ((0, 1), (17, 523), (b.n - 3, b.n)):
        assert bytes(b.text_of(b.range(a, e)).numpy()) == text[int(b.rec_start[a]):int(b.rec_start[e])]
    pick = torch.tensor([5, 4000, 77, b.n - 1], dtype=torch.int64)
    assert bytes(b.text_of(pick).numpy()) == b"".join(text[int(b.rec_start[r]):int(b.rec_start[r + 1])] for r in pick.tolist())


def _plain_parse(text, stride):
    """rows and lengths of FASTQ text by plain Python (CRLF, numeric quality lines)"""
    lines = lt.split_lines(text)
    n = len(lines) // 4
    bases, qual = np.zeros((n, stride), np.uint8), np.zeros((n, stride), np.uint8)
    lens, flags = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for r in range(n):
        s, q = lines[4 * r + 1], lines[4 * r + 3]
        lens[r] = len(s)
        bases[r, :len(s)] = np.frombuffer(s, np.uint8)
        if len(q) != len(s):
            flags[r] = 1
            q = bytes(v + 33 for v in lt._numeric_values(q))
        qual[r, :len(s)] = np.frombuffer(q, np.uint8)
    return bases, qual, lens, flags


@pytest.mark.parametrize("shape", lt.SHAPES)
def test_line_index_and_rows_equal_trusted_parsers(shape):
    b, rr, text = _small(shape)
    a = np.frombuffer(text, np.uint8)
    nl = np.flatnonzero(a == 10)
    starts, ends = b.line_index(rr)
    assert np.array_equal(starts.reshape(-1).numpy(), np.concatenate([[0], nl[:-1] + 1]))
    assert np.array_equal(ends.reshape(-1).numpy(), np.where(a[nl - 1] == 13, nl - 1, nl))
    f = b.fields(rr)
    for stride in ((150, 157) if not b.fasta else (60, 64)):
        eb, eq = b.rows_of(rr, stride)
        if shape == "fastq_lf":
            p = fo.parse_fastq(text, stride=stride)
            assert p["n"] == b.n and np.array_equal(p["lens"][:b.n], f["L"].numpy().astype(np.uint16))
            assert np.array_equal(p["bases"][:b.n], eb.numpy()) and np.array_equal(p["qual"][:b.n], eq.numpy())
        if not b.fasta:
            pb, pq, pl, pf = _plain_parse(text, stride)
            assert np.array_equal(pb, eb.numpy()) and np.array_equal(pq, eq.numpy())
            assert np.array_equal(pl, f["L"].numpy()) and np.array_equal(pf, f["numeric"].numpy())
        else:
            seqs = lt.split_lines(text)[1::2]
            assert eq is None and all(bytes(eb[r, :len(s)].numpy()) == s and not eb[r, len(s):].any() for r, s in enumerate(seqs))


@pytest.mark.parametrize("keep_all", [False, True])
def test_formatter_equals_the_oracle_formatter(keep_all):
    """format_plain, format_sizes and res_of on fastq_lf against helpers.text_through (the oracle's parser and writer) around a stage that keeps
    what res[] says; FASTA output of the same, and fasta_short, against the plain statement"""
    b, rr, text = _small("fastq_lf")
    fwd = 3
    res = b.res_of(rr, fwd, keep_all).numpy()
    keep, ln = ((res >> 16) & 1).astype(bool), res & 0xFFFF
    L = b.fields(rr)["L"].numpy()
    assert (ln[keep] >= 1).all() and (ln[keep] + fwd <= L[keep]).all() and (keep.all() or keep.sum() > b.n // 2) and (res >> 32 == 0).all()
    assert not keep_all or (keep == (L > fwd)).all()

    def run(bases, qual, lens, params):
        idx = np.flatnonzero(keep)
        return dict(out_bases=np.concatenate([bases[r, fwd:fwd + ln[r]] for r in idx]), out_qual=np.concatenate([qual[r, fwd:fwd + ln[r]] for r in idx]),
                    out_len=ln[idx].astype(np.uint16), kept_index=idx.astype(np.uint32))
    want, _ = text_through(run, text, None)
    got = lt.format_plain(text, 4, res, fwd)
    assert b"".join(got) == want
    assert np.array_equal(b.format_sizes(rr, torch.from_numpy(res)).numpy(), np.array([len(x) for x in got]))
    fa = lt.format_plain(text, 4, res, fwd, out_fasta=True)
    assert np.array_equal(b.format_sizes(rr, torch.from_numpy(res), out_fasta=True).numpy(), np.array([len(x) for x in fa]))
    assert b"".join(fa) == b"".join(b">" + x.split(b"\n")[0][1:] + b"\n" + x.split(b"\n")[1] + b"\n" for x in got if x)
    b2, rr2, text2 = _small("fasta_short")
    res2 = b2.res_of(rr2, fwd, keep_all)
    fa2 = lt.format_plain(text2, 2, res2.numpy(), fwd)
    assert np.array_equal(b2.format_sizes(rr2, res2).numpy(), np.array([len(x) for x in fa2]))
    lines = text2.split(b"\n")
    for r in (0, 1, 2, 500, b2.n - 1):
        w = int(res2[r])
        assert fa2[r] == (lines[2 * r] + b"\n" + lines[2 * r + 1][fwd:fwd + (w & 0xFFFF)] + b"\n" if (w >> 16) & 1 else b"")
    # the whole block kept from its first base: empty third lines come back as "+", so the output outgrows the input
    b3 = lt.Block(torch, "fastq_lf", 3000, pad=0)
    rr3 = b3.range(0, 3000)
    grown = int(b3.format_sizes(rr3, b3.res_of(rr3, 0, True)).sum())
    assert grown == b3.text_len + int((b3.fields(rr3)["c2"] == 0).sum()) and grown > b3.text_len


REF = fo.ref_binary()


@pytest.mark.skipif(REF is None, reason="oracle/_ref/fxref not built")
@pytest.mark.parametrize("shape", lt.SHAPES)
def test_formatter_equals_the_reference_trimmer(shape):
    """fastx_trimmer -f 4 -l 43 of the real libfastx on the generated text (CRLF and numeric records included) == format_plain with the res[]
    that stage gives"""
    b, rr, text = _small(shape)
    L = b.fields(rr)["L"].numpy()
    res = np.where(L >= 4, (np.minimum(L, 43) - 3) | (1 << 16), 0)
    p = subprocess.run([REF, "fastx_trimmer", "-f", "4", "-l", "43"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout == b"".join(lt.format_plain(text, b.lpr, res, 3))


def test_weights_equal_a_plain_count():
    """the seven tallies against a plain reading of the identifiers (the number behind the first '-', 1 without one: fastx.c:475-495)"""
    b, rr, text = _small("fasta_short")
    res = b.res_of(rr, 3)
    got = b.weights(rr, res)
    want = [0] * 7
    for r, name in enumerate(text.split(b"\n")[0:-1:2]):
        cnt = int(name.split(b"-")[1].rstrip(b"x")) if b"-" in name else 1
        w = int(res[r])
        why = (w >> 17) & 15
        for k, on in enumerate((True, (w >> 16) & 1, why == 1, (w >> 22) & 1, why == 3, why == 4, why == 5)):
            want[k] += cnt if on else 0
    assert got == want and all(x > 0 for x in want) and want[0] > 50 * b.n
    if REF is not None:                  # the reference's own count of reads: fastx_artifacts_filter -v on the same identifiers
        rep = subprocess.run([REF, "fastx_artifacts_filter", "-v"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120).stderr.decode()
        assert "Input: %d reads." % want[0] in rep


@pytest.mark.parametrize("shape", lt.SHAPES)
@pytest.mark.parametrize("eol", [False, True])
def test_barcode_expectations_equal_the_model(shape, eol):
    b, rr, text = _small(shape, 4000)
    for bins, partial, mm in ((97, 1, 1), (4096, 0, 0), (97, 0, 2)):
        ents = lt.table(bins, partial, eol)
        rb, bb, br, out = M.split_block(text, b.lpr, [x for x, _ in ents], [j for _, j in ents], lt.BL, mm, eol, bins)
        win, F = b.bc_window(rr, eol)
        seqs = text.split(b"\n")[1::b.lpr]            # (up to the LF: a CRLF record's CR is the last byte of its bases line, as in the script)
        for r in (0, 1, 2, 3, 1000, b.n - 1):
            assert bytes(win[r, :int(F[r])].numpy()) == M.window(seqs[r], lt.BL, eol) and not win[r, int(F[r]):].any()
        got = lt.classify_torch(torch, win, F, ents, mm, bins - 1).numpy()
        assert np.array_equal(got, rb)
        tab = np.zeros((len(ents), lt.BL), np.uint8)
        for k, (x, _) in enumerate(ents):
            tab[k, :len(x)] = np.frombuffer(x, np.uint8)
        assert np.array_equal(M.classify(win.numpy(), F.numpy(), tab, [len(x) for x, _ in ents], np.array([j for _, j in ents]), lt.BL, mm, bins - 1), rb)
        # the output: the records in bin order, input order inside a bin
        order = np.argsort(rb, kind="stable")
        assert bytes(b.text_of(torch.from_numpy(order)).numpy()) == out
        matched = int((rb != bins - 1).sum())
        assert matched > (b.n // 2 if bins == 97 else b.n // 2), (bins, matched)
        if bins == 4096:
            assert len(set(rb.tolist())) > 300


def test_window_placement():
    b = lt.Block(torch, "fastq_lf", 40_000, pad=0)
    st = b.rec_start
    for byte in (0, 1, int(st[777]) - 1, int(st[777]), int(st[777]) + 1, b.text_len - 1):
        r = lt.record_at(torch, st, byte)
        assert int(st[r]) <= byte < int(st[r + 1])
    grown = st + torch.arange(b.n + 1)
    w = lt.windows(torch, b.n, st, dict(out=grown), 3, extra=[("bin edge", int(st[20_000]) + 5, st)])
    assert [x[0] for x in w].count("random") == lt.RANDOM_WINDOWS and w[0] == ("prefix", 0) and ("suffix", b.n - lt.KI) in w
    assert ("bin edge", 20_000 - lt.KI // 2) in w and [x[1] for x in w] == sorted(x[1] for x in w) and all(0 <= x[1] <= b.n - lt.KI for x in w)
    marks = lt.MARKS
    try:                                 # marks a small block does cross
        lt.MARKS = (20, 22, 40)
        assert lt.crossed(b.text_len) == (20, 22)
        w = dict(lt.windows(torch, b.n, st, dict(out=grown), 3))
        for name, s in (("input", st), ("out", grown)):
            for m in (20, 22):
                r0 = w["%s 2^%d" % (name, m)]
                assert int(s[r0]) < 1 << m < int(s[r0 + lt.KI]) and abs(lt.record_at(torch, s, 1 << m) - r0 - lt.KI // 2) <= 1
    finally:
        lt.MARKS = marks


@pytest.fixture(scope="module", params=lt.SHAPES)
def big(request):
    """the block of the GPU tier, as record offsets only (int64 [N + 1] on the host)"""
    return lt.Block(torch, request.param, lt.BLOCKS[request.param])


def test_block_size_literals_follow_from_the_size_rule(big):
    assert lt.size_rule(torch, big.shape) == big.n == lt.BLOCKS[big.shape]
    assert big.text_len == lt.CAP == 0xFFFFFFF0 and 0 <= big.pad < 600 and lt.crossed(big.text_len) == (31,) and big.text_len > (1 << 32) - 17
    last = big.fields(big.range(big.n - 1, big.n))
    if big.fasta:
        assert big.n > 1 << 26 and 1 <= int(last["L"][0]) <= lt.FA_LAST
        assert int(big.line_index(big.range(big.n - 1, big.n))[0][0, 1]) > (1 << 32) - 70       # its barcode window starts in the last 70 bytes below 2^32
    else:
        # every record kept from its first base: the formatted output passes 2^32 (an empty third line comes back as "+")
        grown = 0
        for r0, r1 in big.slabs():
            grown += int((big.fields(big.range(r0, r1))["c2"] == 0).sum())
        assert big.text_len + grown > (1 << 32) + 1_000_000
        assert big.n > 1 << 20                                  # the format's scan runs three levels
    assert (big.text_len + 4095) // 4096 == 1 << 20            # the index's scan: exactly 2^20 segments


# ---- 2. the per-thread bodies at high offsets ----------------------------------------------------------------------------------------------
class Sparse:
    """CAP + 16 bytes, private and without reserve: only the pages written become resident"""

    def __init__(self):
        size = lt.CAP + 16
        try:
            self.map = mmap.mmap(-1, size, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, "MAP_NORESERVE", 0x4000))
        except (OSError, ValueError) as e:
            pytest.skip("no sparse mapping of %d bytes: errno %s (%s)" % (size, errno.errorcode.get(getattr(e, "errno", 0), getattr(e, "errno", None)), e))
        self.a = np.frombuffer(self.map, dtype=np.uint8)
        self.addr = self.a.ctypes.data
        assert self.addr % 16 == 0

    def close(self):
        self.a = None
        try:
            self.map.close()
        except BufferError:              # a view is still alive somewhere: the mapping goes with the process
            pass


def _clusters(b):
    mid = lt.record_at(torch, b.rec_start, 1 << 31)
    return [(0, K), (mid - K // 2, mid - K // 2 + K), (b.n - K, b.n)]


@pytest.fixture(scope="module")
def sparse(big):
    sp = Sparse()
    prefix = 62 if big.fasta else 64
    cl = _clusters(big)
    for k, (r0, r1) in enumerate(cl):
        a, e = int(big.rec_start[r0]), int(big.rec_start[r1])
        sp.a[a:e] = big.text_of(big.range(r0, r1)).numpy()
        if k + 1 < len(cl):
            sp.a[e] = prefix             # the zero filler up to the next cluster becomes the head of that cluster's first name line
    a1, e1 = int(big.rec_start[cl[1][0]]), int(big.rec_start[cl[1][1]])
    assert a1 < 1 << 31 < e1 and int(big.rec_start[cl[2][1]]) == lt.CAP
    yield sp, big, cl
    sp.close()


def _newlines(a, n, step=1 << 28):
    out = [np.flatnonzero(a[s:min(n, s + step)] == 10) + s for s in range(0, n, step)]
    return np.concatenate(out)


def test_sparse_index_over_the_whole_mapping(sparse):
    """fxg_emu_fastq_index over all CAP bytes: every line start and end against the newlines numpy finds, the per-record arrays and the block's
    scalars against the closed forms.  The zero filler between the clusters raises FXG_TEXT_IRR_NUL and makes the first name line of the second
    and of the third cluster over-long (FXG_TEXT_IRR_SEQLEN): exactly those two bits, first at record K."""
    sp, b, cl = sparse
    nl = _newlines(sp.a, lt.CAP)
    lines = len(nl)
    assert lines == 3 * K * b.lpr and int(nl[-1]) == lt.CAP - 1
    n = lines // b.lpr
    cap_records = n + 2
    cap_lines = b.lpr * cap_records + 1
    line = np.full(2 * cap_lines, 0xDEADBEEF, np.uint32)
    lens, flags = np.full(cap_records, 0xEEEE, np.uint16), np.full(cap_records, 0xEE, np.uint8)
    state, info = C.create_string_buffer(256), emu_py.TextInfo()
    rc = emu_py.lib().fxg_emu_fastq_index(state, C.c_void_p(sp.addr), C.c_uint64(lt.CAP), C.c_int(1), C.c_int(b.lpr), C.c_void_p(line.ctypes.data),
                                          C.c_uint64(cap_lines), C.c_void_p(lens.ctypes.data), C.c_void_p(flags.ctypes.data), C.byref(info), None, C.c_size_t(0))
    assert rc == 0
    rr = torch.cat([b.range(r0, r1) for r0, r1 in cl])
    f = {k: v.numpy() for k, v in b.fields(rr).items()}
    mixed = b.shape == "fastq_mixed"
    assert (info.lines, info.records, info.consumed, info.has_cr) == (lines, n, lt.CAP, int(mixed))
    assert info.irregular == NUL | SEQLEN and info.first_bad == K
    good = np.ones(n, bool)
    good[[K, 2 * K]] = False
    assert (info.max_len, info.min_len) == (int(f["L"][good].max()), int(f["L"][good].min()))
    assert info.numeric_records == int(f["numeric"][good].sum()) and (not mixed or info.numeric_records > 10)
    starts = np.concatenate([[0], nl + 1]).astype(np.uint32)
    assert np.array_equal(line[:lines + 1], starts), "line starts"
    ends = np.where(sp.a[nl - 1] == 13, nl - 1, nl).astype(np.uint32) if mixed else nl.astype(np.uint32)
    got_ends = line[cap_lines:cap_lines + lines]
    if not np.array_equal(got_ends, ends):
        i = int(np.flatnonzero(got_ends != ends)[0])
        raise AssertionError("line end %d: emulator %d, numpy %d" % (i, got_ends[i], ends[i]))
    assert (line[lines + 1:cap_lines] == 0xDEADBEEF).all() and (line[cap_lines + lines:] == 0xDEADBEEF).all()
    cs, ce = b.line_index(rr)
    cs, ce = cs.numpy().copy(), ce.numpy()
    for k in (1, 2):                     # the name lines that took the filler in start where the cluster before ended
        cs[k * K, 0] = int(b.rec_start[cl[k - 1][1]])
    assert np.array_equal(starts[:-1].astype(np.int64), cs.reshape(-1)) and np.array_equal(ends.astype(np.int64), ce.reshape(-1))
    assert int(starts[-1]) == lt.CAP > 1 << 31
    assert np.array_equal(lens[:n], f["L"].astype(np.uint16)) and (lens[n:] == 0xEEEE).all()
    assert np.array_equal(flags[:n], (f["numeric"] * good).astype(np.uint8)) and (flags[n:] == 0xEE).all()


def _line_arrays(b, rr, base=None):
    """(line uint32 [2 * cap_lines], cap_lines, flags): the hand-built index of the records rr at their own offsets, or laid one after the
    other from offset 0 (base=0)"""
    s, e = b.line_index(rr)
    if base is not None:
        sz = b.fields(rr)["size"]
        shift = (torch.cumsum(sz, 0) - sz) - b.rec_start[rr]
        s, e = s + shift[:, None], e + shift[:, None]
    k = rr.numel()
    cap_lines = b.lpr * k + 1
    line = np.zeros(2 * cap_lines, np.uint32)
    line[:b.lpr * k] = s.reshape(-1).numpy().astype(np.uint32)
    line[b.lpr * k] = int(e[-1, -1]) + int(b.fields(rr[-1:])["el"][0])
    line[cap_lines:cap_lines + b.lpr * k] = e.reshape(-1).numpy().astype(np.uint32)
    return line, cap_lines, b.fields(rr)["numeric"].numpy().astype(np.uint8)


def _emu_pack(text_addr, text_len, lpr, line, cap_lines, flags, n, stride):
    nb = (n * stride + 15) // 16 * 16
    bases, qual = emu_py._aligned(nb), (emu_py._aligned(nb) if lpr == 4 else None)
    irr = C.c_uint32()
    rc = emu_py.lib().fxg_emu_fastq_pack(C.c_void_p(text_addr), C.c_uint64(text_len), C.c_int(lpr), C.c_void_p(line.ctypes.data), C.c_uint64(cap_lines),
                                         C.c_void_p(flags.ctypes.data), C.c_uint64(n), C.c_uint32(stride), C.c_int(33), C.c_void_p(bases.ctypes.data),
                                         C.c_void_p(qual.ctypes.data if qual is not None else None), C.byref(irr), None, C.c_size_t(0))
    assert rc == 0
    return bases[:n * stride].reshape(n, stride), (qual[:n * stride].reshape(n, stride) if qual is not None else None), irr.value


def _emu_format(text_addr, lpr, line, cap_lines, flags, n, res, fwd, rows_qual, stride, out_fasta, cap_out):
    out = np.full(cap_out + 64, 0xA5, np.uint8)
    r = np.ascontiguousarray(res, dtype=np.uint32)
    nb = C.c_uint64()
    rc = emu_py.lib().fxg_emu_fastq_format(C.c_void_p(text_addr), C.c_int(lpr), C.c_void_p(line.ctypes.data), C.c_uint64(cap_lines), C.c_void_p(flags.ctypes.data),
                                           C.c_uint64(n), C.c_void_p(r.ctypes.data), C.c_uint32(fwd), C.c_int(0), None, None, None,
                                           C.c_void_p(rows_qual.ctypes.data if rows_qual is not None else None), C.c_uint32(stride), C.c_int(33),
                                           C.c_int(int(out_fasta)), C.c_void_p(out.ctypes.data), C.byref(nb), None, C.c_size_t(0))
    assert rc == 0 and nb.value <= cap_out and (out[nb.value:] == 0xA5).all()
    return out[:nb.value].tobytes()


def test_sparse_pack_format_weights_on_cluster_records(sparse):
    sp, b, cl = sparse
    rr = torch.cat([b.range(r0, r1) for r0, r1 in cl])
    n = rr.numel()
    flat = np.ascontiguousarray(np.concatenate([b.text_of(rr).numpy(), np.full(16, 0x5A, np.uint8)]))
    hi, lo0 = _line_arrays(b, rr), _line_arrays(b, rr, base=0)
    assert int(hi[0][:b.lpr * n].max()) > (1 << 32) - 600 and int(lo0[0][:b.lpr * n].max()) < 1 << 22
    stride = 60 if b.fasta else 150
    eb, eq = b.rows_of(rr, stride)
    rows = {}
    for name, addr, tl, (line, cap_lines, flags) in (("at their offsets", sp.addr, lt.CAP, hi), ("at offset 0", flat.ctypes.data, len(flat) - 16, lo0)):
        pb, pq, irr = _emu_pack(addr, tl, b.lpr, line, cap_lines, flags, n, stride)
        assert irr == 0, name
        assert np.array_equal(pb, eb.numpy()), "bases rows " + name
        assert b.fasta or np.array_equal(pq, eq.numpy()), "quality rows " + name
        rows[name] = (pb.copy(), None if pq is None else pq.copy())
    fwd = 3
    res = b.res_of(rr, fwd).numpy()
    text = flat[:-16].tobytes()
    for out_fasta in ((False,) if b.fasta else (False, True)):
        want = b"".join(lt.format_plain(text, b.lpr, res, fwd, out_fasta))
        for name, addr, (line, cap_lines, flags) in (("at their offsets", sp.addr, hi), ("at offset 0", flat.ctypes.data, lo0)):
            got = _emu_format(addr, b.lpr, line, cap_lines, flags, n, res, fwd, rows[name][1], stride, out_fasta, len(text) + n + 16)
            assert got == want, "formatted text %s, out_fasta %r" % (name, out_fasta)
        assert want.count(b"\n") == (2 if b.fasta or out_fasta else 4) * int(((res >> 16) & 1).sum())
    if b.fasta:
        want = b.weights(rr, torch.from_numpy(res))
        r32 = np.ascontiguousarray(res, dtype=np.uint32)
        for addr, (line, cap_lines, _) in ((sp.addr, hi), (flat.ctypes.data, lo0)):
            w = (C.c_uint64 * 8)()
            assert emu_py.lib().fxg_emu_fasta_weights(C.c_void_p(addr), C.c_void_p(line.ctypes.data), C.c_uint64(cap_lines), C.c_uint64(n), C.c_void_p(r32.ctypes.data), w) == 0
            assert list(w)[:7] == want


@pytest.fixture(scope="module")
def bcemu(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bcsplit_large"))
    obj = _obj(os.path.join(EMU_DIR, "bcsplit_emu.cpp"), os.path.join(d, "bcsplit_emu.o"))
    subprocess.check_call(emu_py._LINK + [obj, "-o", os.path.join(d, "libbcsplit_emu.so")])
    L = C.CDLL(os.path.join(d, "libbcsplit_emu.so"))
    L.fxg_emu_bc_prepare.restype = C.c_void_p
    L.fxg_emu_bc_prepare.argtypes = [C.POINTER(BarcodeSet), C.c_void_p, C.c_char_p, C.c_size_t]
    L.fxg_emu_bc_free.argtypes = [C.c_void_p]
    L.fxg_emu_bc_split.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    return L


def _emu_split(L, ents, mm, eol, bins, text_addr, text_len, lpr, ls, n, total):
    E = len(ents)
    bases, lens, binv = np.zeros((max(E, 1), 64), np.uint8), np.zeros(max(E, 1), np.uint32), np.zeros(max(E, 1), np.uint32)
    for k, (x, j) in enumerate(ents):
        bases[k, :len(x)] = np.frombuffer(x, np.uint8)
        lens[k], binv[k] = len(x), j
    st = BarcodeSet(bases.ctypes.data, lens.ctypes.data, binv.ctypes.data, E, lt.BL, mm, int(eol), bins)
    t = L.fxg_emu_bc_prepare(C.byref(st), None, None, 0)
    assert t
    rb, out = np.full(n + 8, 0xEEEE, np.uint16), np.full(total + 64, 0xA5, np.uint8)
    bb, br = np.zeros(bins, np.uint64), np.zeros(bins, np.uint64)
    ls = np.ascontiguousarray(ls, dtype=np.uint32)
    rc = L.fxg_emu_bc_split(t, text_addr, text_len, lpr, ls.ctypes.data, len(ls), n, rb.ctypes.data, out.ctypes.data, bb.ctypes.data, br.ctypes.data, None, 0)
    L.fxg_emu_bc_free(t)
    assert rc == 0 and (rb[n:] == 0xEEEE).all() and (out[total:] == 0xA5).all()
    return rb[:n].astype(np.int64), bb, br, out[:total].tobytes()


@pytest.mark.parametrize("eol", [False, True], ids=["bol", "eol"])
def test_sparse_split_on_cluster_records(sparse, bcemu, eol):
    """fxg_emu_bc_split on each cluster at its own offsets (line starts around 2^31, up to the cap: the last window of fasta_short begins in the
    last 70 bytes below 2^32) against the closed forms, the model, and the same records at offset 0"""
    sp, b, cl = sparse
    bins, mm = 97, 1
    ents = lt.table(bins, 1, eol)
    for r0, r1 in cl:
        rr = b.range(r0, r1)
        n = rr.numel()
        text = b.text_of(rr).numpy()
        flat = np.ascontiguousarray(np.concatenate([text, np.full(16, 0x5A, np.uint8)]))
        total = len(text)
        hi, lo0 = _line_arrays(b, rr)[0][:b.lpr * n + 1], _line_arrays(b, rr, base=0)[0][:b.lpr * n + 1]
        assert int(hi[-1]) - int(hi[0]) == total == int(lo0[-1])
        win, F = b.bc_window(rr, eol)
        want_bin = lt.classify_torch(torch, win, F, ents, mm, bins - 1).numpy()
        order = np.argsort(want_bin, kind="stable")
        want_out = bytes(b.text_of(rr[torch.from_numpy(order)]).numpy())
        sizes = b.fields(rr)["size"].numpy()
        got = {}
        for name, addr, tl, ls in (("at their offsets", sp.addr, lt.CAP, hi), ("at offset 0", flat.ctypes.data, total, lo0)):
            rb, bb, br, out = _emu_split(bcemu, ents, mm, eol, bins, addr, tl, b.lpr, ls, n, total)
            ctx = "%s, records %d..%d %s" % (b.shape, r0, r1, name)
            assert np.array_equal(rb, want_bin), "rec_bin " + ctx
            assert np.array_equal(br, np.bincount(want_bin, minlength=bins).astype(np.uint64)), "bin_records " + ctx
            assert np.array_equal(bb, np.bincount(want_bin, weights=sizes, minlength=bins).astype(np.uint64)), "bin_bytes " + ctx
            assert out == want_out, "d_out " + ctx
            got[name] = (rb, out)
        m = M.split_block(text.tobytes(), b.lpr, [x for x, _ in ents], [j for _, j in ents], lt.BL, mm, eol, bins)      # (a CRLF line's CR is part of the bases line)
        assert np.array_equal(m[0], want_bin) and m[3] == want_out
        assert (want_bin != bins - 1).sum() > n // 2


def test_barcode_window_across_the_marks(bcemu):
    """One record at a time, laid so that its barcode window [ws, ws + F) lies across 2^31 at every split of its 8 bytes, begins at 2^31, ends
    just below it, and ends at the last byte a block can hold: the same bin and bytes as at offset 0."""
    sp = Sparse()
    try:
        b = lt.Block(torch, "fasta_short", 400, pad=0)
        ents = lt.table(97, 1, False)
        ents_eol = lt.table(97, 1, True)
        done = 0
        for r in range(40, 400):
            rr = b.range(r, r + 1)
            f = b.fields(rr)
            L, c0 = int(f["L"][0]), int(f["c0"][0])
            if L < 2 * lt.BL:
                continue
            text = b.text_of(rr).numpy()
            size = len(text)
            flat = np.ascontiguousarray(np.concatenate([text, np.full(16, 0x5A, np.uint8)]))
            for eol in (False, True):
                ws_in = c0 + 1 + (L - lt.BL if eol else 0)          # the window's offset inside the record
                places = [(1 << 31) - d - ws_in for d in range(0, lt.BL + 1)] + [(1 << 31) - lt.BL - 3 - ws_in, lt.CAP - size]
                for at in places:
                    sp.a[at:at + size] = text
                    ls = np.array([at, at + c0 + 1, at + size], np.uint32)
                    e = ents_eol if eol else ents
                    hi = _emu_split(bcemu, e, 1, eol, 97, sp.addr, lt.CAP, 2, ls, 1, size)
                    lo0 = _emu_split(bcemu, e, 1, eol, 97, flat.ctypes.data, size, 2, np.array([0, c0 + 1, size], np.uint32), 1, size)
                    want = int(lt.classify_torch(torch, *b.bc_window(rr, eol), e, 1, 96)[0])
                    assert int(hi[0][0]) == int(lo0[0][0]) == want and hi[3] == lo0[3] == text.tobytes(), (r, eol, hex(at))
                    sp.a[at:at + size] = 0
                    done += want != 96
            if done > 200:
                break
        assert done > 200                # matched records among them: an unread window would have gone to `unmatched`
    finally:
        sp.close()


# ---- 3. the package's arithmetic on an index past 2^31 --------------------------------------------------------------------------------------
def test_text_index_offsets_are_unsigned():
    """TextIndex hands out what the engine wrote: u32 offsets.  On a faked index whose records end past 2^31 (and at the cap), starts / ends read
    as 0 .. 2^32 - 1 and record_bytes() -- what Engine.barcode_split sizes d_out by -- is the span of the records, not a negative number."""
    from fastx_toolkit_amd.engine import TextIndex
    lpr, n = 4, 3
    cap_lines = lpr * n + 1 + 4
    st = np.array([16, 20, 30, 32, (1 << 31) - 8, (1 << 31) + 5, 3_000_000_000, 3_000_000_100, 3_000_000_200, 3_000_000_300, 4_000_000_000, 4_100_000_000,
                   lt.CAP], dtype=np.uint64)
    line = np.zeros(2 * cap_lines, np.uint32)
    line[:len(st)] = st
    line[cap_lines:cap_lines + len(st) - 1] = st[1:] - 1
    ix = TextIndex(torch.from_numpy(line.view(np.int32).copy()), cap_lines, torch.zeros(n + 2, dtype=torch.uint8), lpr)
    assert ix.line.dtype == torch.int32 and int(ix.line[12]) < 0                   # what the allocation holds, read as signed
    assert [int(x) for x in ix.starts[:13].to(torch.int64)] == [int(x) for x in st]
    assert np.array_equal(ix.starts[:13].numpy().view(np.uint32), st.astype(np.uint32))       # (the view existing callers apply by hand still holds)
    assert int(ix.starts[12].item()) == lt.CAP and int(ix.ends[11].item()) == lt.CAP - 1 and int(ix.ends[3].item()) == (1 << 31) - 9
    assert ix.starts.numel() == cap_lines and ix.ends.numel() == cap_lines
    assert ix.record_bytes(0) == 0 and ix.record_bytes(1) == (1 << 31) - 8 - 16 and ix.record_bytes(2) == 3_000_000_200 - 16 and ix.record_bytes(3) == lt.CAP - 16


# ---- 4. the format's scan item: offset and rank of more than 2^24 kept records ------------------------------------------------------------
def test_format_from_packed_arrays_past_2_24_kept_records():
    """fxg_fastq_format reads a kept record's packed bases at pk_off[rank], the rank taken from the scanned items, which carry it modulo 2^24.
    More than 2^24 kept four-byte FASTA records (">\\nA\\n", every fifth one dropped), each with one base from the packed array: every kept
    record must come out with its own base (the rank taken as it stands in the item wrapped, and the 2^24-th kept record took the base of
    the first)."""
    n = 5 * (1 << 22) + 5000
    text = np.tile(np.frombuffer(b">\nA\n", np.uint8), n + 4)
    r = np.arange(n, dtype=np.uint64)
    keep = r % np.uint64(5) != 0
    k = int(keep.sum())
    assert k > (1 << 24) + 1000
    cap_lines = 2 * n + 1
    line = np.zeros(2 * cap_lines, np.uint32)
    line[0:2 * n:2], line[1:2 * n:2], line[2 * n] = 4 * r, 4 * r + 2, 4 * n
    line[cap_lines:cap_lines + 2 * n:2], line[cap_lines + 1:cap_lines + 2 * n:2] = 4 * r + 1, 4 * r + 3
    flags = np.zeros(n, np.uint8)
    res = np.where(keep, (1 << 16) | 1, 0).astype(np.uint32)
    rank = np.arange(k, dtype=np.uint64)
    pk = np.frombuffer(b"ACGT", np.uint8)[((rank + (rank >> np.uint64(24))) & np.uint64(3)).astype(np.int64)].copy()
    out = np.full(4 * k + 64, 0xA5, np.uint8)
    nb = C.c_uint64()
    rc = emu_py.lib().fxg_emu_fastq_format(C.c_void_p(text.ctypes.data), C.c_int(2), C.c_void_p(line.ctypes.data), C.c_uint64(cap_lines), C.c_void_p(flags.ctypes.data),
                                           C.c_uint64(n), C.c_void_p(res.ctypes.data), C.c_uint32(0), C.c_int(0), C.c_void_p(pk.ctypes.data), None, C.c_void_p(rank.ctypes.data),
                                           None, C.c_uint32(0), C.c_int(33), C.c_int(0), C.c_void_p(out.ctypes.data), C.byref(nb), None, C.c_size_t(0))
    assert rc == 0 and nb.value == 4 * k and (out[4 * k:] == 0xA5).all()
    got = out[:4 * k].reshape(k, 4)
    assert (got[:, 0] == 62).all() and (got[:, 1] == 10).all() and (got[:, 3] == 10).all()
    bad = np.flatnonzero(got[:, 2] != pk)
    assert bad.size == 0, "kept record %d (of %d differing) has base %r, its packed base is %r" % (bad[0], bad.size, chr(got[bad[0], 2]), chr(pk[bad[0]]))
    assert (pk[1 << 24:] != pk[:k - (1 << 24)]).all()         # (what the wrapped rank would have fetched differs)


# ---- 5. ordinal ids: the closed forms, the decimal width sum, and more than 2^24 kept records with the modes on -----------------------------
@pytest.fixture(scope="module")
def fmtopts():
    """the emulation stub with fxg_fastq_format_opts behind it (tests/emu/fmtopts_stub.cpp)"""
    L = C.CDLL(os.path.join(emu_py.build_fmtopts(), "libfxg.so"))
    L.fxg_emu_dec_width_sum.restype, L.fxg_emu_dec_width_sum.argtypes = C.c_uint64, [C.c_uint64, C.c_uint64]
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    L.fxg_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.fxg_last_error.restype, L.fxg_last_error.argtypes = C.c_char_p, [vp]
    L.fxg_fastq_format_opts.argtypes = [vp, vp, i32, vp, u64, vp, u64, vp, u32, i32, vp, vp, vp, vp, u32, i32, i32, vp, C.POINTER(u64), C.POINTER(emu_py.FormatOpts)]
    ctx = vp()
    assert L.fxg_ctx_create(0, C.byref(ctx)) == 0
    return L, ctx


def test_ordinal_closed_forms_against_plain_python():
    """large_text.ord_text / ord_offset / dec_width_sum on the first and last 10 000 kept ranks of the 2^24 case, every base, against "%d" in
    Python and against the suite's model of the formatter (format_opts_cases.expected)"""
    import format_opts_cases as F
    kept = int(lt.ord_keep(torch, torch.arange(lt.ORD_N, dtype=torch.int64)).sum())
    assert (1 << 24) < kept < lt.ORD_N - (1 << 20) and kept > (1 << 24) + (1 << 22)          # fifteen in sixteen: past 2^24, well short of all
    for base in lt.ORD_BASES:
        for both in (False, True):
            for k0, k1 in ((0, 10000), (kept - 10000, kept), ((1 << 24) - 5000, (1 << 24) + 5000), (lt.ORD_N - 10000, lt.ORD_N)):
                want = b"".join((b"@%d\nA\n+%d\nI\n" % (base + k + 1, base + k + 1)) if both else (b">%d\nA\n" % (base + k + 1)) for k in range(k0, k1))
                assert bytes(lt.ord_text(torch, base, k0, k1, both).numpy()) == want, (base, both, k0)
                assert lt.ord_offset(base, k1, both) - lt.ord_offset(base, k0, both) == len(want)
                assert lt.dec_width_sum(base + 1 + k0, k1 - k0) == sum(len(str(base + 1 + k)) for k in range(k0, k1))
            lpr = 4 if both else 2
            assert bytes(lt.ord_text(torch, base, 0, 3000, both).numpy()) == F.expected(lt.ORD_RECORD[lpr] * 3000, lpr, id_mode=1, id_both=both, base=base)
    line, cap_lines = lt.ord_index(np, 5, 4)
    text = lt.ORD_RECORD[4] * 5
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    assert cap_lines == 21 and np.array_equal(line[1:21], nl + 1) and np.array_equal(line[21:41], nl) and line[0] == 0


def test_decimal_width_sum_at_every_power_of_ten(fmtopts):
    """fxg_dec_width_sum against Python's integers: first at every power of ten, give or take 1, up to 2^64 - 1; counts of 0, 1, 2, 2^24 + 1 and
    up to the last number a u64 holds (the reference sum itself is held against a plain loop above and here for the small counts)"""
    L, _ = fmtopts
    firsts = sorted({10 ** k + d for k in range(20) for d in (-1, 0, 1) if 0 <= 10 ** k + d < 2 ** 64} | {0, 2 ** 64 - 1, 2 ** 64 - 2, 2 ** 63, 2 ** 32 - 1})
    for a in firsts:
        for count in (0, 1, 2, 11, (1 << 24) + 1, 2 ** 64 - a):
            if a + count > 2 ** 64:
                continue
            want = lt.dec_width_sum(a, count)
            if count <= 11:
                assert want == sum(len(str(a + i)) for i in range(count))
            assert want < 2 ** 64 or count > 1 << 25
            if want < 2 ** 64:
                assert L.fxg_emu_dec_width_sum(a, count) == want, (a, count)


def _ordinals_emulated(fmtopts, lpr, keep, base, both):
    """fxg_fastq_format_opts of the emulation stub over lt.ORD_N records ORD_RECORD[lpr] with ordinal ids: the exact-capacity pair, then (out, kept)"""
    L, ctx = fmtopts
    n = lt.ORD_N
    text = np.tile(np.frombuffer(lt.ORD_RECORD[lpr], np.uint8), n + 4)
    line, cap_lines = lt.ord_index(np, n, lpr)
    flags, rows = np.zeros(n, np.uint8), np.full(n, ord("I"), np.uint8)
    res = np.where(keep, (1 << 16) | 1, 0).astype(np.uint32)
    kept = int(keep.sum())
    total = lt.ord_offset(base, kept, both)
    out = np.full(total + 64, 0xA5, np.uint8)
    nb = C.c_uint64(7)

    def call(cap):
        o = emu_py.FormatOpts(1, int(both), base, 0, cap, None)
        return L.fxg_fastq_format_opts(ctx, text.ctypes.data, lpr, line.ctypes.data, cap_lines, flags.ctypes.data, n, res.ctypes.data, 0, 0, None, None, None, rows.ctypes.data, 1, 33, 0,
                                       out.ctypes.data, C.byref(nb), C.byref(o))
    problems = []
    rc = call(total - 1)
    if not (rc == -1 and nb.value == 0 and (out == 0xA5).all() and L.fxg_last_error(ctx).decode() == "the formatted block needs %d bytes, d_out takes %d" % (total, total - 1)):
        problems.append("a d_out of %d bytes, one short of the closed-form total: rc %d, out_bytes %d, \"%s\"" % (total - 1, rc, nb.value, L.fxg_last_error(ctx).decode()))
        out[:] = 0xA5
    rc = call(total)
    if not (rc == 0 and nb.value == total and (out[total:] == 0xA5).all()):
        problems.append("a d_out of the closed-form total %d: rc %d, out_bytes %d, \"%s\"" % (total, rc, nb.value, L.fxg_last_error(ctx).decode()))
    return out[:total], kept, problems


def test_ordinal_ids_past_2_24_kept_records(fmtopts):
    """The rank rebuilt at every 2^23-th record feeds the ordinal id and its closed-form digit offset: 2^24 + 2^23 + 5 records, fifteen in sixteen
    kept, ids that reach nine digits at the rank 2^24 - 1.  out_bytes and the exact-capacity pair (the total is the one thread's sum of
    copies * D(base + 1, kept) and the scanned offset), and the output at the prefix, around the ranks 2^23, 2^24 - 1 (the wrap of the 24-bit field) and the ranks of the
    records 2^23, 2^24 and 2^24 + 2^23, and the suffix, against the closed forms."""
    keep = lt.ord_keep(torch, torch.arange(lt.ORD_N, dtype=torch.int64)).numpy()
    base = lt.ORD_BASES[1]
    out, kept, problems = _ordinals_emulated(fmtopts, 2, keep, base, False)
    rank_of = np.cumsum(keep) - keep
    marks = [0, 1 << 23, (1 << 24) - 1] + [int(rank_of[r]) for r in (1 << 23, 1 << 24, (1 << 24) + (1 << 23))] + [kept - 1]
    for m in marks:
        k0, k1 = max(0, m - 5000), min(kept, m + 5000)
        a, b = lt.ord_offset(base, k0, False), lt.ord_offset(base, k1, False)
        want = lt.ord_text(torch, base, k0, k1, False).numpy()
        if not np.array_equal(out[a:b], want):
            i = int(np.flatnonzero(out[a:b] != want)[0])
            problems.append("the ids of the kept ranks %d..%d: from output byte %d on %r, expected %r" % (k0, k1, a + i, bytes(out[a + max(i - 12, 0):a + i + 24]), bytes(want[max(i - 12, 0):i + 24])))
    if int((out == 10).sum()) != 2 * kept:
        problems.append("%d newlines for %d kept records" % (int((out == 10).sum()), kept))
    assert not problems, "\n".join(problems)


def test_mode_sizes_against_the_model():
    """large_text.Block.mode_sizes / numeric_line (the digit sums from the quality hash) on the first and last 10 000 records of a fastq_mixed block,
    against format_opts_cases.expected on the generated text and against "%d" in plain Python"""
    import format_opts_cases as F
    b, rr, text = _small("fastq_mixed", 20000)
    recs = F.records(text, 4)
    qbytes, minus_one = b.numeric_line(rr)
    assert int(b.fields(rr)["numeric"].sum()) > 200
    for r in list(range(0, 20000, 97)) + list(range(19990, 20000)):
        vals = F.qual_values(recs[r], 33)
        assert int(qbytes[r]) == len(b" ".join(b"%d" % v for v in vals)) and int(minus_one[r]) == vals.count(-1), r
    for mode, (id_mode, both, base, qual_mode) in (("numeric-ordinal", (1, True, 10 ** 19 - 2, 2)), ("ascii-sequence", (2, True, 0, 1))):
        for r0, r1 in ((0, 10000), (10000, 20000)):
            wtext = bytes(b.text_of(b.range(r0, r1)).numpy())
            want = F.expected(wtext, 4, 33, id_mode=id_mode, id_both=both, base=base + r0, qual_mode=qual_mode)
            sz = b.mode_sizes(b.range(r0, r1), mode, base)
            assert int(sz.sum()) == len(want), (mode, r0)
            cut = F.expected(wtext, 4, 33, res=[(1, len(rec[1])) if k < 50 else (0, 0) for k, rec in enumerate(F.records(wtext, 4))], id_mode=id_mode, id_both=both, base=base + r0, qual_mode=qual_mode)
            assert int(sz[:50].sum()) == len(cut), (mode, r0)
            if mode == "numeric-ordinal":
                assert want.count(b" ") == int((b.fields(b.range(r0, r1))["L"] - 1).sum())
            else:
                assert want.count(b" ") == int((minus_one * b.fields(rr)["numeric"])[r0:r1].sum())
