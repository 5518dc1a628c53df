"""Reference code of tests/test_gpu_large_offsets_text.py: blocks of FASTQ / FASTA text of exactly the C-ABI's largest size (0xFFFFFFF0 bytes,
include/fxg.h), whose every byte is a pure function of (seed, record index), and the closed forms of what the device text path (csrc/fxg_text.h)
and the barcode splitter (csrc/fxg_barcode.h) must make of them.  Nothing here touches the engine; tests/test_large_text_cpu.py pins every
piece against trusted code (the oracle's parser and formatter, tests/bcsplit_model.py, the reference driver where it is built) on blocks of a
few thousand records, so that the GPU test does not trust this code on its own word.

Everything is torch on int64 (wrapping multiplies, arithmetic shifts masked to logical ones, as large_offsets.lens_torch): on the device for the
whole block in slabs, on the CPU for windows (`.numpy()`); the host never holds more than a slab.  All functions take a tensor of record
indices, so a window need not be a range (the records of one bin, in output order).

Shapes (a record's fields come from one 64-bit hash of its index; read lengths from the index hash of large_offsets.lens_numpy):
  fastq_lf     four lines: "@s<index>", 1..150 bases (ACGTN), "" / "+" / "+s<index>" (one in eight empty: the formatter then writes one byte more
               than it read, fxg.h:279), qualities 33..126
  fastq_mixed  the same, CRLF on one record in sixteen and on the last one, a numeric quality line (values -15..93, signs, double blanks) on one in sixty-four
  fasta_short  two lines: "><index>" or "><index>-<count>", 20..60 bases; the last record has 1..8 bases
The last record's name is padded with 'x' to the byte that makes text_len == CAP.  Reads carry a barcode of BL bases at their start (seven in
eight) and at their end (reads of 16 bases and more), one in four of them with one base replaced, so that a split has matches in every bin."""
import numpy as np

import large_offsets as lo

CAP = 0xFFFFFFF0                         # the largest text_len fxg_fastq_index and fxg_barcode_split accept
MARKS = (31, 32)                         # byte offsets a block of CAP bytes crosses (2^32 only on the output side of a format that grows)
SEED = 11
KI = 3000                                # records per window, at least (large_offsets.KI: eleven tiles of 256)
RANDOM_WINDOWS = 8
SHAPES = ("fastq_lf", "fastq_mixed", "fasta_short")
STRIDE = 150                             # longest read of the FASTQ shapes
FA_MIN, FA_SPAN, FA_LAST = 20, 40, 8     # fasta_short: 20 + lens(40) bases; the last record 1..FA_LAST
BL = 8                                   # barcode length
NCODES = 4095                            # distinct barcodes (4 096 bins with `unmatched`); the first 96 are the 97-bin table
# records per block: the largest N whose unpadded text fits in CAP (size_rule(); test_large_text_cpu.py recomputes them)
BLOCKS = {"fastq_lf": 17_989_614, "fastq_mixed": 17_591_670, "fasta_short": 69_155_099}

_C1, _C2 = lo._signed(0x9E3779B97F4A7C15), lo._signed(0xD6E8FEB86659FD93)
_P10 = [10 ** k for k in range(19)]


def _mix(x):
    """64-bit mixer of an int64 tensor (multiply, xor-shift, multiply, xor-shift)."""
    h = x * _C1
    h = h ^ ((h >> 32) & 0xFFFFFFFF)
    h = h * _C2
    return h ^ ((h >> 29) & 0x7FFFFFFFF)


def _bits(h, shift, nbits):
    return (h >> shift) & ((1 << nbits) - 1)


def lens_of(torch, rr, stride, min1):
    """large_offsets.lens_torch for a tensor of read indices (int64)."""
    h = rr * _C1
    h = h ^ ((h >> 32) & 0xFFFFFFFF)
    h = h * _C2
    wide = ((h >> 60) & 15) == 0
    u = (h >> 24) & 0xFFFFFFFF
    lo_ = torch.where(wide, 0, stride // 2)
    ln = lo_ + ((u * (stride + 1 - lo_)) >> 32)
    return torch.clamp(ln, min=1) if min1 else ln


def ndigits(torch, v):
    w = torch.ones_like(v)
    for k in range(1, 19):
        w = w + (v >= _P10[k]).to(v.dtype)
    return w


def digit_at(torch, v, w, d):
    """decimal digit d (0 = most significant) of v, which has w digits; d outside 0..w-1 gives garbage the caller masks"""
    p = torch.tensor(_P10, dtype=torch.int64, device=v.device)[torch.clamp(w - 1 - d, 0, 18)]
    return torch.div(v, p, rounding_mode="floor") % 10


def code_bases(torch, k, i):
    """base i (0..BL-1) of barcode k (0..NCODES-1): the 2-bit digits of an odd multiple of k mod 2^16, so all codes differ"""
    v = (k * 40503 + 12345) & 0xFFFF
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.int64, device=k.device)
    return acgt[(v >> (2 * i)) & 3]


def codes_numpy(n=NCODES):
    import torch
    k = torch.arange(n, dtype=torch.int64)[:, None]
    return code_bases(torch, k, torch.arange(BL, dtype=torch.int64)[None, :]).to(torch.uint8).numpy()


def table(bins, partial, eol):
    """[(bases, bin)] of the reference's table for the first bins - 1 codes: every barcode, then its `partial` shortened forms (the script drops
    the first base for --bol, the last for --eol)."""
    ents = []
    for j, c in enumerate(codes_numpy(bins - 1)):
        b = bytes(c)
        ents.append((b, j))
        for _ in range(partial):
            b = b[:-1] if eol else b[1:]
            ents.append((b, j))
    return ents


class Block:
    """One block: `n` records of a shape; the last one's name padded by `pad` bytes (None: up to cap).  rec_start (int64 [n + 1], on `device`)
    holds every record's byte offset; text_len == rec_start[n]."""

    def __init__(self, torch, shape, n, device="cpu", pad=None, cap=CAP, seed=SEED, slab=4_000_000):
        assert shape in SHAPES
        self.torch, self.shape, self.n, self.device, self.seed, self.slab = torch, shape, int(n), device, seed, slab
        self.fasta = shape == "fasta_short"
        self.lpr = 2 if self.fasta else 4
        self.pad = 0
        self.rec_start = torch.zeros(self.n + 1, dtype=torch.int64, device=device)
        run = 0
        for s in range(0, self.n, slab):
            e = min(self.n, s + slab)
            sz = self.fields(torch.arange(s, e, dtype=torch.int64, device=device))["size"]
            self.rec_start[s + 1:e + 1] = torch.cumsum(sz, 0) + run
            run = int(self.rec_start[e])
        self.unpadded = run
        if pad is None:
            pad = cap - run
        assert 0 <= pad < 24000, "a block of %d records of %s is %d bytes without padding, the cap is %d" % (n, shape, run, cap)
        self.pad = int(pad)
        self.rec_start[self.n] += self.pad
        self.text_len = run + self.pad

    # ---- per-record fields ----
    def fields(self, rr):
        """dict of int64 tensors for the records rr: hr (the record's hash), L, w (digits of the index), c0..c3 (content bytes of its lines),
        el (bytes of a line end), numeric, size, and for FASTA hasc / count / wc."""
        t = self.torch
        hr = _mix(rr + self.seed * 0x1000003)
        last = rr == self.n - 1
        w = ndigits(t, rr)
        f = dict(hr=hr, w=w, last=last)
        padv = last.to(t.int64) * self.pad
        one = t.ones_like(rr)
        if self.fasta:
            L = FA_MIN + lens_of(t, rr, FA_SPAN, False)
            L = t.where(last, 1 + _bits(hr, 20, 16) % FA_LAST, L)
            hasc = _bits(hr, 0, 1)
            count = 1 + _bits(hr, 8, 20) % 500
            wc = ndigits(t, count)
            c0 = 1 + w + hasc * (1 + wc) + padv
            f.update(L=L, hasc=hasc, count=count, wc=wc, c0=c0, c1=L, el=one, numeric=t.zeros_like(rr), size=c0 + L + 2)
            return f
        L = lens_of(t, rr, STRIDE, True)
        kind = _bits(hr, 0, 3)                                # 0: empty third line, 1..3: "+", 4..7: "+s<index>"
        c2 = t.where(kind == 0, 0, t.where(kind < 4, 1, 2 + w))
        mixed = self.shape == "fastq_mixed"
        crlf = ((_bits(hr, 3, 4) == 0) | last).to(t.int64) * int(mixed)        # (the last record too: its lines are chomped 16 bytes below 2^32)
        numeric = (_bits(hr, 7, 6) == 0).to(t.int64) * int(mixed)
        c0 = 2 + w + padv
        c3 = t.where(numeric == 1, 4 * L, L)
        el = 1 + crlf
        f.update(L=L, kind=kind, c0=c0, c1=L, c2=c2, c3=c3, el=el, numeric=numeric, size=c0 + L + c2 + c3 + 4 * el)
        return f

    # ---- characters ----
    def base_at(self, rr, hr, L, i):
        """base i of read rr (any broadcastable shapes)"""
        t = self.torch
        hc = _mix(rr * 1024 + 256 + i)
        acgt = t.tensor([65, 67, 71, 84], dtype=t.int64, device=rr.device)
        b = t.where(_bits(hc, 0, 6) == 0, 78, acgt[_bits(hc, 6, 2)])
        # the barcode at the start: seven reads in eight; one in eight of them from the whole table, the others from its first 96 codes
        k0 = t.where(_bits(hr, 15, 3) == 0, _bits(hr, 24, 16) % NCODES, _bits(hr, 24, 16) % 96)
        on0 = (_bits(hr, 12, 3) != 0) & (i < BL) & ~((_bits(hr, 18, 2) == 0) & (i == _bits(hr, 20, 3)))
        b = t.where(on0, code_bases(t, k0, t.clamp(i, 0, BL - 1)), b)
        # ... and at the end of reads of 16 bases and more
        k1 = t.where(_bits(hr, 43, 3) == 0, _bits(hr, 46, 16) % NCODES, _bits(hr, 46, 16) % 96)
        j = i - (L - BL)
        on1 = (_bits(hr, 40, 3) != 0) & (L >= 2 * BL) & (j >= 0) & ~((_bits(hr, 62, 1) == 0) & (_bits(hr, 56, 1) == 0) & (j == _bits(hr, 57, 3)))
        return t.where(on1, code_bases(t, k1, t.clamp(j, 0, BL - 1)), b)

    def qual_value(self, rr, numeric, i):
        """(Phred+33 code of quality i as the packed rows hold it, whether a numeric value is written with a '+')"""
        hq = _mix(rr * 1024 + 768 + i)
        u = _bits(hq, 8, 24)
        return self.torch.where(numeric == 1, 18 + u % 109, 33 + u % 94), _bits(hq, 40, 1)

    def numeric_char(self, rr, i):
        """byte i of a numeric quality line: tokens of four bytes, right-aligned (" -15", "  +7", "  93", "   0")"""
        t = self.torch
        code, plus = self.qual_value(rr, t.ones_like(rr), t.div(i, 4, rounding_mode="floor"))
        v = code - 33
        a = t.abs(v)
        sign = t.where(v < 0, 45, t.where(plus == 1, 43, 32))
        two = a >= 10
        slot = i % 4
        return t.where(slot == 3, 48 + a % 10, t.where(slot == 2, t.where(two, 48 + t.div(a, 10, rounding_mode="floor"), sign),
                                                       t.where((slot == 1) & two, sign, 32)))

    def name_char(self, rr, f, j):
        """byte j of the name behind its prefix character"""
        t = self.torch
        w = f["w"]
        if self.fasta:
            ch = t.where(j < w, 48 + digit_at(t, rr, w, j), 120)
            ch = t.where((f["hasc"] == 1) & (j == w), 45, ch)
            return t.where((f["hasc"] == 1) & (j > w) & (j <= w + f["wc"]), 48 + digit_at(t, f["count"], f["wc"], j - w - 1), ch)
        return t.where(j == 0, 115, t.where(j <= w, 48 + digit_at(t, rr, w, j - 1), 120))

    # ---- the text ----
    def text_of(self, rr):
        """uint8 tensor: the bytes of the records rr, one after the other"""
        t = self.torch
        f = self.fields(rr)
        sz = f["size"]
        k = rr.numel()
        loc = t.cumsum(sz, 0) - sz
        rec = t.repeat_interleave(t.arange(k, dtype=t.int64, device=rr.device), sz)
        off = t.arange(rec.numel(), dtype=t.int64, device=rr.device) - loc[rec]
        g = {key: v[rec] for key, v in f.items()}
        r = rr[rec]
        el = g["el"]
        b1 = g["c0"] + el
        b2 = b1 + g["c1"] + el
        if self.fasta:
            line = (off >= b1).to(t.int64)
            i = off - line * b1
            clen = t.where(line == 0, g["c0"], g["c1"])
        else:
            b3 = b2 + g["c2"] + el
            line = (off >= b1).to(t.int64) + (off >= b2) + (off >= b3)
            i = off - t.where(line == 0, 0, t.where(line == 1, b1, t.where(line == 2, b2, b3)))
            clen = t.where(line == 0, g["c0"], t.where(line == 1, g["c1"], t.where(line == 2, g["c2"], g["c3"])))
        name = self.name_char(r, g, i - 1)
        ch = t.where(i == 0, 62 if self.fasta else 64, name)
        ch = t.where(line == 1, self.base_at(r, g["hr"], g["L"], i), ch)
        if not self.fasta:
            ch = t.where(line == 2, t.where(i == 0, 43, name), ch)
            q, _ = self.qual_value(r, t.zeros_like(r), i)
            ch = t.where(line == 3, t.where(g["numeric"] == 1, self.numeric_char(r, i), q), ch)
        ch = t.where(i >= clen, t.where((el == 2) & (i == clen), 13, 10), ch)
        return ch.to(t.uint8)

    def range(self, r0, r1):
        return self.torch.arange(r0, r1, dtype=self.torch.int64, device=self.device)

    def slabs(self, nbytes=1 << 28):
        """[(r0, r1)]: record ranges of about nbytes bytes of text each"""
        out, r0 = [], 0
        per = max(1, int(self.n * nbytes / max(self.text_len, 1)))
        while r0 < self.n:
            out.append((r0, min(self.n, r0 + per)))
            r0 += per
        return out

    def build(self, tail=16, poison=0x5A):
        """The whole block on the device, slab by slab, followed by `tail` poison bytes."""
        t = self.torch
        d = t.full((self.text_len + tail,), poison, dtype=t.uint8, device=self.device)
        for r0, r1 in self.slabs(1 << 26):
            a, b = int(self.rec_start[r0]), int(self.rec_start[r1])
            d[a:b] = self.text_of(self.range(r0, r1))
        return d

    # ---- closed forms ----
    def line_index(self, rr):
        """(starts, ends) int64 [k, lpr]: every line's first byte and the byte behind its content (its CR or LF), as block offsets"""
        t = self.torch
        f = self.fields(rr)
        s0 = self.rec_start[rr]
        el = f["el"]
        cs = [f["c0"], f["c1"]] + ([] if self.fasta else [f["c2"], f["c3"]])
        starts, ends, at = [], [], s0
        for c in cs:
            starts.append(at)
            ends.append(at + c)
            at = at + c + el
        return t.stack(starts, 1), t.stack(ends, 1)

    def rows_of(self, rr, stride):
        """(bases, qual) uint8 [k, stride] as fxg_fastq_pack writes them at qoffset 33 (qual None for FASTA)"""
        t = self.torch
        f = self.fields(rr)
        i = t.arange(stride, dtype=t.int64, device=rr.device)[None, :]
        r, L = rr[:, None], f["L"][:, None]
        inside = i < L
        b = t.where(inside, self.base_at(r, f["hr"][:, None], L, i), 0).to(t.uint8)
        if self.fasta:
            return b, None
        q, _ = self.qual_value(r, f["numeric"][:, None], i)
        return b, t.where(inside, q, 0).to(t.uint8)

    def res_of(self, rr, fwd_start, keep_all=False):
        """A hand-made res[] (int64; the low 32 bits are the engine's word): kept (bit 16) three records in four whose read is longer than
        fwd_start, with 1 .. L - fwd_start bases (bits 0..15); a drop reason 0..7 (bits 17..20) and the adapter-only bit (22) for the weights."""
        t = self.torch
        f = self.fields(rr)
        hr, room = f["hr"], f["L"] - fwd_start
        keep = (room > 0) & (t.tensor(keep_all, device=rr.device) | (_bits(hr, 32, 2) != 0))
        ln = 1 + _bits(hr, 34, 20) % t.clamp(room, min=1)
        if keep_all:
            ln = room
        why = t.where(keep, 0, _bits(hr, 54, 3))
        return t.where(keep, ln | (1 << 16), 0) | (why << 17) | (_bits(hr, 58, 1) << 22)

    def format_sizes(self, rr, res, out_fasta=False):
        """bytes fxg_fastq_format writes for each record (0: dropped); records with a numeric quality line are not covered"""
        t = self.torch
        f = self.fields(rr)
        keep = ((res >> 16) & 1) == 1
        ln = res & 0xFFFF
        sz = (f["c0"] - 1) + ln + 3
        if not self.fasta and not out_fasta:
            assert int(f["numeric"].sum()) == 0
            sz = sz + t.clamp(f["c2"] - 1, min=0) + ln + 3
        return t.where(keep, sz, 0)

    def numeric_line(self, rr):
        """(bytes of the record's quality line written as numbers -- "%d" joined by single blanks --, how many of its values are -1: the code of a
        blank) for FASTQ records, from the quality hash alone"""
        t = self.torch
        f = self.fields(rr)
        i = t.arange(STRIDE, dtype=t.int64, device=rr.device)[None, :]
        inside = i < f["L"][:, None]
        code, _ = self.qual_value(rr[:, None], f["numeric"][:, None], i)
        v = code - 33
        width = (v < 0).to(t.int64) + t.where(t.abs(v) >= 10, 2, 1)
        return (width * inside).sum(1) + f["L"] - 1, ((code == 32) & inside).sum(1)

    def mode_sizes(self, rr, mode, base=0):
        """bytes fxg_fastq_format_opts writes for each FASTQ record kept whole, rank = index: "numeric-ordinal" = numeric quality lines and the
        ordinal id base + index + 1 on both name lines; "ascii-sequence" = character quality lines and the bases on both name lines"""
        L = self.fields(rr)["L"]
        if mode == "ascii-sequence":
            return 4 * L + 6
        assert mode == "numeric-ordinal"
        return 2 * _ord_parts(self.torch, base, rr)[2] + L + self.numeric_line(rr)[0] + 6

    def weights(self, rr, res):
        """the seven tallies of fxg_fasta_weights over the records rr, as int64 sums"""
        t = self.torch
        f = self.fields(rr)
        w = t.where(f["hasc"] == 1, f["count"], 1)
        why = (res >> 17) & 15
        sel = [t.ones_like(w), (res >> 16) & 1, why == 1, (res >> 22) & 1, why == 3, why == 4, why == 5]
        return [int((w * s.to(t.int64)).sum()) for s in sel]

    def bc_window(self, rr, eol):
        """(win uint8 [k, BL], F int64 [k]): the splitter's window of every record, window r in win[r, :F[r]].  The splitter's bases line runs up
        to its LF, as the script's does: the CR of a CRLF record is its last byte."""
        t = self.torch
        f = self.fields(rr)
        L = f["L"][:, None]
        Lx = L + (f["el"][:, None] - 1)
        F = t.clamp(Lx, max=BL)
        i = t.arange(BL, dtype=t.int64, device=rr.device)[None, :]
        pos = (Lx - F + i) if eol else i + 0 * L
        w = t.where(pos == L, 13, self.base_at(rr[:, None], f["hr"][:, None], L, t.clamp(pos, max=L - 1)))
        return t.where(i < F, w, 0).to(t.uint8), F[:, 0]


def size_rule(torch, shape, device="cpu", cap=CAP, seed=SEED, slab=4_000_000):
    """N of a shape: the largest number of records whose unpadded text fits in cap, the last record in its closing form (FASTA: 1..8 bases).
    Only the last record's size depends on N, so N follows from S[r], the bytes of the ordinary records 0 .. r - 1:
    the largest n with S[n - 1] + size of record n - 1 as the last of n <= cap."""
    probe = Block(torch, shape, 1, device, pad=0, seed=seed)

    def sizes(rr, n):
        probe.n = n
        return probe.fields(rr)["size"]

    S, base, r0 = torch.zeros(1, dtype=torch.int64, device=device), 0, 0          # S[r - base] for r in base .. r0
    while int(S[-1]) <= cap + 1024:
        cs = torch.cumsum(sizes(torch.arange(r0, r0 + slab, dtype=torch.int64, device=device), -1), 0) + S[-1]
        keep = S[-16:]
        base, r0, S = r0 - (keep.numel() - 1), r0 + slab, torch.cat([keep, cs])
    kmax = int(torch.searchsorted(S, torch.tensor([cap], dtype=torch.int64, device=device), right=True)[0]) - 1 + base
    for n in range(kmax + 1, kmax - 8, -1):
        if int(S[n - 1 - base]) + int(sizes(torch.tensor([n - 1], dtype=torch.int64, device=device), n)[0]) <= cap:
            return n
    raise AssertionError("no N for %s" % shape)


# ---- ordinal ids over more than 2^24 kept records ------------------------------------------------------------------------------------------
# The format's scan carries a record's rank in 24 bits; fxg_text_rank rebuilds it at every 2^23-th record, and the rank feeds the ordinal id and
# the closed-form digit offset.  The smallest block that crosses both: 2^24 + 2^23 + 5 records of four bytes (">\nA\n"; as FASTQ "@\nA\n+\nI\n"),
# fifteen in sixteen kept by a hash or all of them -- the kept count passes 2^24 between two 2^23 steps -- and three levels of the scan.
ORD_N = (1 << 24) + (1 << 23) + 5
# the second base: the ids reach nine digits with the rank 2^24 - 1, so every rank from the wrap on has another width than the rank modulo 2^24
# (10^8 is the first power of ten above 2^24: no base puts 10^7 there)
ORD_BASES = [0, 10 ** 8 - 2 ** 24, 10 ** 19 - 2]
ORD_RECORD = {2: b">\nA\n", 4: b"@\nA\n+\nI\n"}
_P = 10 ** 10


def ord_keep(torch, rr):
    """the hash-chosen fifteen records in sixteen"""
    return _bits(_mix(rr + 0x5EED), 11, 4) != 0


def dec_width_sum(first, count):
    """the decimal digits of first .. first + count - 1 together, in Python's integers (what fxg_dec_width_sum states in closed form)"""
    total, lo, w, last = 0, 0, 1, first + count - 1
    while count and lo <= last:
        hi = 10 ** w - 1
        if hi >= first:
            total += w * (min(last, hi) - max(first, lo) + 1)
        lo, w = hi + 1, w + 1
    return total


def ord_offset(base, k, fastq_both):
    """the output byte at which the kept record of rank k begins: ">id\nA\n", or "@id\nA\n+id\nI\n" with the id on both lines"""
    return (8 * k + 2 * dec_width_sum(base + 1, k)) if fastq_both else (4 * k + dec_width_sum(base + 1, k))


def _ord_parts(torch, base, kk):
    """id = base + 1 + kk, which passes 2^63, as (high part, low ten digits, width)"""
    lo = (base + 1) % _P + kk
    carry = (lo >= _P).to(torch.int64)
    lo, hi = lo - carry * _P, (base + 1) // _P + carry
    return hi, lo, torch.where(hi > 0, 10 + ndigits(torch, hi), ndigits(torch, lo))


def ord_text(torch, base, k0, k1, fastq_both, device="cpu"):
    """uint8 tensor: the formatted records of the kept ranks k0 .. k1 - 1, one after the other"""
    kk = torch.arange(k0, k1, dtype=torch.int64, device=device)
    hi, lo, w = _ord_parts(torch, base, kk)
    sz = 2 * w + 8 if fastq_both else w + 4
    rec = torch.repeat_interleave(torch.arange(k1 - k0, dtype=torch.int64, device=device), sz)
    off = torch.arange(rec.numel(), dtype=torch.int64, device=device) - (torch.cumsum(sz, 0) - sz)[rec]
    hi, lo, w = hi[rec], lo[rec], w[rec]
    second = off >= w + 5                                      # (FASTQ: the '+' line's copy)
    j = torch.where(second, off - w - 5, off - 1) if fastq_both else off - 1
    p = torch.clamp(w - 1 - j, 0, 19)
    p10 = torch.tensor(_P10[:10], dtype=torch.int64, device=device)
    digit = 48 + torch.where(p < 10, torch.div(lo, p10[torch.clamp(p, 0, 9)], rounding_mode="floor"), torch.div(hi, p10[torch.clamp(p - 10, 0, 9)], rounding_mode="floor")) % 10
    if not fastq_both:
        ch = torch.where(off == 0, 62, torch.where(off <= w, digit, torch.where(off == w + 2, 65, 10)))
    else:
        fixed = torch.where(off == 0, 64, torch.where(off == w + 2, 65, torch.where(off == w + 4, 43, torch.where(off == 2 * w + 6, 73, 10))))
        ch = torch.where(((off >= 1) & (off <= w)) | ((off >= w + 5) & (off <= 2 * w + 4)), digit, fixed)
    return ch.to(torch.uint8)


def ord_index(np_, n, lpr):
    """the line index of n records ORD_RECORD[lpr] as fxg_fastq_index makes it: (line u32 [2 * cap_lines], cap_lines)"""
    cap_lines = lpr * n + 1
    line = np_.zeros(2 * cap_lines, np_.uint32)
    rec = len(ORD_RECORD[lpr])
    r = np_.arange(n, dtype=np_.uint64) * np_.uint64(rec)
    for k in range(lpr):                                       # line k of a record: the prefix line has one byte, the others one too ('+' and 'I')
        line[k:lpr * n:lpr] = r + np_.uint64(2 * k)
        line[cap_lines + k:cap_lines + lpr * n:lpr] = r + np_.uint64(2 * k + 1)
    line[lpr * n] = rec * n
    return line, cap_lines


def crossed(nbytes):
    return tuple(m for m in MARKS if nbytes > (1 << m))


# ---- plain host code: what the windows are compared with ----
def split_lines(text):
    """[(content, line end)] of every line of `text` (bytes), the content cut at its first CR as chomp does"""
    out = []
    for l in bytes(text).split(b"\n")[:-1]:
        cr = l.find(b"\r")
        out.append(l if cr < 0 else l[:cr])
    return out


def _numeric_values(qline):
    return [int(x) for x in qline.split()]


def format_plain(text, lpr, res, fwd_start, out_fasta=False):
    """[bytes per record] of the formatter's forward output for the records of `text`: b"" for a dropped one; a numeric quality line is
    written as its values joined by single blanks (the reference's "%d" output)"""
    lines = split_lines(text)
    out = []
    for r, w in enumerate(res):
        w = int(w)
        if not (w >> 16) & 1:
            out.append(b"")
            continue
        ln = w & 0xFFFF
        name, seq = lines[lpr * r][1:], lines[lpr * r + 1]
        if lpr == 2 or out_fasta:
            out.append(b">" + name + b"\n" + seq[fwd_start:fwd_start + ln] + b"\n")
            continue
        n2, q = lines[lpr * r + 2][1:], lines[lpr * r + 3]
        if len(q) != len(seq):
            q = b" ".join(b"%d" % v for v in _numeric_values(q)[fwd_start:fwd_start + ln])
        else:
            q = q[fwd_start:fwd_start + ln]
        out.append(b"@" + name + b"\n" + seq[fwd_start:fwd_start + ln] + b"\n+" + n2 + b"\n" + q + b"\n")
    return out


def revcomp_plain(text, qoffset=33):
    """[bytes per record] of fastx_reverse_complement's output for the FASTQ records of `text` (character qualities)"""
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    lines = split_lines(text)
    return [b"@" + lines[r][1:] + b"\n" + lines[r + 1].translate(comp)[::-1] + b"\n+" + lines[r + 2][1:] + b"\n" + lines[r + 3][::-1] + b"\n"
            for r in range(0, len(lines), 4)]


_M7F, _M80, _M01 = 0x7F7F7F7F7F7F7F7F, lo._signed(0x8080808080808080), 0x0101010101010101


def _pack8(torch, w):
    """uint8 [k, 8] -> int64 [k], byte i in bits 8 i .."""
    out = torch.zeros(w.shape[0], dtype=torch.int64, device=w.device)
    for i in range(8):
        out |= w[:, i].to(torch.int64) << (8 * i)
    return out


def _zero_bytes(x):
    """number of zero bytes of every int64 of x (exact: no carry passes from byte to byte)"""
    nz = (((x & _M7F) + _M7F) | x) & _M80
    z = ((~nz & _M80) >> 7) & _M01
    return ((z * _M01) >> 56) & 0xFF


def classify_torch(torch, win, F, entries, mismatches, unmatched, chunk=64):
    """bcsplit_model.classify as a torch expression: the first entry with the fewest mismatches, if fewer than BL and <= mismatches.  A window and
    an entry are eight bytes each, compared as one int64: the window is padded with 0x00 behind F, the entry with 0xFF behind its length, so
    padding never equals anything."""
    assert BL == 8
    dev = win.device
    E = len(entries)
    n = win.shape[0]
    if E == 0:
        return torch.full((n,), unmatched, dtype=torch.int64, device=dev)
    tab = np.full((E, BL), 0xFF, dtype=np.uint8)
    tl = np.zeros(E, dtype=np.int64)
    for k, (b, _) in enumerate(entries):
        tab[k, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        tl[k] = len(b)
    tab64, tlen = _pack8(torch, torch.from_numpy(tab).to(dev)), torch.from_numpy(tl).to(dev)
    tbin = torch.tensor([j for _, j in entries], dtype=torch.int64, device=dev)
    pos = torch.arange(BL, dtype=torch.int64, device=dev)
    inF = pos[None, :] < F[:, None]
    w = torch.where(inF, win, 0)
    w64 = _pack8(torch, w)
    isnul = (w == 0) & inF
    nul_behind = torch.stack([(isnul & (pos[None, :] >= Le)).sum(1) for Le in range(BL + 1)], 1)      # [n, BL + 1]: NUL window bytes behind an entry of Le bases
    best = torch.full((n,), (BL << 16) | 0xFFFF, dtype=torch.int64, device=dev)
    for k0 in range(0, E, chunk):
        k1 = min(E, k0 + chunk)
        eq = _zero_bytes(w64[:, None] ^ tab64[None, k0:k1])
        # (a NUL window byte inside F equals no entry base, and no padding)
        mm = F[:, None] - eq - nul_behind[:, tlen[k0:k1]] + (BL - tlen[k0:k1])[None, :]
        key = (mm << 16) | torch.arange(k0, k1, dtype=torch.int64, device=dev)[None, :]
        best = torch.minimum(best, key.min(1).values)
    mm, k = best >> 16, best & 0xFFFF
    ok = (mm < BL) & (mm <= mismatches)
    return torch.where(ok, tbin[torch.clamp(k, max=E - 1)], unmatched)


# ---- window placement by byte position ----
def record_at(torch, starts, byte):
    """the record whose bytes hold `byte` of a stream whose record k starts at starts[k] (int64 [n + 1]); records of no bytes are passed over"""
    k = int(torch.searchsorted(starts, torch.tensor([byte], dtype=starts.dtype, device=starts.device), right=True)[0]) - 1
    return max(0, min(starts.numel() - 2, k))


def windows(torch, n, in_starts, out_starts, seed, k=KI, extra=()):
    """[(label, first record)] in record order: prefix, suffix, one window centred on every crossed mark of the input (in_starts: int64
    [n + 1]) and of each output (out_starts: {name: int64 [n + 1]}), RANDOM_WINDOWS seeded ones, and `extra` [(label, byte, starts)]."""
    k = min(k, n)
    w = [("prefix", 0), ("suffix", n - k)]
    for m in crossed(int(in_starts[-1])):
        w.append(("input 2^%d" % m, lo.window_start(record_at(torch, in_starts, 1 << m), n, k)))
    for name, st in out_starts.items():
        for m in crossed(int(st[-1])):
            w.append(("%s 2^%d" % (name, m), lo.window_start(record_at(torch, st, 1 << m), n, k)))
    for label, byte, st in extra:
        w.append((label, lo.window_start(record_at(torch, st, byte), n, k)))
    if n > 3 * k:
        w += [("random", int(x)) for x in np.random.default_rng(1000 + seed).integers(k, n - 2 * k, size=RANDOM_WINDOWS)]
    return sorted(w, key=lambda x: x[1])
