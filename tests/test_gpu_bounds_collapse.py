"""Bounds tier, GPU half, for the two entries that read a caller's indexed block: fxg_collapse_add and fxg_bases_change with every input array a view of
EXACTLY its size inside poison, in the manner of emu_py._tight --

  d_text   text_len bytes and the 16 bytes of slack include/fxg.h grants behind them, poison from the 17th byte on;
  d_line   the lines the call may read and no more: with cap_lines = lpr * n + 1, the starts of lines 0 .. lpr * n and the ends of lines 0 .. lpr * n - 1,
           that is 2 * cap_lines - 1 words (the last word of the 2 * cap_lines array is the end of a line the block does not have);
  d_len    n values.

Poison is 0x5A: 'Z' as a base (outside every alphabet, so a read that reaches a check makes the block irregular), 23 130 as a length, an offset far outside
the text as a line mark.  A read past an array therefore changes a result, and the results must equal collapse_model / nucchange_model and, where the case is
recorded, the reference's bytes.  d_out of fxg_collapse_write is exact already (test_gpu_collapse.write: between canaries).  Records per block: 1, 255 (one
short of a workgroup of the insert launch) and TRIP + 1 (a second trip of the copy launch, for one record)."""
import ctypes as C

import numpy as np
import pytest

import collapse_cases as K
import collapse_model as M
import nucchange_model as NM
import test_gpu_collapse as GC
from fastx_toolkit_amd.engine import NO_RECORD, FxgBasesChangeInfo, FxgCollapseInfo

pytestmark = pytest.mark.gpu

POISON, PAD = 0x5A, 4096
SIZES = [1, 255, K.TRIP + 1]


def tight(eng, src, nbytes, end_aligned=False):
    """`nbytes` bytes of the device tensor `src` (a uint8 view) copied into the middle of a poisoned allocation: the view begins on a 16-byte boundary
    (the text and the line arrays of fxg_fastq_index do), or -- end_aligned -- ends on one, so that both ends of an array meet poison inside one piece"""
    T = eng.torch
    lead = PAD + ((-nbytes) % 16 if end_aligned else 0)
    buf = T.full((lead + nbytes + PAD,), POISON, dtype=T.uint8, device=eng.device)
    buf[lead:lead + nbytes] = src.view(T.uint8).reshape(-1)[:nbytes]
    return buf, buf[lead:lead + nbytes]


def poison_intact(buf, view):
    lead = view.data_ptr() - buf.data_ptr()
    return bool((buf[:lead] == POISON).all()) and bool((buf[lead + view.numel():] == POISON).all())


class TightBlock:
    """a block indexed by fxg_fastq_index into arrays of its own, then copied into exact-size views"""

    def __init__(self, eng, text, n, lpr=2):
        T = eng.torch
        self.n, self.text_len, self.lpr, self.cap_lines = n, len(text), lpr, lpr * n + 1
        d = T.full((len(text) + 16,), 0x20, dtype=T.uint8, device=eng.device)
        d[:len(text)] = T.frombuffer(bytearray(text), dtype=T.uint8).to(eng.device)
        ix, lens, info = eng.fastq_index(d, len(text), True, cap_records=n, fasta=lpr == 2)
        assert (info.records, info.consumed, info.irregular) == (n, len(text), 0) and ix.cap_lines == self.cap_lines
        eng.sync()
        self.slack = d[len(text):].cpu().numpy().copy()
        self.bufs = [tight(eng, d, len(text) + 16), tight(eng, ix.line, 4 * (2 * self.cap_lines - 1)), tight(eng, lens, 2 * n, end_aligned=True)]
        self.d_text, self.d_line, self.d_len = (v for _, v in self.bufs)

    def check(self, what):
        assert all(poison_intact(b, v) for b, v in self.bufs), what + ": a write into the poison around an input"


def collapse_records(n):
    if n == 1:
        return [(b"only-7", K.seq(3, 36))]
    return [c for c in K.abi_cases() if c[0] == "records_%d" % n][0][1]


@pytest.mark.parametrize("n", SIZES)
def test_bounds_collapse_add_exact_arrays(engine, n):
    eng = engine
    records = collapse_records(n)
    text = M.block_text(records)
    blk = TightBlock(eng, text, n)
    assert GC.begin(eng) == 0, GC.message(eng)
    info = FxgCollapseInfo()
    eng._after_torch()
    rc = eng.lib.fxg_collapse_add(eng.ctx, blk.d_text.data_ptr(), blk.text_len, 2, blk.d_line.data_ptr(), blk.cap_lines, n, blk.d_len.data_ptr(), C.byref(info))
    assert rc == 0 and (info.irregular, info.first_bad, info.records) == (0, NO_RECORD, n), GC.message(eng)
    blk.check("collapse_add")
    assert blk.d_text[:blk.text_len].cpu().numpy().tobytes() == text           # (add reads the caller's text, it never writes it)
    rc, info = GC.order(eng)
    want = GC.expected_info([records], False, 0)
    assert rc == 0 and {k: getattr(info, k) for k in want} == want, GC.message(eng)
    _, out, w = GC.write(eng, 0, info.out_bytes)
    assert w.rank_end == info.uniques
    M.check_against(text, out)
    if n > 1:
        K.assert_output("records_%d" % n, out)


def change_records(n):
    """bases of 1 to 40 letters with T in every position class, ids of every width modulo 16, one record in seven all T"""
    return [(K.ident(i), b"T" * (1 + i % 40) if i % 7 == 0 else K.seq(i, 1 + (i * 11) % 40)) for i in range(n)]


@pytest.mark.parametrize("n", SIZES)
def test_bounds_bases_change_exact_arrays(engine, n):
    eng = engine
    records = change_records(n)
    model = NM.Block(records, "r")
    assert model.changed > 0 and model.first_to == NM.NONE and not model.irregular
    blk = TightBlock(eng, model.text, n)
    info = FxgBasesChangeInfo()
    eng._after_torch()
    rc = eng.lib.fxg_bases_change(eng.ctx, blk.d_text.data_ptr(), blk.text_len, 2, blk.d_line.data_ptr(), blk.cap_lines, n, ord("T"), ord("U"), C.byref(info))
    assert rc == 0, GC.message(eng)
    assert (info.changed, info.first_to_record, info.irregular) == (model.changed, NO_RECORD, 0)
    blk.check("bases_change")
    host = blk.d_text.cpu().numpy()
    assert host[:blk.text_len].tobytes() == model.rewritten                    # every T of a bases line, and no byte outside the bases lines
    assert np.array_equal(host[blk.text_len:], blk.slack)                      # the 16 bytes behind the text stay
