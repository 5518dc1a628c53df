"""fastx_uncollapser on the MI355X: the C-ABI (fxg_fasta_uncollapse) against the block model of uncollapse_model.py -- counts each side of the
piece marks, record counts each side of the launch tile and the scan block and enough for two scan levels, base counts up to 65 535, a block
walked in windows of every capacity, ordinals across every power of ten, a count of 2^31 - 1 reached through a window, the refusals --
inside poison and canaries; and the tool on the GPU build.  Reads the model and tests/golden/uncollapse only."""
import ctypes as C

import pytest

import uncollapse_model as M
from fastx_toolkit_amd.engine import FxgUncollapseInfo, FxgUncollapseOpts
from uncollapse_cases import (TEXT_MAX, abi_blocks, assert_tool_case, collapsed_text, galaxy_pair, golden_cases, ordinal_blocks, rec, run_tool, two_level_block,
                              window_block)

pytestmark = pytest.mark.gpu

POISON, CANARY, GUARD = 0x5A, 0xA5, 64


class Indexed:
    """a block of records uploaded (16 bytes of poison behind it) and indexed by fxg_fastq_index"""

    def __init__(self, eng, records):
        text = M.block_text(records)
        self.n, self.text_len = len(records), len(text)
        self.d_text = eng.torch.full((len(text) + 16,), POISON, dtype=eng.torch.uint8, device=eng.device)
        self.d_text[:len(text)] = eng.torch.frombuffer(bytearray(text), dtype=eng.torch.uint8).to(eng.device)
        self.ix, self.lens, info = eng.fastq_index(self.d_text, len(text), True, cap_records=len(records), fasta=True)
        assert info.records == len(records) and info.consumed == len(text)


def call(eng, ix, base, copy_begin, out, out_cap, text_len=None):
    """the C-ABI itself: (rc, info, message)"""
    o, info = FxgUncollapseOpts(base, copy_begin, out_cap), FxgUncollapseInfo()
    eng._after_torch()
    rc = eng.lib.fxg_fasta_uncollapse(eng.ctx, ix.d_text.data_ptr(), ix.text_len if text_len is None else text_len, ix.ix.line.data_ptr(), ix.ix.cap_lines, ix.n,
                                      ix.lens.data_ptr(), C.byref(o), out.data_ptr() if out is not None else None, C.byref(info))
    eng._before_torch()
    return rc, info, eng.lib.fxg_last_error(eng.ctx).decode(errors="replace")


def canaried(eng, total, off=0):
    buf = eng.torch.full((GUARD + off + total + GUARD,), CANARY, dtype=eng.torch.uint8, device=eng.device)
    buf[GUARD + off:GUARD + off + total] = POISON
    return buf


def window_call(eng, ix, base, copy_begin, out_cap, off=0):
    """one call into a poisoned d_out of exactly out_cap bytes between canaries: (copy_end, bytes written, info)"""
    buf = canaried(eng, out_cap, off)
    rc, info, msg = call(eng, ix, base, copy_begin, buf[GUARD + off:], out_cap)
    assert rc == 0, msg
    host = buf.cpu().numpy()
    lo = GUARD + off
    assert (host[:lo] == CANARY).all() and (host[lo + out_cap:] == CANARY).all(), "write outside d_out"
    assert (host[lo + info.out_bytes:lo + out_cap] == POISON).all(), "write past out_bytes"
    return info.copy_end, host[lo:lo + info.out_bytes].tobytes(), info


def check_whole(eng, records, base, tag=None, off=0):
    """the block in one call into exactly its bytes, then in windows of about a third of them"""
    blk = M.Block(records, base)
    want = blk.whole()
    ix = Indexed(eng, records)
    end, out, info = window_call(eng, ix, base, 0, len(want), off)
    assert (info.copies, end, info.out_bytes) == (blk.copies, blk.copies, len(want)), tag
    assert out == want, tag
    cap = max(len(want) // 3, max(len(b) for b in blk.bases) + 24)
    got, g = b"", 0
    while g < blk.copies:
        end, out, info = window_call(eng, ix, base, g, cap, off + 3)
        assert end > g, tag
        got, g = got + out, end
    assert got == want, tag


# ---- 1. counts, records, bases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,records,base", abi_blocks(), ids=[b[0] for b in abi_blocks()])
def test_abi_blocks(engine, name, records, base):
    check_whole(engine, records, base, tag=name, off=len(name) % 17)


def test_abi_two_scan_levels(engine):
    """1 050 076 records, more than 1024 * 1024: the scans recurse twice"""
    records, base = two_level_block()
    blk = M.Block(records, base)
    want = blk.whole()
    ix = Indexed(engine, records)
    end, out, info = window_call(engine, ix, base, 0, len(want))
    assert (info.copies, end) == (blk.copies, blk.copies) and out == want


# ---- 2. windows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(19, 24), (24, 40), (40, 80), (80, 201)])
def test_abi_windows_every_capacity(engine, lo, hi):
    """about 300 copies walked with out_cap of exactly the largest copy (19 bytes), one byte more, and every size up to 200: copy_end and out_bytes
    as the model says each time, d_out written up to out_bytes and no further, the windows concatenated equal the one-call output"""
    tc = engine.torch
    records, base = window_block()
    blk = M.Block(records, base)
    whole = blk.whole()
    ix = Indexed(engine, records)
    assert max(len(blk.copy_of(g)) for g in range(blk.copies)) == 19
    for cap in range(lo, hi):
        exact = cap in (19, 20, 39, 79, 200)                  # these walks look at every window between its canaries
        buf = tc.full((GUARD + len(whole) + cap + GUARD,), CANARY, dtype=tc.uint8, device=engine.device)
        buf[GUARD:GUARD + len(whole)] = POISON
        g, pos = 0, 0
        while g < blk.copies:
            want_end, want = blk.window(g, cap)
            if exact:
                end, out, info = window_call(engine, ix, base, g, cap, off=pos % 5)
                assert out == want, (cap, g)
            else:                                             # the windows land one behind the other in one array, looked at once
                rc, info, msg = call(engine, ix, base, g, buf[GUARD + pos:], cap)
                assert rc == 0, msg
                end = info.copy_end
            assert (end, info.out_bytes, info.copies) == (want_end, len(want), blk.copies), (cap, g)
            g, pos = end, pos + len(want)
        assert pos == len(whole)
        if not exact:
            host = buf.cpu().numpy()
            assert host[GUARD:GUARD + len(whole)].tobytes() == whole, cap
            assert (host[:GUARD] == CANARY).all() and (host[GUARD + len(whole):] == CANARY).all(), cap


# ---- 3. ordinals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 20))
def test_abi_ordinals_cross_a_power_of_ten(engine, k):
    """9 -> 10, 99 -> 100, ..., 10^19 - 1 -> 10^19: between two records, inside a record's first piece, inside a further piece"""
    blocks = [b for b in ordinal_blocks() if b[0].startswith("k%d_" % k)]
    assert len(blocks) == (2 if k == 1 else 3)
    for name, records, base in blocks:
        check_whole(engine, records, base, tag=name)


# ---- 4. a large count -------------------------------------------------------------------------------------------------------------------
def test_abi_large_count_through_a_window(engine):
    """one record with count 2^31 - 1, written only through windows of a few copies: at copy 2 000 000 000 the byte offset is above 2^35"""
    records = [rec(0, 3, 5), (b"big-2147483647", b"ACGTNACGTN"), rec(2, 2, 4)]
    blk = M.Block(records, 0)
    ix = Indexed(engine, records)
    for g0, cap in ((0, 200), (2000000000, 100), (blk.copies - 4, 1000), (3 + 2147483647 - 1, 50)):
        end, out, info = window_call(engine, ix, 0, g0, cap)          # (the calls with copy_begin > 0 reuse the scans the first one made)
        assert (info.copies, end, out) == (blk.copies,) + blk.window(g0, cap), g0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_abi_refusals(engine):
    records, base = window_block()
    blk = M.Block(records, base)
    ix = Indexed(engine, records)
    first = len(blk.copy_of(0))
    buf = engine.torch.full((256,), CANARY, dtype=engine.torch.uint8, device=engine.device)

    def untouched():
        return bool((buf == CANARY).all())

    rc, _, msg = call(engine, ix, base, 0, buf, first - 1)                            # one byte short of the next copy
    assert rc == -1 and "needs %d bytes" % first in msg and "takes %d" % (first - 1) in msg and untouched()
    rc, info, msg = call(engine, ix, base, 0, buf, first)                             # exactly enough
    assert rc == 0 and (info.copy_end, info.out_bytes) == (1, first) and buf[:first].cpu().numpy().tobytes() == blk.copy_of(0), msg
    assert bool((buf[first:] == CANARY).all())
    buf[:] = CANARY
    rc, _, msg = call(engine, ix, base, blk.copies + 1, buf, 100)
    assert rc == -1 and "copy_begin" in msg and untouched()
    rc, _, msg = call(engine, ix, (1 << 64) - blk.copies, 0, buf, 100)                # the last number would be 2^64
    assert rc == -1 and "2^64" in msg and untouched()
    rc, info, msg = call(engine, ix, (1 << 64) - 1 - blk.copies, 0, buf, 100)         # ... and 2^64 - 1 is a number
    assert rc == 0 and info.copies == blk.copies, msg
    rc, info, msg = call(engine, ix, (1 << 64) - 1 - blk.copies, blk.copies - 1, buf, 100)
    last = b">18446744073709551615\n" + blk.bases[-1] + b"\n"
    assert rc == 0 and buf[:info.out_bytes].cpu().numpy().tobytes() == last, msg
    buf[:] = CANARY
    rc, _, msg = call(engine, ix, base, 0, buf, 100, text_len=TEXT_MAX + 1)
    assert rc == -1 and "at most" in msg and untouched()
    rc, info, msg = call(engine, ix, base, 0, buf, 100)
    assert rc == 0, msg
    buf[:] = CANARY
    rc, info, msg = call(engine, ix, base, blk.copies, buf, 0)                        # the empty call
    assert rc == 0 and (info.copies, info.copy_end, info.out_bytes) == (blk.copies, blk.copies, 0) and untouched(), msg
    rc, info, msg = call(engine, ix, base, blk.copies, None, 0)
    assert rc == 0 and info.out_bytes == 0, msg
    other = Indexed(engine, records[:5])                                              # a window of a block the context holds no scans of
    rc, _, msg = call(engine, other, base, 1, buf, 100)
    assert rc == -1 and "continues a block" in msg and untouched()


def test_engine_binding(engine):
    records, base = window_block()
    blk = M.Block(records, base)
    ix = Indexed(engine, records)
    out = engine.torch.empty(1000, dtype=engine.torch.uint8, device=engine.device)
    got, g = b"", 0
    while g < blk.copies:
        view, info = engine.fasta_uncollapse(ix.d_text, ix.text_len, ix.ix, ix.n, ix.lens, out, ordinal_base=base, copy_begin=g)
        got, g = got + view.cpu().numpy().tobytes(), info.copy_end
    assert got == blk.whole()


# ---- 6. the tool on the GPU build ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_tool_recorded_case(case):
    assert_tool_case(None, case)


def test_tool_galaxy_pair():
    src, want = galaxy_pair()
    assert run_tool(None, [], src)[:2] == (0, want)
    code, out, err, outfile = run_tool(None, ["-v"], src, files=True)
    assert (code, outfile, err, out) == (0, want, "", M.report(12, 42))


def test_tool_many_blocks():
    """2 MB of collapsed text in 1 MB blocks and 1 MB windows against the model, report included; then with a lower-case record near the end,
    which hands the rest of the input to the record API"""
    text = collapsed_text(2 << 20)
    want, status, seqs, reads = M.uncollapse_whole(text)
    code, out, err, _ = run_tool(None, ["-v"], text, {"FXH_READ_BUFFER_MB": "1"})
    assert code == 0, err
    assert out == want and err.encode() == M.report(seqs, reads)
    bad = text + b">x-3\nacgt\n>y-2\nAC\n"
    code, out, err, _ = run_tool(None, [], bad, {"FXH_READ_BUFFER_MB": "1"})
    assert code == 1 and out == want
    assert "found invalid nucleotide sequence (acgt) on line %d" % (text.count(b"\n") + 2) in err
