"""fastx_collapser on the MI355X: the C-ABI (fxg_collapse_begin / _add / _order / _write) on every case of collapse_cases.py against the
reference's recorded outputs -- text in front of 16 poison bytes, d_out of exactly out_bytes between canaries, info field by field, every
case twice on one context and once on a fresh context as its first calls -- the irregular blocks, the refusals with untouched outputs,
the seeded 300 000-read case, and the tool on the GPU build.  Reads the model and tests/golden/collapser only."""
import ctypes as C

import pytest

import collapse_cases as K
import collapse_model as M
from fastx_toolkit_amd.engine import NO_RECORD, FxgCollapseInfo, FxgCollapseOpts, FxgCollapseWindow

pytestmark = pytest.mark.gpu

POISON, CANARY, GUARD = 0x5A, 0xA5, 64
IRR_BASE = 0x10             # FXG_TEXT_IRR_BASE


class Indexed:
    """a block of records uploaded (16 bytes of poison behind it) and indexed by fxg_fastq_index"""

    def __init__(self, eng, records, fastq=False):
        text = M.block_text(records, fastq)
        self.n, self.text_len = len(records), len(text)
        self.d_text = eng.torch.full((len(text) + 16,), POISON, dtype=eng.torch.uint8, device=eng.device)
        self.d_text[:len(text)] = eng.torch.frombuffer(bytearray(text), dtype=eng.torch.uint8).to(eng.device)
        self.ix, self.lens, self.info = eng.fastq_index(self.d_text, len(text), True, cap_records=len(records), fasta=not fastq)
        assert self.info.records == len(records) and self.info.consumed == len(text)


def message(eng):
    return eng.lib.fxg_last_error(eng.ctx).decode(errors="replace")


def begin(eng, initial=0, bits=0):
    return eng.lib.fxg_collapse_begin(eng.ctx, C.byref(FxgCollapseOpts(initial, bits)))


def add(eng, ix, lpr=None, text=True, text_len=None, cap_lines=None, n=None):
    """the C-ABI itself: (rc, info)"""
    info = FxgCollapseInfo()
    eng._after_torch()
    rc = eng.lib.fxg_collapse_add(eng.ctx, ix.d_text.data_ptr() if text else None, ix.text_len if text_len is None else text_len, ix.ix.lpr if lpr is None else lpr,
                                  ix.ix.line.data_ptr(), ix.ix.cap_lines if cap_lines is None else cap_lines, ix.n if n is None else n, ix.lens.data_ptr(), C.byref(info))
    return rc, info


def order(eng):
    info = FxgCollapseInfo()
    return eng.lib.fxg_collapse_order(eng.ctx, C.byref(info)), info


def write(eng, rank_begin, out_cap, off=0, must=True):
    """one window into a poisoned d_out of exactly out_cap bytes between canaries: (rc, bytes written, window)"""
    buf = eng.torch.full((GUARD + off + out_cap + GUARD,), CANARY, dtype=eng.torch.uint8, device=eng.device)
    buf[GUARD + off:GUARD + off + out_cap] = POISON
    w = FxgCollapseWindow()
    eng._after_torch()
    rc = eng.lib.fxg_collapse_write(eng.ctx, rank_begin, out_cap, buf[GUARD + off:].data_ptr(), C.byref(w))
    eng._before_torch()
    host = buf.cpu().numpy()
    lo = GUARD + off
    assert (host[:lo] == CANARY).all() and (host[lo + out_cap:] == CANARY).all(), "write outside d_out"
    assert (host[lo + w.out_bytes:lo + out_cap] == POISON).all(), "write past out_bytes"
    if must:
        assert rc == 0, message(eng)
    else:
        assert rc == 0 or (host[lo:lo + out_cap] == POISON).all(), "a refused call wrote to d_out"
    return rc, host[lo:lo + w.out_bytes].tobytes(), w


def expected_info(blocks, fastq, initial):
    """what the set's info says after the blocks, by the model and the documented growth rule"""
    seen, steps, recs = {}, [], []
    for blk in blocks:
        steps.append((len(seen), len(blk)))
        blk = [(M.chomp(n), M.chomp(b)) for n, b in blk]
        recs += blk
        seen.update((b, 1) for _, b in blk)
    sums = M.collapse(recs, fastq)
    slots, rebuilds = K.slots_after(initial, steps)
    reads = sum(M.get_reads_count(n, fastq) for n, _ in recs) & M.M64
    return dict(records=len(recs), reads=reads, uniques=len(sums), slots=slots, rebuilds=rebuilds, out_reads=M.out_reads(sums), out_bytes=M.out_bytes(sums))


def run_blocks(eng, blocks, fastq=False, initial=0, bits=0, windows=None, off=0):
    """begin, the blocks, order, and the whole output in one window of exactly its bytes (or in windows of `windows` bytes).  Returns (out, info)."""
    assert begin(eng, initial, bits) == 0, message(eng)
    for blk in blocks:
        rc, info = add(eng, Indexed(eng, blk, fastq))
        assert rc == 0 and info.irregular == 0 and info.first_bad == NO_RECORD, message(eng)
    rc, info = order(eng)
    assert rc == 0, message(eng)
    want = expected_info(blocks, fastq, initial)
    assert {k: getattr(info, k) for k in want} == want
    out, rank = b"", 0
    while rank < info.uniques:
        _, got, w = write(eng, rank, windows or info.out_bytes, off)
        assert w.rank_end > rank
        out, rank = out + got, w.rank_end
    assert len(out) == info.out_bytes
    rc, got, w = write(eng, info.uniques, 0)               # the empty call
    assert (rc, got, w.rank_end, w.out_bytes) == (0, b"", info.uniques, 0)
    return out, info


def _variants():
    for name, records, fastq, ways, opts in K.abi_cases():
        for w in ways:
            for initial, bits in opts:
                yield pytest.param(name, records, fastq, w, initial, bits, id="%s-%dblocks-slots%d-bits%d" % (name, w, initial, bits))


# ---- 1. every shared case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,records,fastq,ways,initial,bits", _variants())
def test_abi_cases(engine, name, records, fastq, ways, initial, bits):
    """the whole output against the reference's recorded one, then once more on the same context in windows: begin resets everything"""
    out, _ = run_blocks(engine, K.split(records, ways), fastq, initial, bits, off=len(name) % 17)
    K.assert_output(name, out)
    out2, _ = run_blocks(engine, K.split(records, ways), fastq, initial, bits, windows=max(len(out) // 3, max(len(b) for _, b in records) + 40), off=3)
    assert out2 == out
    from fastx_toolkit_amd import Engine
    fresh = Engine(0)                                      # and as a new context's first calls: nothing depends on an earlier entry having run
    try:
        out3, _ = run_blocks(fresh, K.split(records, ways), fastq, initial, bits)
        assert out3 == out
    finally:
        fresh.close()


def test_abi_growth_from_four_slots(engine):
    """4 slots growing to 4 096 through ten rebuilds (ten doublings), one per block from the third block on"""
    records, sizes = K.growth_case()
    out, info = run_blocks(engine, K.split_sizes(records, sizes), initial=4)
    K.assert_output("growth", out)
    assert (info.slots, info.rebuilds, info.uniques) == (4096, 10, 2048)


@pytest.mark.parametrize("name,records,sizes", K.threshold_cases(), ids=[c[0] for c in K.threshold_cases()])
def test_abi_growth_threshold(engine, name, records, sizes):
    out, info = run_blocks(engine, K.split_sizes(records, sizes), initial=64)
    K.assert_output(name, out)
    for n, want in ((31, (64, 0)), (32, (64, 0)), (33, (128, 1))):          # the first block alone: 2 x 31 and 2 x 32 fit 64 slots, 2 x 33 do not
        if n == sizes[0]:
            _, info = run_blocks(engine, [records[:n]], initial=64)
            assert (info.slots, info.rebuilds) == want


# ---- 2. windows -------------------------------------------------------------------------------------------------------------------------
def test_abi_windows_after_every_record(engine):
    """an out_cap that ends a window after every record of a small case in turn, and one byte less, which ends it a record earlier"""
    records = [c for c in K.abi_cases() if c[0] == "ties"][0][1]
    whole, info = run_blocks(engine, [records])
    sizes = [len(M.record_text(r, c, b)) for r, c, b in M.parse_output(whole)]
    assert sum(sizes) == len(whole)
    for k in range(1, len(sizes) + 1):
        rc, got, w = write(engine, 0, sum(sizes[:k]), off=k % 7)
        assert (w.rank_end, got) == (k, whole[:sum(sizes[:k])]), k
        rc, got, w = write(engine, 0, sum(sizes[:k]) - 1, must=False)
        if k == 1:
            assert rc == -1 and "rank 0 needs %d bytes, d_out takes %d" % (sizes[0], sizes[0] - 1) in message(engine)
        else:
            assert (rc, w.rank_end, got) == (0, k - 1, whole[:sum(sizes[:k - 1])]), k
        rc, got, w = write(engine, k - 1, sizes[k - 1])
        assert (w.rank_end, got) == (k, whole[sum(sizes[:k - 1]):sum(sizes[:k])]), k


# ---- 3. irregular blocks and refusals -----------------------------------------------------------------------------------------------------
def _index_raw(eng, records):
    """a block with a bad record, uploaded and indexed without the checks of Indexed: the index itself may flag it (an empty bases line)"""
    ix = Indexed.__new__(Indexed)
    text = M.block_text(records)
    ix.n, ix.text_len = len(records), len(text)
    ix.d_text = eng.torch.full((len(text) + 16,), POISON, dtype=eng.torch.uint8, device=eng.device)
    ix.d_text[:len(text)] = eng.torch.frombuffer(bytearray(text), dtype=eng.torch.uint8).to(eng.device)
    ix.ix, ix.lens, ix.info = eng.fastq_index(ix.d_text, len(text), True, cap_records=len(records), fasta=True)
    return ix


@pytest.mark.parametrize("name,records", K.irregular_blocks(), ids=[b[0] for b in K.irregular_blocks()])
def test_abi_irregular_block_leaves_the_set_as_it_was(engine, name, records):
    good = [(K.ident(i), K.seq(i % 5, 33)) for i in range(300)]
    bad_at = M.block_irregular(records)
    want, want_info = run_blocks(engine, [good[:100], good[100:]])
    assert begin(engine) == 0
    bad = _index_raw(engine, records)
    rc, info = add(engine, bad)                            # the first block of an empty set
    assert (rc, info.irregular, info.first_bad, info.records, info.uniques) == (0, IRR_BASE, bad_at, 0, 0), message(engine)
    rc, info = add(engine, Indexed(engine, good[:100]))
    assert rc == 0 and info.irregular == 0 and info.records == 100
    rc, info = add(engine, bad)
    assert (rc, info.irregular, info.first_bad, info.records, info.reads) == (0, IRR_BASE, bad_at, 100, 100), message(engine)
    rc, info = add(engine, Indexed(engine, good[100:]))
    assert rc == 0 and info.irregular == 0
    rc, info = order(engine)
    assert rc == 0 and all(getattr(info, k) == getattr(want_info, k) for k in ("records", "reads", "uniques", "out_reads", "out_bytes"))
    _, got, _ = write(engine, 0, info.out_bytes)
    assert got == want


def test_abi_refusals():
    """the refusal table on a context of its own, from its first call on: the code and the text, the set and d_out untouched"""
    from fastx_toolkit_amd import Engine
    eng = Engine(0)
    try:
        recs = [(K.ident(i), K.seq(i, 20)) for i in range(10)]
        ix = Indexed(eng, recs)
        said = {}
        said["add_before_begin"] = (add(eng, ix)[0], message(eng))
        said["order_before_begin"] = (order(eng)[0], message(eng))
        said["write_before_begin"] = (write(eng, 0, 100, must=False)[0], message(eng))
        said["hash_bits_65"] = (begin(eng, 0, 65), message(eng))
        assert begin(eng) == 0
        said["write_before_order"] = (write(eng, 0, 100, must=False)[0], message(eng))
        said["lines_per_record_3"] = (add(eng, ix, lpr=3)[0], message(eng))
        said["null_text"] = (add(eng, ix, text=False)[0], message(eng))
        said["too_many_lines"] = (add(eng, ix, cap_lines=20)[0], message(eng))
        said["text_too_long"] = (add(eng, ix, text_len=0xFFFFFFF1)[0], message(eng))
        said["records_do_not_fit"] = (add(eng, ix, text_len=39)[0], message(eng))
        rc, info = add(eng, ix)
        assert rc == 0 and info.records == 10              # the refused calls left nothing behind
        rc, info = order(eng)
        assert rc == 0 and info.uniques == 10
        said["add_after_order"] = (add(eng, ix)[0], message(eng))
        said["order_after_order"] = (order(eng)[0], message(eng))
        said["rank_begin_past_end"] = (write(eng, 11, 100, must=False)[0], message(eng))
        first = 20 + 6
        said["out_cap_too_small"] = (write(eng, 0, first - 1, must=False)[0], message(eng))
        for name, text in K.REFUSALS:
            rc, msg = said[name]
            assert rc == -1 and (text % (first, first - 1) if "%d" in text else text) in msg, (name, rc, msg)
        assert set(said) == {n for n, _ in K.REFUSALS}
        _, got, w = write(eng, 0, info.out_bytes)          # the set is still there
        assert len(got) == info.out_bytes and w.rank_end == 10
        M.check_against(M.block_text(recs), got)
    finally:
        eng.close()


def test_engine_binding(engine):
    records = [c for c in K.abi_cases() if c[0] == "counts"][0][1]
    engine.collapse_begin()
    for blk in K.split(records, 2):
        ix = Indexed(engine, blk)
        info = engine.collapse_add(ix.d_text, ix.text_len, ix.ix, ix.n, ix.lens)
        assert not info.irregular
    info = engine.collapse_order()
    out = engine.torch.empty(200, dtype=engine.torch.uint8, device=engine.device)
    got, rank = b"", 0
    while rank < info.uniques:
        view, w = engine.collapse_write(rank, out)
        got, rank = got + view.cpu().numpy().tobytes(), w.rank_end
    K.assert_output("counts", got)


# ---- 4. the seeded case -------------------------------------------------------------------------------------------------------------------
def test_abi_seeded_case_in_1mb_blocks(engine):
    """300 000 reads of 36 to 50 bases from 40 000 templates with a skewed draw, about 14 MB of text in blocks of 1 MB, against its recorded md5"""
    text = K.seeded_text()
    assert begin(engine) == 0
    at = 0
    while at < len(text):
        end = len(text) if len(text) - at <= 1 << 20 else text.rfind(b"\n>", at, at + (1 << 20)) + 1
        blk = text[at:end]
        d_text = engine.torch.full((len(blk) + 16,), POISON, dtype=engine.torch.uint8, device=engine.device)
        d_text[:len(blk)] = engine.torch.frombuffer(bytearray(blk), dtype=engine.torch.uint8).to(engine.device)
        ix, lens, ti = engine.fastq_index(d_text, len(blk), True, fasta=True)
        assert ti.irregular == 0 and ti.consumed == len(blk)
        info = engine.collapse_add(d_text, len(blk), ix, ti.records, lens)
        assert not info.irregular
        at = end
    info = engine.collapse_order()
    assert (info.records, info.reads, info.out_reads) == (300000, 300000, 300000)
    out, rank = [], 0
    buf = engine.torch.empty(1 << 20, dtype=engine.torch.uint8, device=engine.device)
    while rank < info.uniques:
        view, w = engine.collapse_write(rank, buf)
        out.append(view.cpu().numpy().tobytes())
        rank = w.rank_end
    K.assert_output("seeded", b"".join(out))


# ---- 5. the tool on the GPU build ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.golden_cli(), ids=lambda c: c["name"])
def test_tool_recorded_case(case):
    K.assert_tool_case(None, case, {"FXH_READ_BUFFER_MB": "1"})


def test_tool_galaxy_pair_and_seeded_case():
    src, want = K.galaxy_pair()
    code, out, err, _ = K.run_tool(None, [], src, {"FXH_READ_BUFFER_MB": "1"})
    assert code == 0 and M.same_up_to_ties(out, want), err
    K.assert_output("galaxy", out)
    code, out, err, outfile = K.run_tool(None, ["-v"], K.seeded_text(), {"FXH_READ_BUFFER_MB": "1"}, files=True)
    assert code == 0 and err == "", err
    K.assert_output("seeded", outfile)
    assert out.decode() == "Input: 300000 sequences (representing 300000 reads)\nOutput: %d sequences (representing 300000 reads)\n" % outfile.count(b">")
