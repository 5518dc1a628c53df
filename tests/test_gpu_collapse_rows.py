"""fxg_collapse_add_rows and fastx_clip_collapser on the MI355X.  The main property is equivalence with the text entry: a block goes through
fxg_fastq_index, fxg_fastq_pack and fxg_run_pipeline with the clip stage; its kept rows go into set A through the new entry, and the same kept
reads, formatted to text by fxg_fastq_format and indexed again, go into set B through fxg_collapse_add on a second context.  After order the
infos must be equal field by field and the written bytes equal over windows that end after every record.  Poison lies behind every input: the
text, the packed rows' bytes past the kept ones, and the entries of out_off / out_len / kept_index past the kept count.  Then the shapes at which
the copy can go wrong (rows made on the host, against the text entry too), the zero-length rule, the refusal table, the binding, and the tool
against the recorded answers of the reference pipe and against this project's own clipper and collapser run as two processes."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import collapse_cases as K
import collapse_model as M
import collapse_rows_cases as RC
import test_collapse_rows_cpu as TC
from fastx_toolkit_amd import make_params
from fastx_toolkit_amd.engine import NO_RECORD, FxgCollapseInfo, FxgCollapseOpts, FxgCollapseWindow
from test_gpu_collapse import Indexed, message, order, write

pytestmark = pytest.mark.gpu

POISON = 0x5A
IRR_BASE = RC.IRR_BASE
AD = RC.golden()["adapter"].encode()
FIELDS = TC.FIELDS


@pytest.fixture(scope="module")
def second():
    """set B's context"""
    from fastx_toolkit_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def fields(info):
    return {k: getattr(info, k) for k in FIELDS}


def begin(eng, initial=0, bits=0):
    assert eng.lib.fxg_collapse_begin(eng.ctx, C.byref(FxgCollapseOpts(initial, bits))) == 0, message(eng)


def poisoned(eng, data):
    t = eng.torch.full((len(data) + 16,), POISON, dtype=eng.torch.uint8, device=eng.device)
    if len(data):
        t[:len(data)] = eng.torch.frombuffer(bytearray(data), dtype=eng.torch.uint8).to(eng.device)
    return t


def insert(key, n=None):
    rng = random.Random(key)
    return bytes(rng.choice(b"ACGT") for _ in range(n or 18 + key % 11))


def clip_read(key, i, length=60, adapter=True):
    """a read whose bases up to the adapter depend on `key` alone and whose bases behind it depend on i: reads of one key differ before clipping
    and are equal after it"""
    rng = random.Random(1000003 * i + 7)
    tail = bytes(rng.choice(b"ACGT") for _ in range(length))
    return (insert(key) + (AD if adapter else b"") + tail)[:length]


class Clipped:
    """a FASTA block through index, pack and fxg_run_pipeline with the clip stage, its compacted outputs poisoned beforehand"""

    def __init__(self, eng, records, flags=1, min_len=5):
        T = eng.torch
        text = M.block_text(records)
        self.records, self.n, self.text_len = records, len(records), len(text)
        self.d_text = poisoned(eng, text)
        self.ix, self.lens, ti = eng.fastq_index(self.d_text, len(text), True, cap_records=len(records), fasta=True)
        assert ti.records == len(records) and not ti.irregular
        stride = ti.max_len
        bases, _, irr = eng.fastq_pack(self.d_text, len(text), self.ix, self.n, stride, want_qual=False)
        assert irr == 0
        out = eng.alloc_outputs(self.n, stride, True, True, False)
        for k in ("out_bases", "out_len", "kept_index", "out_off"):
            out[k].view(T.uint8).fill_(POISON)
        p = make_params(stages=1, adapter=AD, clip_min_len=min_len, clip_flags=flags)
        self.result = eng.run(bases, None, p, lens=None if ti.min_len == ti.max_len else self.lens, fixed_len=ti.max_len, outputs=out)
        self.kept = self.result.kept
        self.kept_text = eng.fastq_format(self.d_text, len(text), self.ix, self.n, res=self.result.res).cpu().numpy().tobytes()


def kept_records(text):
    lines = text.split(b"\n")[:-1]
    return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines), 2)]


def add_text(eng, records):
    ix = Indexed(eng, records)
    info = FxgCollapseInfo()
    eng._after_torch()
    rc = eng.lib.fxg_collapse_add(eng.ctx, ix.d_text.data_ptr(), ix.text_len, 2, ix.ix.line.data_ptr(), ix.ix.cap_lines, ix.n, ix.lens.data_ptr(), C.byref(info))
    assert rc == 0 and not info.irregular, message(eng)
    return info


def finish_both(a, b, every_record=True):
    """order on both, every field equal, bytes equal: whole, and over windows that end after every record"""
    rc_a, ia = order(a)
    rc_b, ib = order(b)
    assert rc_a == 0 and rc_b == 0, (message(a), message(b))
    assert fields(ia) == fields(ib)
    if ia.uniques == 0:
        return b"", ia
    _, out_a, _ = write(a, 0, ia.out_bytes, off=5)
    _, out_b, _ = write(b, 0, ib.out_bytes)
    assert out_a == out_b
    if every_record:
        sizes = [len(M.record_text(r, c, s)) for r, c, s in M.parse_output(out_b)]
        ends = np.cumsum(sizes)
        for k in ([int(e) for e in ends] if len(sizes) <= 80 else [int(ends[j]) for j in range(0, len(sizes), max(1, len(sizes) // 40))]):
            _, ga, wa = write(a, 0, k, off=k % 16)
            _, gb, wb = write(b, 0, k)
            assert ga == gb == out_b[:k] and wa.rank_end == wb.rank_end
    return out_a, ia


def dup_records(n=1500):
    """equal after clipping in neighbouring lanes, within a wave, across the waves of a workgroup, across workgroups and -- in 2 or 5 blocks -- across
    blocks; collapsed ids of several forms; some reads without the adapter, which -c drops between the kept ones; one insert a prefix of another"""
    recs = []
    ids = [b"r%d", b"r%d-5", b"r%d-", b"r%d-0", b"r%d-3", b"x-%d"]
    for i in range(n):
        key = i // 2 if i < 200 else (i - 200) % 50 if i < 600 else i % 257 if i < 1200 else i
        name = ids[i % len(ids)] % i
        if i % 7 == 3:
            recs.append((b"gone%d-%d" % (i, 900 + i), clip_read(key, i, adapter=False)))
        elif i % 97 == 5:
            recs.append((name, (insert(4)[:12] + AD + clip_read(0, i))[:60]))          # insert(4)[:12]: a proper prefix of key 4's reads
        else:
            recs.append((name, clip_read(key, i)))
    return recs


@pytest.mark.parametrize("ways,mixed,initial,bits,first,last", [(1, False, 0, 0, 1, 0), (2, False, 0, 0, 1, 0), (5, False, 0, 1, 1, 0), (5, True, 0, 0, 1, 0), (2, True, 4, 0, 1, 0),
                                                                (1, False, 4, 0, 1, 0), (2, False, 0, 0, 2, 19), (5, True, 4, 1, 1, 15), (1, False, 0, 0, 25, 0)])
def test_rows_of_a_clipped_block_equal_its_formatted_text(engine, second, ways, mixed, initial, bits, first, last):
    records = dup_records()
    begin(engine, initial, bits), begin(second, initial, bits)
    for k, blk in enumerate(K.split(records, ways)):
        c = Clipped(engine, blk)
        assert 0 < c.kept < c.n
        kept = kept_records(c.kept_text)
        assert len(kept) == c.kept
        want = TC.trimmed(kept, first, last)
        if mixed and k % 2 == 1:
            ia = add_text(engine, want)
        else:
            ia = engine.collapse_add_rows(c.result, d_text=c.d_text, ix=c.ix, first_base=first, last_base=last)
            assert not ia.irregular and ia.first_bad == NO_RECORD
        ib = add_text(second, want)
        assert (ia.records, ia.reads, ia.uniques) == (ib.records, ib.reads, ib.uniques)
    out, info = finish_both(engine, second)
    assert info.uniques < info.records < len(records) and info.reads > info.records


def test_a_block_that_keeps_nothing_between_two_regular_ones(engine, second):
    good = [(b"g%d-2" % i, clip_read(i % 9, i)) for i in range(300)]
    none = [(b"n%d-9" % i, (b"ACG" + AD + clip_read(i, i))[:60]) for i in range(40)]      # three bases in front of the adapter: too short, every one
    begin(engine), begin(second)
    for blk in (good[:150], none, good[150:]):
        c = Clipped(engine, blk)
        ia = engine.collapse_add_rows(c.result, d_text=c.d_text, ix=c.ix)
        if blk is none:
            assert c.kept == 0 and (ia.records, ia.reads) == (150, 300)
        else:
            add_text(second, kept_records(c.kept_text))
    finish_both(engine, second)


def test_counts_come_from_the_kept_records_own_id(engine, second):
    ids = [b"x-5", b"x-", b"x-0", b"x-abc", b"1-2-3", b"nodash", b"x- 7", b"x--4", b"x-+9", b"a-2000000000", b"b-2000000000", b"c-4294967297"]
    recs = []
    for k, name in enumerate(ids * 3):
        recs.append((b"gone-%d" % (40 + k), (b"ACG" + AD + clip_read(k, k))[:60]))     # too short: dropped, with a count of its own, before every kept one
        recs.append((name, clip_read(k % 4, k)))
    begin(engine), begin(second)
    c = Clipped(engine, recs)
    assert c.kept == len(ids) * 3
    ia = engine.collapse_add_rows(c.result, d_text=c.d_text, ix=c.ix)
    assert ia.reads == sum(M.get_reads_count(n, False) for n in ids * 3) & M.M64
    add_text(second, kept_records(c.kept_text))
    finish_both(engine, second)
    begin(engine)                                                                   # without the count source every record counts 1
    assert engine.collapse_add_rows(c.result).reads == c.kept


# ---- rows made on the host: the shapes ----------------------------------------------------------------------------------------------------
class HostRows:
    """packed rows with gaps (every d_off residue), lower-case bytes between them and poison behind them, and the count source of collapse_rows_cases.with_dropped"""

    def __init__(self, eng, records, source=True):
        recs = RC.chomped(records)
        bases, off, lens = RC.pack_rows([b for _, b in recs], lead=len(records) % 16)
        T = eng.torch
        self.n = len(recs)
        self.bases = poisoned(eng, bases.tobytes())
        up = lambda a, dt: T.from_numpy(np.concatenate([a.view(dt), np.frombuffer(bytes([POISON]) * 32, dtype=dt)])).to(eng.device)      # (poison behind the entries)
        self.off, self.len = up(off, np.int64), up(lens, np.int16)
        self.ix = self.kept = None
        if source:
            block, kept = RC.with_dropped(records)
            self.ix, self.kept = Indexed(eng, block), up(kept, np.int32)


def add_rows(eng, r, n=None, bases=True, off=True, lens=True, kept=True, text=True, line=True, cap_lines=None, lpr=None, first=1, last=0):
    """the C-ABI itself: (rc, info)"""
    info = FxgCollapseInfo()
    p = lambda t, on: t.data_ptr() if (on and t is not None) else None
    ix = r.ix
    eng._after_torch()
    rc = eng.lib.fxg_collapse_add_rows(eng.ctx, p(r.bases, bases), p(r.off, off), p(r.len, lens), r.n if n is None else n, first, last, p(r.kept, kept),
                                       p(ix.d_text, text) if ix else None, p(ix.ix.line, line) if ix else None, (ix.ix.cap_lines if ix else 0) if cap_lines is None else cap_lines,
                                       (ix.ix.lpr if ix else 0) if lpr is None else lpr, C.byref(info))
    return rc, info


def host_case(engine, second, blocks, initial=0, bits=0, every_record=False):
    begin(engine, initial, bits), begin(second, initial, bits)
    for blk in blocks:
        rc, info = add_rows(engine, HostRows(engine, blk))
        assert rc == 0 and not info.irregular and info.first_bad == NO_RECORD, message(engine)
        if blk:
            add_text(second, blk)
    return finish_both(engine, second, every_record)


@pytest.mark.parametrize("n", RC.RECORDS)
def test_record_counts(engine, second, n):
    good = [(b"g%d" % i, K.seq(1000 + i, 20)) for i in range(5)]
    host_case(engine, second, [good, [(K.ident(i, 1 + i % 3), K.seq(i % 5003, 18 + i % 23)) for i in range(n)], good])


@pytest.mark.parametrize("L", RC.LENGTHS)
def test_lengths(engine, second, L):
    records = [c for c in K.abi_cases() if c[0] == "len_%d" % L][0][1]
    out, _ = host_case(engine, second, [records], every_record=True)
    K.assert_output("len_%d" % L, out)


@pytest.mark.parametrize("initial,bits", [(0, 0), (0, 1), (4, 0)])
def test_offsets_at_every_residue_prefixes_and_a_rebuild(engine, second, initial, bits):
    records = RC.residue_case() + RC.prefix_case()
    _, info = host_case(engine, second, [records[:30], records[30:]], initial, bits, every_record=True)
    assert (info.rebuilds > 0) == (initial == 4)


@pytest.mark.parametrize("name", ["dups", "counts", "ties", "records_%d" % (K.TRIP + 1)])
def test_recorded_cases_as_rows(engine, second, name):
    _, records, fastq, ways, opts = [c for c in K.abi_cases() if c[0] == name][0]
    out, _ = host_case(engine, second, K.split(records, ways[-1]), opts[-1][0], opts[-1][1])
    K.assert_output(name, out)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_zero_length_row_leaves_the_set_as_it_was(engine, second, where):
    good = [(K.ident(i), K.seq(i % 5, 33)) for i in range(300)]
    bad = [(K.ident(i), K.seq(i, 17)) for i in range(40)]
    at = {"first": 0, "middle": 17, "last": 39}[where]
    bad[at] = (b"bad", b"")
    if where == "middle":
        bad[29] = (b"bad2", b"")
    begin(engine), begin(second)
    rows = HostRows(engine, bad)
    rc, info = add_rows(engine, rows)                       # the first call on an empty set
    assert (rc, info.irregular, info.first_bad, info.records, info.uniques, info.reads) == (0, IRR_BASE, at, 0, 0, 0), message(engine)
    rc, info = add_rows(engine, HostRows(engine, good[:100]))
    assert rc == 0 and info.records == 100
    rc, info = add_rows(engine, rows)
    assert (rc, info.irregular, info.first_bad, info.records, info.reads, info.uniques) == (0, IRR_BASE, at, 100, 100, 5)
    rc, info = add_rows(engine, HostRows(engine, good[100:]))
    assert rc == 0 and not info.irregular
    add_text(second, good[:100]), add_text(second, good[100:])
    finish_both(engine, second)


def test_refusals():
    """the refusal table on a context of its own, from its first call on: the code and the text, the set's counts unchanged after every one"""
    from fastx_toolkit_amd import Engine
    eng = Engine(0)
    try:
        recs = [(K.ident(i, 2), K.seq(i, 20)) for i in range(10)]
        rows, plain = HostRows(eng, recs), HostRows(eng, recs, source=False)

        class S:
            message = property(lambda self: message(eng))

            def add_rows(self, r, **kw):
                return add_rows(eng, r, **kw)
        rc, info = add_rows(eng, rows)
        said = {"rows_before_begin": (rc, message(eng), info)}
        assert (info.records, info.first_bad) == (0, NO_RECORD)
        begin(eng)
        rc, info = add_rows(eng, rows)
        assert rc == 0 and (info.records, info.reads) == (10, 20)
        said.update(TC.refusal_calls(S(), rows, plain))
        for name in said:
            if name != "rows_before_begin":
                i = said[name][2]
                assert (i.records, i.reads, i.uniques, i.irregular, i.first_bad) == (10, 20, 10, 0, NO_RECORD), name
        rc, info = add_rows(eng, rows, n=0)                # records == 0: a valid call that changes nothing
        assert rc == 0 and (info.records, info.reads) == (10, 20)
        rc, info = add_rows(eng, rows)
        assert rc == 0 and (info.records, info.reads, info.uniques) == (20, 40, 10)
        rc, info = order(eng)
        assert rc == 0 and info.uniques == 10
        rc, refused = add_rows(eng, rows)
        said["rows_after_order"] = (rc, message(eng), refused)
        for name, text in TC.REFUSALS:
            rc, msg, _ = said[name]
            assert rc == -1 and text in msg, (name, rc, msg)
        assert set(said) == {n for n, _ in TC.REFUSALS}
        _, got, w = write(eng, 0, info.out_bytes)          # the set is still there
        assert w.rank_end == 10
        M.check_against(M.block_text(recs + recs), got)
    finally:
        eng.close()


def test_profiling_records_the_text_entrys_intervals(engine):
    """three intervals for a block that forces a rebuild, as fxg_collapse_add records them"""
    records = [(K.ident(i), K.seq(i, 24)) for i in range(100)]
    begin(engine, 4)
    rows = HostRows(engine, records)
    engine._check(engine.lib.fxg_set_profiling(engine.ctx, 1))
    try:
        rc, info = add_rows(engine, rows)
        assert rc == 0 and info.rebuilds == 1
        ms, n = (C.c_float * 16)(), C.c_uint32()
        engine._check(engine.lib.fxg_profiled_kernel_ms(engine.ctx, ms, 16, C.byref(n)))
        assert n.value == 3
    finally:
        engine._check(engine.lib.fxg_set_profiling(engine.ctx, 0))


def test_engine_binding(engine):
    recs = [(b"a-3", clip_read(1, 1)), (b"b", clip_read(2, 2, adapter=False)), (b"c-4", clip_read(1, 3)), (b"d", clip_read(5, 4))]
    c = Clipped(engine, recs)
    engine.collapse_begin()
    info = engine.collapse_add_rows(c.result, d_text=c.d_text, ix=c.ix)
    assert (info.records, info.reads, info.uniques) == (3, 8, 2)
    info = engine.collapse_add_rows((c.result.out_bases, c.result.out_off, c.result.out_len), n=c.kept, first_base=2, last_base=10)
    assert (info.records, info.reads, info.uniques) == (6, 11, 4)
    info = engine.collapse_order()
    out = engine.torch.empty(400, dtype=engine.torch.uint8, device=engine.device)
    view, w = engine.collapse_write(0, out)
    assert w.rank_end == 4 and view.cpu().numpy().tobytes().startswith(b">1-7\n" + insert(1) + b"\n")


# ---- the tool on the GPU build ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RC.golden_cases(), ids=lambda c: c["name"])
def test_tool_recorded_case(case):
    RC.assert_golden_case(None, case, {"FXH_READ_BUFFER_MB": "1"})


def test_tool_equals_this_projects_own_pipe_on_a_seeded_input(tmp_path):
    """about 300 000 reads: the same bytes and the same -v text as fastx_clipper | fastx_collapser run as two processes"""
    text, argv = RC.seeded_clip_input()
    code, report, err, out = RC.run_tool(None, argv, text, {"FXH_READ_BUFFER_MB": "1"})
    assert code == 0 and err == "", err
    bin_ = os.path.dirname(RC.TOOL)
    src, mid = tmp_path / "in.fq", tmp_path / "mid.fq"
    src.write_bytes(text)
    p1 = subprocess.run([os.path.join(bin_, "fastx_clipper"), "-v"] + argv + ["-i", str(src), "-o", str(mid)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    p2 = subprocess.run([os.path.join(bin_, "fastx_collapser"), "-v", "-i", str(mid)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert (p1.returncode, p2.returncode) == (0, 0), (p1.stderr, p2.stderr)
    assert out == p2.stdout and report == p1.stdout + p2.stderr
    assert out.count(b">") > 1000
