"""GPU tier (-m gpu -k context_state): the collapser's set -- an arena and three per-record arrays that move when they grow, a table that is swapped on a
rebuild, result words shared by four entries, the order's arrays carved from one block -- among everything else a context does, and fxg_bases_change on a
buffer the set has copied from.  Outputs lie between canaries and text before 16 poison bytes (test_gpu_collapse.write, Indexed); the set's output is compared
exactly with the reference's recorded bytes (golden/collapser/cases.json: dups, ties, seeded), every foreign call with its own oracle or model through the
Runner of test_gpu_context_state.py.

  a  three sets in turn on one context, a call of another family between every two adds and before every window (collapse_state_sequence.py; its CPU half
     holds the list against the grow rule: text_ws, rf_ws and status are reallocated while a set is alive)
  b  fxg_bases_change on the very buffer a block was added from, then the next block in the same buffer: the set holds the original bases
  c  one text buffer, one line array and one length array for every block, at the same addresses, as host/fxh_collapse.c uses them
  d  sets in succession: large, begin while ordered with 4 slots, begin with more slots than the context's table holds, large again
  e  two contexts with a set each, calls strictly alternating; two threads with a context each
  f  an irregular block after the arena has been reallocated, foreign calls around it
  g  the profiling ring after an add that rebuilt the table and after an add refused at a request check
"""
import ctypes as C
import threading
import zlib

import numpy as np
import pytest

import collapse_cases as CK
import collapse_model as M
import collapse_state_sequence as Q
import context_state_sequence as S
import nucchange_model as NM
import test_gpu_collapse as GC
import test_gpu_context_state as CS
from fastx_toolkit_amd.engine import NO_RECORD, FxgBasesChangeInfo, FxgCollapseInfo, FxgTextInfo

pytestmark = pytest.mark.gpu

POISON = GC.POISON
IRR_BASE = GC.IRR_BASE


# ---- references, made once (no GPU needed) ----------------------------------------------------------------------------------------------------------
_ref = {}


def case_records(name):
    return [c for c in CK.abi_cases() if c[0] == name][0][1]


def expected_info(blocks, initial=0):
    """info after order for [(text, records)] blocks, by the model and the documented growth rule.  Cached under the texts' lengths and checksums: the
    seeded case takes the model a second, and seven tests ask for it"""
    key = (tuple((len(t), n, zlib.crc32(t)) for t, n in blocks), initial)
    if key not in _ref:
        sums, steps, records, reads = {}, [], 0, 0
        for text, n in blocks:
            steps.append((len(sums), n))
            for name, bases in M.records_of(text):
                c = M.get_reads_count(name)
                sums[bases] = (sums.get(bases, 0) + c) & M.M64
                reads += c
            records += n
        slots, rebuilds = CK.slots_after(initial, steps)
        _ref[key] = dict(records=records, reads=reads & M.M64, uniques=len(sums), slots=slots, rebuilds=rebuilds, out_reads=M.out_reads(sums), out_bytes=M.out_bytes(sums))
    return _ref[key]


class Block:
    """a block's text uploaded (16 bytes of poison behind it) and indexed by `eng`: what GC.add takes"""

    def __init__(self, eng, text, n):
        T = eng.torch
        self.n, self.text_len = n, len(text)
        self.d_text = T.full((len(text) + 16,), POISON, dtype=T.uint8, device=eng.device)
        self.d_text[:len(text)] = T.frombuffer(bytearray(text), dtype=T.uint8).to(eng.device)
        self.ix, self.lens, self.info = eng.fastq_index(self.d_text, len(text), True, cap_records=n, fasta=True)
        assert (self.info.records, self.info.consumed) == (n, len(text))


def add_ok(eng, blk, what=""):
    rc, info = GC.add(eng, blk)
    assert rc == 0 and info.irregular == 0 and info.first_bad == NO_RECORD, (what, GC.message(eng))
    return info


def order_ok(eng, want, what=""):
    rc, info = GC.order(eng)
    assert rc == 0, (what, GC.message(eng))
    assert {k: getattr(info, k) for k in want} == want, what
    return info


def windows(eng, info, cap, between=None):
    out, rank = [], 0
    while rank < info.uniques:
        if between:
            between()
        _, got, w = GC.write(eng, rank, cap, off=rank % 5)
        assert w.rank_end > rank
        out.append(got)
        rank = w.rank_end
    return b"".join(out)


def whole_set(eng, name, blocks, initial=0, cap=None):
    """begin .. write of a recorded case on `eng`, nothing between: info by the model, the bytes the reference's"""
    assert GC.begin(eng, initial) == 0, GC.message(eng)
    for text, n in blocks:
        add_ok(eng, Block(eng, text, n), name)
    info = order_ok(eng, expected_info(blocks, initial), name)
    CK.assert_output(name, windows(eng, info, cap or info.out_bytes))
    return info


# ---- a. the set among all families ------------------------------------------------------------------------------------------------------------------
class SetRunner(CS.Runner):
    """the Runner of the context-state tier with the collapser's four calls as steps"""
    cl = None

    def do_cl_begin(self, st):
        assert GC.begin(self.eng) == 0, GC.message(self.eng)
        ways = dict(Q.CASES)[st["case"]]
        self.cl = dict(case=st["case"], blocks=Q.case_blocks(st["case"], ways), rank=0, out=[], records=0, info=None)

    def do_cl_add(self, st):
        text, n = self.cl["blocks"][st["block"]]
        info = add_ok(self.eng, Block(self.eng, text, n), st["label"])
        self.cl["records"] += n
        assert info.records == self.cl["records"], st["label"]

    def do_cl_order(self, st):
        self.cl["info"] = order_ok(self.eng, expected_info(self.cl["blocks"]), st["label"])

    def do_cl_write(self, st):
        _, got, w = GC.write(self.eng, self.cl["rank"], st["cap"], off=st["window"] % 7)
        assert w.rank_end > self.cl["rank"] or self.cl["rank"] == self.cl["info"].uniques, st["label"]
        self.cl["out"].append(got)
        self.cl["rank"] = w.rank_end

    def case_done(self):
        return self.cl["rank"] == self.cl["info"].uniques


def test_context_state_collapse_set_among_all_families(monkeypatch):
    steps = Q.build()
    with CS.fresh_engine(monkeypatch) as eng:
        run = SetRunner(eng, monkeypatch)
        recov, extra = eng.scan_recoveries(), 0
        try:
            for k, st in enumerate(steps):
                run.step(st)
                if st["kind"] == "cl_write" and (k + 1 == len(steps) or steps[k + 1].get("where") != "windows"):          # the case's last listed window
                    while not run.case_done():
                        for g in S.annotate(Q.gap(Q.EXTRA + extra)):
                            run.step(g)
                        extra += 1
                        run.step(dict(kind="cl_write", case=st["case"], window=st["window"] + extra, cap=st["cap"], label="%s.extra%d" % (st["case"], extra)))
                    CK.assert_output(st["case"], b"".join(run.cl["out"]))
            for label in list(run.results):                   # counters no later gap has read
                run.finish(label)
            run.step(dict(kind="uc", block=Q.U_BLOCK, parts=Q.UC_PARTS, rest=True, label="end.uc"))          # the walk that began before the first set, to its end
            assert eng.scan_recoveries() == recov and extra <= 3
        finally:
            run.close()


# ---- b. the caller's buffer is not the set's ----------------------------------------------------------------------------------------------------------
def test_context_state_collapse_keeps_its_own_copy_of_the_bases(monkeypatch):
    records = case_records("dups")
    halves = CK.split(records, 2)
    blocks = [(M.block_text(h), len(h)) for h in halves]
    with CS.fresh_engine(monkeypatch) as eng:
        T = eng.torch
        cap = max(len(t) for t, _ in blocks)
        buf = T.full((cap + 16,), POISON, dtype=T.uint8, device=eng.device)
        assert GC.begin(eng) == 0, GC.message(eng)
        for k, (text, n) in enumerate(blocks):
            buf[:] = POISON
            buf[:len(text)] = T.frombuffer(bytearray(text), dtype=T.uint8).to(eng.device)
            blk = Block.__new__(Block)
            blk.n, blk.text_len, blk.d_text = n, len(text), buf
            blk.ix, blk.lens, blk.info = eng.fastq_index(buf, len(text), True, cap_records=n, fasta=True)
            assert (blk.info.records, blk.info.consumed, blk.info.irregular) == (n, len(text), 0)
            add_ok(eng, blk, "block %d" % k)
            if k == 0:                                        # T -> U in the buffer the set has just read
                model = NM.Block(halves[0], "r")
                info = FxgBasesChangeInfo()
                eng._after_torch()
                rc = eng.lib.fxg_bases_change(eng.ctx, buf.data_ptr(), len(text), 2, blk.ix.line.data_ptr(), blk.ix.cap_lines, n, ord("T"), ord("U"), C.byref(info))
                assert rc == 0 and (info.changed, info.first_to_record, info.irregular) == (model.changed, NO_RECORD, 0), GC.message(eng)
                assert model.changed > 1000
                host = buf.cpu().numpy()
                assert host[:len(text)].tobytes() == model.rewritten and (host[len(text):] == POISON).all()
        info = order_ok(eng, expected_info(blocks))
        CK.assert_output("dups", windows(eng, info, info.out_bytes))


# ---- c. one buffer and one line array for every block --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties", "seeded"])
def test_context_state_collapse_reused_buffers_at_one_address(monkeypatch, name):
    blocks = Q.case_blocks(name, dict(Q.CASES)[name])
    with CS.fresh_engine(monkeypatch) as eng:
        T = eng.torch
        cap_text, cap_records = max(len(t) for t, _ in blocks), max(n for _, n in blocks)
        cap_lines = 2 * cap_records + 1
        buf = T.full((cap_text + 16,), POISON, dtype=T.uint8, device=eng.device)
        line = T.zeros(2 * cap_lines, dtype=T.int32, device=eng.device)
        lens = T.empty(cap_records, dtype=T.int16, device=eng.device)
        flags = T.zeros(cap_records, dtype=T.uint8, device=eng.device)
        assert GC.begin(eng) == 0, GC.message(eng)
        for k, (text, n) in enumerate(blocks):
            buf[:len(text)] = T.frombuffer(bytearray(text), dtype=T.uint8).to(eng.device)
            buf[len(text):] = POISON                          # (what an earlier, longer block left behind this one is no part of it)
            ti = FxgTextInfo()
            eng._after_torch()
            rc = eng.lib.fxg_fastq_index(eng.ctx, buf.data_ptr(), len(text), 1, 2, line.data_ptr(), cap_lines, lens.data_ptr(), flags.data_ptr(), C.byref(ti))
            assert rc == 0 and (ti.records, ti.consumed, ti.irregular) == (n, len(text), 0), (k, GC.message(eng))
            info = FxgCollapseInfo()
            rc = eng.lib.fxg_collapse_add(eng.ctx, buf.data_ptr(), len(text), 2, line.data_ptr(), cap_lines, n, lens.data_ptr(), C.byref(info))
            assert rc == 0 and info.irregular == 0, (k, GC.message(eng))
        info = order_ok(eng, expected_info(blocks), name)
        CK.assert_output(name, windows(eng, info, Q.window_cap(name)))


# ---- d. sets in succession --------------------------------------------------------------------------------------------------------------------------------
def test_context_state_collapse_sets_in_succession(monkeypatch):
    seeded = Q.case_blocks("seeded", 0)
    ties = [(M.block_text(case_records("ties")), len(case_records("ties")))]
    dups = Q.case_blocks("dups", 5)
    with CS.fresh_engine(monkeypatch) as eng:
        big = whole_set(eng, "seeded", seeded, cap=Q.ONE_MB)
        assert big.slots > CK.DEFAULT_SLOTS and big.rebuilds >= 1
        # begin while ordered: the windows are gone, and four slots of the large table serve a tiny case
        assert GC.begin(eng, 4) == 0, GC.message(eng)
        rc, _, _ = GC.write(eng, 0, 4096, must=False)
        assert rc == -1 and "the set is not ordered; fxg_collapse_order comes first" in GC.message(eng)
        small = whole_set(eng, "ties", ties, initial=4)
        assert small.slots < big.slots and small.rebuilds >= 1
        # more slots than the table the context holds: a new table
        many = 4 * big.slots
        info = whole_set(eng, "dups", dups, initial=many)
        assert (info.slots, info.rebuilds) == (many, 0)
        again = whole_set(eng, "seeded", seeded, cap=Q.ONE_MB)
        assert (again.slots, again.rebuilds, again.uniques, again.out_bytes) == (big.slots, big.rebuilds, big.uniques, big.out_bytes)
        # a begin between order and write
        assert GC.begin(eng) == 0
        add_ok(eng, Block(eng, *ties[0]))
        order_ok(eng, expected_info(ties))
        assert GC.begin(eng) == 0
        rc, _, _ = GC.write(eng, 0, 4096, must=False)
        assert rc == -1 and "the set is not ordered; fxg_collapse_order comes first" in GC.message(eng)


# ---- e. two contexts, two threads ----------------------------------------------------------------------------------------------------------------------
def test_context_state_collapse_two_contexts_alternating(monkeypatch):
    work = [("dups", Q.case_blocks("dups", 5)), ("ties", Q.case_blocks("ties", 5))]
    with CS.fresh_engine(monkeypatch) as a, CS.fresh_engine(monkeypatch) as b:
        engines = (a, b)
        for e in engines:
            assert GC.begin(e) == 0, GC.message(e)
        for j in range(5):
            for e, (name, blocks) in zip(engines, work):
                add_ok(e, Block(e, *blocks[j]), (name, j))
        infos = [order_ok(e, expected_info(blocks), name) for e, (name, blocks) in zip(engines, work)]
        outs, ranks = [[], []], [0, 0]
        while any(r < i.uniques for r, i in zip(ranks, infos)):
            for k, e in enumerate(engines):
                if ranks[k] < infos[k].uniques:
                    _, got, w = GC.write(e, ranks[k], Q.window_cap(work[k][0]), off=k)
                    assert w.rank_end > ranks[k]
                    outs[k].append(got)
                    ranks[k] = w.rank_end
        for k in (0, 1):
            assert len(outs[k]) >= 3
            CK.assert_output(work[k][0], b"".join(outs[k]))


def test_context_state_collapse_two_threads_one_context_each(monkeypatch):
    """the seeded case in 1 MB blocks on two contexts at once: texts, line arrays and the expected info made before the threads start"""
    blocks = Q.case_blocks("seeded", 0)
    want = expected_info(blocks)
    with CS.fresh_engine(monkeypatch) as a, CS.fresh_engine(monkeypatch) as b:
        engines = (a, b)
        outs, failures = [None, None], []
        a.torch.cuda.synchronize()

        def loop(t):
            try:
                e = engines[t]
                assert GC.begin(e) == 0, GC.message(e)
                for text, n in blocks:
                    add_ok(e, Block(e, text, n), "thread %d" % t)
                info = order_ok(e, want, "thread %d" % t)
                outs[t] = windows(e, info, Q.ONE_MB)
            except BaseException as err:      # reported after the join
                failures.append((t, repr(err)))
        threads = [threading.Thread(target=loop, args=(t,), daemon=True) for t in (0, 1)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(120)
        assert not any(th.is_alive() for th in threads), "a thread did not finish"
        assert not failures, failures
        for t in (0, 1):
            CK.assert_output("seeded", outs[t])


# ---- f. an irregular block, a regrown arena, foreign calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,records", CK.irregular_blocks(), ids=["context_state_" + b[0] for b in CK.irregular_blocks()])
def test_context_state_collapse_irregular_block_among_foreign_calls(monkeypatch, name, records):
    good = [(CK.ident(i), CK.seq(i % 5, 33)) for i in range(300)]
    large = Q.case_blocks("seeded", 0)[0]                     # 1 MB behind 3 KB of bases: the arena moves
    bad_at = M.block_irregular(records)
    blocks = [(M.block_text(good[:100]), 100), large, (M.block_text(good[100:]), 200)]
    with CS.fresh_engine(monkeypatch) as eng:
        run = CS.Runner(eng, monkeypatch)
        try:
            clean = whole_set_bytes(eng, blocks)
            assert GC.begin(eng) == 0
            bad = GC._index_raw(eng, records)
            add_ok(eng, Block(eng, *blocks[0]))
            run.step(dict(kind="reflow", lines=2000, width=60, label="f.reflow"))
            add_ok(eng, Block(eng, *blocks[1]))               # reallocates the arena and the per-record arrays
            run.step(dict(kind="stats", n=2000, label="f.stats"))
            rc, info = GC.add(eng, bad)
            assert (rc, info.irregular, info.first_bad, info.records) == (0, IRR_BASE, bad_at, 100 + large[1]), GC.message(eng)
            run.step(S._run("rows38", 3000, "f.run"))         # a foreign call before the next good block
            add_ok(eng, Block(eng, *blocks[2]))
            rc, info = GC.add(eng, bad)
            assert (rc, info.irregular, info.first_bad, info.records) == (0, IRR_BASE, bad_at, 300 + large[1]), GC.message(eng)
            info = order_ok(eng, expected_info(blocks), name)
            out = windows(eng, info, info.out_bytes)
            assert out == clean
            M.check_against(b"".join(t for t, _ in blocks), out)
        finally:
            run.close()


def whole_set_bytes(eng, blocks):
    assert GC.begin(eng) == 0, GC.message(eng)
    for text, n in blocks:
        add_ok(eng, Block(eng, text, n))
    info = order_ok(eng, expected_info(blocks))
    return windows(eng, info, info.out_bytes)


# ---- g. the profiling ring --------------------------------------------------------------------------------------------------------------------------------
def test_context_state_collapse_profiled_intervals(monkeypatch):
    """include/fxg.h: add records an interval for lengths + scan + copy + check, one for a rebuild if the block caused one, one for the insert; order two;
    write one; a refused call launches nothing, so the ring is after it what it was before.  (An interval that fxg_cl_add opens and leaves through an error return is not counted: the ring's count moves
    only when an interval closes, so the next interval records over the same pair of events.  Such a return needs a failing HIP call and is not provoked here.)"""
    records = [(CK.ident(i), CK.seq(i, 24)) for i in range(40)]
    with CS.fresh_engine(monkeypatch) as eng:
        first, second = Block(eng, M.block_text(records[:8]), 8), Block(eng, M.block_text(records[8:]), 32)
        assert GC.begin(eng, 16) == 0
        eng.set_profiling(True)                               # (the ring starts empty: the index calls above are not in it)
        info = add_ok(eng, first)
        assert (info.slots, info.rebuilds) == (16, 0) and len(eng.profiled_kernel_ms()) == 2
        eng.set_profiling(True)
        info = add_ok(eng, second)                            # 2 x (8 + 32) > 16: the table is rebuilt
        assert (info.slots, info.rebuilds) == CK.slots_after(16, [(0, 8), (8, 32)]) and info.rebuilds == 1
        ms = eng.profiled_kernel_ms()
        assert len(ms) == 3 and all(m >= 0.0 for m in ms)
        rc, refused = GC.add(eng, second, lpr=3)              # refused at a request check: the ring stays as the add before left it
        assert rc == -1 and "lines_per_record 3" in GC.message(eng) and eng.profiled_kernel_ms() == ms
        assert (refused.records, refused.reads, refused.uniques, refused.slots, refused.rebuilds) == (info.records, info.reads, info.uniques, info.slots, info.rebuilds)
        assert (refused.irregular, refused.first_bad) == (0, NO_RECORD)          # (include/fxg.h: a call refused for its arguments leaves the set's counts)
        rc, info = GC.order(eng)
        assert rc == 0 and len(eng.profiled_kernel_ms()) == 5 and eng.profiled_kernel_ms()[:3] == ms
        _, out, _ = GC.write(eng, 0, info.out_bytes)
        assert len(eng.profiled_kernel_ms()) == 6
        M.check_against(M.block_text(records), out)
        eng.set_profiling(False)
