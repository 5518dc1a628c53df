"""GPU tier: launch shapes of the collapser that no recorded case reaches (generators, closed forms and the arithmetic of each shape: tests/collapse_shapes.py,
pinned on the CPU tier by tests/test_collapse_shapes_cpu.py).

  trips       the slot launches (init, rebuild, mark, scatter) take further trips above 2^24 slots: a table of 2^25 slots rebuilt into 2^26 by one block of
              2^24 + 1 records made on the device
  boundary    the insert launch stages a workgroup's span of the arena in LDS when it fits FXG_CL_STAGE_BYTES: spans of exactly 49 152 bytes (staged) and
              49 168 (not), and one block whose workgroups alternate between the two
  contention  2^20 identical reads among 1 000 singletons: every workgroup's lanes on one slot, the count summed through atomics past 2^32 and up to 2^51,
              and 2^14 records with hash_bits = 1 (two probe chains for everything)

Expected values come from collapse_model and the closed forms, never from the engine."""
import numpy as np
import pytest

import collapse_cases as CK
import collapse_model as M
import collapse_shapes as SH
import test_gpu_collapse as GC
from fastx_toolkit_amd.engine import NO_RECORD

pytestmark = pytest.mark.gpu

POISON = GC.POISON


class DeviceBlock:
    """a block whose text is already a device tensor (text_len bytes and 16 of poison), indexed by `eng`: what GC.add takes"""

    def __init__(self, eng, d_text, text_len, n):
        self.d_text, self.text_len, self.n = d_text, text_len, n
        self.ix, self.lens, self.info = eng.fastq_index(d_text, text_len, True, cap_records=n, fasta=True)
        assert (self.info.records, self.info.consumed, self.info.irregular) == (n, text_len, 0)


def upload(eng, text):
    T = eng.torch
    d = T.full((len(text) + 16,), POISON, dtype=T.uint8, device=eng.device)
    d[:len(text)] = T.frombuffer(bytearray(text), dtype=T.uint8).to(eng.device)
    return d


def whole_output(eng, info):
    _, out, w = GC.write(eng, 0, info.out_bytes)
    assert w.rank_end == info.uniques and len(out) == info.out_bytes
    return out


# ---- trips ------------------------------------------------------------------------------------------------------------------------------------------------
def test_slot_launches_in_several_trips():
    from fastx_toolkit_amd import Engine
    eng = Engine(0)
    try:
        T, dev = eng.torch, eng.device
        NT, N, L = SH.TRIPS_NT, SH.TRIPS_N, SH.TRIPS_L
        W = SH.row_width(L)
        table = SH.bases_of(T, T.arange(NT), L, SH.TRIPS_SEED, dev)
        assert GC.begin(eng, SH.TRIPS_SLOTS) == 0, GC.message(eng)          # 805 MB of slots: init in two trips
        small = T.full((NT * W + 16,), POISON, dtype=T.uint8, device=dev)
        small[:NT * W] = SH.rows(T, T.arange(NT, dtype=T.int64, device=dev), table).reshape(-1)
        rc, info = GC.add(eng, DeviceBlock(eng, small, NT * W, NT))
        assert rc == 0 and (info.irregular, info.uniques, info.slots, info.rebuilds) == (0, NT, SH.TRIPS_SLOTS, 0), GC.message(eng)
        big = T.full((N * W + 16,), POISON, dtype=T.uint8, device=dev)
        slab = 1 << 21
        for r0 in range(0, N, slab):
            r1 = min(r0 + slab, N)
            big[r0 * W:r1 * W] = SH.trips_block(T, r0, r1, table, dev).reshape(-1)
        rc, info = GC.add(eng, DeviceBlock(eng, big, N * W, N))
        assert rc == 0 and (info.irregular, info.first_bad) == (0, NO_RECORD), GC.message(eng)
        assert (info.records, info.reads, info.uniques, info.slots, info.rebuilds) == (NT + N, NT + N, NT, 1 << 26, 1)          # rebuild in two trips, init in four
        del big
        rc, info = GC.order(eng)                                             # mark and scatter in four trips
        assert rc == 0 and (info.uniques, info.slots, info.rebuilds, info.out_reads) == (NT, 1 << 26, 1, NT + N), GC.message(eng)
        host = table.cpu()
        sums = {bytes(host[t].tolist()): 1 + c for t, c in enumerate(SH.trips_counts(N))}
        assert info.out_bytes == M.out_bytes(sums)
        SH.check_sums(sums, whole_output(eng, info))
    finally:
        eng.close()


# ---- the staging boundary ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [16, 17, 31])
def test_staging_boundary_spans_of_49152_and_49168_bytes(engine, lead):
    blocks = SH.boundary_case(lead)
    spans = SH.staged_spans([[len(b) for _, b in blk] for blk in blocks])
    assert sorted(s for s, _ in spans[1] + spans[3]) == [SH.STAGE_BYTES, SH.STAGE_BYTES + 16]
    out, info = GC.run_blocks(engine, blocks)
    M.check_against(b"".join(M.block_text(b) for b in blocks), out)
    assert engine.last_launch()["kernel"] == "fxg_kernel_cl_write"


def test_staging_alternates_between_workgroups(engine):
    blocks = SH.alternating_case()
    assert [st for _, st in SH.staged_spans([[len(b) for _, b in blocks[0]]])[0]] == [True, False] * 3
    out, info = GC.run_blocks(engine, blocks)
    M.check_against(M.block_text(blocks[0]), out)


# ---- contention -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,count,bits", [(1 << 20, 4100, 0), (1 << 20, (1 << 31) - 1, 0), (1 << 14, 4100, 1)], ids=["past_2_32", "largest_counts", "hash_bits_1"])
def test_contention_on_one_slot(engine, n, count, bits):
    """the common read's count is (n - 1 000) x count: 2^32 + 94 304 (printed 94 304), about 2^51 (printed negative), and with one bit of hash every key of
    the 1 001 lies on two probe chains.  No two counts are equal, so the output is compared byte for byte.  (A sum past 2^64 needs 2^33 records: an id's count
    is below 2^31.)"""
    text, sums = SH.contention_block(np, n, count)
    assert GC.begin(engine, 0, bits) == 0, GC.message(engine)
    rc, info = GC.add(engine, DeviceBlock(engine, upload(engine, text), len(text), n))
    assert rc == 0 and (info.irregular, info.records, info.uniques) == (0, n, len(sums)), GC.message(engine)
    assert info.reads == sum(sums.values()) & M.M64
    rc, info = GC.order(engine)
    assert rc == 0 and (info.out_reads, info.out_bytes) == (M.out_reads(sums), M.out_bytes(sums)), GC.message(engine)
    if n == 1 << 20 and count == 4100:
        assert sums[CK.seq(0, SH.CONT_L)] == (1 << 32) + 94304 and M.printed(sums[CK.seq(0, SH.CONT_L)]) == 94304
    SH.check_sums(sums, whole_output(engine, info), exact_order=True)
