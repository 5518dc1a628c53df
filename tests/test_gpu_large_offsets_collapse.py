"""Large-offsets tier (-m gpu -k large_offsets): the collapser's arena -- the one structure of the set addressed by u64 offsets summed over blocks
(off[g] = off0 + scan[r]) -- taken past 2^31 and 2^32 bytes.  One set of 182 559 records of 24 997 bases (the longest line the index takes, so the fewest
records whose bases end above 2^32 + 2^28), made on the device in two blocks of 2.28 GB (tests/collapse_shapes.py::Arena; the CPU tier parses the same
construction at small size and asserts the placement: sequences that occur only above 2^32, sequences first seen below 2^31 or between the marks and again
above 2^32, and at every offset above 2^32 taken modulo 2^32 the bytes of ANOTHER template, so that a truncated offset changes the output).

The output (3.96 GB: one record in eight repeats an earlier one) is taken through windows of 1 MB laid end to end in one device buffer between canaries and compared on the device, exactly up to the
order of equal counts: every record's header by arithmetic on its rank, its bases against the generator's for the template its first twelve bases spell,
every template once with its closed-form count, counts descending."""
import ctypes as C

import pytest

import collapse_model as M
import collapse_shapes as SH
import test_gpu_collapse as GC
from fastx_toolkit_amd.engine import NO_RECORD, FxgCollapseWindow
from test_gpu_geometry_collapse import DeviceBlock

pytestmark = pytest.mark.gpu

POISON, CANARY, GUARD = GC.POISON, GC.CANARY, 4096
ONE_MB = 1 << 20
LIMIT = 120 << 30                       # the tier's bound on device memory


def used(T):
    free, total = T.cuda.mem_get_info()
    return total - free


def test_large_offsets_collapse_arena_past_2_32():
    from fastx_toolkit_amd import Engine
    A = SH.Arena()
    eng = Engine(0)
    try:
        T, dev = eng.torch, eng.device
        L, W = A.L, SH.row_width(A.L)
        ts, counts = A.counts(T)                                              # closed form: the templates that occur and their counts
        U = len(ts)
        before = used(T)                                                      # (of the whole device: what this test adds is measured from here)
        peak = before
        assert GC.begin(eng) == 0, GC.message(eng)
        for g0, g1 in A.blocks():
            n = g1 - g0
            text = T.empty(n * W + 16, dtype=T.uint8, device=dev)
            text[n * W:] = POISON
            for a in range(g0, g1, 1024):
                b = min(a + 1024, g1)
                text[(a - g0) * W:(b - g0) * W] = A.text_rows(T, a, b, dev).reshape(-1)
            rc, info = GC.add(eng, DeviceBlock(eng, text, n * W, n))
            assert rc == 0 and (info.irregular, info.first_bad, info.records, info.reads) == (0, NO_RECORD, g1, g1), GC.message(eng)
            peak = max(peak, used(T))
            del text
        rc, info = GC.order(eng)
        assert rc == 0, GC.message(eng)
        peak = max(peak, used(T))
        sums = {SH.Seq(int(t), L): int(c) for t, c in zip(ts.tolist(), counts.tolist())}
        assert (info.records, info.reads, info.uniques, info.out_reads) == (A.R, A.R, U, A.R)
        assert info.out_bytes == M.out_bytes(sums)
        # the windows, end to end
        total = info.out_bytes
        buf = T.full((GUARD + total + GUARD,), CANARY, dtype=T.uint8, device=dev)
        buf[GUARD:GUARD + total] = POISON
        base, at, rank, calls = buf.data_ptr() + GUARD, 0, 0, 0
        w = FxgCollapseWindow()
        eng._after_torch()
        while rank < U:
            rc = eng.lib.fxg_collapse_write(eng.ctx, rank, min(ONE_MB, total - at), base + at, C.byref(w))
            assert rc == 0 and w.rank_end > rank and 0 < w.out_bytes <= ONE_MB, GC.message(eng)
            at, rank, calls = at + w.out_bytes, w.rank_end, calls + 1
        eng._before_torch()
        assert at == total and calls >= total // ONE_MB
        peak = max(peak, used(T)) - before
        assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + total:] == CANARY).all()), "write outside d_out"
        # the records, by rank: ranks of one digit count are a matrix of records of 4 + digits + 1 + L bytes (every count is one digit)
        out = buf[GUARD:GUARD + total]
        code = T.full((256,), 255, dtype=T.int64, device=dev)
        code[T.tensor(list(b"ACGT"), device=dev)] = T.arange(4, device=dev)
        got_t, got_c, pos, lo = [], [], 0, 1
        while lo <= U:
            d = len(str(lo))
            hi = min(U, 10 ** d - 1)
            size = 5 + d + L
            for r0 in range(lo, hi + 1, 1024):
                r1 = min(r0 + 1024, hi + 1)
                m = out[pos:pos + (r1 - r0) * size].view(r1 - r0, size)
                rank_ = T.arange(r0, r1, dtype=T.int64, device=dev)
                ok = (m[:, 0] == ord(">")) & (m[:, 1 + d] == ord("-")) & (m[:, 3 + d] == 10) & (m[:, -1] == 10)
                for k in range(d):
                    ok &= m[:, d - k] == (48 + (rank_ // 10 ** k) % 10).to(T.uint8)
                assert bool(ok.all()), "a header of ranks %d .. %d" % (r0, r1)
                bases = m[:, 4 + d:4 + d + L]
                t = (code[bases[:, :12].to(T.int64)] << (2 * T.arange(12, device=dev)).reshape(1, -1)).sum(1)
                assert bool((bases == SH.bases_of(T, t, L, A.seed, dev)).all()), "bases of ranks %d .. %d" % (r0, r1)
                got_t.append(t)
                got_c.append(m[:, 2 + d].to(T.int64) - 48)
                pos += (r1 - r0) * size
            lo = hi + 1
        assert pos == total
        got_t, got_c = T.cat(got_t).cpu(), T.cat(got_c).cpu()
        assert T.equal(T.sort(got_t).values, ts)                              # every sequence once
        want = T.zeros(A.R, dtype=T.int64)
        want[ts] = counts
        assert T.equal(got_c, want[got_t])                                    # with its count
        assert bool((got_c[1:] <= got_c[:-1]).all())                          # most frequent first
        assert peak < LIMIT, "peak device memory %d MB" % (peak >> 20)
        print("large_offsets collapse: %d records, %d uniques, %d windows, out_bytes %d, peak %d MB" % (A.R, U, calls, total, peak >> 20))
    finally:
        eng.close()
