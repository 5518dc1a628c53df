"""GPU tier (-m gpu): the order of the LDS stores of the unpredicated pack of the rows kernels (fxg_rows_pack, fastx_toolkit_amd/csrc/fxg_rows.h).

A tile whose kept reads all have at least 4 bytes is packed without predicates: every lane writes all its dwords from the top down, one
ds_write_b32 of the wave per dword, and what it writes past its own bytes must be overwritten by a LATER instruction of a later lane
(tests/test_rows_pack_cpu.py checks the schedule on the host; here the instructions run).  For every stride and instance of
test_gpu_rows_sparse_fetch.FORMS, batches of 3 tiles + 37 reads, rows of fixed length and ragged, with kept lengths in the patterns that
stress the order: all of 4..7; one full-length read, then a tile of reads of length 4 (its overshoot covers dozens of them); alternating
full and 4; descending by one; and a tile with exactly one read of length 3, which sends that whole tile down the predicated path, between
tiles that take the fast one.  Quality bytes come from a wide range (53..126 kept, 33..52 low), so that a wrong winner of a shared dword
shows.  Every array must equal the oracle's, and each run asserts the instance that ran.
"""
import numpy as np
import pytest

from helpers import assert_same, oracle_params
from oracle import fxoracle_py as fo
from test_gpu_rows_sparse_fetch import FORMS

pytestmark = pytest.mark.gpu

HI, LO = (53, 127), (33, 53)           # quality 20 and above / below, Phred+33
PD = dict(stages=6, qt_threshold=20, qt_min_len=1, qf_min_quality=20, qf_min_percent=50)
PATTERNS = ("4..7", "full then 4", "alternating", "descending", "one of 3")


def _kept(pattern, i, T, L, rng):
    """the kept length of read i (tile i // T) of a row of L >= 4 bytes"""
    t, r = divmod(i, T)
    if pattern == "4..7":
        return 4 + (i * 3 + t) % 4
    if pattern == "full then 4":
        return L if r == 0 else 4
    if pattern == "alternating":
        return L if (r + t) & 1 else 4
    if pattern == "descending":
        return max(4, L - r % max(L - 3, 1))
    if t == 1 and r == 17:                 # "one of 3": the only short read of the batch, in the middle tile
        return 3
    return int(rng.integers(4, L + 1))


def _batch(stride, T, ragged, pattern, seed):
    rng = np.random.default_rng(seed * 1000 + stride)
    n = 3 * T + 37
    b = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=(n, stride), p=[0.24, 0.24, 0.24, 0.24, 0.04])
    q = rng.integers(*LO, size=(n, stride), dtype=np.uint8)
    if ragged:                             # at least 4 bases: a shorter read would send its tile down the predicated path
        lens = rng.integers(4, stride + 1, size=n).astype(np.uint16)
        lens[rng.random(n) < 0.2] = stride
    else:
        lens = None
    want = np.zeros(n, dtype=np.int64)
    for i in range(n):
        L = stride if lens is None else int(lens[i])
        d = min(L, _kept(pattern, i, T, L, rng))
        q[i, :d] = rng.integers(*HI, size=d)
        want[i] = d
    return np.ascontiguousarray(b), np.ascontiguousarray(q), lens, want


@pytest.mark.parametrize("stride", sorted(FORMS))
def test_rows_pack_store_order(engine, monkeypatch, stride):
    import torch
    from fastx_toolkit_amd import make_params
    kernel, T, rows = FORMS[stride]
    if rows:
        monkeypatch.setenv("FXG_ROWS", rows)
    else:
        monkeypatch.delenv("FXG_ROWS", raising=False)
    dev = torch.device("cuda", 0)
    for ragged in (False, True):
        for pattern in PATTERNS:
            name = "stride %d ragged %s pattern %s" % (stride, ragged, pattern)
            b, q, lens, want = _batch(stride, T, ragged, pattern, 5)
            o = fo.run_pipeline(b, q, lens, oracle_params(PD), fixed_len=None if ragged else stride)
            # the batch is what it was built to be: every read kept, at the pattern's length -- so only the "one of 3" batch has a predicated tile
            assert int(o["counters"][fo.C_KEPT]) == b.shape[0] and np.array_equal(np.asarray(o["out_len"], dtype=np.int64), want), name
            assert (int(want.min()) == 3) == (pattern == "one of 3"), name
            db, dq = torch.from_numpy(b).to(dev), torch.from_numpy(q).to(dev)
            dl = torch.from_numpy(lens.astype(np.int16)).to(dev) if lens is not None else None
            h = engine.run(db, dq, make_params(**PD), lens=dl, fixed_len=None if ragged else stride).to_host()
            assert_same(o, h, name)
            ll = engine.last_launch()
            assert ll["kernel"].startswith(kernel), (name, ll)
            assert ll["tile_reads"] == T, (name, ll)
