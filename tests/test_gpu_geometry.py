"""GPU tier (-m gpu): ordered compaction across launch geometries and scanner counts.

Every compacting kernel gets its output placement from a protocol between workgroups: sharded ticket dispensers, one central scanner
(fxg_scanner_k) or nscan scanner waves (fxg_scanner_multi, the rows kernels), and epoch-tagged status granules reused across launches.
The emulator of the CPU tier never runs it, and the rest of the GPU tier runs it at the one geometry a dedicated MI355X picks.  Here the
same batches run under forced worker counts, ticket groups, workgroups per CU, scanner counts, tile sizes and clip pipeline depths, at
tile and scanner-batch counts on the protocol's edges, and every array must equal the oracle's.  Each run also asserts

  * engine.scan_recoveries() unchanged: the in-kernel protocol produced the result, not the host's redo without the scanner (which
    gives correct output after a 2-s wait, so a geometry that deadlocks or publishes late would otherwise pass);
  * the kernel family and tile size of engine.last_launch(), and its grid where the knobs fix it: min(workers, ntiles) + nscan.

The oracle result of a batch is computed once and reused across geometries: it does not depend on them.
"""
import contextlib
import time
import zlib

import numpy as np
import pytest

from helpers import assert_same, oracle_params, random_batch
from oracle import fxoracle_py as fo

pytestmark = pytest.mark.gpu

QTF = dict(qt_threshold=20, qt_min_len=30, qf_min_quality=20, qf_min_percent=80)
AD13 = b"AGATCGGAAGAGC"
AD40 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCACATCTCG"
BATCH = 512                     # tiles per batch of fxg_scanner_multi (FXG_ROWS_SCAN_K * 64)
ENGINE_KNOBS = ("FXG_WORKERS", "FXG_TICKET_GROUPS", "FXG_BLOCKS_PER_CU", "FXG_NSCAN")
CALL_KNOBS = ("FXG_TILE", "FXG_CLIP_DEPTH_RT", "FXG_ROWS", "FXG_CLIP_GLOBAL", "FXG_REV_DW")

# kernel families: stride (fixed-length batches use all of it), parameters, kernel name (prefix of last_launch()["kernel"]), the plan's tile size,
# call knobs (env), rows: FXG_NSCAN applies (fxg_kernel_rows*), tile: FXG_TILE applies (fxg_pick_tile), clip: seeded reads with adapters (random_batch)
FAM = {
    "rows26": dict(stride=100, pd=dict(stages=6, **QTF), kernel="fxg_kernel_rows<26>", T=64, rows=True),
    "rows38": dict(stride=150, pd=dict(stages=6, **QTF), kernel="fxg_kernel_rows<38>", T=64, rows=True),
    "rows26x2": dict(stride=200, pd=dict(stages=6, **QTF), kernel="fxg_kernel_rows<26,2>", T=32, rows=True),
    "multi4": dict(stride=36, pd=dict(stages=6, qt_threshold=20, qt_min_len=10, qf_min_quality=20, qf_min_percent=80), kernel="fxg_kernel_rows_multi<10,4>", T=256, rows=True),
    "multi3": dict(stride=50, pd=dict(stages=6, qt_threshold=20, qt_min_len=15, qf_min_quality=20, qf_min_percent=80), kernel="fxg_kernel_rows_multi<14,3>", T=192, rows=True),
    "multi2": dict(stride=76, pd=dict(stages=6, **QTF), kernel="fxg_kernel_rows_multi<20,2>", T=128, rows=True),
    "tiles00": dict(stride=150, pd=dict(stages=6, **QTF), kernel="fxg_kernel_tiles<0,0>", T=128, env=dict(FXG_ROWS="0"), tile=True),
    "clip13": dict(stride=100, pd=dict(stages=1, adapter=AD13, clip_min_len=15, clip_flags=4), kernel="fxg_kernel_tiles<-13,0> clip(packed)", T=256,
                   env=dict(FXG_CLIP_GLOBAL="0"), tile=True, clip=True),
    "clip13gl": dict(stride=100, pd=dict(stages=1, adapter=AD13, clip_min_len=15, clip_flags=4), kernel="fxg_kernel_tiles<-13,0> clip(packed)", T=256,
                     env=dict(FXG_CLIP_GLOBAL="1"), clip=True),
    "clip40k": dict(stride=150, pd=dict(stages=1, adapter=AD40, clip_min_len=15, clip_flags=0), kernel="fxg_kernel_tiles<-40,0> clip(packed)", T=256, clip=True),
    "cfg5": dict(stride=150, pd=dict(stages=7, adapter=AD13, clip_min_len=15, clip_flags=4, **QTF), kernel="fxg_kernel_tiles<-13,0> clip(packed)", T=256, tile=True, clip=True),
    "ftrim": dict(stride=150, pd=dict(stages=16, ft_first=3, ft_last=100), kernel="fxg_kernel_tiles<0,1> ftrim", T=128, tile=True),
    "rev2": dict(stride=150, pd=dict(stages=24, ft_first=5, ft_last=145), kernel="fxg_kernel_tiles<0,2> revcomp", T=128, tile=True),
    "rev5": dict(stride=158, pd=dict(stages=8), kernel="fxg_kernel_tiles<0,5> revcomp", T=128, tile=True),
    "mask": dict(stride=150, pd=dict(stages=64, mask_min_quality=20), kernel="fxg_kernel_tiles<0,3> mask", T=128, tile=True),
    "artifacts": dict(stride=100, pd=dict(stages=128), kernel="fxg_kernel_tiles<0,4> base census", T=128, tile=True),
    "nfilter": dict(stride=100, pd=dict(stages=256, nf_keep_n=0), kernel="fxg_kernel_tiles<0,4> base census", T=128, tile=True),
}
ROWS = [f for f in FAM if FAM[f].get("rows")]
TILES = [f for f in FAM if not FAM[f].get("rows")]
# the clip instance with history: ragged input whose stale tails the reference aligner sees (set_clip_history), the DP over the staged tile
HIST = dict(stride=100, pd=dict(stages=1, adapter=AD13, clip_min_len=5, clip_flags=0), kernel="fxg_kernel_tiles<-13,0> clip(packed)", T=256, clip=True)

_batches, _oracles = {}, {}


def _batch(fam, n, ragged=False, seed=0):
    """(host bases, host qual, host lens, device bases, device qual, device lens, fixed_len) of a seeded batch, uploaded once."""
    import torch
    key = (fam, n, ragged, seed)
    if key not in _batches:
        f = FAM.get(fam, HIST)
        st = f["stride"]
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        if ragged or f.get("clip"):
            b, q, lens = random_batch(rng, n, st, 1, st, not ragged, adapter=f["pd"].get("adapter", AD13))
        else:
            b, q = fo.synth_batch(17 + seed, 1000 * n, n, st, False, st)
            lens = None
        dev = torch.device("cuda", 0)
        db, dq = torch.from_numpy(b).to(dev), torch.from_numpy(q).to(dev)
        dl = torch.from_numpy(lens.astype(np.int16)).to(dev) if lens is not None else None
        _batches[key] = (b, q, lens, db, dq, dl, None if lens is not None else st)
    return _batches[key]


def _oracle(fam, n, ragged=False, seed=0, pd=None):
    key = (fam, n, ragged, seed, repr(pd))
    if key not in _oracles:
        b, q, lens, _, _, _, fl = _batch(fam, n, ragged, seed)
        al = fo.aligner_new() if fam == "hist" else None
        _oracles[key] = fo.run_pipeline(b, q, lens, oracle_params(pd or FAM.get(fam, HIST)["pd"]), fixed_len=fl, aligner=al)
        if al is not None:
            fo.aligner_free(al)
    return _oracles[key]


@contextlib.contextmanager
def _engine(monkeypatch, **env):
    """A fresh Engine(0) under the engine-level knobs (read at context creation); closed afterwards."""
    from fastx_toolkit_amd import Engine
    for k in ENGINE_KNOBS + CALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    eng = Engine(0)
    eng.geo = dict(env)
    eng.cus = eng.device_info()["compute_units"]
    try:
        yield eng
    finally:
        eng.close()
        for k in env:
            monkeypatch.delenv(k, raising=False)


def _expected_grid(eng, ntiles, nscan_default, compact):
    """min(workers, ntiles) + nscan where the engine's knobs fix the number of workers, else None."""
    g = eng.geo
    if "FXG_WORKERS" not in g and "FXG_BLOCKS_PER_CU" not in g:
        return None
    cap = eng.cus * int(g["FXG_BLOCKS_PER_CU"]) if "FXG_BLOCKS_PER_CU" in g else 1 << 62
    if "FXG_WORKERS" in g:
        cap = min(cap, int(g["FXG_WORKERS"]))
    workers = max(1, min(cap, ntiles))
    if not compact:
        return workers
    return workers + nscan_default(workers)


def _run(eng, monkeypatch, fam, n, ragged=False, seed=0, call=None, T=None, kernel=None, compact=True, meta=True, pd=None, what=""):
    """One launch of family `fam` on a batch of n reads under the call knobs `call`; every array against the oracle, no recovery, the
    intended instance, tile size and grid.  Returns last_launch()."""
    from fastx_toolkit_amd import make_params
    f = FAM.get(fam, HIST)
    env = dict(f.get("env", {}))
    env.update(call or {})
    for k in CALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    T = T or f["T"]
    pd = pd or f["pd"]
    b, q, lens, db, dq, dl, fl = _batch(fam, n, ragged, seed)
    o = _oracle(fam, n, ragged, seed, pd)
    name = "%s n=%d ragged=%s call=%r geo=%r %s" % (fam, n, ragged, call, eng.geo, what)
    if fam == "hist":
        eng.set_clip_history(True)                 # a fresh aligner, like the oracle's
    before = eng.scan_recoveries()
    try:
        r = eng.run(db, dq, make_params(**pd), lens=dl, fixed_len=fl, compact=compact, meta=meta)
        h = r.to_host()
    finally:
        if fam == "hist":
            eng.set_clip_history(False)
        for k in env:
            monkeypatch.delenv(k, raising=False)
    assert eng.scan_recoveries() == before, "%s: the launch's waits ran out and it was redone without the scanner" % name
    if compact and meta:
        assert_same(o, h, name)
    else:
        assert np.array_equal(o["res"], h["res"]), name + ": res"
        assert np.array_equal(o["counters"][:13], h["counters"][:13]), name + ": counters"
        if compact:
            assert h["out_len"] is None and h["kept_index"] is None
            assert np.array_equal(o["out_bases"], h["out_bases"]) and np.array_equal(o["out_qual"], h["out_qual"]), name + ": packed stream"
    ll = eng.last_launch()
    assert ll["kernel"].startswith(kernel or f["kernel"]), (name, ll)
    assert ll["tile_reads"] == T, (name, ll)
    ntiles = -(-n // T)
    nscan = eng.geo.get("FXG_NSCAN")
    nscan_default = (lambda w: int(nscan) if nscan else (8 if w >= 512 else 1)) if f.get("rows") else (lambda w: 1)
    grid = _expected_grid(eng, ntiles, nscan_default, compact)
    if grid is not None:
        assert ll["grid"] == grid, (name, ll, grid)
    return ll


def _n(T, ntiles, part=None):
    """Reads for `ntiles` tiles of T with a partial last tile (T > 1)."""
    if T == 1:
        return ntiles
    return (ntiles - 1) * T + (part if part is not None else max(1, (T * 5) // 8))


TILE_EDGES = (1, 2, 511, 512, 513)
# engine geometries: worker counts on both sides of the ticket-group threshold (8 groups, one scanner: a grid of 16), other group counts,
# one and sixteen workgroups per CU (sixteen: more workgroups than can be resident for the 256-thread and clip instances), the default
ENGINE_GEOS = (dict(FXG_WORKERS=1), dict(FXG_WORKERS=2, FXG_TICKET_GROUPS=1), dict(FXG_WORKERS=7, FXG_TICKET_GROUPS=3), dict(FXG_WORKERS=14),
               dict(FXG_WORKERS=15), dict(FXG_WORKERS=37, FXG_TICKET_GROUPS=5), dict(FXG_WORKERS=15, FXG_TICKET_GROUPS=5),
               dict(FXG_BLOCKS_PER_CU=1), dict(FXG_BLOCKS_PER_CU=16, FXG_TICKET_GROUPS=3), dict())


@pytest.mark.parametrize("geo", range(len(ENGINE_GEOS)))
def test_rows_kernels_across_workers_and_ticket_groups(monkeypatch, geo):
    """fxg_kernel_rows<26>, <38>, <26,2> and fxg_kernel_rows_multi r = 4 / 3 / 2 at 1, 2, 511, 512 and 513 tiles (partial last tile)
    and one ragged batch, under each engine geometry.  At sixteen workgroups per CU, 512 tiles is the first count at which the plan
    runs eight scanner waves instead of one."""
    with _engine(monkeypatch, **ENGINE_GEOS[geo]) as eng:
        for fam in ROWS:
            T = FAM[fam]["T"]
            for nt in TILE_EDGES:
                _run(eng, monkeypatch, fam, _n(T, nt))
            _run(eng, monkeypatch, fam, _n(T, 300), ragged=True)
            if ENGINE_GEOS[geo].get("FXG_BLOCKS_PER_CU") == 16:
                _run(eng, monkeypatch, fam, _n(T, 4500), what="grid above residency")


def _scanner_cases(S):
    """(family, batches, tiles in the last batch, workers, ticket groups) for S forced scanner waves: nb = S - 1, S, S + 1 and 2S + 1,
    the last batch one tile or 511 tiles; at least seven families meet the ticket-group threshold (a grid of 8 (S + 1)) from just below and at it."""
    sizes = [(S - 1, 1), (S, 511), (S + 1, 1), (2 * S + 1, 511)]
    sizes = [(nb, last) for nb, last in sizes if nb >= 1]
    if S == 64:      # the largest batches through the families with the fewest reads per tile
        fams = ["rows26", "rows38", "rows26", "rows26x2"]
    else:
        fams = [ROWS[i % len(ROWS)] for i in range(len(sizes))] + ROWS[len(sizes):]
        sizes = sizes + [sizes[i % len(sizes)] for i in range(len(fams) - len(sizes))]
    out = []
    for i, (fam, (nb, last)) in enumerate(zip(fams, sizes)):
        out.append((fam, nb, last, (2, 7, 37, 15)[i % 4], (8, 3, 5, 1)[i % 4]))
    thr = 8 * (S + 1)
    out.append((ROWS[S % len(ROWS)], 2, 300, thr - S - 1, 8))         # grid 8 (S + 1) - 1: one dispenser
    out.append((ROWS[(S + 1) % len(ROWS)], 2, 300, thr - S, 8))       # grid 8 (S + 1): eight
    return out


@pytest.mark.parametrize("S", [2, 3, 8, 64])
def test_scanner_multi_publishes_run_by_run_when_a_batch_cannot_fill(monkeypatch, S):
    """FXG_NSCAN = S scanner waves over nb = S - 1 .. 2S + 1 batches of 512 tiles, with at most 37 workers.  A worker holds at most two
    decided tiles, so 37 workers cannot fill a 512-tile batch: the run-by-run publication of fxg_scanner_multi (fxg_device.h) is what
    lets every batch complete -- the path a dedicated GPU never takes at full occupancy.  Also the grids just below and at the ticket-group
    threshold for S scanners."""
    for fam, nb, last, workers, groups in _scanner_cases(S):
        T = FAM[fam]["T"]
        with _engine(monkeypatch, FXG_NSCAN=S, FXG_WORKERS=workers, FXG_TICKET_GROUPS=groups) as eng:
            _run(eng, monkeypatch, fam, _n(T, (nb - 1) * BATCH + last), what="S=%d nb=%d" % (S, nb))


def test_scanner_multi_slow_start(monkeypatch):
    """One worker, eight scanner waves, twelve batches: wave j starts waiting for batch j while batches 0 .. j - 1 are still being filled
    two tiles at a time.  The run must finish inside the waits' bound with no recovery; its kernel time is printed."""
    T = FAM["rows38"]["T"]
    n = _n(T, 11 * BATCH + 300)
    with _engine(monkeypatch, FXG_NSCAN=8, FXG_WORKERS=1) as eng:
        eng.set_profiling(True)
        t0 = time.time()
        _run(eng, monkeypatch, "rows38", n, what="slow start")
        print("slow start: 1 worker, 8 scanner waves, %d tiles (12 batches): kernel %.1f ms, wall %.1f ms"
              % (-(-n // T), eng.last_kernel_ms(), 1e3 * (time.time() - t0)))


@pytest.mark.parametrize("geo", range(len(ENGINE_GEOS)))
def test_tile_kernels_across_geometries(monkeypatch, geo):
    """Every fxg_kernel_tiles family -- the quality form (FXG_ROWS=0), the 13-base clip instance staged and over the batch, the two-pass
    k-form with checkpoint scratch (40-base adapter, 150-base reads), the cfg5 chain, fixed trim, revcomp + trim through <0,2> and <0,5>
    (the plan's choice for 158-base rows, then FXG_REV_DW=0 on the same batch), the masker, the base census and NFILTER, clip with history
    on ragged input -- at 1, 2, 511, 512 and 513 tiles with one central scanner, under each engine geometry; ragged batches for the
    streaming families; the clip instances at each forced pipeline depth."""
    with _engine(monkeypatch, **ENGINE_GEOS[geo]) as eng:
        for fam in TILES:
            T = FAM[fam]["T"]
            for nt in TILE_EDGES:
                _run(eng, monkeypatch, fam, _n(T, nt))
            if FAM[fam].get("tile"):
                _run(eng, monkeypatch, fam, _n(T, 257), ragged=not FAM[fam].get("clip"),
                     kernel="fxg_kernel_tiles<0,2> revcomp" if fam == "rev5" else None)          # (ragged reverse complement: <0,2>)
            if FAM[fam].get("clip"):
                for d in (2, 3, 4):
                    _run(eng, monkeypatch, fam, _n(T, 511), call=dict(FXG_CLIP_DEPTH_RT=d))
        if ENGINE_GEOS[geo].get("FXG_BLOCKS_PER_CU") == 16:      # 4 500 tiles of four reads: more workgroups than can be resident
            for fam in TILES:
                if FAM[fam].get("tile"):
                    _run(eng, monkeypatch, fam, 4 * 4499 + 3, call=dict(FXG_TILE=4), T=4, what="grid above residency")
        _run(eng, monkeypatch, "rev5", _n(128, 513), call=dict(FXG_REV_DW="0"), kernel="fxg_kernel_tiles<0,2> revcomp")
        _run(eng, monkeypatch, "hist", 3000, ragged=True)
        _run(eng, monkeypatch, "hist", 70000, ragged=True)


@pytest.mark.parametrize("tile", [1, 2, 4, 64, 256])
def test_tile_kernels_by_tile_size(monkeypatch, tile):
    """FXG_TILE = 1 .. 256 reads per tile for the tile kernels whose tile the plan picks (the clip instance staged, the others streaming),
    at 2 and 513 tiles, with few workers (and the default geometry for the small tiles); <0,5> only where the tile is a multiple of four."""
    for geo in (dict(FXG_WORKERS=7, FXG_TICKET_GROUPS=3), dict(FXG_WORKERS=37)):
        with _engine(monkeypatch, **geo) as eng:
            for fam in TILES:
                if not FAM[fam].get("tile"):
                    continue
                kern = "fxg_kernel_tiles<0,2> revcomp" if fam == "rev5" and tile % 4 else None
                for nt in (2, 513):
                    _run(eng, monkeypatch, fam, _n(tile, nt), call=dict(FXG_TILE=tile), T=tile, kernel=kern)


def test_uncompacted_and_bench_call_shapes(monkeypatch):
    """compact=False (no scanner: grid = min(workers, ntiles)) and meta=False (bench.py's call shape: no per-kept-read arrays) under few workers."""
    for geo in (dict(FXG_WORKERS=1), dict(FXG_WORKERS=15), dict(FXG_WORKERS=37, FXG_NSCAN=3)):
        with _engine(monkeypatch, **geo) as eng:
            for fam in ("rows38", "tiles00", "clip13", "rev2"):
                T = FAM[fam]["T"]
                for nt in (1, 513):
                    n = _n(T, nt)
                    # (uncompacted launches never take the rows kernel: they need no output placement)
                    _run(eng, monkeypatch, fam, n, compact=False, kernel="fxg_kernel_tiles<0,0>" if FAM[fam].get("rows") else None,
                         T=128 if FAM[fam].get("rows") else None)
                    _run(eng, monkeypatch, fam, n, meta=False)


def test_epochs_and_status_reuse_over_600_launches(monkeypatch):
    """One Engine, 640 consecutive compacting launches (two and a half cycles of the 8-bit epoch) cycling through five batches of different
    families; the tile count grows twice in the middle of an epoch cycle (a bigger status array, cleared once) and then shrinks again, so
    the granules of the higher tiles keep older tags behind the current launch.  Each result must equal its oracle answer."""
    small = [("rows26", _n(64, 1100), None), ("tiles00", _n(128, 3), None), ("clip13", _n(256, 2), None), ("rev2", _n(128, 9), None),
             ("ftrim", 40, dict(FXG_TILE=1))]
    big1, big2 = ("ftrim", 3000, dict(FXG_TILE=1)), ("mask", 6000, dict(FXG_TILE=1))      # (the first status array holds 1100 + 275 + 1024 tiles)
    with _engine(monkeypatch, FXG_WORKERS=15, FXG_NSCAN=3) as eng:
        recov = eng.scan_recoveries()
        for i in range(640):
            cyc = list(small)
            if 150 <= i < 160 or 420 <= i < 430:
                cyc[4] = big1 if i < 300 else big2         # the status array grows (launch 150, then 420) ...
            fam, n, call = cyc[i % 5]                       # ... and the next launches use only its first tiles again
            T = FAM[fam]["T"] if not call else 1
            _run(eng, monkeypatch, fam, n, call=call, T=T, what="launch %d" % i)
        assert eng.scan_recoveries() == recov
