#!/usr/bin/env python3
"""Here (CPU, the oracle): how many base bytes the sparse base fetch of the rows kernels needs, per granule size -- the prediction the
measured FETCH_SIZE drop of stage B is compared with (fxg_rows_need_mask, fastx_toolkit_amd/csrc/fxg_rows.h).

    python scripts/sparse_fetch_count.py [--config cfg2] [--reads 2000000] [--granules 16 64 128] [--now-gb 22.75]

The oracle decides the first --reads reads of the config (seed, length, parameters of bench.CONFIGS).  The kernel fetches the 16-byte chunks
of each tile (grid from the tile's first byte) that overlap a kept prefix; at a coarser granule g, every g-byte block of the array (grid from
the array's first byte) that holds a fetched chunk counts whole.  Per launch figures scale the sample to the config's size; --now-gb is the
measured traffic of the full fetch (read + written), the baseline of the last column.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from oracle import fxoracle_py as fo  # noqa: E402


def tile_reads(stride):
    """reads per tile of the rows kernel the plan picks for this stride (fxg_plan.h; FXG_ROWS=2 above 208 bytes)"""
    if stride < 28 or stride > 304:
        raise SystemExit("stride %d: no rows kernel" % stride)
    if stride <= 40:
        return 256
    if stride <= 56:
        return 192
    if stride < 80:
        return 128
    return 64 if stride <= 152 else 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--granules", type=int, nargs="+", default=[16, 64, 128])
    ap.add_argument("--now-gb", type=float, default=22.75, help="measured read + write traffic per launch with the full base fetch")
    a = ap.parse_args()
    cfg = bench.CONFIGS[a.config]
    L, N = cfg["L"], a.reads
    if cfg["params"] is None or not (cfg["params"]["stages"] & 6) or cfg["params"]["stages"] & ~6:
        raise SystemExit("%s does not run the rows kernels" % a.config)
    b, q = fo.synth_batch(cfg["seed"], 0, N, L, cfg["adapter"], L)
    o = fo.run_pipeline(b, q, None, fo.make_params(**cfg["params"]), fixed_len=L)
    res = o["res"].astype(np.uint32)
    keep = (res >> 16) & 1
    klen = np.where(keep == 1, res & 0xFFFF, 0).astype(np.int64)
    T = tile_reads(L)
    # byte mask of kept prefixes over the array, then the 16-byte chunks of each tile that hold one of them
    starts = np.arange(N, dtype=np.int64) * L
    kept_bytes = int(klen.sum())
    need = np.zeros(N * L, dtype=bool)
    for r in np.nonzero(klen)[0]:
        need[starts[r]:starts[r] + klen[r]] = True
    fetched = np.zeros(N * L, dtype=bool)
    for t0 in range(0, N, T):
        lo, hi = t0 * L, min(N, t0 + T) * L
        m = need[lo:hi]
        nch = -(-(hi - lo) // 16)
        pad = np.zeros(nch * 16, dtype=bool)
        pad[:hi - lo] = m
        ch = pad.reshape(nch, 16).any(axis=1)
        fetched[lo:hi] = np.repeat(ch, 16)[:hi - lo]
    scale = cfg["reads"] / N
    print("%s: %d of %d reads (seed %d, %d bp), tile %d reads; kept fraction %.4f, kept bases %.1f per read (%.2f GB per launch)" % (
        a.config, N, cfg["reads"], cfg["seed"], L, T, keep.mean(), kept_bytes / N, kept_bytes * scale / 1e9))
    print("| granule | share of base granules needed | base bytes per read fetched | saved per launch | total bytes per launch (now %.2f GB) |" % a.now_gb)
    print("|---|---|---|---|---|")
    full = N * L
    for g in a.granules:
        if g == 16:
            share = fetched.sum() / full
            per_read = fetched.sum() / N
        else:
            nb = -(-full // g)
            pad = np.zeros(nb * g, dtype=bool)
            pad[:full] = fetched
            blk = pad.reshape(nb, g).any(axis=1)
            share = blk.mean()
            per_read = min(full, blk.sum() * g) / N
        saved = (L - per_read) * cfg["reads"] / 1e9
        now = a.now_gb
        print("| %d B | %.3f | %.1f | %.2f GB | %.1f GB (%+.0f %%) |" % (g, share, per_read, saved, now - saved, -100 * saved / now))


if __name__ == "__main__":
    main()
