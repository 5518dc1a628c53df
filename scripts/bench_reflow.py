"""fasta_formatter measurements.

  python scripts/bench_reflow.py abi [--mb 1024] [--reps 20] [--out profiles/reflow_abi.json]
      fxg_fasta_reflow on one block made on the device, both directions: records wrapped at 60 columns in and one line per record out
      (-w 0), and one line per record in and 60 columns out (-w 60).  With profiling on, a call leaves three HIP-event intervals
      (classify + segmented scan, sizes + scans, copy); the whole call, line index included, is timed with fxg_timer_start / _stop.  Medians
      over --reps calls after --warmup, and (text_len + out_bytes) / time against 8 TB/s.
  python scripts/bench_reflow.py cli [--mb 1024] [--dir /dev/shm] [--out profiles/reflow_cli.json]
      the tool end to end on the wrapped file of the same shape, input and output on tmpfs.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
RECORD_BASES, WIDTH = 60000, 60
HEADER = b">chr\n"


def record(wrapped, seed=1):
    """one record of 60 000 random bases: on lines of 60, or on one line"""
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=RECORD_BASES)]
    if not wrapped:
        return HEADER + bases.tobytes() + b"\n"
    rows = np.empty((RECORD_BASES // WIDTH, WIDTH + 1), dtype=np.uint8)
    rows[:, :WIDTH] = bases.reshape(-1, WIDTH)
    rows[:, WIDTH] = 10
    return HEADER + rows.tobytes()


def bench_abi(a):
    import torch
    from fastx_toolkit_amd import Engine
    from fastx_toolkit_amd.engine import FxgReflowInfo, FxgReflowOpts, reflow_bound
    eng = Engine(0)
    rows = []
    for name, wrapped, width in (("wrapped at 60 in, -w 0 out", True, 0), ("one line per record in, -w 60 out", False, WIDTH)):
        unit = record(wrapped)
        reps = (a.mb << 20) // len(unit)
        n = reps * len(unit)
        d = torch.empty(n + 16, dtype=torch.uint8, device=eng.device)
        d[:n] = torch.frombuffer(bytearray(unit), dtype=torch.uint8).to(eng.device).repeat(reps)
        lines = unit.count(b"\n") * reps
        line = torch.empty(2 * (lines + 1), dtype=torch.int32, device=eng.device)
        out = torch.empty(reflow_bound(n) if width else n + 16, dtype=torch.uint8, device=eng.device)
        o, info = FxgReflowOpts(width, 0, 0, out.numel()), FxgReflowInfo()
        eng.set_profiling(True)
        phases, whole = [], []
        for r in range(a.warmup + a.reps):
            eng._after_torch()
            eng.timer_start()
            eng._check(eng.lib.fxg_fasta_reflow(eng.ctx, d.data_ptr(), n, 1, 0, C.byref(o), line.data_ptr(), lines + 1, out.data_ptr(), C.byref(info)))
            t = eng.timer_stop()
            ms = eng.profiled_kernel_ms(3)
            if r >= a.warmup:
                phases.append(ms)
                whole.append(t)
        eng.set_profiling(False)
        want = unit.replace(b"\n", b"")[len(HEADER) - 1:]                # the record's bases
        first = out[:info.out_bytes // reps].cpu().numpy().tobytes()
        assert first.replace(b"\n", b"")[len(HEADER) - 1:] == want and info.consumed == n and info.open_bases == 0
        med = [statistics.median(p[k] for p in phases) for k in range(3)]
        kernels = statistics.median(sum(p) for p in phases)
        moved = n + info.out_bytes
        rows.append({"case": name, "text_bytes": n, "out_bytes": info.out_bytes, "lines": info.lines, "records": reps, "reps": a.reps,
                     "classify_segscan_ms": round(med[0], 4), "sizes_scans_ms": round(med[1], 4), "copy_ms": round(med[2], 4),
                     "three_phases_ms": round(kernels, 4), "whole_call_ms": round(statistics.median(whole), 4),
                     "moved_bytes": moved, "fraction_of_8tb_s_three_phases": round(moved / (kernels * 1e-3) / HBM_PEAK, 4),
                     "fraction_of_8tb_s_whole_call": round(moved / (statistics.median(whole) * 1e-3) / HBM_PEAK, 4)})
        print(json.dumps(rows[-1]), flush=True)
        del d, line, out
    res = {"what": "fxg_fasta_reflow, one block made on the device, records of 60 000 bases", "device": eng.device_info()["name"], "rows": rows}
    eng.close()
    return res


def bench_cli(a):
    tool = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fasta_formatter")
    unit = record(True)
    reps = (a.mb << 20) // len(unit)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        inp, outp = os.path.join(d, "in.fa"), os.path.join(d, "out.fa")
        with open(inp, "wb") as f:
            for k in range(0, reps, 256):
                f.write(unit * min(256, reps - k))
        size = os.path.getsize(inp)
        runs = []
        for r in range(a.cli_reps):
            t0 = time.time()
            p = subprocess.run([tool, "-w", "0", "-i", inp, "-o", outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1800)
            dt = time.time() - t0
            if p.returncode != 0:
                raise RuntimeError(p.stderr.decode()[-2000:])
            runs.append(dt)
            print("cli run %d: %.2f s" % (r, dt), flush=True)
        assert os.path.getsize(outp) == reps * (len(HEADER) + RECORD_BASES + 1)
        med = statistics.median(runs)
        return {"what": "fasta_formatter -w 0, records of 60 000 bases wrapped at 60, tmpfs to tmpfs", "input_bytes": size,
                "wall_s": [round(x, 3) for x in runs], "median_s": round(med, 3), "gb_per_s": round(size / med / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["abi", "cli"])
    ap.add_argument("--mb", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = bench_abi(a) if a.mode == "abi" else bench_cli(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
