"""fastx_barcode_splitter measurements.

  python scripts/bench_barcode.py abi  [--mb 64] [--reps 20] [--out profiles/barcode_abi.json]
      fxg_barcode_split on one block of 150-base FASTQ (96 eight-base barcodes at the read's start, --mismatches 1, --partial 0 and 1):
      fxg_timer_start / fxg_timer_stop around the call, median of --reps, and the bytes the split must move (the records read once and
      written once) against 8 TB/s.  Run it under `rocprofv3 --kernel-trace --stats -- python ...` for the split per kernel.
  python scripts/bench_barcode.py cli  [--reads 50000000] [--dir /dev/shm] [--out profiles/barcode_cli.json]
      the tool end to end, input file and 97 output files on tmpfs (fewer reads when the file system cannot hold input and output).
  python scripts/bench_barcode.py perl --script PATH [--reads 200000] [--out profiles/barcode_perl.json]
      the reference script's rate on this machine's host cores (one process: the script is single-threaded).
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
READ_LEN, BL, NBC = 150, 8, 96


def make_reads(n, seed=1):
    """n FASTQ records of 150 bases ("@r<k>" names), 85 % starting with one of 96 barcodes, 30 % of those with one substitution"""
    rs = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    codes = acgt[rs.integers(0, 4, size=(NBC, BL))]
    seq = acgt[rs.integers(0, 4, size=(n, READ_LEN))]
    has = rs.random(n) < 0.85
    seq[has, :BL] = codes[rs.integers(0, NBC, size=n)[has]]
    mut = rs.random(n) < 0.3
    seq[mut, rs.integers(0, BL, size=n)[mut]] = acgt[rs.integers(0, 4, size=int(mut.sum()))]
    rec = np.empty((n, 3 + READ_LEN + 3 + READ_LEN + 1), dtype=np.uint8)
    rec[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + READ_LEN] = seq
    rec[:, 3 + READ_LEN:6 + READ_LEN] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + READ_LEN:6 + 2 * READ_LEN] = ord("I")
    rec[:, -1] = 10
    return codes, rec.reshape(-1)


def barcode_file(codes):
    return "".join("BC%02d\t%s\n" % (k, bytes(c).decode()) for k, c in enumerate(codes))


def bench_abi(a):
    import ctypes as C
    import torch
    from fastx_toolkit_amd import Engine
    eng = Engine(0)
    n = (a.mb << 20) // 307
    codes, data = make_reads(n)
    d = torch.empty(len(data) + 16, dtype=torch.uint8, device="cuda:0")
    d[:len(data)] = torch.from_numpy(data).to("cuda:0")
    ix, _, info = eng.fastq_index(d, len(data), cap_records=n + 2)
    assert info.records == n
    out = torch.empty(len(data), dtype=torch.uint8, device="cuda:0")
    rows = []
    for partial in (0, 1):
        ents = []
        for k, c in enumerate(codes):
            b = bytes(c)
            ents.append((b, k))
            ents += [(b[p:], k) for p in range(1, partial + 1)]
        eng.barcode_prepare(ents, BL, NBC + 1, mismatches=1, eol=False)
        bb, br = (C.c_uint64 * (NBC + 1))(), (C.c_uint64 * (NBC + 1))()
        ms = []
        for r in range(a.warmup + a.reps):
            eng._after_torch()
            eng._check(eng.lib.fxg_timer_start(eng.ctx))
            eng._check(eng.lib.fxg_barcode_split(eng.ctx, d.data_ptr(), len(data), 4, ix.line.data_ptr(), ix.cap_lines, n, None, out.data_ptr(), bb, br))
            t = C.c_float()
            eng._check(eng.lib.fxg_timer_stop(eng.ctx, C.byref(t)))
            if r >= a.warmup:
                ms.append(t.value)
        med = statistics.median(ms)
        moved = 2 * len(data)
        rows.append({"partial": partial, "entries": len(ents), "records": n, "block_bytes": len(data), "median_ms": round(med, 4),
                     "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": a.reps, "moved_bytes": moved,
                     "moved_tb_s": round(moved / (med * 1e-3) / 1e12, 3), "fraction_of_8tb_s": round(moved / (med * 1e-3) / HBM_PEAK, 3),
                     "unmatched": int(br[NBC])})
        print(json.dumps(rows[-1]), flush=True)
    res = {"what": "fxg_barcode_split, one block of 150-base FASTQ, 96 eight-base barcodes (--bol --mismatches 1)",
           "device": eng.device_info()["name"], "rows": rows}
    eng.close()
    return res


def bench_cli(a):
    tool = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fastx_barcode_splitter")
    free = shutil.disk_usage(a.dir).free
    n = a.reads
    while n > 1_000_000 and 2.2 * 307 * n > free:
        n //= 2
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        bc = os.path.join(d, "bc.txt")
        open(bc, "w").write(barcode_file(make_reads(1)[0]))          # (the same 96 barcodes as every chunk below: seed 1)
        inp = os.path.join(d, "in.fq")
        chunk = 2_000_000
        with open(inp, "wb") as f:
            for k in range(0, n, chunk):
                f.write(make_reads(min(chunk, n - k), seed=1)[1].tobytes())
        size = os.path.getsize(inp)
        os.makedirs(os.path.join(d, "o"))
        runs = []
        for r in range(a.cli_reps):
            t0 = time.time()
            with open(inp, "rb") as fin:
                p = subprocess.run([tool, "--bcfile", bc, "--prefix", os.path.join(d, "o") + "/", "--suffix", ".fq", "--bol", "--mismatches", "1"],
                                   stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1800)
            dt = time.time() - t0
            if p.returncode != 0:
                raise RuntimeError(p.stderr.decode()[-2000:])
            runs.append(dt)
            print("cli run %d: %.2f s" % (r, dt), flush=True)
        lines = p.stdout.decode().splitlines()
        total = int(lines[-1].split("\t")[1])
        assert total == n
        med = statistics.median(runs)
        return {"what": "fastx_barcode_splitter --bol --mismatches 1, 96 barcodes, tmpfs to tmpfs, 97 output files", "reads": n, "input_bytes": size,
                "wall_s": [round(x, 3) for x in runs], "median_s": round(med, 3), "mreads_per_s": round(n / med / 1e6, 2),
                "gb_per_s": round(size / med / 1e9, 2), "files": len(os.listdir(os.path.join(d, "o")))}


def bench_perl(a):
    codes, data = make_reads(a.reads)
    with tempfile.TemporaryDirectory() as d:
        bc = os.path.join(d, "bc.txt")
        open(bc, "w").write(barcode_file(codes))
        t0 = time.time()
        p = subprocess.run(["perl", a.script, "--bcfile", bc, "--prefix", os.path.join(d, "o_"), "--bol", "--mismatches", "1"], input=data.tobytes(),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        dt = time.time() - t0
        assert p.returncode == 0, p.stderr.decode()[-2000:]
    return {"what": "reference scripts/fastx_barcode_splitter.pl --bol --mismatches 1, 96 barcodes, one process", "reads": a.reads,
            "wall_s": round(dt, 2), "kreads_per_s": round(a.reads / dt / 1e3, 1), "host_cores": os.cpu_count(),
            "perl": subprocess.run(["perl", "-e", "print $^V"], stdout=subprocess.PIPE).stdout.decode()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["abi", "cli", "perl"])
    ap.add_argument("--mb", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--script", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "abi":
        res = bench_abi(a)
    elif a.mode == "cli":
        a.reads = a.reads or 50_000_000
        res = bench_cli(a)
    else:
        a.reads = a.reads or 200_000
        res = bench_perl(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
