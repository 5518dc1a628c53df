"""fastx_uncollapser measurements.

  python scripts/bench_uncollapse.py abi [--records 2000000] [--reps 20] [--out profiles/uncollapse/abi.json]
      fxg_fasta_uncollapse on two blocks made on the device: --records records of 22 to 30 bases whose counts follow a discrete Pareto law
      (count = floor(u ** (-1 / 1.5)) for u uniform in (0, 1], capped at 10 000: about two records in three have count 1, the mean is about 2.7,
      the tail reaches the cap), and the same block with every count 1.  One call writes the whole block (out_cap = its size).  With profiling
      on, a call leaves three HIP-event intervals (counts + scan, sizes + scans + window, copy); the whole call is timed with fxg_timer_start /
      _stop (the block's index by fxg_fastq_index is made once, outside).  Medians over --reps calls after --warmup, and output bytes / time
      against 8 TB/s.  The library is the one FXG_LIB names, else the product's.
  python scripts/bench_uncollapse.py lanes [--out profiles/uncollapse/lane_mappings.json]
      the copy kernels' two lane mappings (csrc/fxg_uncollapse.h: FXG_UC_SIDE_BY_SIDE) side by side: `abi` in a child process per library, the
      product's and a build with -DFXG_UC_SIDE_BY_SIDE=1 (--side-lib, made by `build-side` where there is a compiler), alternating, --rounds times.
  python scripts/bench_uncollapse.py build-side
      builds that second library into build/uc_side/libfxg_uc_side.so.
  python scripts/bench_uncollapse.py cli [--dir /dev/shm] [--out profiles/uncollapse/cli.json]
      the tool end to end on the first block's text, input and output on tmpfs.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
SIDE_LIB = os.path.join(ROOT, "build", "uc_side", "libfxg_uc_side.so")      # (a name of its own: build.compile_engine keeps its objects by the library's name)
ALPHA, COUNT_CAP = 1.5, 10000
ID_BYTES = 16                      # ">" + 7 digits of the record's index + "-" + 6 digits of its count + "\n"


def make_block(torch, device, records, heavy, seed=11):
    """(text tensor with 16 bytes of slack, text_len, counts, lens): ">0000017-000003\\nBASES\\n" records built on the device"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    lens = torch.randint(22, 31, (records,), generator=g, device=device, dtype=torch.int64)
    if heavy:
        u = 1.0 - torch.rand((records,), generator=g, device=device, dtype=torch.float64)      # (0, 1]
        counts = torch.clamp(torch.floor(u ** (-1.0 / ALPHA)), max=COUNT_CAP).to(torch.int64)
    else:
        counts = torch.ones(records, dtype=torch.int64, device=device)
    size = ID_BYTES + lens + 1
    start = torch.cumsum(size, 0) - size
    n = int(size.sum())
    r = torch.randint(0, 4, (n + 16,), generator=g, device=device, dtype=torch.uint8)
    text = r * 2 + 65 + (r >= 2).to(torch.uint8) * 2 + (r == 3).to(torch.uint8) * 11                # A C G T
    ids = torch.empty((records, ID_BYTES), dtype=torch.uint8, device=device)
    ids[:, 0], ids[:, 8], ids[:, 15] = 62, 45, 10
    idx = torch.arange(records, device=device, dtype=torch.int64) % 10 ** 7
    for k in range(7):
        ids[:, 7 - k] = (48 + (idx // 10 ** k) % 10).to(torch.uint8)
    for k in range(6):
        ids[:, 14 - k] = (48 + (counts // 10 ** k) % 10).to(torch.uint8)
    text[(start[:, None] + torch.arange(ID_BYTES, device=device)[None, :]).reshape(-1)] = ids.reshape(-1)
    text[start + size - 1] = 10
    return text, n, counts, lens


def bench_abi(a):
    import torch
    from fastx_toolkit_amd import Engine
    from fastx_toolkit_amd.engine import FxgUncollapseInfo, FxgUncollapseOpts
    eng = Engine(0)
    rows = []
    for name, heavy in (("discrete Pareto counts (alpha 1.5, cap 10000)", True), ("every count 1", False)):
        text, n, counts, lens = make_block(torch, eng.device, a.records, heavy)
        ix, l16, info_ix = eng.fastq_index(text, n, True, cap_records=a.records, fasta=True)
        assert info_ix.records == a.records and not info_ix.irregular
        copies = int(counts.sum())
        first = torch.cumsum(counts, 0) - counts + 1                                             # the first number of each record
        last = first + counts - 1
        digits = sum(int(((last.clamp(min=10 ** (w - 1)) - first.clamp(min=10 ** (w - 1)) + 1).clamp(min=0) * ((last >= 10 ** (w - 1)).to(torch.int64))).sum())
                     for w in range(1, 12))                                                      # digit w is there for every number >= 10^(w-1)
        total = int((counts * (lens + 3)).sum()) + digits
        out = torch.empty(total + 16, dtype=torch.uint8, device=eng.device)
        o, info = FxgUncollapseOpts(0, 0, total), FxgUncollapseInfo()
        eng.set_profiling(True)
        phases, whole = [], []
        for r in range(a.warmup + a.reps):
            eng._after_torch()
            eng.timer_start()
            eng._check(eng.lib.fxg_fasta_uncollapse(eng.ctx, text.data_ptr(), n, ix.line.data_ptr(), ix.cap_lines, a.records, l16.data_ptr(), C.byref(o),
                                                    out.data_ptr(), C.byref(info)))
            t = eng.timer_stop()
            ms = eng.profiled_kernel_ms(3)
            if r >= a.warmup:
                phases.append(ms)
                whole.append(t)
        eng.set_profiling(False)
        assert (info.copies, info.copy_end, info.out_bytes) == (copies, copies, total), (info.copies, info.copy_end, info.out_bytes, copies, total)
        assert int((out[:total] == 62).sum()) == copies and int((out[:total] == 10).sum()) == 2 * copies
        l0 = int(lens[0])
        assert out[:l0 + 4].cpu().numpy().tobytes() == b">1\n" + text[ID_BYTES:ID_BYTES + l0].cpu().numpy().tobytes() + b"\n"
        med = [statistics.median(p[k] for p in phases) for k in range(3)]
        kernels = statistics.median(sum(p) for p in phases)
        w = statistics.median(whole)
        rows.append({"case": name, "records": a.records, "text_bytes": n, "copies": copies, "out_bytes": total, "largest_count": int(counts.max()), "reps": a.reps,
                     "counts_scan_ms": round(med[0], 4), "sizes_scans_window_ms": round(med[1], 4), "copy_ms": round(med[2], 4),
                     "three_phases_ms": round(kernels, 4), "whole_call_ms": round(w, 4),
                     "copy_out_gb_s": round(total / (med[2] * 1e-3) / 1e9, 1), "whole_call_out_gb_s": round(total / (w * 1e-3) / 1e9, 1),
                     "fraction_of_8tb_s_copy": round(total / (med[2] * 1e-3) / HBM_PEAK, 4), "fraction_of_8tb_s_whole_call": round(total / (w * 1e-3) / HBM_PEAK, 4)})
        print(json.dumps(rows[-1]), flush=True)
        del text, out
    res = {"what": "fxg_fasta_uncollapse, one call per block made on the device, 22 to 30 bases", "library": os.environ.get("FXG_LIB", "product"),
           "device": eng.device_info()["name"], "rows": rows}
    eng.close()
    return res


def bench_lanes(a):
    if not os.path.exists(a.side_lib):
        raise SystemExit("%s is missing: run `python scripts/bench_uncollapse.py build-side` where hipcc is" % a.side_lib)
    runs = {"16 lanes to a copy (product)": [], "a copy per lane, side by side": []}
    for rnd in range(a.rounds):
        for name, lib in (("16 lanes to a copy (product)", None), ("a copy per lane, side by side", a.side_lib)):
            env = dict(os.environ)
            env.pop("FXG_LIB", None)
            if lib:
                env["FXG_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "abi", "--records", str(a.records), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=900)
            if p.returncode != 0:
                raise RuntimeError(p.stderr.decode()[-3000:])
            runs[name].append(json.loads(p.stdout.decode().strip().splitlines()[-1])["rows"])
            print(name, "round", rnd, [(r["case"], r["copy_ms"], r["whole_call_ms"]) for r in runs[name][-1]], flush=True)
    rows = []
    for name, rr in runs.items():
        for k in range(len(rr[0])):
            rows.append({"mapping": name, "case": rr[0][k]["case"], "out_bytes": rr[0][k]["out_bytes"], "copy_ms_per_round": [r[k]["copy_ms"] for r in rr],
                         "whole_call_ms_per_round": [r[k]["whole_call_ms"] for r in rr], "copy_ms": statistics.median(r[k]["copy_ms"] for r in rr),
                         "copy_out_gb_s": round(rr[0][k]["out_bytes"] / (statistics.median(r[k]["copy_ms"] for r in rr) * 1e-3) / 1e9, 1)})
    return {"what": "the copy kernels' two lane mappings, alternating child processes in one session", "records": a.records, "rounds": a.rounds, "rows": rows}


def bench_cli(a):
    import torch
    tool = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fastx_uncollapser")
    text, n, counts, lens = make_block(torch, "cuda:0", a.records, True)
    copies = int(counts.sum())
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        inp, outp = os.path.join(d, "in.fa"), os.path.join(d, "out.fa")
        with open(inp, "wb") as f:
            f.write(text[:n].cpu().numpy().tobytes())
        del text
        torch.cuda.empty_cache()
        runs = []
        for r in range(a.cli_reps):
            t0 = time.time()
            p = subprocess.run([tool, "-v", "-i", inp, "-o", outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1800)
            dt = time.time() - t0
            if p.returncode != 0:
                raise RuntimeError(p.stderr.decode()[-2000:])
            runs.append(dt)
            print("cli run %d: %.2f s" % (r, dt), flush=True)
        assert ("Output: %d sequences" % copies).encode() in p.stdout, p.stdout
        out_size = os.path.getsize(outp)
        med = statistics.median(runs)
        return {"what": "fastx_uncollapser -v, the Pareto block, tmpfs to tmpfs", "records": a.records, "input_bytes": n, "output_bytes": out_size, "copies": copies,
                "wall_s": [round(x, 3) for x in runs], "median_s": round(med, 3), "output_gb_per_s": round(out_size / med / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["abi", "lanes", "cli", "build-side"])
    ap.add_argument("--records", type=int, default=2000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--side-lib", default=SIDE_LIB)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "build-side":
        from fastx_toolkit_amd import build
        os.makedirs(os.path.dirname(a.side_lib), exist_ok=True)
        print(build.compile_engine(a.side_lib, ["-DFXG_UC_SIDE_BY_SIDE=1"]))
        return
    res = {"abi": bench_abi, "lanes": bench_lanes, "cli": bench_cli}[a.mode](a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
