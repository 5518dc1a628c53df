"""fastx_collapser measurements.

  python scripts/bench_collapse.py abi [--mb 64] [--reps 20] [--out profiles/collapse/abi.json]
      fxg_collapse_begin / _add / _add / _order / _write on blocks made on the device: --mb megabytes of two-line FASTA (">0000017\\nBASES\\n") of
      36-base and of 150-base reads that are (a) all unique, (b) drawn from a pool of records / 8 templates with a skewed draw (template
      floor(T u^6), u uniform: a tenth of the templates carries two thirds of the reads), (c) all identical.  A repetition begins a set, adds
      the block, adds a second block of the same make (another seed; for (a) that doubles the distinct sequences, so the table is rebuilt with
      the first block's in it), orders and writes the set in windows of --mb megabytes.  With profiling on, an add leaves an interval for
      lengths + scan + copy + check, one for a rebuild if there was one, one for the insert; order leaves two (mark + scan + scatter, sizes +
      scan) and its host replay is the call's wall time less those; write leaves one per window.  Beside them: the upload of the block from
      page-locked memory and fxg_fastq_index on it, by HIP events in the same script.  Medians over --reps repetitions after --warmup.
  python scripts/bench_collapse.py cli [--reads 50000000] [--dir /dev/shm] [--ref-exe PATH] [--out profiles/collapse/cli.json]
      the tool end to end on --reads 36-base reads of mix (b), input and output on tmpfs, and -- where --ref-exe names it -- the reference's
      fastx_collapser built with -O3 -DHAVE_CXX11=1 on the same file on the same box's CPU; the two outputs must be the same bytes.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ID_BYTES = 9                       # ">" + 7 digits of the record's index + "\n"
CASES = (("a: all unique", "unique"), ("b: skewed template pool", "skewed"), ("c: all identical", "identical"))


def make_block(torch, device, records, L, kind, seed):
    """(text tensor with 16 bytes of slack, text_len): ">0000017\\nBASES\\n" records built on the device"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    T = records if kind == "unique" else max(records // 8, 1) if kind == "skewed" else 1
    r = torch.randint(0, 4, (T, L), generator=g, device=device, dtype=torch.uint8)
    pool = r * 2 + 65 + (r >= 2).to(torch.uint8) * 2 + (r == 3).to(torch.uint8) * 11                # A C G T
    if kind == "unique":
        t = None
    elif kind == "skewed":
        g2 = torch.Generator(device=device)
        g2.manual_seed(seed + 1000)
        t = torch.floor(T * torch.rand((records,), generator=g2, device=device, dtype=torch.float64) ** 6).to(torch.int64).clamp(max=T - 1)
    else:
        t = torch.zeros(records, dtype=torch.int64, device=device)
    row = ID_BYTES + L + 1
    text = torch.empty((records, row), dtype=torch.uint8, device=device)
    text[:, 0], text[:, ID_BYTES - 1], text[:, row - 1] = 62, 10, 10
    idx = torch.arange(records, device=device, dtype=torch.int64) % 10 ** 7
    for k in range(7):
        text[:, 7 - k] = (48 + (idx // 10 ** k) % 10).to(torch.uint8)
    text[:, ID_BYTES:ID_BYTES + L] = pool if t is None else pool[t]
    flat = torch.zeros(records * row + 16, dtype=torch.uint8, device=device)
    flat[:records * row] = text.reshape(-1)
    return flat, records * row


def bench_abi(a):
    import torch
    from fastx_toolkit_amd import Engine
    eng = Engine(0)
    rows = []
    med = lambda xs: round(statistics.median(xs), 4)
    for L in (36, 150):
        records = (a.mb << 20) // (ID_BYTES + L + 1)
        for name, kind in CASES:
            blocks = []
            for seed in (11, 12):
                text, n = make_block(torch, eng.device, records, L, kind, seed)
                ix, l16, ti = eng.fastq_index(text, n, True, cap_records=records, fasta=True)
                assert ti.records == records and not ti.irregular
                blocks.append((text, n, ix, l16))
            # the text path beside it: the block's upload from page-locked memory and its index
            pinned = blocks[0][0][:blocks[0][1]].cpu().pin_memory()
            dst = torch.empty_like(blocks[0][0])
            up, index = [], []
            for r in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst[:blocks[0][1]].copy_(pinned, non_blocking=True)
                e1.record()
                e1.synchronize()
                eng._after_torch()
                eng.timer_start()
                eng.fastq_index(dst, blocks[0][1], True, cap_records=records, fasta=True)
                t = eng.timer_stop()
                if r >= a.warmup:
                    up.append(e0.elapsed_time(e1))
                    index.append(t)
            del pinned, dst
            out = torch.empty((a.mb << 20) + 16, dtype=torch.uint8, device=eng.device)
            eng.set_profiling(True)
            T = {k: [] for k in ("copy_check_ms", "insert_ms", "copy_check_2_ms", "rebuild_2_ms", "insert_2_ms", "order_device_ms", "order_host_replay_ms", "write_ms", "whole_ms")}
            for r in range(a.warmup + a.reps):
                t_all = time.perf_counter()
                eng.collapse_begin()
                got = {}
                for k, (text, n, ix, l16) in enumerate(blocks):
                    before = got.get("rebuilds", 0)
                    info = eng.collapse_add(text, n, ix, records, l16)
                    assert not info.irregular
                    grew = info.rebuilds - before
                    ms = eng.profiled_kernel_ms(2 + grew)
                    sfx = "" if k == 0 else "_2"
                    got["copy_check%s_ms" % sfx], got["insert%s_ms" % sfx] = ms[0], ms[-1]
                    if k == 1:
                        got["rebuild_2_ms"] = ms[1] if grew else 0.0
                    got["rebuilds"] = info.rebuilds
                t0 = time.perf_counter()
                info = eng.collapse_order()
                wall = (time.perf_counter() - t0) * 1e3
                dev = sum(eng.profiled_kernel_ms(2))
                got["order_device_ms"], got["order_host_replay_ms"] = dev, wall - dev
                rank, wms, md5 = 0, 0.0, hashlib.md5()
                while rank < info.uniques:
                    view, w = eng.collapse_write(rank, out, out_cap=a.mb << 20)
                    wms += eng.profiled_kernel_ms(1)[0]
                    if r == 0:
                        md5.update(view.cpu().numpy().tobytes())
                    rank = w.rank_end
                got["write_ms"] = wms
                got["whole_ms"] = (time.perf_counter() - t_all) * 1e3
                if r == 0:
                    first_md5 = md5.hexdigest()
                if r >= a.warmup:
                    for k in T:
                        T[k].append(got[k])
            eng.set_profiling(False)
            assert info.records == 2 * records and info.reads == 2 * records and info.out_reads == 2 * records
            row = {"case": name, "read_length": L, "records_per_block": records, "block_bytes": blocks[0][1], "uniques_after_two_blocks": info.uniques, "slots": info.slots,
                   "rebuilds": info.rebuilds, "out_bytes": info.out_bytes, "out_md5": first_md5, "reps": a.reps, "upload_ms": med(up), "fastq_index_ms": med(index)}
            row.update({k: med(v) for k, v in T.items()})
            rows.append(row)
            print(json.dumps(row), flush=True)
            del blocks, out
            torch.cuda.empty_cache()
    res = {"what": "fxg_collapse_*: two blocks made on the device per set, HIP-event intervals, medians", "library": os.environ.get("FXG_LIB", "product"),
           "device": eng.device_info()["name"], "rows": rows}
    eng.close()
    return res


def bench_cli(a):
    import torch
    tool = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fastx_collapser")
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        inp, outp, refp = os.path.join(d, "in.fa"), os.path.join(d, "out.fa"), os.path.join(d, "ref.fa")
        chunk, n_bytes, at = 5000000, 0, 0
        with open(inp, "wb") as f:
            pool_text, _ = make_block(torch, "cuda:0", max(a.reads // 8, 1), 36, "unique", 7)      # the templates: one pool for the whole file
            T = max(a.reads // 8, 1)
            pool = pool_text[:T * 46].reshape(T, 46)[:, ID_BYTES:ID_BYTES + 36].contiguous()
            g = torch.Generator(device="cuda:0")
            g.manual_seed(99)
            while at < a.reads:
                k = min(chunk, a.reads - at)
                t = torch.floor(T * torch.rand((k,), generator=g, device="cuda:0", dtype=torch.float64) ** 6).to(torch.int64).clamp(max=T - 1)
                text = torch.empty((k, 46), dtype=torch.uint8, device="cuda:0")
                text[:, 0], text[:, 8], text[:, 45] = 62, 10, 10
                idx = (torch.arange(k, device="cuda:0", dtype=torch.int64) + at) % 10 ** 7
                for j in range(7):
                    text[:, 7 - j] = (48 + (idx // 10 ** j) % 10).to(torch.uint8)
                text[:, ID_BYTES:45] = pool[t]
                f.write(text.cpu().numpy().tobytes())
                n_bytes += k * 46
                at += k
        del pool, pool_text
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
        res = {"what": "fastx_collapser -v, 36-base reads of mix (b), tmpfs to tmpfs", "reads": a.reads, "input_bytes": n_bytes, "output_bytes": os.path.getsize(outp),
               "report": p.stdout.decode(), "wall_s": [round(x, 3) for x in runs], "median_s": round(statistics.median(runs), 3)}
        if a.ref_exe:
            t0 = time.time()
            q = subprocess.run([a.ref_exe, "-v", "-i", inp, "-o", refp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=3000)
            res["reference_wall_s"] = round(time.time() - t0, 3)
            assert q.returncode == 0, q.stderr
            same = subprocess.run(["cmp", "-s", outp, refp]).returncode == 0
            res["same_bytes_as_reference"] = same and q.stdout == p.stdout
            res["speedup"] = round(res["reference_wall_s"] / res["median_s"], 2)
            print("reference: %.2f s, same bytes: %s" % (res["reference_wall_s"], res["same_bytes_as_reference"]), flush=True)
        return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["abi", "cli"])
    ap.add_argument("--mb", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=50000000)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--ref-exe", default=None)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"abi": bench_abi, "cli": bench_cli}[a.mode](a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
