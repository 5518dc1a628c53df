"""fastx_clip_collapser and fxg_collapse_add_rows measurements.

  python scripts/bench_clip_collapse.py abi [--records 1000000] [--reps 20] [--out profiles/collapse/rows_abi.json]
      one block of --records 36-base FASTA reads (an insert of 18 to 26 bases from a skewed pool, the adapter, filler) indexed, packed and run
      through fxg_run_pipeline with the clip stage once.  A repetition then adds the kept rows to a fresh set through fxg_collapse_add_rows, and
      the same kept reads to another fresh set the way the pipe has to: fxg_fastq_format to text, fxg_fastq_index on that text, fxg_collapse_add.
      With profiling on, both adds leave an interval for their copy (rows: row lens + scans + copy rows + counts, with the download of the byte
      count in it; text: lengths + scan + copy + check) and one for the insert; the format and the index of the text route are timed by the
      context's timer.  Medians over --reps repetitions after --warmup.
  python scripts/bench_clip_collapse.py cli [--reads 50000000] [--dir /dev/shm] [--pipe-bin DIR] [--out profiles/collapse/clip_collapse_cli.json]
      the fused tool against  fastx_clipper -a A -l 15 -c -i IN | fastx_collapser -o OUT  as two processes joined by a pipe (the tools of
      --pipe-bin: a build of the parent commit; default: this build's, whose two tools this change does not touch), on the same FASTQ file of
      --reads reads of 36 bases, tmpfs to tmpfs, --cli-reps runs each, medians.  The two outputs must be the same bytes.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
AD = b"CTGTAGGCACCATCAAT"
L = 36


def make_reads(torch, device, n, seed, templates):
    """uint8 [n, L]: insert (its length 18 + template % 9) + adapter + filler; a tenth of the reads have no adapter"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)
    pool = letters[torch.randint(0, 4, (templates, L), generator=g, device=device)]
    ad = torch.tensor(list(AD), dtype=torch.uint8, device=device)
    t = torch.floor(templates * torch.rand((n,), generator=g, device=device, dtype=torch.float64) ** 6).to(torch.int64).clamp(max=templates - 1)
    rows = pool[t]
    ilen = 18 + t % 9
    col = torch.arange(L, device=device).unsqueeze(0)
    k = col - ilen.unsqueeze(1)
    with_ad = (torch.rand((n,), generator=g, device=device) >= 0.1).unsqueeze(1)
    in_ad = (k >= 0) & (k < len(AD)) & with_ad
    rows = torch.where(in_ad, ad[k.clamp(0, len(AD) - 1)], rows)
    filler = letters[torch.randint(0, 4, (n, L), generator=g, device=device)]
    return torch.where((k >= len(AD)) & with_ad, filler, rows)


def fasta_block(torch, rows, first=0):
    n = rows.shape[0]
    text = torch.empty((n, 9 + L + 1), dtype=torch.uint8, device=rows.device)
    text[:, 0], text[:, 8], text[:, 9 + L] = 62, 10, 10
    idx = (torch.arange(n, device=rows.device, dtype=torch.int64) + first) % 10 ** 7
    for j in range(7):
        text[:, 7 - j] = (48 + (idx // 10 ** j) % 10).to(torch.uint8)
    text[:, 9:9 + L] = rows
    return text


def bench_abi(a):
    import torch
    from fastx_toolkit_amd import Engine, make_params
    eng = Engine(0)
    med = lambda xs: round(statistics.median(xs), 4)
    rows = make_reads(torch, eng.device, a.records, 11, max(a.records // 8, 1))
    text = fasta_block(torch, rows).reshape(-1)
    d_text = torch.zeros(text.numel() + 16, dtype=torch.uint8, device=eng.device)
    d_text[:text.numel()] = text
    n = text.numel()
    ix, l16, ti = eng.fastq_index(d_text, n, True, cap_records=a.records, fasta=True)
    bases, _, irr = eng.fastq_pack(d_text, n, ix, a.records, ti.max_len, want_qual=False)
    assert not ti.irregular and not irr
    res = eng.run(bases, None, make_params(stages=1, adapter=AD, clip_min_len=15, clip_flags=1), fixed_len=ti.max_len)
    kept = res.kept
    T = {k: [] for k in ("rows_copy_ms", "rows_insert_ms", "rows_call_ms", "text_format_ms", "text_index_ms", "text_copy_check_ms", "text_insert_ms", "text_route_ms")}
    eng.set_profiling(True)
    for r in range(a.warmup + a.reps):
        got = {}
        eng.collapse_begin(initial_slots=4 * a.records)
        t0 = time.perf_counter()
        ia = eng.collapse_add_rows(res, d_text=d_text, ix=ix)
        got["rows_call_ms"] = (time.perf_counter() - t0) * 1e3
        ms = eng.profiled_kernel_ms(2)
        got["rows_copy_ms"], got["rows_insert_ms"] = ms[0], ms[1]
        ua = eng.collapse_order().uniques
        eng.collapse_begin(initial_slots=4 * a.records)
        t0 = time.perf_counter()
        eng.timer_start()
        kt = eng.fastq_format(d_text, n, ix, a.records, res=res.res)
        got["text_format_ms"] = eng.timer_stop()
        eng.timer_start()
        kix, kl16, kti = eng.fastq_index(kt, kt.numel(), True, cap_records=kept, fasta=True)      # (the formatter's tensor has its slack behind the view)
        got["text_index_ms"] = eng.timer_stop()
        ib = eng.collapse_add(kt, kt.numel(), kix, kept, kl16)
        got["text_route_ms"] = (time.perf_counter() - t0) * 1e3
        ms = eng.profiled_kernel_ms(2)
        got["text_copy_check_ms"], got["text_insert_ms"] = ms[0], ms[1]
        assert (ia.records, ia.reads, ia.uniques) == (ib.records, ib.reads, ib.uniques) and eng.collapse_order().uniques == ua
        if r >= a.warmup:
            for k in T:
                T[k].append(got[k])
    eng.set_profiling(False)
    row = {"what": "one block of 36-base FASTA reads through the clip stage; its kept rows into a fresh set by fxg_collapse_add_rows, and as formatted text by fxg_collapse_add",
           "device": eng.device_info()["name"], "records": a.records, "kept": kept, "uniques": ua, "reps": a.reps}
    row.update({k: med(v) for k, v in T.items()})
    eng.close()
    return row


def bench_cli(a):
    import torch
    bin_ = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin")
    pipe_bin = a.pipe_bin or bin_
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        inp, fused, piped = os.path.join(d, "in.fq"), os.path.join(d, "fused.fa"), os.path.join(d, "pipe.fa")
        chunk, at, n_bytes = 5000000, 0, 0
        templates = max(a.reads // 8, 1)
        with open(inp, "wb") as f:
            while at < a.reads:
                k = min(chunk, a.reads - at)
                rows = make_reads(torch, "cuda:0", k, 99 + at // chunk, templates)
                rec = torch.empty((k, 9 + L + 1 + 2 + L + 1), dtype=torch.uint8, device="cuda:0")
                rec[:, :9 + L + 1] = fasta_block(torch, rows, at)
                rec[:, 0] = 64
                rec[:, 9 + L + 1], rec[:, 9 + L + 2], rec[:, -1] = 43, 10, 10
                rec[:, 9 + L + 3:-1] = 73
                f.write(rec.cpu().numpy().tobytes())
                n_bytes += rec.numel()
                at += k
        torch.cuda.empty_cache()
        argv = ["-a", AD.decode(), "-l", "15", "-c"]
        res = {"what": "fastx_clip_collapser against fastx_clipper | fastx_collapser (two processes, a pipe), 36-base FASTQ reads, tmpfs to tmpfs", "reads": a.reads,
               "input_bytes": n_bytes, "pipe_tools": pipe_bin}
        t_fused, t_pipe = [], []
        for r in range(a.cli_reps):
            t0 = time.time()
            p = subprocess.run([os.path.join(bin_, "fastx_clip_collapser"), "-v"] + argv + ["-i", inp, "-o", fused], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1800)
            t_fused.append(time.time() - t0)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            t0 = time.time()
            p1 = subprocess.Popen([os.path.join(pipe_bin, "fastx_clipper")] + argv + ["-i", inp], stdout=subprocess.PIPE)
            p2 = subprocess.Popen([os.path.join(pipe_bin, "fastx_collapser"), "-o", piped], stdin=p1.stdout)
            p1.stdout.close()
            rc2, rc1 = p2.wait(timeout=3000), p1.wait(timeout=3000)
            t_pipe.append(time.time() - t0)
            assert (rc1, rc2) == (0, 0)
            print("run %d: fused %.2f s, pipe %.2f s" % (r, t_fused[-1], t_pipe[-1]), flush=True)
        res["same_bytes"] = subprocess.run(["cmp", "-s", fused, piped]).returncode == 0
        res.update(report=p.stdout.decode(), output_bytes=os.path.getsize(fused), fused_wall_s=[round(x, 3) for x in t_fused], pipe_wall_s=[round(x, 3) for x in t_pipe],
                   fused_median_s=round(statistics.median(t_fused), 3), pipe_median_s=round(statistics.median(t_pipe), 3))
        res["speedup"] = round(res["pipe_median_s"] / res["fused_median_s"], 2)
        assert res["same_bytes"]
        return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["abi", "cli"])
    ap.add_argument("--records", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=50000000)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--pipe-bin", default=None)
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
