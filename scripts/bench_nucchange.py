"""fasta_nucleotide_changer measurements.

  python scripts/bench_nucchange.py abi [--mb 64] [--reps 20] [--out profiles/nucchange/abi.json]
      fxg_bases_change (T -> U) on two blocks made on the device: --mb megabytes of two-line FASTA and of four-line FASTQ, reads of 150 random
      A C G T bases under ten-byte id lines.  The call rewrites the text, so every call gets a fresh copy of the block (made outside the timed
      interval).  With profiling on, a call leaves one HIP-event interval around its one launch; the whole call is timed with fxg_timer_start /
      _stop (the block's index by fxg_fastq_index is made once, outside).  Medians over --reps calls after --warmup.  The bytes the kernel must
      move are the bases, read once, plus what it writes: 16 bytes for every aligned piece inside a bases line that holds a T, one byte for
      every T in a line's ragged head or tail (counted on the device); that sum over the kernel's time is set against 8 TB/s.
  python scripts/bench_nucchange.py cli [--gb 1] [--dir /dev/shm] [--out profiles/nucchange/cli.json]
      the tool end to end (-r -v) on --gb gigabytes of the FASTA block's records, input and output on tmpfs; --host-parse adds one run of the
      record path (FXH_HOST_PARSE=1) for comparison.
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
READ = 150
ID_BYTES = 11                      # the prefix character, nine digits of the record's index, "\n"


def make_block(torch, device, nbytes, fastq, seed=11):
    """(text tensor with 16 bytes of slack, text_len, records): records of one size built on the device"""
    size = ID_BYTES + READ + 1 + ((2 + READ + 1) if fastq else 0)
    n = max(nbytes // size, 1)
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    rec = torch.empty((n, size), dtype=torch.uint8, device=device)
    r = torch.randint(0, 4, (n, READ), generator=g, device=device, dtype=torch.uint8)
    rec[:, ID_BYTES:ID_BYTES + READ] = r * 2 + 65 + (r >= 2).to(torch.uint8) * 2 + (r == 3).to(torch.uint8) * 11      # A C G T
    rec[:, 0] = 64 if fastq else 62
    idx = torch.arange(n, device=device, dtype=torch.int64)
    for k in range(9):
        rec[:, 9 - k] = (48 + (idx // 10 ** k) % 10).to(torch.uint8)
    rec[:, 10] = 10
    rec[:, ID_BYTES + READ] = 10
    if fastq:
        q0 = ID_BYTES + READ + 1
        rec[:, q0], rec[:, q0 + 1] = 43, 10
        rec[:, q0 + 2:q0 + 2 + READ] = torch.randint(35, 74, (n, READ), generator=g, device=device, dtype=torch.uint8)
        rec[:, q0 + 2 + READ] = 10
    text = torch.full((n * size + 16,), 0x5A, dtype=torch.uint8, device=device)
    text[:n * size] = rec.reshape(-1)
    return text, n * size, n, size


def must_move(torch, text, n, size):
    """(bases read, bytes written): the write side as the kernel deals it -- aligned 16-byte pieces whole inside a bases line that hold a T, and
    the T bytes of the ragged heads and tails (the text tensor is 16-byte aligned)"""
    assert text.data_ptr() % 16 == 0
    written = 0
    for r0 in range(0, n, 1 << 18):                          # in slabs: positions are int64
        r1 = min(n, r0 + (1 << 18))
        start = torch.arange(r0, r1, device=text.device, dtype=torch.int64) * size + ID_BYTES
        pos = start[:, None] + torch.arange(READ, device=text.device, dtype=torch.int64)[None, :]
        is_t = text[pos.reshape(-1)].reshape(pos.shape) == 84
        piece = pos // 16
        whole = (piece * 16 >= start[:, None]) & (piece * 16 + 16 <= start[:, None] + READ)
        written += int((is_t & ~whole).sum())
        written += 16 * int(torch.unique(piece[is_t & whole]).numel())
    return n * READ, written


def bench_abi(a):
    import torch
    from fastx_toolkit_amd import Engine
    from fastx_toolkit_amd.engine import NO_RECORD, FxgBasesChangeInfo
    eng = Engine(0)
    rows = []
    for name, fastq in (("FASTA, 150-base reads", False), ("FASTQ, 150-base reads", True)):
        orig, n_bytes, n, size = make_block(torch, eng.device, a.mb << 20, fastq)
        text = orig.clone()
        ix, _, info_ix = eng.fastq_index(text, n_bytes, True, cap_records=n, fasta=not fastq)
        assert info_ix.records == n and not info_ix.irregular
        read, written = must_move(torch, orig, n, size)
        ts = int((orig[:n_bytes].view(n, size)[:, ID_BYTES:ID_BYTES + READ] == 84).sum())
        info = FxgBasesChangeInfo()
        eng.set_profiling(True)
        kernel, whole = [], []
        for r in range(a.warmup + a.reps):
            text.copy_(orig)
            eng._after_torch()
            torch.cuda.synchronize()
            eng.timer_start()
            eng._check(eng.lib.fxg_bases_change(eng.ctx, text.data_ptr(), n_bytes, 4 if fastq else 2, ix.line.data_ptr(), ix.cap_lines, n, ord("T"), ord("U"), C.byref(info)))
            t = eng.timer_stop()
            ms = eng.profiled_kernel_ms(1)
            if r >= a.warmup:
                kernel.append(ms[0])
                whole.append(t)
        eng.set_profiling(False)
        assert (info.changed, info.first_to_record, info.irregular) == (ts, NO_RECORD, 0), (info.changed, ts)
        want = orig[:n_bytes].view(n, size).clone()
        b = want[:, ID_BYTES:ID_BYTES + READ]
        b[b == 84] = 85
        assert torch.equal(text[:n_bytes].view(n, size), want) and bool((text[n_bytes:] == 0x5A).all())
        k, w = statistics.median(kernel), statistics.median(whole)
        rows.append({"case": name, "records": n, "text_bytes": n_bytes, "bases_read": read, "bytes_written": written, "changed": ts, "reps": a.reps,
                     "kernel_ms": round(k, 4), "kernel_ms_min": round(min(kernel), 4), "kernel_ms_max": round(max(kernel), 4), "whole_call_ms": round(w, 4),
                     "must_move_bytes": read + written, "must_move_gb_s": round((read + written) / (k * 1e-3) / 1e9, 1),
                     "fraction_of_8tb_s": round((read + written) / (k * 1e-3) / HBM_PEAK, 4),
                     "text_gb_s_whole_call": round(n_bytes / (w * 1e-3) / 1e9, 1)})
        print(json.dumps(rows[-1]), flush=True)
        del text, orig, want
    res = {"what": "fxg_bases_change T -> U, one call per block made on the device, a fresh copy of the block per call", "library": os.environ.get("FXG_LIB", "product"),
           "device": eng.device_info()["name"], "rows": rows}
    eng.close()
    return res


def bench_cli(a):
    import torch
    tool = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fasta_nucleotide_changer")
    text, n_bytes, n, size = make_block(torch, "cuda:0", 64 << 20, False)
    chunk = text[:n_bytes].cpu().numpy().tobytes()
    ts = chunk.count(b"T")                                   # (the id lines hold digits only)
    del text
    torch.cuda.empty_cache()
    copies = max(int(a.gb * (1 << 30)) // n_bytes, 1)
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        inp, outp = os.path.join(d, "in.fa"), os.path.join(d, "out.fa")
        with open(inp, "wb") as f:
            for _ in range(copies):
                f.write(chunk)
        runs, host = [], None
        for r in range(a.cli_reps):
            t0 = time.time()
            p = subprocess.run([tool, "-r", "-v", "-i", inp, "-o", outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1800)
            dt = time.time() - t0
            if p.returncode != 0:
                raise RuntimeError(p.stderr.decode()[-2000:])
            runs.append(dt)
            print("cli run %d: %.2f s" % (r, dt), flush=True)
        assert ("Nucleotides changed: %d\n" % (ts * copies)).encode() in p.stdout and ("Input: %d reads." % (n * copies)).encode() in p.stdout, p.stdout
        out_size = os.path.getsize(outp)
        with open(outp, "rb") as f:
            assert f.read(n_bytes) == chunk.replace(b"T", b"U")
        if a.host_parse:
            t0 = time.time()
            subprocess.run([tool, "-r", "-v", "-i", inp, "-o", outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1800, check=True, env=dict(os.environ, FXH_HOST_PARSE="1"))
            host = round(time.time() - t0, 3)
        med = statistics.median(runs)
        return {"what": "fasta_nucleotide_changer -r -v, FASTA of 150-base reads, tmpfs to tmpfs", "records": n * copies, "input_bytes": n_bytes * copies, "output_bytes": out_size,
                "wall_s": [round(x, 3) for x in runs], "median_s": round(med, 3), "input_gb_per_s": round(n_bytes * copies / med / 1e9, 2), "record_path_wall_s": host}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["abi", "cli"])
    ap.add_argument("--mb", type=int, default=64)
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--host-parse", action="store_true")
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
