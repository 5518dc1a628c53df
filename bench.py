#!/usr/bin/env python3
"""bench.py -- benchmark of the MI355X FASTQ engine (driver contract in the task statement).

Default workload (BASELINE.json configs[1], the configuration the metric is quoted on):
    fastq_quality_trimmer -t 20 -l 30 | fastq_quality_filter -q 20 -p 80
on 50 M synthetic 150 bp Phred+33 reads PER GPU (seed 2, SURVEY.md 8d generator, generated on the
device so inputs are resident in HBM when the timed region starts), fused into ONE pass that also
stream-compacts the kept, trimmed reads in input order.  One "step" = one such pass over the batch.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--reads R] [--config cfg2|cfg3|cfg4|cfg5shard|stats] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W

A plain run does only what the headline line needs: it generates the inputs on the device, warms up, times the steps, writes
--dump-outputs and prints the line (value, roofline and self-check of the timed launches themselves).  --full adds what takes
runs of its own, after the headline's measurement and without touching its keys: the reference's CPU rate on a bounded sample
(cpu_baseline; --no-cpu-baseline drops it), the other BASELINE configs at their stated sizes (configs and roofline.other_configs,
cfg2 at its own size only; --headline-only drops them) and the command-line tools end to end (e2e, cfg2 only; --no-e2e drops it).

--config selects another BASELINE.json configuration (same JSON shape, its own roofline object):
    cfg3       fastx_clipper -a AGATCGGAAGAGC -l 15 -n, 50 M x 100 bp                (VALU-bound: GCUPS)
    cfg4       fastx_reverse_complement | fastx_trimmer -f 5 -l 145 fused, 200 M x 150 bp
    cfg5shard  clip -> quality-trim -> filter in one pass, 125 M x 150 bp per GPU (1 B reads over 8 GPUs)
    stats      fastx_quality_stats histogram reduction, 50 M x 150 bp

--dump-outputs DIR writes what the timed path computed in its last step as DIR/<name>.npy (float64 / float32, under 64 MB): the counter
block, res[] and the packed bases and qualities at fixed seeded sample positions, and the stream checksum over all of them (statistics:
the histogram one step added).  The inputs are seeded, so two builds run with the same arguments can be compared output for output.

Multi-GPU: reads shard by contiguous index range (rank g owns reads [g*R, (g+1)*R) of the global set),
no data-path collective; each step ends with one 192-byte all-gather of the counter blocks (RCCL) from
which every rank derives the job totals and its offset in the global output.  scaling = weak.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md); ~6.3 TB/s is the measured copy ceiling
# VALU peak: a SIMD issues one wave64 VALU instruction per 2 cycles (MI355X_MICROARCH.md "Wave scheduling" and the per-instruction
# table: v_fma_f32 wave64 = 2 cycles; 157.3 TFLOP/s fp32 vector = 78.6 T lane-ops/s x 2 flops), 256 CUs x 4 SIMDs x 64 lanes at 2.4 GHz.
# The clip kernel's own instruction classes reach 1.6-2.6 cycles at four waves per SIMD (scripts/ubench/valu_rate.hip, profiles/r02_valu_rate_a.txt,
# profiles/r03/g_valu_rate_dependent.txt), so a fraction of this peak near 0.8 is the practical ceiling for its mix.
VALU_CYCLES = 2.0
VALU_PEAK_GLANEOPS = 256 * 4 * 64 / VALU_CYCLES * 2.4
ADAPTER = b"AGATCGGAAGAGC"
QTF = dict(qt_threshold=20, qt_min_len=30, qf_min_quality=20, qf_min_percent=80)

CONFIGS = {
    "cfg2": dict(seed=2, reads=50_000_000, L=150, adapter=False, params=dict(stages=2 | 4, **QTF),
                 metric="Mreads/s (150 bp) quality-trim+filter", bound="hbm",
                 what="fastq_quality_trimmer -t 20 -l 30 | fastq_quality_filter -q 20 -p 80"),
    "cfg3": dict(seed=3, reads=50_000_000, L=100, adapter=True, params=dict(stages=1, adapter=ADAPTER, clip_min_len=15, clip_flags=4),
                 metric="Mreads/s (100 bp) adapter clip", bound="valu", what="fastx_clipper -a AGATCGGAAGAGC -l 15 -n"),
    "cfg4": dict(seed=2, reads=200_000_000, L=150, adapter=False, params=dict(stages=8 | 16, ft_first=5, ft_last=145),
                 metric="Mreads/s (150 bp) reverse-complement+trim", bound="hbm",
                 what="fastx_reverse_complement | fastx_trimmer -f 5 -l 145"),
    "cfg5shard": dict(seed=5, reads=125_000_000, L=150, adapter=True,
                      params=dict(stages=1 | 2 | 4, adapter=ADAPTER, clip_min_len=15, clip_flags=4, **QTF),
                      metric="Mreads/s (150 bp) clip+quality-trim+filter", bound="valu",
                      what="fastx_clipper -a AGATCGGAAGAGC -l 15 -n | fastq_quality_trimmer -t 20 -l 30 | fastq_quality_filter -q 20 -p 80"),
    "stats": dict(seed=2, reads=50_000_000, L=150, adapter=False, params=None,
                  metric="Mreads/s (150 bp) quality statistics", bound="hbm", what="fastx_quality_stats (per-cycle histogram reduction)"),
}
# roofline.frac of the VALU-bound lines prices the cells at the FEWEST VALU instructions the reference's score recurrence takes on this ISA (5, below), so
# it follows from this run's timing alone.  What the kernel really issues per cell (SQ_INSTS_VALU x 64 / cells, scripts/pmc_sq.sh) is a counter of one
# particular build: it is attached as `issued_*` only from profiles/pmc_sq_<config>.json collected on the SAME kernel sources (csrc_sha16), like the
# HBM traffic files (round 5 multiplied by a round-4 constant: verdict, weak 2).
CLIP_MIN_VALU_PER_CELL = 5.0

# What the timed launches of the default workloads must produce: (kept reads, kept bases, Result.checksum()).  The same tuples are
# asserted by tests/test_gpu_parity.py::test_full_size_* on runs whose res[] and packed streams are compared with the oracle in a
# prefix window, a suffix window and seeded interior windows -- so a bench line whose self_check matches is the oracle-verified output.
# One tuple per RANK of a weak-scaling run: rank g owns reads [g * R, (g + 1) * R) of the config's seed (R = the config's size), so each rank of an N-GPU
# job checks its own launches (tests/test_gpu_parity.py::test_every_rank_shard_is_pinned verifies shards 1..7 the same way as shard 0, one after
# another on one GPU; scripts/pin_shards.py printed them).  The driver's 1/2/4/8-GPU curve runs cfg2; cfg5shard IS rank g's eighth of config 5's 1 B reads.
EXPECTED = {
    "cfg2": [(33431448, 3558930905, 2378887646053514995), (33427658, 3558387229, 4328753190306870522), (33427499, 3558429462, 5122451479550132608),
             (33430505, 3558962275, 3660201661073056593), (33438724, 3559531052, 2907356342622187104), (33432089, 3558722046, 5093690086307672043),
             (33433761, 3559087569, 2696102762881492209), (33428857, 3558618226, 8789052924520016587)],
    "cfg3": [(44712033, 3240876702, 531446952678075522)],
    "cfg4": [(200000000, 28200000000, 8156573128088355123)],
    "cfg5shard": [(71509386, 6067408648, 8691884730239237722), (71514097, 6069132454, 8438137191787113985), (71501289, 6067858775, 8352292930493294139),
                  (71503024, 6067203890, 7734193212479304412), (71509668, 6068082071, 8087916189659338308), (71499098, 6067284163, 2262037768823059192),
                  (71499359, 6066769491, 6301825060380288858), (71502490, 6068265645, 4082786155604905187)],
}


def csrc_sha16():
    """Hash of the kernel sources: counters replayed from profiles/ are only attached to a bench line built from the same code."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "fastx_toolkit_amd", "csrc")
    for f in sorted(os.listdir(d)):
        h.update(f.encode()); h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


DUMP_SEED = 20251015
DUMP_RES = 1 << 21          # sampled res[] entries (float64: 16 MB)
DUMP_STREAM = 1 << 22       # sampled bytes of each packed stream (float32: 16 MB each)
DUMP_COUNTERS = 17          # counter slots FXG_C_INPUT .. FXG_C_ARTIFACT_DROPPED (include/fxg.h); the rest are not results


def _sample(t, n, count, salt):
    """t[i] for a fixed, seeded, sorted set of `count` positions in [0, n) (all of them when n <= count), on the host."""
    import numpy as np
    import torch
    if n <= count:
        return t[:n].cpu().numpy()
    idx = np.unique(np.random.default_rng([DUMP_SEED, salt]).integers(0, n, size=count, dtype=np.int64))
    return t.index_select(0, torch.from_numpy(idx).to(t.device)).cpu().numpy()


def dump_outputs(d, suffix, res=None, hist=None, per_step=1):
    """The arrays a caller of the timed path receives from its last step, as DIR/<name><suffix>.npy."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    out = {}
    if hist is not None:                             # quality_stats accumulates: every step added the same counts
        h = hist.cpu().numpy()
        assert not (h % per_step).any()
        out["hist"] = (h // per_step).astype(np.float64)
    else:
        c = np.asarray(res.counters[:DUMP_COUNTERS], dtype=np.uint64)
        out["counters"] = c.astype(np.float64)
        out["res_sample"] = _sample(res.res, res.res.numel(), DUMP_RES, 1).view(np.uint32).astype(np.float64)
        if res.out_bases is not None:
            nbytes = res.kept_bytes
            out["out_bases_sample"] = _sample(res.out_bases, nbytes, DUMP_STREAM, 2).astype(np.float32)
            if res.out_qual is not None:
                out["out_qual_sample"] = _sample(res.out_qual, nbytes, DUMP_STREAM, 3).astype(np.float32)
            cs = res.checksum()                      # the whole of res[] and both streams, 63 bits as two exact 32-bit halves
            out["checksum_hi_lo"] = np.array([cs >> 32, cs & 0xFFFFFFFF], dtype=np.float64)
    for k, a in out.items():
        np.save(os.path.join(d, k + suffix + ".npy"), a)
    return sorted(out)


def physical_cores():
    try:
        sibs = set()
        base = "/sys/devices/system/cpu"
        for d in os.listdir(base):
            p = os.path.join(base, d, "topology", "thread_siblings_list")
            if d.startswith("cpu") and d[3:].isdigit() and os.path.exists(p):
                sibs.add(open(p).read().strip())
        return len(sibs) or (os.cpu_count() or 1)
    except OSError:
        return os.cpu_count() or 1


def _pipe_cmds(config, ref, inp, out):
    """The reference command line of a config as a real pipe of single-threaded processes (last one writes `out`)."""
    ad = ADAPTER.decode()
    stages = {
        "cfg2": [["fastq_quality_trimmer", "-t", "20", "-l", "30"], ["fastq_quality_filter", "-q", "20", "-p", "80"]],
        "cfg3": [["fastx_clipper", "-a", ad, "-l", "15", "-n"]],
        "cfg4": [["fastx_reverse_complement"], ["fastx_trimmer", "-f", "5", "-l", "145"]],
        "cfg5shard": [["fastx_clipper", "-a", ad, "-l", "15", "-n"], ["fastq_quality_trimmer", "-t", "20", "-l", "30"], ["fastq_quality_filter", "-q", "20", "-p", "80"]],
        "stats": [["fastx_quality_stats"]],
    }[config]
    cmds = [[ref] + st for st in stages]
    cmds[0] += ["-i", inp]
    cmds[-1] += ["-o", out]
    return cmds


def cpu_baseline(config="cfg2", reads_per_pipe=250_000, one_pipe_reads=1_000_000, max_procs=128):
    """Reference CPU path on this box's host cores, bounded sample of the config's workload (rank 0, N=1 only).

    SURVEY 8d: the reference is single-threaded, so (i) ONE pipe of the config's tools is timed alone on its first 1 M reads and
    (ii) the input is split at record boundaries into chunks and as many pipes as the physical cores hold run concurrently;
    the aggregate rate is reported with the core counts next to it.
    """
    from concurrent.futures import ThreadPoolExecutor
    from oracle import fxoracle_py as fo
    cfg = CONFIGS[config]
    ref = fo.ref_binary()
    try:
        fo.lib()
    except Exception:
        return None
    logical, phys = os.cpu_count() or 2, physical_cores()
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
        if ref:
            per_pipe = len(_pipe_cmds(config, ref, "i", "o"))
            pipes = max(1, min(max_procs, phys) // per_pipe)
            nchunks = max(pipes, (one_pipe_reads + reads_per_pipe - 1) // reads_per_pipe)
            files = [os.path.join(td, "in%d.fq" % k) for k in range(nchunks)]

            def gen(k):
                with open(files[k], "wb") as f:
                    f.write(fo.synth_fastq(cfg["seed"], k * reads_per_pipe, reads_per_pipe, cfg["L"], cfg["adapter"]))
            with ThreadPoolExecutor(max_workers=min(logical, 32)) as ex:     # the generator is C (ctypes releases the GIL)
                list(ex.map(gen, range(nchunks)))
            one = os.path.join(td, "one.fq")                                 # the single pipe's input: the first one_pipe_reads reads
            n_one = (one_pipe_reads + reads_per_pipe - 1) // reads_per_pipe
            with open(one, "wb") as f:
                for k in range(n_one):
                    f.write(open(files[k], "rb").read())

            def run(inputs):
                t0 = time.perf_counter()
                procs = []
                for k, inp in enumerate(inputs):
                    cmds = _pipe_cmds(config, ref, inp, os.path.join(td, "out%d.fq" % k))
                    prev = None
                    for i, c in enumerate(cmds):
                        p = subprocess.Popen(c, stdin=prev.stdout if prev else None, stdout=subprocess.PIPE if i + 1 < len(cmds) else None)
                        if prev:
                            prev.stdout.close()
                        procs.append(p)
                        prev = p
                ok = all(p.wait() == 0 for p in procs)
                return ok, time.perf_counter() - t0
            ok1, dt1 = run([one])
            okp, dtp = run(files[:pipes])
            if ok1 and okp:
                n = pipes * reads_per_pipe
                return dict(value=round(n / dtp / 1e6, 4), unit="Mreads/s", cores=per_pipe * pipes, kind="reference",
                            kind_detail="the reference's libfastx object code (reader, writer, argument parsing, aligner: compiled in place from /root/reference/src/libfastx) under the tools' "
                                        "loop bodies as restated in oracle/ref_driver.cpp -- the tools' own main()s need an autoconf-generated config.h, for which no stand-in is written",
                            one_pipe_value=round(n_one * reads_per_pipe / dt1 / 1e6, 4), one_pipe_cores=per_pipe, one_pipe_reads=n_one * reads_per_pipe,
                            host_logical_cpus=logical, host_physical_cores=phys,
                            sample="%s: `%s`; first %d reads of the same seed-%d %d bp set as FASTQ text on tmpfs, split into %d chunks; each chunk piped "
                                   "through the reference libfastx reader/writer and aligner (compiled -O3 from /root/reference/src/libfastx) with the "
                                   "tools' loop bodies of oracle/ref_driver.cpp; %d concurrent single-threaded processes = %d cores "
                                   "(the box has %d physical cores / %d logical CPUs); one_pipe_value = one pipe (%d processes) alone on the first %d reads"
                                   % (config, cfg["what"], n, cfg["seed"], cfg["L"], pipes, per_pipe * pipes, per_pipe * pipes, phys, logical, per_pipe, n_one * reads_per_pipe))
        if cfg["params"] is None:
            return None                                   # (the plain-C port has no stand-alone statistics entry point worth timing)
        # fall back to the plain-C port (SoA in memory, no text I/O), 1 thread
        n = 1_000_000 if cfg["bound"] == "valu" else 4_000_000
        b, q = fo.synth_batch(cfg["seed"], 0, n, cfg["L"], cfg["adapter"])
        t0 = time.perf_counter()
        fo.run_pipeline(b, q, None, fo.make_params(**cfg["params"]))
        dt = time.perf_counter() - t0
        return dict(value=round(n / dt / 1e6, 4), unit="Mreads/s", cores=1, kind="port", host_logical_cpus=logical, host_physical_cores=phys,
                    sample="oracle/fxoracle.c on %d in-memory SoA reads (no FASTQ text parsing/formatting), 1 thread" % n)


def _gen_fastq(path, reads, seed=2, L=150, chunk=250_000):
    from concurrent.futures import ThreadPoolExecutor
    from oracle import fxoracle_py as fo
    with open(path, "wb") as f:
        with ThreadPoolExecutor(max_workers=min(os.cpu_count() or 2, 48)) as ex:     # the generator is C (ctypes releases the GIL)
            for part in ex.map(lambda k: fo.synth_fastq(seed, k * chunk, chunk, L, False), range(reads // chunk)):
                f.write(part)


def _same_bytes(parts, single, chunk=1 << 28):
    """cat(parts) == single, compared in parallel slices (numpy releases the GIL)."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    sizes = [os.path.getsize(f) for f in parts]
    if sum(sizes) != os.path.getsize(single):
        return False
    jobs, off = [], 0
    for f, n in zip(parts, sizes):
        for o in range(0, n, chunk):
            jobs.append((f, o, min(chunk, n - o), off + o))
        off += n

    def cmp(j):
        f, o, n, so = j
        return np.array_equal(np.fromfile(f, dtype=np.uint8, count=n, offset=o), np.fromfile(single, dtype=np.uint8, count=n, offset=so))
    with ThreadPoolExecutor(max_workers=16) as ex:
        return all(ex.map(cmp, jobs))


def e2e_leg(reads=16_000_000, big_reads=64_000_000, parts=4, lanes=2):
    """End to end on one GPU: FASTQ text on tmpfs -> the C tools (host/bin) -> FASTQ text; the same seed-2 reads the CPU baseline uses.

    `pipe`   = fastq_quality_trimmer -t 20 -l 30 | fastq_quality_filter -q 20 -p 80 (two processes, both on the GPU, as a user would type it)
    `fused`  = fastq_quality_trim_filter -t 20 -l 30 -q 20 -p 80 (one process, one pass; byte-identical output)
    `fused_to_devnull` = the same with -o /dev/null: what the tool does when the output file system is not the limit
    `sharded` = the same command with FXH_PARTS=k (host/fxh_parts.c): k byte ranges of the input cut at record boundaries, k runs side by
               side in the process (own reader threads, lanes and writer thread each), k output parts; md5 of their concatenation
    `sharded_big` = the sharded run on a sample four times the size (process start and the first HIP context are ~0.2 s of every run),
               checked byte for byte against the one-stream output of the same input
    Wall time of the command, file to file, best of two runs (the previous output is removed outside the timed region);
    Mreads/s and Gbases/s of INPUT."""
    import hashlib
    bindir = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin")
    trimmer, filt, fused = (os.path.join(bindir, t) for t in ("fastq_quality_trimmer", "fastq_quality_filter", "fastq_quality_trim_filter"))
    if not (os.path.exists(trimmer) and os.path.exists(filt)):
        return None
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
        inp = os.path.join(td, "in.fq")
        _gen_fastq(inp, reads)
        out = {"reads": reads, "input_bytes": os.path.getsize(inp)}

        def md5(paths):
            h = hashlib.md5()
            for path in paths:
                with open(path, "rb") as f:
                    for blk in iter(lambda: f.read(1 << 24), b""):
                        h.update(blk)
            return h.hexdigest()

        def timed(dst, name, fn, outfiles, nreads, want_md5=True):
            best = None
            for _ in range(2):                             # the first run pays the library load and context creation from cold caches
                for f in outfiles or []:
                    if os.path.exists(f):
                        os.unlink(f)
                t0 = time.perf_counter()
                ok = fn()
                dt = time.perf_counter() - t0
                if not ok:
                    return
                best = dt if best is None else min(best, dt)
            dst[name] = dict(wall_s=round(best, 3), mreads_s=round(nreads / best / 1e6, 2), gbases_s=round(nreads * 150 / best / 1e9, 3))
            if outfiles:
                dst[name]["output_bytes"] = sum(os.path.getsize(f) for f in outfiles)
                if want_md5:
                    dst[name]["output_md5"] = md5(outfiles)

        def pipe():
            p1 = subprocess.Popen([trimmer, "-t", "20", "-l", "30", "-i", inp], stdout=subprocess.PIPE)
            p2 = subprocess.Popen([filt, "-q", "20", "-p", "80", "-o", os.path.join(td, "pipe.fq")], stdin=p1.stdout)
            p1.stdout.close()
            return p1.wait() == 0 and p2.wait() == 0
        timed(out, "pipe", pipe, [os.path.join(td, "pipe.fq")], reads)
        if os.path.exists(fused):
            fa = [fused, "-t", "20", "-l", "30", "-q", "20", "-p", "80", "-i", inp]
            penv = dict(os.environ, FXH_PARTS=str(parts), FXH_LANES=str(lanes))
            pnames = [os.path.join(td, "part.%d.fq" % r) for r in range(parts)]
            one_env = dict(os.environ, FXH_ONE_FILE="0")       # the one-stream loop (one reader, lanes, ONE writer stream): what `-o FILE` was before round 5
            timed(out, "fused", lambda: subprocess.call(fa + ["-o", os.path.join(td, "fused.fq")]) == 0, [os.path.join(td, "fused.fq")], reads)
            timed(out, "fused_one_stream", lambda: subprocess.call(fa + ["-o", os.path.join(td, "fused1.fq")], env=one_env) == 0, [os.path.join(td, "fused1.fq")], reads)
            if "fused" in out and "fused_one_stream" in out:
                out["fused"]["identical_to_one_stream"] = out["fused"]["output_md5"] == out["fused_one_stream"]["output_md5"]
            timed(out, "fused_to_devnull", lambda: subprocess.call(fa + ["-o", "/dev/null"]) == 0, None, reads)
            timed(out, "sharded", lambda: subprocess.call(fa + ["-o", os.path.join(td, "part.%r.fq")], env=penv) == 0, pnames, reads)
            if "sharded" in out:
                out["sharded"].update(parts=parts, lanes_per_part=lanes, md5_of_concatenation_equals_fused=out["sharded"].get("output_md5") == out.get("fused", {}).get("output_md5"))
            if big_reads and "sharded" in out:
                for f in os.listdir(td):
                    os.unlink(os.path.join(td, f))
                _gen_fastq(inp, big_reads)
                big = {"reads": big_reads, "input_bytes": os.path.getsize(inp), "parts": parts, "lanes_per_part": lanes}
                single = os.path.join(td, "single.fq")
                timed(big, "one_stream", lambda: subprocess.call(fa + ["-o", single], env=one_env) == 0, [single], big_reads, want_md5=False)
                onef = os.path.join(td, "one_file.fq")
                timed(big, "one_file", lambda: subprocess.call(fa + ["-o", onef]) == 0, [onef], big_reads, want_md5=False)
                if "one_file" in big and "one_stream" in big:
                    big["one_file"]["identical_to_one_stream"] = _same_bytes([onef], single)
                    # what crossed the PCIe link, per read and per second, in the default command: the text goes up once, the formatted text comes down once
                    ob, dtw = big["one_file"]["output_bytes"], big["one_file"]["wall_s"]
                    big["one_file"]["link"] = dict(bytes_up_per_read=round(big["input_bytes"] / big_reads, 1), bytes_down_per_read=round(ob / big_reads, 1),
                                                   up_gbs_over_wall=round(big["input_bytes"] / dtw / 1e9, 1), down_gbs_over_wall=round(ob / dtw / 1e9, 1))
                    # the link's own rate in this call (scripts/ubench/pcie_bw: 64 MB blocks from page-locked memory, four streams, both directions at once)
                    pb = os.path.join(ROOT, "scripts", "ubench", "pcie_bw")
                    if os.path.exists(pb):
                        try:
                            txt = subprocess.run([pb], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120).stdout.decode()
                            row = [l for l in txt.splitlines() if l.startswith("4 stream(s), input hipHostRegister")][0]
                            nums = [float(x) for x in __import__("re").findall(r"[0-9]+\.[0-9]+", row)]
                            lk = big["one_file"]["link"]
                            lk.update(ubench_up_alone_gbs=nums[0], ubench_down_alone_gbs=nums[1], ubench_each_way_both_busy_gbs=nums[2],
                                      up_frac_of_both_busy=round(lk["up_gbs_over_wall"] / nums[2], 3), down_frac_of_both_busy=round(lk["down_gbs_over_wall"] / nums[2], 3),
                                      note="GB/s over the whole wall time of the command (start-up and exit included), against the link measured in this call")
                        except Exception:
                            pass
                if os.path.exists(onef):
                    os.unlink(onef)
                timed(big, "sharded", lambda: subprocess.call(fa + ["-o", os.path.join(td, "part.%r.fq")], env=penv) == 0, pnames, big_reads, want_md5=False)
                if "sharded" in big and "one_stream" in big:
                    big["concatenation_identical_to_one_stream"] = _same_bytes(pnames, single)
                # one GPU's share of the 8-GPU box: 16 of the node's 64 cores (32 of its 128 CPUs) for the whole tool -- readers, lanes, writers
                share = _cpu_share(16)
                if share:
                    timed(big, "sharded_host_share_16c", lambda: subprocess.call(fa + ["-o", os.path.join(td, "part.%r.fq")], env=penv,
                                                                                  preexec_fn=lambda: os.sched_setaffinity(0, share)) == 0, pnames, big_reads, want_md5=False)
                    timed(big, "one_file_host_share_16c", lambda: subprocess.call(fa + ["-o", onef], preexec_fn=lambda: os.sched_setaffinity(0, share)) == 0, [onef], big_reads, want_md5=False)
                    if os.path.exists(onef):
                        os.unlink(onef)
                    if "sharded_host_share_16c" in big:
                        big["sharded_host_share_16c"].update(cpus=len(share), cores=16, note="the same sharded command restricted to 16 physical cores (with their SMT siblings) of the "
                                                             "GPU's NUMA node: what each GPU's tool chain has on an 8-GPU box with 2 x 64 cores")
                out["sharded_big"] = big
        if "pipe" in out and "fused" in out:
            out["fused_equals_pipe"] = out["pipe"]["output_md5"] == out["fused"]["output_md5"]
        if "fused" in out:
            # what a user gets WITHOUT knowing any knob: the reference's own command line, one process, no environment variables, ONE output file.
            # Since round 5 a regular-file input of >= 512 MB is run by many strands into that one file (host/fxh_strands.c); `one_stream` is the
            # loop it replaces (FXH_ONE_FILE=0), `sharded` the k-part form that no reference caller would type (-o out.%r.fq).
            bigd = out.get("sharded_big", {})
            out["default_invocation"] = dict(command="fastq_quality_trim_filter -t 20 -l 30 -q 20 -p 80 -i in.fq -o out.fq", env="none",
                                             sample_16m=out["fused"], sample_64m=bigd.get("one_file"),
                                             sample_64m_one_stream_before=bigd.get("one_stream"), sample_64m_four_part_files=bigd.get("sharded"),
                                             sink_note="one tmpfs file takes fresh pages from one thread at a time: 9 GB/s through one pwrite() stream, 4-5 GB/s through many, "
                                                       "10.5 GB/s with fallocate() and parallel copies taking turns (this tool's sink; 15 GB/s after a head start), 30-90 GB/s into "
                                                       "k files -- profiles/r05/a_one_file_write.txt, d_one_file_gate.txt")
        return out


def _cpu_share(cores):
    """`cores` physical cores (all their SMT siblings) out of the CPUs this process may use, lowest numbered first; None if there are not more than that."""
    try:
        allowed = os.sched_getaffinity(0)
        groups, seen = [], set()
        for c in sorted(allowed):
            if c in seen:
                continue
            sib = set()
            for part in open("/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list" % c).read().strip().split(","):
                a, _, b = part.partition("-")
                sib.update(range(int(a), int(b or a) + 1))
            sib &= allowed
            seen |= sib
            groups.append(sib)
        if len(groups) <= cores:
            return None
        out = set()
        for g in groups[:cores]:
            out |= g
        return out
    except Exception:
        return None


def _gpu_node_cpus(index):
    """(NUMA node, its CPUs) of GPU `index`, or (None, None): the boxes are two-socket machines with four GPUs per node, and a tool
    process whose page-locked buffers sit on the other socket uploads across the socket link (profiles/r03/z_e2e_numa.txt: -8 %)."""
    try:
        import torch
        pr = torch.cuda.get_device_properties(index)
        bdf = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        node = int(open("/sys/bus/pci/devices/%s/numa_node" % bdf).read())
        if node < 0:
            return None, None
        cpus = set()
        for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
            a, _, b = part.partition("-")
            cpus.update(range(int(a), int(b or a) + 1))
        cpus &= os.sched_getaffinity(0)
        return (node, cpus) if cpus else (None, None)
    except Exception:
        return None, None


class _on_gpu_node:
    """The launcher's part of NUMA placement: this process (and the tool processes and tmpfs pages it creates) on the CPUs of the GPU's node."""
    def __init__(self, index):
        self.node, self.cpus = _gpu_node_cpus(index)
    def __enter__(self):
        self.saved = os.sched_getaffinity(0)
        if self.cpus and not os.environ.get("FXG_BENCH_NO_NUMA"):
            os.sched_setaffinity(0, self.cpus)
        else:
            self.node = None
        return self
    def __exit__(self, *exc):
        os.sched_setaffinity(0, self.saved)
        return False


def e2e_ranks(config, rank, local, world, reads_per_rank, dist, device):
    """--e2e: the config's command line end to end, one process per GPU, weak scaling like the kernel line (reads_per_rank x world reads in all).

    A config that is ONE tool (cfg2, cfg3, cfg5shard) runs the way a user of a multi-GPU node runs it: ONE input file, ONE output file, the same command
    line on every rank with FXH_RANK / FXH_WORLD in the environment (host/fxh_strands.c: rank g takes byte range g of the input, keeps its formatted text
    on its GPU, the ranks exchange their counter blocks in one RCCL all-gather opened by the tool itself, every rank writes its slice of the output at the
    sum of the bytes before it; rank 0 prints the report).  A config that is a pipe of reference tools (cfg4) has no file for ranks to share: every rank
    runs the pipe on its own shard.  Barrier on both sides, the slowest rank's wall time counts; FASTQ text on tmpfs in and out."""
    import torch
    cfg = CONFIGS[config]
    bindir = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin")
    ad = ADAPTER.decode()
    tf = ["fastq_quality_trim_filter", "-t", "20", "-l", "30", "-q", "20", "-p", "80"]
    chain = {"cfg2": [tf], "cfg3": [["fastx_clipper", "-a", ad, "-l", "15", "-n"]],
             "cfg4": [["fastx_reverse_complement"], ["fastx_trimmer", "-f", "5", "-l", "145"]],
             "cfg5shard": [["fastx_clip_trim_filter", "-a", ad, "-l", "15", "-n", "-t", "20", "-m", "30", "-q", "20", "-p", "80"]]}[config]
    from concurrent.futures import ThreadPoolExecutor
    from oracle import fxoracle_py as fo
    import hashlib
    import shutil
    one_job = len(chain) == 1
    cpu_or_dev = device if (world > 1 and dist.get_backend() == "nccl") else "cpu"
    shared = [tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)] if rank == 0 else [None]
    if world > 1:
        dist.broadcast_object_list(shared, src=0)
    jobdir = shared[0]
    td = jobdir if one_job else os.path.join(jobdir, "rank%d" % rank)
    os.makedirs(td, exist_ok=True)
    try:
        inp, outp = os.path.join(td, "in.fq"), os.path.join(td, "out.fq")
        chunk = 250_000
        first = rank * reads_per_rank
        with ThreadPoolExecutor(max_workers=max(2, min(32, (os.cpu_count() or 2) // max(1, world)))) as ex:
            parts = list(ex.map(lambda k: fo.synth_fastq(cfg["seed"], first + k * chunk, chunk, cfg["L"], cfg["adapter"]), range(reads_per_rank // chunk)))
        my_bytes = sum(len(x) for x in parts)
        off = 0
        if one_job and world > 1:                 # the ranks' shards side by side in the ONE input file
            sizes = [None] * world
            dist.all_gather_object(sizes, my_bytes)
            off = sum(sizes[:rank])
            if rank == 0:
                open(inp, "wb").close()
            dist.barrier()
        with open(inp, "r+b" if (one_job and world > 1) else "wb") as f:
            f.seek(off)
            for x in parts:
                f.write(x)
        del parts
        env = dict(os.environ, FXG_DEVICE=str(local))
        env.pop("FXG_DEVICES", None)
        if one_job:
            env.update(FXH_RANK=str(rank), FXH_WORLD=str(world), FXH_RENDEZVOUS=os.path.join(td, "job.rdv"), FXG_COMM_JOB=os.path.basename(jobdir))
            if os.environ.get("FXG_BENCH_FAKE_RCCL"):     # ranks sharing ONE GPU (the test box): RCCL refuses two ranks on a device, the test-only transport does not
                env["LD_LIBRARY_PATH"] = os.environ["FXG_BENCH_FAKE_RCCL"] + os.pathsep + env.get("LD_LIBRARY_PATH", "")
                env["FXG_FAKE_RCCL_HIP"] = "1"
        else:
            env["FXH_CLIP_PARALLEL"] = "1"

        def once():
            if (rank == 0 or not one_job) and os.path.exists(outp):
                os.unlink(outp)
            if world > 1:
                dist.barrier()
            t0 = time.perf_counter()
            procs, prev = [], None
            for i, st in enumerate(chain):
                cmd = [os.path.join(bindir, st[0])] + st[1:] + (["-i", inp] if i == 0 else []) + (["-o", outp] if i + 1 == len(chain) else [])
                p = subprocess.Popen(cmd, env=env, stdin=prev.stdout if prev else None, stdout=subprocess.PIPE if i + 1 < len(chain) else None)
                if prev:
                    prev.stdout.close()
                procs.append(p)
                prev = p
            ok = all(p.wait() == 0 for p in procs)
            dt = time.perf_counter() - t0
            t = torch.tensor([dt, 0.0 if ok else 1.0], dtype=torch.float64, device=cpu_or_dev)
            if world > 1:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t[0]), float(t[1]) == 0.0
        best = None
        for _ in range(2):
            dt, ok = once()
            if not ok:
                return {"error": "a tool of the chain failed"}
            best = dt if best is None else min(best, dt)
        recs, nbytes = 0, 0
        if rank == 0 or not one_job:
            with open(outp, "rb") as f:
                for blk in iter(lambda: f.read(1 << 24), b""):
                    recs += blk.count(b"\n"); nbytes += len(blk)
        t = torch.tensor([recs // 4, nbytes], dtype=torch.int64, device=cpu_or_dev)
        if world > 1:
            dist.all_reduce(t)
        total = reads_per_rank * world
        # the job's output: the one file, or the ranks' private outputs in rank order -- its md5 must not depend on the number of ranks
        names = [outp]
        if world > 1 and not one_job:
            names = [None] * world
            dist.all_gather_object(names, outp)
        md5 = None
        if rank == 0:
            h = hashlib.md5()
            for fn in names:
                with open(fn, "rb") as f:
                    for blk in iter(lambda: f.read(1 << 24), b""):
                        h.update(blk)
            md5 = h.hexdigest()
        if world > 1:
            dist.barrier()
        return dict(command=" | ".join(" ".join(st) for st in chain), reads_per_rank=reads_per_rank, ranks=world, wall_s=round(best, 3),
                    mreads_s=round(total / best / 1e6, 2), gbases_s=round(total * cfg["L"] / best / 1e9, 3), kept_reads=int(t[0]), output_bytes=int(t[1]),
                    output_md5=md5, mode="one input file, one output file, the tool's own rank mode (FXH_RANK / FXH_WORLD, RCCL epilogue inside the tool)" if one_job else
                    "one pipe of reference tools per rank on its own shard",
                    note="barrier to barrier, slowest rank, best of two; output_md5 is equal for every number of ranks over the same reads")
    finally:
        if world > 1:
            dist.barrier()
        if rank == 0:
            shutil.rmtree(jobdir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=sorted(CONFIGS), default="cfg2")
    ap.add_argument("--reads", type=int, default=0, help="reads per GPU (default: the configuration's size)")
    ap.add_argument("--full", action="store_true", help="after the headline: the CPU baseline, the other BASELINE configs and the tools end to end (one GPU)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-e2e", action="store_true", help="--full without the tools end to end")
    ap.add_argument("--e2e", action="store_true", help="also time the config's command line end to end, one tool chain per GPU (weak scaling; any --gpus)")
    ap.add_argument("--e2e-reads", type=int, default=32_000_000, help="reads per rank of the --e2e leg")
    ap.add_argument("--decision-only", action="store_true", help="no compaction: 154 B/read variant (not the headline)")
    ap.add_argument("--headline-only", action="store_true", help="--full without the other BASELINE configs")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs of the measured config as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")

    import torch
    import torch.distributed as dist
    from fastx_toolkit_amd import Engine, make_params
    from fastx_toolkit_amd import distributed as fxd

    rank, local, world = fxd.init_from_env()
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run" % (args.gpus, world))
    if os.environ.get("FXG_BENCH_SHARED_GPU"):      # smoke-testing the N>1 path on a 1-GPU box (with FXG_DIST_BACKEND=gloo)
        local = 0
    torch.cuda.set_device(local)
    # One stream for everything: torch allocations/fills, the engine's kernels (it adopts torch's current stream) and the
    # RCCL all-gather, which orders itself after that stream -- so the gather reads the counters of the pass just enqueued.
    torch.cuda.set_stream(torch.cuda.Stream(device=local))
    eng = Engine(local)

    def measure(config, steps, warmup, reads, want_e2e, dump=None):
        cfg = CONFIGS[config]
        R, L = (reads or cfg["reads"]), cfg["L"]
        lo = rank * R                                  # weak scaling: rank g owns reads [g*R, (g+1)*R) of the global set
        bases, qual = eng.synth(cfg["seed"], lo, R, L, cfg["adapter"])
        is_stats = cfg["params"] is None
        compact = not args.decision_only and not is_stats
        if is_stats:
            hist = torch.zeros((L, 5, 128), dtype=torch.int64, device=eng.device)
            counters_dev = torch.zeros(24, dtype=torch.int64, device=eng.device)
        else:
            params = make_params(**cfg["params"])
            # per-kept-read metadata (out_len / kept_index / out_off, 14 B per kept read) is not requested: the packed stream and res[] are
            outs = eng.alloc_outputs(R, L, compact=compact, meta=False)
        torch.cuda.synchronize()

        gathered = [None]

        def step():
            if is_stats:
                eng.quality_stats(bases, qual, fixed_len=L, hist=hist, sync=False)
                return None
            r = eng.run(bases, qual, params, fixed_len=L, compact=compact, meta=False, outputs=outs)
            if world > 1:
                gathered[0] = fxd.gather_counters(outs["counters"])   # 192-byte all-gather, enqueued after the kernels, no host sync
            return r

        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        # HIP events around the dominant kernel of every TIMED launch (two event records per step on the launch stream, read after the final
        # synchronisation: a ring of the last 64 launches in the context) -- kernel_ms_avg below is of these very launches
        eng.set_profiling(True)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            res = step()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        kms = eng.profiled_kernel_ms(min(steps, 64))
        eng.set_profiling(False)
        dumped = None
        if dump:                                       # after the timed region: sampling and the checksum are not timed
            dumped = dump_outputs(dump, "" if world == 1 else "_rank%d" % rank, res=None if is_stats else res,
                                  hist=hist if is_stats else None, per_step=warmup + steps)
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=eng.device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())

        if is_stats:
            kept, kept_bytes = R, R * L
            assert int(hist.sum().item()) == R * L * (warmup + steps)
        else:
            counters = res.counters
            kept, kept_bytes = int(counters[1]), int(counters[2])
            if world > 1:                              # job totals and this rank's offsets in the global output, from the last step's gather
                totals, read_off, byte_off, _ = fxd.offsets_from_gathered(gathered[0], rank)
                assert int(totals[0]) == R * world

        kavg = sum(kms) / len(kms)          # the timed loop's own launches (the last min(steps, 64) of them)
        launch = eng.last_launch()
        # algorithmic bytes per launch: read 2L per read, write 4 B result per read + 2*new_len per kept read
        if is_stats:
            alg_bytes = R * 2 * L
        else:
            alg_bytes = R * (2 * L + 4) + 2 * kept_bytes if compact else R * (L + 4)
        achieved = alg_bytes / (kavg * 1e-3) / 1e9
        # what the launches produced: counters and a device-side checksum of res[] + the packed stream, against the pinned tuple
        # EVERY rank checks its own shard (rank g's tuple is EXPECTED[config][g]); the verdicts are reduced so that one bad rank fails the whole job
        self_check = None
        if not is_stats and compact:
            pinned = EXPECTED.get(config) if R == cfg["reads"] else None
            exp = pinned[rank] if pinned and rank < len(pinned) else None
            got = (kept, kept_bytes, res.checksum())
            ok = None if exp is None else bool(got[:2] == tuple(exp[:2]) and (exp[2] is None or got[2] == exp[2]))
            verdicts = [(rank, ok, got)]
            if world > 1:
                verdicts = [None] * world
                dist.all_gather_object(verdicts, (rank, ok, got))
                verdicts = [v for v in verdicts]
            bad = [v for v in verdicts if v[1] is False]
            self_check = dict(kept=got[0], kept_bases=got[1], checksum=got[2], pinned=list(exp) if exp else None, matches_pinned=ok,
                              ranks_checked=sum(1 for v in verdicts if v[1] is not None), ranks_ok=sum(1 for v in verdicts if v[1] is True),
                              ranks_unpinned=[v[0] for v in verdicts if v[1] is None],
                              per_rank=[dict(rank=v[0], ok=v[1], kept=v[2][0], kept_bases=v[2][1], checksum=v[2][2]) for v in verdicts] if world > 1 else None)
            if bad:
                raise SystemExit("bench self-check failed on rank(s) %s: launches produced %r, pinned %r" % (
                    [v[0] for v in bad], [v[2] for v in bad], [pinned[v[0]] for v in bad]))
        # HBM traffic: rocprofv3 FETCH_SIZE / WRITE_SIZE passes of this config (scripts/pmc_traffic.py), attached only when they were
        # collected on the SAME kernel sources (hash of fastx_toolkit_amd/csrc) and the same launch shape
        traffic, traffic_source = None, None
        pmc = os.path.join(ROOT, "profiles", "pmc_traffic_%s.json" % config)
        if os.path.exists(pmc):
            try:
                pj = json.load(open(pmc))
                if pj.get("reads_per_launch") == R and (compact or is_stats) and pj.get("csrc_sha16") == csrc_sha16() and pj.get("kernel_name", "").split("(")[0].replace(",1>", ">").replace(",false>", ">").replace(",true>", ">") in launch["kernel"].replace(" ", ""):
                    traffic = pj.get("hbm_bytes_per_launch")
                    traffic_source = "replayed from profiles/pmc_traffic_%s.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of %s on csrc %s); not measured in this run" % (
                        config, pj.get("command", "scripts/pmc_run.py"), pj.get("csrc_sha16"))
                else:
                    traffic_source = "profiles/pmc_traffic_%s.json is of other kernel sources or another launch shape: not attached" % config
            except Exception:
                traffic = None

        e2e_r = None
        if want_e2e and not is_stats:
            try:
                with _on_gpu_node(local) as place:
                    e2e_r = e2e_ranks(config, rank, local, world, args.e2e_reads, dist, eng.device)
                if isinstance(e2e_r, dict):
                    e2e_r["numa_node"] = place.node                 # the tool chain ran on its GPU's NUMA node (None: not pinned)
            except Exception as e:
                e2e_r = {"error": repr(e)[:200]}
        if rank == 0:
            total_reads = R * world * steps
            out = {
                "metric": cfg["metric"],
                "value": round(total_reads / dt / 1e6, 2),
                "unit": "Mreads/s",
                "n_gpus": world, "steps": steps, "warmup": warmup,
                "ms_per_step": round(dt / steps * 1e3, 4),
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "f32" if cfg["bound"] == "valu" else "u8", "data": "synthetic",
                "config": {
                    "workload": "%s: %s, %d x %d bp Phred+33 reads per GPU, %s" % (
                        config, cfg["what"], R, L,
                        "histogram hist[column][A,C,G,T,N][quality] accumulated on the device" if is_stats else
                        "one fused pass with order-preserving compaction of the kept trimmed reads (packed bases + qualities and the 4-byte per-read "
                        "result res[]; the optional per-kept-read out_len/kept_index/out_off arrays are not requested)" if compact
                        else "decision-only pass (no compaction)"),
                    "reads_per_gpu": R, "read_len": L, "seed": cfg["seed"], "kept_reads_per_gpu": kept, "kept_bases_per_gpu": kept_bytes,
                    "gbases_per_s_in": round(total_reads * L / dt / 1e9, 2), "parallelism": "reads sharded x%d, no data-path collective" % world,
                },
            }
            hbm = {
                "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": traffic, "traffic_source": traffic_source,
                "algorithmic_bytes_per_launch": alg_bytes, "bytes_per_read": round(alg_bytes / R, 2),
                "traffic_over_algorithmic": round(traffic / alg_bytes, 4) if traffic else None,
            }
            shape = {"kernel": launch["kernel"], "kernel_ms_avg": round(kavg, 4), "kernel_ms_min": round(min(kms), 4), "kernel_ms_launches": len(kms),
                     "kernel_ms_source": "HIP events around the dominant kernel of the timed loop's own launches (fxg_profiled_kernel_ms)",
                     "grid": launch["grid"], "block": launch["block"], "lds_bytes": launch["lds"], "tile_reads": launch["tile_reads"]}
            if cfg["bound"] == "valu":
                # the aligner is a per-thread fp32 dynamic program: L x 13 cells per read, bounded by VALU issue, not by HBM -- the roofline object
                # describes THAT resource; the HBM figures (low by construction) sit in the sub-object
                cells = R * L * len(ADAPTER)
                gcups = cells / (kavg * 1e-3) / 1e9
                glane = gcups * CLIP_MIN_VALU_PER_CELL
                issued = {}
                sq = os.path.join(ROOT, "profiles", "pmc_sq_%s.json" % config)
                if os.path.exists(sq):
                    try:
                        sj = json.load(open(sq))
                        if sj.get("csrc_sha16") == csrc_sha16():
                            ipc = float(sj["valu_instr_per_cell"])
                            issued = {"issued_valu_instr_per_cell": ipc, "issued_frac": round(gcups * ipc / VALU_PEAK_GLANEOPS, 4),
                                      "issued_source": "replayed from profiles/pmc_sq_%s.json (rocprofv3 --pmc SQ_INSTS_VALU of %s on csrc %s): SQ_INSTS_VALU x 64 / cells, "
                                                       "whole kernel (both passes, staging, write-out); not measured in this run" % (config, sj.get("command", "scripts/pmc_sq.sh"), sj.get("csrc_sha16"))}
                        else:
                            issued = {"issued_source": "profiles/pmc_sq_%s.json is of other kernel sources: not attached" % config}
                    except Exception:
                        issued = {}
                out["roofline"] = {
                    "bound": "valu", "achieved": round(glane, 1), "peak": round(VALU_PEAK_GLANEOPS, 1), "unit": "G lane-ops/s",
                    "frac": round(glane / VALU_PEAK_GLANEOPS, 4), "traffic": traffic,
                    "gcups": round(gcups, 1), "cells_per_launch": cells,
                    # frac prices every cell of the L x 13 matrix at the fewest VALU instructions the reference's score recurrence takes on this ISA;
                    # a kernel cannot raise it by issuing more
                    "useful_valu_instr_per_cell": CLIP_MIN_VALU_PER_CELL, "useful_frac": round(glane / VALU_PEAK_GLANEOPS, 4),
                    "useful_note": "5 = v_cmp_eq (read base == adapter base) + v_cndmask (pair score +1 / -1) + v_add_f32 (diagonal candidate) + v_max3_f32 "
                                   "(diag, up, left; the -5 of `up` and `left` comes from one shared subtraction) + v_add_f32 (S - 5 kept beside S): the score "
                                   "recurrence of sequence_alignment.cpp:380-417 alone, no path summary, no staging, no write-out.  (Round 6 takes the pair score "
                                   "out of an LDS table, 3 VALU instructions per cell in pass 1; the yardstick stays at 5 so that rounds compare.)",
                    **issued, **shape, "hbm": hbm,
                    "note": "bound is VALU issue; peak = 256 CUs x 4 SIMDs x 64 lanes / %.0f cycles x 2.4 GHz (MI355X_MICROARCH.md: one wave64 VALU instruction "
                            "per 2 cycles per SIMD); achieved = cells/s x 5 (frac = useful_frac: this run's timing only)" % VALU_CYCLES,
                }
            else:
                out["roofline"] = {
                    "bound": "hbm", **hbm, **shape,
                    **({"note": "not measured in this run: a plain streaming kernel that reads 15 GB and writes 7.3 GB (this config's algorithmic bytes, nothing "
                                "else) takes 4.21-4.56 ms on this part (4.21-4.38 with every workgroup in one narrow window, loads a trip ahead and the non-temporal policy both ways), "
                                "read alone 2.20-2.50 ms, write alone 1.17-1.25 ms (scripts/ubench/read_stream.hip, mix_rw.hip; profiles/r06/x_read_stream_*.txt, profiles/r02/z_mix_rw.txt)"}
                       if config == "cfg2" and compact else {}),
                }
            if self_check is not None:
                out["self_check"] = self_check
            if e2e_r is not None:
                out["e2e_ranks"] = e2e_r
            if dumped is not None:
                out["dumped_outputs"] = dict(dir=os.path.abspath(dump), arrays=dumped)
            return out
        return None

    out = measure(args.config, args.steps, args.warmup, args.reads, args.e2e, dump=args.dump_outputs)
    # Everything below takes runs of its own (about 160 s on one MI355X; a whole plain run takes about 3 s), so it is done with --full only.
    if rank == 0:
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.config)
        # Every BASELINE config in one invocation (round-4 verdict item 3): after the headline line's own measurement the other
        # workloads run in this process at their stated sizes (buffers freed in between: config 4 alone needs 120 GB), each with its roofline object,
        # its self-check against the oracle-verified tuple and the reference's CPU rate on a bounded sample.  The headline keys stay what they were.
        if world == 1 and args.full and args.config == "cfg2" and not args.reads and not args.decision_only and not args.headline_only:
            out["configs"] = {}
            for c in ("cfg3", "cfg4", "cfg5shard", "stats"):
                torch.cuda.empty_cache()
                try:
                    t0 = time.perf_counter()
                    o = measure(c, max(5, args.steps // 2), min(args.warmup, 2), 0, False)
                    line = {k: o[k] for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "dtype", "config", "roofline") if k in o}
                    if "self_check" in o:
                        line["self_check"] = o["self_check"]
                    if not args.no_cpu_baseline:
                        line["cpu_baseline"] = cpu_baseline(c)
                    line["wall_s_incl_generation_and_cpu_baseline"] = round(time.perf_counter() - t0, 1)
                    out["configs"][c] = line
                    # the same figures in brief INSIDE the headline's roofline object, which is a key every consumer of the line keeps
                    rf, sc, cb = line.get("roofline", {}), line.get("self_check") or {}, line.get("cpu_baseline") or {}
                    hb = rf.get("hbm", rf)
                    out["roofline"].setdefault("other_configs", {})[c] = {
                        "workload": CONFIGS[c]["what"], "reads": CONFIGS[c]["reads"], "read_len": CONFIGS[c]["L"], "mreads_s": line.get("value"),
                        "ms_per_step": line.get("ms_per_step"), "kernel": rf.get("kernel"), "kernel_ms_avg": rf.get("kernel_ms_avg"), "bound": rf.get("bound"),
                        "frac": rf.get("frac"), "issued_frac": rf.get("issued_frac"), "gcups": rf.get("gcups"), "hbm_frac": hb.get("frac"),
                        "traffic_over_algorithmic": hb.get("traffic_over_algorithmic"), "self_check_matches_pinned": sc.get("matches_pinned"),
                        "cpu_baseline_mreads_s": cb.get("value"), "cpu_baseline_cores": cb.get("cores"), "cpu_baseline_kind": cb.get("kind")}
                except SystemExit:
                    raise
                except Exception as e:                     # a failing extra config must not take the headline line down -- but it must be seen
                    out["configs"][c] = {"error": repr(e)[:300]}
            torch.cuda.empty_cache()
        if world == 1 and args.full and not args.no_e2e and args.config == "cfg2":
            try:
                with _on_gpu_node(local) as place:
                    out["e2e"] = e2e_leg()
                out["e2e"]["numa_node"] = place.node
            except Exception as e:                         # the end-to-end leg must never take the headline line down
                out["e2e"] = {"error": repr(e)[:200]}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    eng.close()


if __name__ == "__main__":
    main()
