"""What the context-state tier shares between its CPU half (tests/test_context_state_cpu.py) and its GPU half (tests/test_gpu_context_state.py):

  * FIRST_CALLS: one row per entry point of csrc/fxg_engine.hip that takes a context, saying how the call must end when it is the FIRST call a new
    context sees -- 0 and the reference's answer, or the documented refusal (code, fxg_last_error text, outputs untouched);
  * the requests that reach each of the 43 tile kernels by name, and the launch sequences of the kernel-attribute tests built from them;
  * the grow rule of the context's workspaces (fxg_ws_grow's callers) as plain arithmetic, so that a table of "which step regrows what" can be
    held against it;
  * the attribute policy the engine had before csrc/fxg_attr.h, as a model, so that the invariant test can be shown to fail on it.

Nothing here needs a GPU or torch at import.
"""
import zlib

import numpy as np

from helpers import CLIP_BUCKETS, CLIP_MAX_ADAPTER, random_batch

E_INVALID = -1
OK = "ok"


def refusal(text, code=E_INVALID, device=True):
    """device=False: the check needs no device state, so the CPU tier's stub refuses the same way"""
    return ("refused", code, text, device)


# (id, the entry point that is the new context's first call, outcome)
FIRST_CALLS = [
    ("destroy_untouched", "fxg_ctx_destroy", OK),
    ("last_error_empty", "fxg_last_error", OK),
    ("set_stream", "fxg_set_stream", OK),
    ("sync", "fxg_sync", OK),
    ("device_info", "fxg_device_info", OK),
    ("malloc_device", "fxg_malloc_device", OK),
    ("free_device", "fxg_free_device", OK),
    ("malloc_host", "fxg_malloc_host", OK),
    ("free_host", "fxg_free_host", OK),
    ("memcpy_h2d", "fxg_memcpy_h2d", OK),
    ("memcpy_d2h", "fxg_memcpy_d2h", OK),
    ("memset_device", "fxg_memset_device", OK),
    ("timer_start", "fxg_timer_start", OK),
    ("timer_stop", "fxg_timer_stop", OK),
    ("host_register", "fxg_host_register", OK),
    ("host_unregister", "fxg_host_unregister", OK),                               # (of a range another context registered: the registration is the process's)
    ("concat_peer", "fxg_concat_peer", OK),
    ("set_profiling", "fxg_set_profiling", OK),
    ("last_kernel_ms_nothing_profiled", "fxg_last_kernel_ms", refusal("no profiled launch recorded")),
    ("profiled_kernel_ms_none", "fxg_profiled_kernel_ms", OK),
    ("last_launch_info_none", "fxg_last_launch_info", OK),
    ("scan_recoveries_zero", "fxg_scan_recoveries", OK),
    ("synth", "fxg_synth_generate", OK),
    ("run_rows", "fxg_run_pipeline", OK),
    ("run_tiles", "fxg_run_pipeline", OK),
    ("run_clip", "fxg_run_pipeline", OK),
    ("run_qtrim_qfilter", "fxg_run_qtrim_qfilter", OK),
    ("run_clip_entry", "fxg_run_clip", OK),
    ("run_revcomp_trim", "fxg_run_revcomp_trim", OK),
    ("quality_stats", "fxg_run_quality_stats", OK),
    ("read_counters_zeroed", "fxg_read_counters", OK),
    ("fastq_index", "fxg_fastq_index", OK),
    ("fastq_pack_other_contexts_lines", "fxg_fastq_pack", OK),
    ("fastq_format_opts_len_no_res", "fxg_fastq_format_opts", OK),
    ("fastq_format_plain", "fxg_fastq_format", OK),
    ("fasta_weights_unindexed", "fxg_fasta_weights", refusal("fxg_fasta_weights: index the block first")),
    ("barcode_prepare", "fxg_barcode_prepare", OK),
    ("barcode_split_without_prepare", "fxg_barcode_split", refusal("fxg_barcode_split: no table (fxg_barcode_prepare)", device=False)),
    ("fasta_reflow", "fxg_fasta_reflow", OK),
    ("fasta_reflow_empty_closes_record", "fxg_fasta_reflow", OK),
    ("fasta_uncollapse_from_zero", "fxg_fasta_uncollapse", OK),
    ("fasta_uncollapse_continue_nothing", "fxg_fasta_uncollapse",
     refusal("fxg_fasta_uncollapse: copy_begin > 0 continues a block, and the context holds no scans of 5 records numbered from 8 on")),
    ("clip_history_then_batch", "fxg_set_clip_history", OK),
    ("bases_change_other_contexts_lines", "fxg_bases_change", OK),
    ("bases_change_no_records", "fxg_bases_change", OK),
    ("collapse_begin", "fxg_collapse_begin", OK),
    ("collapse_add_no_set", "fxg_collapse_add", refusal("fxg_collapse_add: no set; fxg_collapse_begin makes one", device=False)),
    ("collapse_order_no_set", "fxg_collapse_order", refusal("fxg_collapse_order: no set; fxg_collapse_begin makes one", device=False)),
    ("collapse_write_no_set", "fxg_collapse_write", refusal("fxg_collapse_write: no set; fxg_collapse_begin makes one", device=False)),
    ("collapse_add_other_contexts_lines", "fxg_collapse_add", OK),                # (the first call after begin, on line arrays another context made)
]


# What a refused collapser call leaves in its results (include/fxg.h): a call refused for the set's state leaves *info zeroed with first_bad = ~0, a
# refused write leaves *window zeroed with rank_end = rank_begin; d_out is untouched.
COLLAPSE_INFO_FIELDS = ("records", "reads", "uniques", "slots", "rebuilds", "first_bad", "out_reads", "out_bytes", "irregular")
COLLAPSE_INFO_REFUSED = (0, 0, 0, 0, 0, (1 << 64) - 1, 0, 0, 0)


# ---- the 43 tile kernels ---------------------------------------------------------------------------------------------------------------
QTF = dict(qt_threshold=20, qt_min_len=30, qf_min_quality=20, qf_min_percent=80)
CLIP_GENERAL = [16, 32, 64, 100]
KNOBS = ("FXG_TILE", "FXG_CLIP_DEPTH_RT", "FXG_ROWS", "FXG_CLIP_GLOBAL", "FXG_REV_DW", "FXG_NO_PACKED_CLIP", "FXG_CLIP_K_ONE_PASS",
         "FXG_WORKERS", "FXG_TICKET_GROUPS", "FXG_BLOCKS_PER_CU", "FXG_NSCAN", "FXG_TEST_SCAN_TIMEOUT")


def adapter_of(length, seed=0):
    """`length` bases of ACGT (four distinct bytes: the packed forms take it at every length)"""
    rng = np.random.default_rng(1000 * seed + length)
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=length))


def tile_kernel_requests():
    """[dict(kernel, stride, pd, env)]: one request per tile kernel, in the order the attribute tests launch them -- the 13 rows of
    csrc/fxg_instances.h, the 26 packed clip instances by bucket, the 4 general ones.  `kernel` is the whole name fxg_last_launch_info reports."""
    R = []

    def add(kernel, stride, pd, **env):
        R.append(dict(kernel=kernel, stride=stride, pd=pd, env=env))
    q = " qtrim+qfilter"
    add("fxg_kernel_rows<26,2>" + q, 200, dict(stages=6, **QTF))
    add("fxg_kernel_rows<38,2>" + q, 250, dict(stages=6, **QTF), FXG_ROWS="2")
    add("fxg_kernel_rows_multi<10,4>" + q, 36, dict(stages=6, **dict(QTF, qt_min_len=10)))
    add("fxg_kernel_rows_multi<14,3>" + q, 50, dict(stages=6, **dict(QTF, qt_min_len=15)))
    add("fxg_kernel_rows_multi<20,2>" + q, 76, dict(stages=6, **QTF))
    add("fxg_kernel_rows<26>" + q, 100, dict(stages=6, **QTF))
    add("fxg_kernel_rows<38>" + q, 150, dict(stages=6, **QTF))
    add("fxg_kernel_tiles<0,0>" + q, 150, dict(stages=6, **QTF), FXG_ROWS="0")
    add("fxg_kernel_tiles<0,3> mask", 150, dict(stages=64, mask_min_quality=20))
    add("fxg_kernel_tiles<0,4> base census", 100, dict(stages=128))
    add("fxg_kernel_tiles<0,5> revcomp[+ftrim], dword-aligned windows", 158, dict(stages=8))
    add("fxg_kernel_tiles<0,2> revcomp[+ftrim]", 150, dict(stages=24, ft_first=5, ft_last=145))
    add("fxg_kernel_tiles<0,1> ftrim", 150, dict(stages=16, ft_first=3, ft_last=100))
    for b in CLIP_BUCKETS:
        add("fxg_kernel_tiles<-%d,0> clip(packed)[+qtrim+qfilter]" % b, 100, dict(stages=1, adapter=adapter_of(min(b, CLIP_MAX_ADAPTER)), clip_min_len=5, clip_flags=4),
            FXG_CLIP_GLOBAL="0")
    for g in CLIP_GENERAL:
        add("fxg_kernel_tiles<%d,0> clip[+qtrim+qfilter]" % g, 100, dict(stages=1, adapter=adapter_of(min(g, CLIP_MAX_ADAPTER), 1), clip_min_len=5, clip_flags=4),
            FXG_NO_PACKED_CLIP="1")
    return R


N_TILE_KERNELS = 13 + len(CLIP_BUCKETS) + len(CLIP_GENERAL)
ALTERNATING = [-3, -10, -1]          # of tile_kernel_requests(): among the last eleven to be first seen (a packed bucket, the smallest and the largest general form)
ALT_STRIDES = (100, 60)              # two read lengths, two dynamic LDS sizes (the staged tile's bytes follow the stride)
THREAD_STRIDES = ((100, 60), (152, 80))      # the two threads' requests of the one instance below: four LDS sizes
THREAD_RUNS = 40


def thread_request(stride):
    return dict(kernel="fxg_kernel_tiles<-13,0> clip(packed)[+qtrim+qfilter]", stride=stride, pd=dict(stages=1, adapter=b"AGATCGGAAGAGC", clip_min_len=5, clip_flags=4),
                env=dict(FXG_CLIP_GLOBAL="0"))


def with_stride(req, stride):
    return dict(req, stride=stride)


def batch_of(req, n, seed=0):
    """(bases, qual): a seeded fixed-length batch for a request (adapters planted for the clip requests)"""
    rng = np.random.default_rng(zlib.crc32(repr((req["kernel"], req["stride"], n, seed)).encode()))
    st = req["stride"]
    b, q, _ = random_batch(rng, n, st, st, st, True, adapter=req["pd"].get("adapter"))
    return b, q


def attr_sequences(lds_of, threads_seed=0):
    """The launch sequences of part c as [(context, device, kernel index, lds)], given lds_of(request) -> dynamic LDS bytes:
    "all" (one context, every kernel once), then "alternating" continuing it (large, small, large, small, large for each of ALTERNATING),
    "two_contexts" (A large, B small, A large), "threads" (two contexts, THREAD_RUNS runs each, interleaved by a seeded coin)."""
    reqs = tile_kernel_requests()
    one = [(0, 0, k, lds_of(r)) for k, r in enumerate(reqs)]
    alt = []
    for k in ALTERNATING:
        k = k % len(reqs)
        a, b = (lds_of(with_stride(reqs[k], s)) for s in ALT_STRIDES)
        assert a != b, (reqs[k]["kernel"], a)
        big, small = max(a, b), min(a, b)
        alt += [(0, 0, k, l) for l in (big, small, big, small, big)]
    k = ALTERNATING[0] % len(reqs)
    a, b = (lds_of(with_stride(reqs[k], s)) for s in ALT_STRIDES)
    two = [(0, 0, k, max(a, b)), (1, 0, k, min(a, b)), (0, 0, k, max(a, b))]
    rng = np.random.default_rng(threads_seed)
    todo = [[lds_of(thread_request(THREAD_STRIDES[t][i % 2])) for i in range(THREAD_RUNS)] for t in (0, 1)]
    thr = []
    while todo[0] or todo[1]:
        t = int(rng.integers(0, 2))
        if not todo[t]:
            t ^= 1
        thr.append((t, 0, len(reqs), todo[t].pop(0)))          # (one more kernel index: the instance's GL = false function, whoever met it first)
    return dict(all=one, alternating=one + alt, two_contexts=two, threads=thr)


def uncovered(launches, sets):
    """The invariant: at every launch, the value last set for that kernel on that device in the process is at least the launch's LDS size.
    sets: [(step, device, kernel, lds)], each made before the launch of its step.  Returns the launches that break it as (step, launch, last set)."""
    last, bad, s = {}, [], 0
    for step, (ctx, dev, k, lds) in enumerate(launches):
        while s < len(sets) and sets[s][0] <= step:
            last[(sets[s][1], sets[s][2])] = sets[s][3]
            s += 1
        if last.get((dev, k), 0) < lds:
            bad.append((step, (ctx, dev, k, lds), last.get((dev, k))))
    assert s == len(sets)
    return bad


def old_policy(launches):
    """The log of attribute sets of fxg_kernel_fit as it was before csrc/fxg_attr.h: per context, an 8-entry cache of (kernel, lds) and a table of 32
    kernels with the largest value set; a kernel that finds no slot has its attribute set to the current lds on every cache miss."""
    ctxs, log = {}, []
    for step, (c, dev, k, lds) in enumerate(launches):
        x = ctxs.setdefault(c, dict(cache=[None] * 8, nxt=0, kern=[None] * 32, mx=[0] * 32))
        if (k, lds) in x["cache"]:
            continue
        slot = -1
        for i in range(32):
            if x["kern"][i] == k:
                slot = i
                break
            if x["kern"][i] is None and slot < 0:
                slot = i
        if slot < 0 or x["kern"][slot] != k or x["mx"][slot] < lds:
            log.append((step, dev, k, lds))
            if slot >= 0:
                x["kern"][slot], x["mx"][slot] = k, lds
        if None in x["cache"]:
            x["cache"][x["cache"].index(None)] = (k, lds)
        else:
            x["cache"][x["nxt"]] = (k, lds)
            x["nxt"] = (x["nxt"] + 1) % 8
    return log


# ---- the grow rule ------------------------------------------------------------------------------------------------------------------------
# need and capacity (in the workspace's own units) of each workspace for a call, as fxg_ws_grow's callers compute them (csrc/fxg_host.h, fxg_engine.hip)
TEXT_SEG, BC_TILE, QS_PART_WORDS, FB_BLOCK, CK_SLOTS, TBLOCK, HIST_BLOCK = 4096, 256, 160 * 5 * 64, 1024, 7, 256, 256


def _margin(words):
    return words + words // 4 + 4096


def ws_status(ntiles):
    return ntiles, ntiles + ntiles // 4 + 1024


def ws_text_index(text_len):
    nseg = -(-text_len // TEXT_SEG)
    words = nseg + nseg // 512 + 4096
    return words, _margin(words)


def ws_text_format(n):
    words = n + n // 512 + 4096
    return words, _margin(words)


def ws_bc(n, bins, rec_bin=True):
    N = bins * -(-n // BC_TILE)
    words = N + (N // 512 + 64) + 2 * bins + (0 if rec_bin else (n + 3) // 4)
    return words, _margin(words)


def ws_rf(lines):
    words = 4 * (lines + 2) + 2 * ((lines + 2) // 256 + 128) + 8
    return words, _margin(words)


def ws_uc(records):
    words = 3 * (records + 1) + ((records + 1) // 512 + 64) + 16
    return words, _margin(words)


def ws_stats(n, cus):
    need = min(-(-n // 256), cus) * QS_PART_WORDS
    return need, need


def ws_clip_ck(grid, bucket):
    need = grid * CK_SLOTS * bucket * TBLOCK
    return need, need


def ws_hist(n, stride, tile, estride):
    r = 255
    ntiles = -(-n // tile)
    nblk = -(-ntiles // HIST_BLOCK)
    S2 = stride + 2
    b = ((ntiles * S2 * 4 + r) & ~r) + ((nblk * S2 * 4 + r) & ~r) + ((n * estride + 16 + r) & ~r) + ((n * 2 + r) & ~r)
    return b, b + b // 8


def ws_fb(n):
    need = 2 * -(-n // FB_BLOCK) + 2
    return need, need


class GrowModel:
    """capacities of a context's workspaces as the rule leaves them: use(name, (need, cap)) -> True when the call reallocates the workspace"""

    def __init__(self):
        self.have, self.log = {}, []

    def use(self, step, name, need_cap):
        need, cap = need_cap
        grown = self.have.get(name, 0) < need
        if grown:
            self.have[name] = cap
            self.log.append((step, name))
        return grown

    def regrown(self):
        """{workspace: [steps at which an existing block was replaced by a larger one]} (the first allocation is no reallocation)"""
        out, seen = {}, set()
        for step, name in self.log:
            if name in seen:
                out.setdefault(name, []).append(step)
            seen.add(name)
        return out
