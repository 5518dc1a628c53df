"""The interleaved sequence of tests/test_gpu_context_state.py (part b): about 150 calls on ONE context, drawn from every family of entry points, four sizes
per family in the order small, large, small, larger, chosen from the grow rule of fxg_ws_grow's callers (need + need / 4 + margin) so that every workspace
of the context that a normal run grows is reallocated at least twice while other families' kept data must survive.  (fb_blk grows only when a launch is done
again without the scanner: the GPU half walks it on a context of its own, fallback_steps.)

A step is a dict: kind, label, the sizes, and `regrows`: the workspaces the step is expected to reallocate -- the table.  tests/test_context_state_cpu.py
replays the steps through the rule (workspace_use + context_state_cases.GrowModel) and requires the table to be what the rule says; the GPU half runs them.

Strands keep their own order; groups (lists inside a strand) run back to back; a seeded coin merges the strands.  The orders the issue names are groups:
  text_a   index A, reflow of an unrelated larger block, format of A from A's line arrays
  text_b   index A, index B (larger), pack A
  uc_walk  one block's windows with an index, a pack, a format, a reflow that regrows rf_ws, a pipeline run that regrows status, a barcode split and a
           statistics call between consecutive windows
  uc_host  the order of host/fxh_uncollapse.c (dev_block): per block index, pack, then ALL its windows back to back with the ordinal base carried on --
           that file never puts the next block's index and pack between two windows of one block, it puts them between the LAST window of block k and
           the first of block k + 1, and that is what is reproduced here
  history  history on, batches 1..3 of a ragged input with a non-clip run, a clip run of another adapter bucket (refused: a history has one adapter, and
           batch 3 must come out as if nobody had asked) and a quality_stats between them, history off (a fixed-length batch: there alone the oracle's
           aligner and the engine without history agree by contract) and on again
  fb       a compacting meta=False run, a text call, a statistics call, then read_counters of the run
"""
import numpy as np

import context_state_cases as K

WORKSPACES = ["status", "text_ws", "bc_ws", "rf_ws", "uc_ws", "stats_ws", "clip_ck", "hist_ws"]
AD13 = b"AGATCGGAAGAGC"
AD40 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCACATCTCG"
READ_LEN = 36                                     # of the FASTQ blocks (oracle/fxoracle.c's generator)
RF_LINE, RF_LINES_PER_RECORD = 60, 4              # the multi-line FASTA blocks: a header and three lines of 60 bases
BC_BINS, BC_LEN = 97, 6

# pipeline families: stride, parameters, reads per tile, knobs, the start of the kernel's name
FAM = {
    "ftrim1": dict(stride=60, pd=dict(stages=16, ft_first=3, ft_last=50), T=1, env=dict(FXG_TILE="1"), kernel="fxg_kernel_tiles<0,1> ftrim"),
    "rows38": dict(stride=150, pd=dict(stages=6, **K.QTF), T=64, kernel="fxg_kernel_rows<38>"),
    "rows26": dict(stride=100, pd=dict(stages=6, **K.QTF), T=64, kernel="fxg_kernel_rows<26>"),
    "multi4": dict(stride=36, pd=dict(stages=6, **dict(K.QTF, qt_min_len=10)), T=256, kernel="fxg_kernel_rows_multi<10,4>"),
    "rev2": dict(stride=150, pd=dict(stages=24, ft_first=5, ft_last=145), T=128, kernel="fxg_kernel_tiles<0,2> revcomp"),
    "census": dict(stride=100, pd=dict(stages=128), T=128, kernel="fxg_kernel_tiles<0,4> base census"),
    "mask": dict(stride=150, pd=dict(stages=64, mask_min_quality=20), T=128, kernel="fxg_kernel_tiles<0,3> mask"),
    "clip40k": dict(stride=150, pd=dict(stages=1, adapter=AD40, clip_min_len=15, clip_flags=0), T=256, bucket=40, clip=True, kernel="fxg_kernel_tiles<-40,0> clip(packed)"),
    "clip13": dict(stride=100, pd=dict(stages=1, adapter=AD13, clip_min_len=5, clip_flags=0), T=256, clip=True, env=dict(FXG_CLIP_GLOBAL="0"), kernel="fxg_kernel_tiles<-13,0> clip(packed)"),
    "clip40h": dict(stride=100, pd=dict(stages=1, adapter=AD40, clip_min_len=5, clip_flags=0), T=256, bucket=40, clip=True, env=dict(FXG_CLIP_GLOBAL="0"), kernel="fxg_kernel_tiles<-40,0> clip(packed)"),
}
SIZES = dict(          # small, large, small, larger
    ftrim1=(2000, 4000, 2000, 16000), rows38=(3000, 9000, 3000, 20000), rows26=(2000, 5000, 2000, 9000), multi4=(2000, 6000, 2000, 12000),
    rev2=(2000, 4000, 2000, 6000), census=(2000, 4000, 2000, 6000), clip40k=(2000, 256 * 60, 2000, 256 * 120),
    stats=(2000, 256 * 20, 2000, 256 * 40), fastq=(2000, 6000, 2000, 14000), reflow=(2000, 8000, 2000, 60000), uncollapse=(2000, 8000, 2000, 24000),
    barcode=(2000, 20000, 2000, 40000), history=(2000, 8000, 2000, 16000),
)
HUGE_REFLOW, HUGE_RUN = 40000, 12000              # inside uc_walk: larger than everything of their workspaces but the families' last sizes, so they regrow them wherever the group lands behind a first call
NAMES = ("small", "large", "small2", "larger")
# one history is one reference process with one adapter (include/fxg.h): the run of another adapter bucket between two batches of a history is refused, nothing moves
OTHER_ADAPTER = "clip history: the adapter differs from the one this history began with; fxg_set_clip_history(ctx, 1) begins another"


def _run(fam, n, label, ragged=False, meta=True, **more):
    return dict(kind="run", fam=fam, n=n, ragged=ragged, meta=meta, label=label, **more)


def build(cus=256, seed=2036):
    """the steps, merged; the same list for every cus >= 128 (the sizes keep the statistics' and the clipper's grids below that)"""
    assert cus >= 128
    strands = []
    for fam in ("ftrim1", "rows38", "rows26", "multi4", "rev2", "census", "clip40k"):
        strands.append([_run(fam, n, "%s.%s" % (fam, NAMES[i])) for i, n in enumerate(SIZES[fam])])
    for fam in ("mask", "clip13", "rev2", "census"):          # (the last two once more on ragged input)
        tag = fam if fam in ("mask", "clip13") else fam + "_ragged"
        strands.append([_run(fam, n, "%s.%s" % (tag, NAMES[i]), ragged=tag != fam) for i, n in enumerate(SIZES.get(fam, (2000, 5000, 2000, 8000)))])
    strands.append([dict(kind="stats", n=n, label="stats." + NAMES[i]) for i, n in enumerate(SIZES["stats"])])
    strands.append([[dict(kind="index", block=("fastq", n), label="fastq.%s.index" % NAMES[i]), dict(kind="pack", block=("fastq", n), label="fastq.%s.pack" % NAMES[i]),
                     dict(kind="format", block=("fastq", n), label="fastq.%s.format" % NAMES[i])] for i, n in enumerate(SIZES["fastq"])])
    strands.append([dict(kind="reflow", lines=n, width=(0, 70, 1, 33)[i], label="reflow." + NAMES[i]) for i, n in enumerate(SIZES["reflow"])])
    strands.append([[dict(kind="index", block=("collapsed", n, i), label="uc.%s.index" % NAMES[i]), dict(kind="uc", block=("collapsed", n, i), first=True, parts=3, label="uc.%s.w0" % NAMES[i]),
                     dict(kind="uc", block=("collapsed", n, i), parts=3, label="uc.%s.w1" % NAMES[i]), dict(kind="uc", block=("collapsed", n, i), parts=3, rest=True, label="uc.%s.rest" % NAMES[i])]
                    for i, n in enumerate(SIZES["uncollapse"])])
    bc = [dict(kind="bc_prepare", table="t97", label="bc.prepare97")]
    for i, n in enumerate(SIZES["barcode"]):
        bc.append([dict(kind="index", block=("fastq", n), label="bc.%s.index" % NAMES[i]), dict(kind="bc_split", block=("fastq", n), label="bc.%s.split" % NAMES[i])])
    bc += [dict(kind="bc_prepare", table="t3", label="bc.prepare3"), [dict(kind="index", block=("fastq", 2000), label="bc.after3.index"), dict(kind="bc_split", block=("fastq", 2000), label="bc.after3.split")]]
    strands.append(bc)
    A, B = ("fastq", 3000), ("fastq", 9000)
    strands.append([[dict(kind="index", block=A, label="text_a.index"), dict(kind="reflow", lines=12000, width=60, label="text_a.reflow"), dict(kind="format", block=A, label="text_a.format")],
                    [dict(kind="index", block=A, label="text_b.indexA"), dict(kind="index", block=B, label="text_b.indexB"), dict(kind="pack", block=A, label="text_b.packA")]])
    U, F = ("collapsed", 6000, 7), ("fastq", 2500)
    between = [dict(kind="index", block=F, label="uc_walk.index"), dict(kind="pack", block=F, label="uc_walk.pack"), dict(kind="format", block=F, label="uc_walk.format"),
               dict(kind="reflow", lines=HUGE_REFLOW, width=0, label="uc_walk.reflow"), _run("ftrim1", HUGE_RUN, "uc_walk.run"),
               dict(kind="bc_split", block=F, label="uc_walk.split"), dict(kind="stats", n=3000, label="uc_walk.stats")]
    walk = [dict(kind="index", block=U, label="uc_walk.indexU"), dict(kind="uc", block=U, first=True, parts=8, label="uc_walk.w0")]
    for j, x in enumerate(between):
        walk += [x, dict(kind="uc", block=U, parts=8, rest=(j == len(between) - 1), label="uc_walk.w%d" % (j + 1))]
    host = []
    for k in range(3):
        blk = ("collapsed", 1500 + 700 * k, 20 + k)
        host += [dict(kind="index", block=blk, label="uc_host.b%d.index" % k), dict(kind="pack", block=blk, label="uc_host.b%d.pack" % k),
                 dict(kind="uc", block=blk, first=True, parts=3, chain="host", label="uc_host.b%d.w0" % k),
                 dict(kind="uc", block=blk, parts=3, chain="host", rest=True, label="uc_host.b%d.rest" % k)]
    # (the barcode table must be there for uc_walk.split: the group comes behind bc.prepare97 in one strand)
    strands[-2] = [bc[0], walk] + bc[1:]
    strands.append([host])
    h = SIZES["history"]
    strands.append([[dict(kind="history", on=True, label="history.on"), _run("clip13", h[0], "history.batch1", ragged=True), _run("rows26", 2500, "history.nonclip"),
                     _run("clip13", h[1], "history.batch2", ragged=True), _run("clip40h", 3000, "history.other_bucket", ragged=True, refused=OTHER_ADAPTER), _run("clip13", h[2], "history.batch3", ragged=True),
                     dict(kind="stats", n=2500, label="history.stats"), dict(kind="history", on=False, label="history.off"), _run("clip13", 3000, "history.none"),
                     dict(kind="history", on=True, label="history.on_again"), _run("clip13", 2500, "history.again1", ragged=True), _run("clip13", h[3], "history.again2", ragged=True),
                     dict(kind="history", on=False, label="history.off_again")]])
    strands.append([[_run("mask", 5000, "fb.run", meta=False), dict(kind="index", block=("fastq", 2000), label="fb.text"), dict(kind="stats", n=2000, label="fb.stats"),
                     dict(kind="read_counters", of="fb.run", label="fb.read_counters")]])
    rng = np.random.default_rng(seed)
    steps, todo = [], [list(s) for s in strands]
    while any(todo):
        live = [s for s in todo if s]
        s = live[int(rng.integers(0, len(live)))]
        x = s.pop(0)
        steps += x if isinstance(x, list) else [x]
    for st in steps:
        st["regrows"] = REGROWS.get(st["label"], ())
    return annotate(steps)


# the table: which step reallocates which workspace (a first allocation is none).  Held against the rule by tests/test_context_state_cpu.py.
REGROWS = {
    "ftrim1.small": ("status",), "uc_walk.run": ("status",),
    "fastq.large.format": ("text_ws",), "fastq.larger.format": ("text_ws",),
    "bc.large.split": ("bc_ws",), "bc.larger.split": ("bc_ws",),
    "text_a.reflow": ("rf_ws",), "uc_walk.reflow": ("rf_ws",), "reflow.larger": ("rf_ws",),
    "uc.large.w0": ("uc_ws",), "uc.larger.w0": ("uc_ws",),
    "stats.large": ("stats_ws",), "stats.larger": ("stats_ws",),
    "clip40k.large": ("clip_ck",), "clip40k.larger": ("clip_ck",),
    "history.batch2": ("hist_ws",), "history.again2": ("hist_ws",),
}


def fastq_text_len(n):
    """bytes of the oracle generator's n records of READ_LEN bases: "@<seed>_<i>\\n" ... -- only an upper bound matters here (the newline census of fxg_line_index
    needs 4096 words plus one per 4 KiB of text: no block of this sequence comes near what the format calls need)"""
    return n * (2 * READ_LEN + 32)


def workspace_use(st, cus=256, state=None):
    """[(workspace, (need, cap))] of a step, in the order the engine's code grows them"""
    k = st["kind"]
    if k == "run":
        if st.get("refused"):
            return []
        f = FAM[st["fam"]]
        ntiles = -(-st["n"] // f["T"])
        use = [("status", K.ws_status(ntiles))]
        if f.get("bucket"):                                   # the two-pass form with checkpoint scratch: one block per workgroup, scanner included
            assert ntiles <= cus                              # (every tile has a worker of its own: the grid is the tiles and the scanner)
            use.append(("clip_ck", K.ws_clip_ck(ntiles + 1, f["bucket"])))
        if st.get("hist"):
            use.insert(0, ("hist_ws", K.ws_hist(st["n"], f["stride"], f["T"], st["hist"])))
        return use
    if k == "stats":
        return [("stats_ws", K.ws_stats(st["n"], cus))]
    if k == "index":
        n = st["block"][1]
        return [("text_ws", K.ws_text_index(fastq_text_len(n) if st["block"][0] == "fastq" else 40 * n))]
    if k == "format":
        return [("text_ws", K.ws_text_format(st["block"][1]))]
    if k == "reflow":
        return [("text_ws", K.ws_text_index(st["lines"] * (RF_LINE + 1))), ("rf_ws", K.ws_rf(st["lines"]))]
    if k == "uc":
        return [("uc_ws", K.ws_uc(st["block"][1]))] if st.get("first") else []
    if k == "bc_split":
        return [("bc_ws", K.ws_bc(st["block"][1], st["bins"]))]
    return []


def annotate(steps):
    """what a step's workspaces depend on beyond its own sizes: the bins of the table a split runs under, the widest row the clip history has seen"""
    bins, hist_on, wcap = 0, False, 0
    for st in steps:
        if st["kind"] == "bc_prepare":
            bins = dict(t97=BC_BINS, t3=3)[st["table"]]
        if st["kind"] == "bc_split":
            st["bins"] = bins
        if st["kind"] == "history":
            hist_on, wcap = st["on"], 0
        if st["kind"] == "run" and FAM[st["fam"]].get("clip") and hist_on and not st.get("refused"):
            stride = FAM[st["fam"]]["stride"]
            st["aligner"] = True
            if st["ragged"] or wcap > stride:                  # (else fxg_hist_shortcut: no workspace)
                st["hist"] = max(wcap, stride)
            wcap = max(wcap, stride)
    return steps


def fallback_steps():
    """fb_blk: a context whose compacting launches all time out (FXG_TEST_SCAN_TIMEOUT) does each again without the scanner; block sums for n / 1024 blocks,
    grown to exactly the need: small, large, small, larger, with a text call and a statistics call between the run and its read_counters"""
    out = []
    for i, n in enumerate((2000, 9000, 2000, 20000)):
        out += [_run(("rows38", "rev2", "mask", "rows26")[i], n, "fb_blk.%s.run" % NAMES[i]), dict(kind="index", block=("fastq", 2000), label="fb_blk.%s.text" % NAMES[i]),
                dict(kind="stats", n=2000, label="fb_blk.%s.stats" % NAMES[i]), dict(kind="read_counters", of="fb_blk.%s.run" % NAMES[i], label="fb_blk.%s.read" % NAMES[i])]
    return out
