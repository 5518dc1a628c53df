"""The collapser's set among everything else a context does: the call list of tests/test_gpu_context_state_collapse.py part (a), shared with its CPU half
(tests/test_collapse_state_cpu.py), which holds the list against what it claims.

Three recorded cases of golden/collapser/cases.json go through ONE context one after the other -- `dups` in 5 blocks, `ties` in 5 blocks, `seeded` in blocks
of 1 MB -- and between every two fxg_collapse_add calls, and between fxg_collapse_order and each fxg_collapse_write window, stands one call (or one short
group of calls) of another family, dealt round-robin over all three cases -- the gaps between adds in one deal, the gaps before windows in another -- from the nine
families of context_state_sequence.py:

  index          fxg_fastq_index of an unrelated block of wide FASTA records, sized so that two of them reallocate text_ws (sizes cycle large, small, larger, small)
  pack_format    fxg_fastq_pack and fxg_fastq_format_opts of a block indexed before the first set began: its line arrays and lengths must have survived
  reflow         fxg_fasta_reflow of 8 000, 2 000, 40 000, 2 000 lines: two of them reallocate rf_ws
  uc             the next window of ONE uncollapse walk that began before the first set: the context's kept scans must have survived
  barcode        fxg_barcode_prepare (97 bins and 3 bins in turn) and a split of the block indexed before the first set
  run            a compacting fxg_run_pipeline, one read per tile, of 2 000, 8 000 and 20 000 reads in that order in time (status reallocated twice), its counters left unread ...
  stats          fxg_run_quality_stats
  history        clip history on, one ragged clip batch, history off
  read_counters  ... until here: fxg_read_counters of the last `run`, three gaps later

Every foreign step is a step of context_state_sequence.py's kinds, so the GPU half runs it through the same Runner, against the same oracles and models.
The window sizes make at least ceil(out_bytes / cap) windows per case; should the engine need one more (records do not straddle windows), the GPU half
takes further gaps from gap(EXTRA + k)."""
import functools

import numpy as np

import collapse_cases as CK
import collapse_model as M
import context_state_cases as K
import context_state_sequence as S

FAMILIES = ["index", "pack_format", "reflow", "uc", "barcode", "run", "stats", "history", "read_counters"]
F_BLOCK, U_BLOCK = ("fastq", 2500), ("collapsed", 6000, 7)          # indexed before the first set; U's walk takes one window per `uc` gap
UC_PARTS = 64
WIDE = [(12000, 2038), (300, 150), (32000, 2038), (300, 150)]       # (records, bases per record) of the unrelated blocks: 24.6 MB, 48 KB, 65.5 MB, 48 KB
WIDE_ID = 7                                                         # digits of a wide record's id
REFLOW_SETUP, REFLOW = 2000, [8000, 2000, 40000, 2000]
RUN = [2000, 20000, 2000, 8000]                                     # (the deal before windows takes the last size, and comes between the first two in time)
STATS = [2000, 256 * 20, 2000, 256 * 40]
HISTORY = [2000, 8000, 2000, 16000]
WINDOW_BASE = 99                                                    # the gaps before windows are dealt on their own, numbered from here (a multiple of 9 too)
EXTRA = 900                                                         # gap numbers of windows beyond the listed ones (a multiple of 9: the deal goes on from `index`)
ONE_MB = 1 << 20
CASES = [("dups", 5), ("ties", 5), ("seeded", 0)]                   # (recorded case, blocks; 0: blocks of 1 MB)


def wide_text_len(n, L):
    return n * (1 + WIDE_ID + 1 + L + 1)


@functools.lru_cache(maxsize=2)
def wide_block(n, L):
    """n two-line FASTA records ">%07d\\n" + L bases: every record of one width, so that the text's length is plain arithmetic"""
    rng = np.random.default_rng(1000 * n + L)
    rows = np.empty((n, 1 + WIDE_ID + 1 + L + 1), np.uint8)
    rows[:, 0] = ord(">")
    ids = np.arange(n)
    for d in range(WIDE_ID):
        rows[:, WIDE_ID - d] = 48 + ids // 10 ** d % 10
    rows[:, WIDE_ID + 1] = 10
    rows[:, WIDE_ID + 2:-1] = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, size=(n, L))]
    rows[:, -1] = 10
    text = rows.tobytes()
    assert len(text) == wide_text_len(n, L)
    return dict(kind="wide", lpr=2, text=text, n=n, qual=None, lens=np.full(n, L, np.uint16))


@functools.lru_cache(maxsize=None)
def case_blocks(name, ways):
    """[(text, records)] of a recorded case: in `ways` blocks of nearly equal record counts, or (ways = 0) cut at record starts into blocks of at most 1 MB"""
    if name == "seeded":
        assert ways == 0
        text, out, at = CK.seeded_text(), [], 0
        while at < len(text):
            end = len(text) if len(text) - at <= ONE_MB else text.rfind(b"\n>", at, at + ONE_MB) + 1
            out.append((text[at:end], text.count(b"\n", at, end) // 2))
            at = end
        return out
    records = [c for c in CK.abi_cases() if c[0] == name][0][1]
    return [(M.block_text(blk), len(blk)) for blk in CK.split(records, ways)]


def window_cap(name):
    """out_cap of a case's windows: about five windows for dups, four for ties, 1 MB for seeded"""
    total = CK.expected(name)["len"]
    return ONE_MB if name == "seeded" else total // (5 if name == "dups" else 4) + 64


def least_windows(name):
    return -(-CK.expected(name)["len"] // window_cap(name))


def gap(i):
    """the foreign steps of gap number i: family i % 9, its occurrence i // 9 choosing the size"""
    fam, o = FAMILIES[i % 9], i // 9
    tag = "%s.g%d" % (fam, i)
    if fam == "index":
        n, L = WIDE[o % 4]
        steps = [dict(kind="index", block=("wide", n, L), label=tag)]
    elif fam == "pack_format":
        steps = [dict(kind="pack", block=F_BLOCK, label=tag + ".pack"), dict(kind="format", block=F_BLOCK, label=tag + ".format")]
    elif fam == "reflow":
        steps = [dict(kind="reflow", lines=REFLOW[o % 4], width=(0, 70, 1, 33)[o % 4], label=tag)]
    elif fam == "uc":
        steps = [dict(kind="uc", block=U_BLOCK, parts=UC_PARTS, label=tag)]
    elif fam == "barcode":
        steps = [dict(kind="bc_prepare", table=("t97", "t3")[o % 2], label=tag + ".prepare"), dict(kind="bc_split", block=F_BLOCK, label=tag + ".split")]
    elif fam == "run":
        steps = [S._run("ftrim1", RUN[o % 4], "fb.g%d.run" % i, meta=False)]          # (the label's form leaves its counters unread: Runner.do_run)
    elif fam == "stats":
        steps = [dict(kind="stats", n=STATS[o % 4], label=tag)]
    elif fam == "history":
        steps = [dict(kind="history", on=True, label=tag + ".on"), S._run("clip13", HISTORY[o % 4], tag + ".batch", ragged=True), dict(kind="history", on=False, label=tag + ".off")]
    else:
        steps = [dict(kind="read_counters", of="fb.g%d.run" % (i - 3), label=tag)]
    for st in steps:
        st.update(gap=i, family=fam)
    return steps


def setup_steps():
    """before the first set: the blocks other families return to, the first window of the uncollapse walk, a first reflow, a barcode table"""
    return [dict(kind="index", block=F_BLOCK, label="setup.indexF"), dict(kind="index", block=U_BLOCK, label="setup.indexU"),
            dict(kind="uc", block=U_BLOCK, first=True, parts=UC_PARTS, label="setup.uc0"), dict(kind="reflow", lines=REFLOW_SETUP, width=60, label="setup.reflow"),
            dict(kind="bc_prepare", table="t97", label="setup.prepare")]


def build():
    """the whole list: setup, then per case begin, add, (gap, add) ..., order, (gap, write) ... with at least least_windows(case) windows; `where` on a
    foreign step says which kind of gap it stands in"""
    steps, i, iw = setup_steps(), 0, WINDOW_BASE
    for name, ways in CASES:
        blocks = case_blocks(name, ways)
        steps.append(dict(kind="cl_begin", case=name, label=name + ".begin"))
        for j in range(len(blocks)):
            if j:
                steps += [dict(st, where="adds") for st in gap(i)]
                i += 1
            steps.append(dict(kind="cl_add", case=name, ways=ways, block=j, label="%s.add%d" % (name, j)))
        steps.append(dict(kind="cl_order", case=name, label=name + ".order"))
        for w in range(least_windows(name)):
            steps += [dict(st, where="windows") for st in gap(iw)]
            iw += 1
            steps.append(dict(kind="cl_write", case=name, window=w, cap=window_cap(name), label="%s.write%d" % (name, w)))
    return S.annotate(steps)


def workspace_use(st, cus=256):
    """context_state_sequence.workspace_use, with the text workspace of the blocks this list adds: wide blocks by their exact length, a case's block by its
    own (fxg_fastq_index runs on it before the add)"""
    if st["kind"] == "index" and st["block"][0] == "wide":
        return [("text_ws", K.ws_text_index(wide_text_len(*st["block"][1:])))]
    if st["kind"] == "cl_add":
        return [("text_ws", K.ws_text_index(len(case_blocks(st["case"], st["ways"])[st["block"]][0])))]
    if st["kind"].startswith("cl_"):
        return []
    return S.workspace_use(st, cus)
