"""CPU half of tests/test_gpu_context_state_collapse.py: the call list of its part (a) (tests/collapse_state_sequence.py) held against what it claims --
every foreign family at least twice between two adds and at least once between two windows, the unrelated blocks and the reflows sized so that text_ws and
rf_ws are reallocated by the grow rule pinned in tests/test_context_state_cpu.py (context_state_cases.GrowModel), the blocks of each case its own text."""
import collections

import collapse_cases as CK
import collapse_model as M
import collapse_state_sequence as Q
import context_state_cases as K


def test_every_family_stands_between_adds_and_between_windows():
    steps = Q.build()
    labels = [st["label"] for st in steps]
    assert len(labels) == len(set(labels))
    seen = dict(adds=collections.Counter(), windows=collections.Counter())
    gaps = {}
    for st in steps:
        if "gap" in st:
            gaps.setdefault(st["gap"], (st["family"], st["where"]))
            assert gaps[st["gap"]] == (st["family"], st["where"])
    for i, (fam, where) in sorted(gaps.items()):
        assert fam == Q.FAMILIES[i % 9]                               # dealt in turn over all three cases
        seen[where][fam] += 1
    adds, wins = [i for i in sorted(gaps) if i < Q.WINDOW_BASE], [i for i in sorted(gaps) if i >= Q.WINDOW_BASE]
    assert adds == list(range(len(adds))) and wins == list(range(Q.WINDOW_BASE, Q.WINDOW_BASE + len(wins))) and Q.WINDOW_BASE % 9 == 0
    assert all(gaps[i][1] == "adds" for i in adds) and all(gaps[i][1] == "windows" for i in wins)
    for fam in Q.FAMILIES:
        assert seen["adds"][fam] >= 2 and seen["windows"][fam] >= 1, (fam, seen)
    # the shape: no two adds of a case and no order / write pair without a foreign call between them
    kinds = [st["kind"] for st in steps]
    for a, b in zip(kinds, kinds[1:]):
        assert (a, b) not in (("cl_add", "cl_add"), ("cl_order", "cl_write"), ("cl_write", "cl_write")), (a, b)
    assert kinds.count("cl_begin") == 3 and kinds.count("cl_order") == 3


def test_counters_are_read_three_gaps_after_their_run():
    steps = Q.build()
    pending, read = [], 0
    for st in steps:
        if st["kind"] == "run" and st["label"].startswith("fb."):
            assert not st["meta"]
            pending.append(st["label"])
        if st["kind"] == "read_counters":
            assert st["of"] in pending and st["of"] == "fb.g%d.run" % (st["gap"] - 3), (st, pending)
            pending.remove(st["of"])
            read += 1
    assert read >= 3 and len(pending) <= 2                            # (the GPU half reads what is left when the list ends)
    assert Q.EXTRA % 9 == 0 and Q.EXTRA > max(st.get("gap", 0) for st in steps) + 9


def test_unrelated_blocks_and_reflows_regrow_their_workspaces():
    steps = Q.build()
    model = K.GrowModel()
    for i, st in enumerate(steps):
        for name, need_cap in Q.workspace_use(st):
            model.use(i, name, need_cap)
    regrown = model.regrown()
    by_wide = [i for i in regrown["text_ws"] if steps[i]["kind"] == "index" and steps[i]["block"][0] == "wide"]
    assert len(by_wide) >= 2 and by_wide == regrown["text_ws"], (regrown["text_ws"], [steps[i]["label"] for i in regrown["text_ws"]])
    by_reflow = [i for i in regrown["rf_ws"] if steps[i].get("family") == "reflow"]
    assert len(by_reflow) >= 2, regrown["rf_ws"]
    assert len([i for i in regrown["status"] if steps[i].get("family") == "run"]) >= 2, regrown["status"]
    # each of them with a set alive: after a begin and before that case's last window
    alive = False
    for i, st in enumerate(steps):
        if st["kind"] == "cl_begin":
            alive = True
        if i in by_wide + by_reflow:
            assert alive, st["label"]
    assert Q.wide_block(300, 150)["text"].count(b"\n") == 600 and len(Q.wide_block(300, 150)["text"]) == Q.wide_text_len(300, 150)


def test_blocks_are_the_cases_own_text():
    for name, ways in Q.CASES:
        blocks = Q.case_blocks(name, ways)
        if name == "seeded":
            whole = CK.seeded_text()
            assert len(blocks) >= 12 and all(len(t) <= Q.ONE_MB for t, _ in blocks)
        else:
            whole = CK.case_text([c for c in CK.abi_cases() if c[0] == name][0][1])
            assert len(blocks) == 5
        assert b"".join(t for t, _ in blocks) == whole
        assert all(t[:1] == b">" and t[-1:] == b"\n" and t.count(b"\n") == 2 * n for t, n in blocks)
        assert Q.least_windows(name) >= 2
    sums = M.collapse(M.records_of(CK.case_text([c for c in CK.abi_cases() if c[0] == "dups"][0][1])))
    assert M.out_bytes(sums) == CK.expected("dups")["len"]            # the window count is worked out from the recorded length: the model's
