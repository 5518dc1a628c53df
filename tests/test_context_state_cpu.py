"""CPU tier of the context-state tests (the GPU half: tests/test_gpu_context_state.py; what they share: tests/context_state_cases.py).

  * The first-call table has a row for every entry point of csrc/fxg_engine.hip that takes a context, held against the export list tests/test_abi.py reads;
    the refusals that need no device state go through the emulation stub.
  * The kernel-attribute invariant -- at every launch, the value last set for that kernel on that device in the process is at least the launch's LDS
    size -- over the exact launch sequences of the GPU half and over 20 seeded random ones (43 kernels, 1 to 3 contexts, 2 devices), replayed through the
    engine's own decision function (csrc/fxg_attr.h, emu_py.attr_replay).  The policy the engine had before (a 32-slot table per context) is kept here
    as a model and must FAIL the same check on the same sequences: that is what shows the check can see the defect.
  * The sizes of the GPU half's interleaved sequence regrow every workspace at least twice by the grow rule.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import context_state_cases as K
import emu_py as emu
from conftest import ROOT
from fastx_toolkit_amd.engine import EXPORTS, make_params


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in K.KNOBS:
        monkeypatch.delenv(k, raising=False)


CSRC = os.path.join(ROOT, "fastx_toolkit_amd", "csrc")


def spelled_extern_c():
    """the functions of csrc/fxg_engine.hip that spell extern "C" at their definition and take a context first (what this table was held against before
    the entries that take their linkage from include/fxg.h)"""
    src = open(os.path.join(CSRC, "fxg_engine.hip")).read()
    return sorted(set(re.findall(r'^extern "C" [^\n(]*?\b(fxg_[a-z0-9_]+)\((?:const )?fxg_ctx \*', src, re.M)))


def engine_entry_points():
    """the functions include/fxg.h declares with a context as their first parameter that csrc/fxg_engine.hip or fxg_engine_clip.hip defines, whatever the
    definition's spelling of linkage: at the start of a line, with or without extern "C", a body and no semicolon before it"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fxg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fxg_[a-z0-9_]+)\s*\(\s*(?:const\s+)?fxg_ctx\s*\*", hdr))
    srcs = [open(os.path.join(CSRC, f)).read() for f in ("fxg_engine.hip", "fxg_engine_clip.hip")]

    def defined(name):
        pat = re.compile(r"^(?![ \t/#*])[^\n;=]*\b%s\((?:const )?fxg_ctx \*[^;{]*\{" % name, re.M)
        return any(pat.search(s) for s in srcs)
    return sorted(n for n in declared if defined(n))


def test_first_call_table_has_every_entry_point():
    spelled = spelled_extern_c()
    assert set(spelled) - set(EXPORTS) == {"fxg_debug_phase_clocks"}          # (only the ablation builds have it: #ifdef FXG_ABLATION, not in include/fxg.h)
    entries = engine_entry_points()
    assert {e for e in spelled if e in EXPORTS} <= set(entries)               # what the table was held against before: reading the header can only add names
    assert set(entries) <= set(EXPORTS)
    assert len(entries) >= 44
    assert {"fxg_bases_change", "fxg_collapse_begin", "fxg_collapse_add", "fxg_collapse_order", "fxg_collapse_write"} <= set(entries)      # (no extern "C" at their definitions)
    rows = {entry for _, entry, _ in K.FIRST_CALLS}
    assert rows == set(entries), (sorted(set(entries) - rows), sorted(rows - set(entries)))
    ids = [i for i, _, _ in K.FIRST_CALLS]
    assert len(ids) == len(set(ids))
    # the entry points the issue names as families, each present under the form it asks for
    for want in ("run_rows", "run_tiles", "run_clip", "quality_stats", "read_counters_zeroed", "fastq_index", "fastq_pack_other_contexts_lines", "fastq_format_opts_len_no_res",
                 "fasta_weights_unindexed", "barcode_split_without_prepare", "fasta_reflow", "fasta_reflow_empty_closes_record", "fasta_uncollapse_from_zero",
                 "fasta_uncollapse_continue_nothing", "clip_history_then_batch",
                 "bases_change_other_contexts_lines", "bases_change_no_records", "collapse_begin", "collapse_add_no_set", "collapse_order_no_set", "collapse_write_no_set",
                 "collapse_add_other_contexts_lines"):
        assert want in ids


def collapse_stub_dir(tmp):
    """a libfxg.so of the objects of emu_py.build_fmtopts (the stub and the entries request_cases.Session declares) plus the four collapser entries
    (emu/collapse_stub.cpp over collapse_emu.cpp, as tests/test_collapse_cpu.py links them)"""
    stock, fmt = emu.build_stub(), emu.build_fmtopts()
    objs = [os.path.join(fmt, f + ".o") for f in ("fmtopts_stub", "bcsplit_stub", "bcsplit_emu")]
    for f in ("collapse_emu", "collapse_stub"):
        objs.append(os.path.join(tmp, f + ".o"))
        subprocess.check_call(emu._CXX + ["-c", os.path.join(ROOT, "tests", "emu", f + ".cpp"), "-o", objs[-1]])
    d = os.path.join(tmp, "stub")
    os.makedirs(d)
    subprocess.check_call(emu._LINK + [os.path.join(stock, "fxg_stub.o")] + objs + emu._emu_objects([]) + ["-o", os.path.join(d, "libfxg.so"), "-ldl"])
    return d


def test_refusals_that_need_no_device_on_the_stub(tmp_path):
    """a new context of the stub, the refused call its first: the code and the text of the table, every output as include/fxg.h leaves it"""
    import ctypes as C
    import request_cases as R
    from fastx_toolkit_amd.engine import FxgCollapseInfo, FxgCollapseWindow
    rows = {i: o for i, e, o in K.FIRST_CALLS if o != K.OK and not o[3]}
    assert sorted(rows) == ["barcode_split_without_prepare", "collapse_add_no_set", "collapse_order_no_set", "collapse_write_no_set"]
    s = R.Session(os.path.join(emu.build_fmtopts(), "libfxg.so"))
    try:
        out = (C.c_uint8 * 64)(*([0xA5] * 64))
        args = (s.p, 64, 4, s.p, 9, 2, None, C.addressof(out), s.bin_bytes, s.bin_records)
        rc = s.lib.fxg_barcode_split(s.ctx, *args)
        assert (rc, s.last_error()) == rows["barcode_split_without_prepare"][1:3]
        assert bytes(out) == b"\xa5" * 64 and list(s.bin_bytes) == [0, 0]
    finally:
        s.close()
    lib = os.path.join(collapse_stub_dir(str(tmp_path)), "libfxg.so")
    vp, u64 = C.c_void_p, C.c_uint64
    for cid in ("collapse_add_no_set", "collapse_order_no_set", "collapse_write_no_set"):          # each on a context of its own: its very first call
        s = R.Session(lib)
        try:
            L = s.lib
            L.fxg_collapse_add.argtypes = [vp, vp, u64, C.c_int, vp, u64, u64, vp, C.POINTER(FxgCollapseInfo)]
            L.fxg_collapse_order.argtypes = [vp, C.POINTER(FxgCollapseInfo)]
            L.fxg_collapse_write.argtypes = [vp, u64, u64, vp, C.POINTER(FxgCollapseWindow)]
            info, win = FxgCollapseInfo(), FxgCollapseWindow(77, 77)
            C.memset(C.byref(info), 0xEE, C.sizeof(info))
            out = (C.c_uint8 * 64)(*([0xA5] * 64))
            if cid == "collapse_add_no_set":
                rc = L.fxg_collapse_add(s.ctx, s.p, 64, 2, s.p, 9, 2, s.p, C.byref(info))
            elif cid == "collapse_order_no_set":
                rc = L.fxg_collapse_order(s.ctx, C.byref(info))
            else:
                rc = L.fxg_collapse_write(s.ctx, 3, 64, C.addressof(out), C.byref(win))
            assert (rc, s.last_error()) == rows[cid][1:3], cid
            assert bytes(out) == b"\xa5" * 64, cid
            if cid == "collapse_write_no_set":
                assert (win.rank_end, win.out_bytes) == (3, 0), cid               # zeroed, rank_end = rank_begin
            else:
                assert tuple(getattr(info, k) for k in K.COLLAPSE_INFO_FIELDS) == K.COLLAPSE_INFO_REFUSED, cid
        finally:
            s.close()


# ---- the attribute invariant ----------------------------------------------------------------------------------------------------------------
def plan_of(monkeypatch, req):
    for k in K.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in req["env"].items():
        monkeypatch.setenv(k, v)
    try:
        return emu.plan(req["stride"], make_params(**req["pd"]), n=700)
    finally:
        for k in req["env"]:
            monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def sequences():
    mp = pytest.MonkeyPatch()
    try:
        plans = {}

        def lds_of(req):
            key = (req["kernel"], req["stride"])
            if key not in plans:
                plans[key] = plan_of(mp, req)
                assert plans[key]["kernel"] == req["kernel"] and not plans[key]["clip_global"], (key, plans[key])
            return plans[key]["lds"]
        return K.attr_sequences(lds_of), plans
    finally:
        mp.undo()


def test_the_requests_reach_all_43_tile_kernels(sequences):
    reqs = K.tile_kernel_requests()
    names = [r["kernel"] for r in reqs]
    assert len(names) == len(set(names)) == K.N_TILE_KERNELS == 43
    table, _ = emu.clip_table()
    engine_names = emu.instance_names() + [emu.clip_instance_name(-b) for b, _ in table] + [emu.clip_instance_name(g) for g in K.CLIP_GENERAL]
    assert sorted(names) == sorted(engine_names)
    assert all(emu.clip_instance_name(g) is None for g in (8, 17, 48, 99, 128))          # the general forms are those four
    seq, plans = sequences
    assert [k for _, _, k, _ in seq["all"]] == list(range(43))
    for k in K.ALTERNATING:                                   # "among the last eleven to be first seen", and two LDS sizes each
        assert 43 - 11 <= k % 43 < 43
        assert len({plans[(reqs[k]["kernel"], s)]["lds"] for s in K.ALT_STRIDES}) == 2
    assert len({l for _, _, _, l in seq["threads"]}) == 4 and len(seq["threads"]) == 2 * K.THREAD_RUNS


PART_C = ["alternating", "two_contexts", "threads"]


@pytest.mark.parametrize("name", ["all"] + PART_C)
def test_attribute_covers_every_launch_of_the_gpu_sequences(sequences, name):
    launches = sequences[0][name]
    sets, asked = emu.attr_replay(launches)
    assert K.uncovered(launches, sets) == []
    assert all(b[3] > a[3] for a, b in zip(sets, sets[1:]) if (a[1], a[2]) == (b[1], b[2])), "an attribute was lowered"
    assert len(sets) <= asked <= len(launches)
    per_kernel = {}
    for _, dev, k, lds in sets:
        per_kernel.setdefault((dev, k), []).append(lds)
    assert all(v == sorted(set(v)) for v in per_kernel.values())          # raised only, never set twice to one value


@pytest.mark.parametrize("name", PART_C)
def test_the_old_policy_fails_the_same_check(sequences, name):
    """the check is not vacuous: fxg_kernel_fit's earlier logic, replayed over the same launches, leaves launches uncovered"""
    launches = sequences[0][name]
    bad = K.uncovered(launches, K.old_policy(launches))
    print("old policy, %s: %d of %d launches with more LDS than was last set; first %r" % (name, len(bad), len(launches), bad[:1]))
    assert bad
    if name == "alternating":                                  # the order of the issue: K large, K small, K large -- the third one, through the cache
        k = K.ALTERNATING[0] % 43
        mine = [b for b in bad if b[1][2] == k]
        assert [b[0] for b in mine] == [43 + 2, 43 + 4] and all(b[2] < b[1][3] for b in mine)
    if name == "all":
        assert K.uncovered(sequences[0]["all"], K.old_policy(sequences[0]["all"])) == []


def random_launches(seed):
    rng = np.random.default_rng(seed)
    nctx = 1 + seed % 3
    dev_of = [int(rng.integers(0, 2)) for _ in range(nctx)]
    if nctx > 1:
        dev_of[1] = 1 - dev_of[0]                              # both devices in use, and (three contexts) two contexts on one of them
    sizes = [0, 1024, 9 * 1024, 26 * 1024, 26 * 1024 + 16, 60 * 1024, 160 * 1024]
    hot = [int(x) for x in rng.choice(43, size=6, replace=False)]
    out = []
    for _ in range(600):
        c = int(rng.integers(0, nctx))
        k = hot[int(rng.integers(0, 6))] if rng.random() < 0.5 else int(rng.integers(0, 43))
        out.append((c, dev_of[c], k, sizes[int(rng.integers(0, len(sizes)))]))
    return out, nctx


@pytest.mark.parametrize("seed", range(20))
def test_attribute_covers_every_launch_of_random_sequences(seed):
    launches, nctx = random_launches(seed)
    sets, asked = emu.attr_replay(launches, nctx)
    assert K.uncovered(launches, sets) == []
    assert len({(d, k) for _, d, k, _ in sets}) == len({(d, k) for _, d, k, _ in launches})          # one table entry per (device, kernel) met: none lost, none doubled


def test_the_old_policy_fails_on_random_sequences_with_several_contexts():
    bad = {seed: len(K.uncovered(*(lambda l: (l, K.old_policy(l)))(random_launches(seed)[0]))) for seed in range(20)}
    print("old policy, launches uncovered per seed:", bad)
    assert all(bad[seed] > 0 for seed in range(20) if seed % 3 == 2)          # three contexts, two of them on one device: one lowers what the other raised


def test_uncovered_sees_a_lowered_attribute():
    launches = [(0, 0, 5, 100), (0, 0, 5, 50), (0, 0, 5, 100)]
    assert K.uncovered(launches, [(0, 0, 5, 100)]) == []
    assert K.uncovered(launches, [(0, 0, 5, 100), (1, 0, 5, 50)]) == [(2, (0, 0, 5, 100), 50)]
    assert K.uncovered(launches, [(0, 1, 5, 100)]) == [(0, (0, 0, 5, 100), None), (1, (0, 0, 5, 50), None), (2, (0, 0, 5, 100), None)]      # another device's


# ---- the grow rule ------------------------------------------------------------------------------------------------------------------------------
def test_the_interleaved_sequence_regrows_every_workspace_twice():
    import context_state_sequence as S
    steps = S.build(cus=256)
    model = K.GrowModel()
    for i, st in enumerate(steps):
        for name, need_cap in S.workspace_use(st, cus=256):
            model.use(i, name, need_cap)
    regrown = model.regrown()
    named = {}
    for i, st in enumerate(steps):
        for ws in st.get("regrows", ()):
            named.setdefault(ws, []).append(i)
    assert named == regrown, (named, regrown)
    for ws in S.WORKSPACES:
        assert len(regrown.get(ws, [])) >= 2, (ws, regrown.get(ws))
    assert 140 <= len(steps) <= 170


# ---- the table under threads ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.sanitizers
@pytest.mark.parametrize("san", ["thread", "address,undefined"])
def test_attribute_table_under_sanitizers(tmp_path, san):
    """a program with a main of its own (emu/attr_san_main.cpp), built with -fsanitize and run directly, nothing preloaded: six threads, a context's cache
    each, 20 000 launches each of 69 kernels on two devices through one process table; every launch covered, no set ever lowers"""
    exe = str(tmp_path / "attr_san_main")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-x", "c++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wno-option-ignored", "-fsanitize=" + san,
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "emu", "attr_san_main.cpp"), "-o", exe, "-lpthread"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=dict(os.environ, TSAN_OPTIONS="exitcode=66", ASAN_OPTIONS="detect_leaks=1:exitcode=99"))
    assert p.returncode == 0 and p.stderr == b"", (p.returncode, p.stdout, p.stderr[-2000:])
    assert b" 0 launches uncovered, 0 sets that lowered" in p.stdout
