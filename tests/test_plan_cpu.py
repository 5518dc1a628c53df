"""CPU tier: what a request runs, through the emulator's plan-only door (emu.plan: fxg_plan_request of csrc/fxg_plan.h, the very code the engine calls,
and the name the engine would report for the planned instance).  The plan never dereferences the batch, so every family of the GPU tier is planned
here at the sizes it runs there, 8 GiB arrays included, at no cost.

  * the instance table (csrc/fxg_instances.h) against the tests' own list of names, and the two name formats of the clip instances;
  * the choice per family of tests/test_gpu_geometry.py and tests/large_offsets.py, and the overrides those GPU tests rely on;
  * the stride boundaries of the rows kernels;
  * the knob table (csrc/fxg_knobs.h): every variable unset, valid, out of range and empty, against the parsed struct and the planned result.
"""
import pytest

import emu_py as emu
import large_offsets as lo
from helpers import oracle_params
from test_gpu_geometry import CALL_KNOBS, ENGINE_KNOBS, FAM, HIST, QTF

# the tests' OWN statement of the instances besides the clipper's (never read out of the code under test): what fxg_last_launch_info reports,
# bench.py matches stored counter files on, and the GPU tier matches prefixes of
INSTANCE_NAMES = [
    "fxg_kernel_rows<26> qtrim+qfilter",
    "fxg_kernel_rows<38> qtrim+qfilter",
    "fxg_kernel_rows<26,2> qtrim+qfilter",
    "fxg_kernel_rows<38,2> qtrim+qfilter",
    "fxg_kernel_rows_multi<10,4> qtrim+qfilter",
    "fxg_kernel_rows_multi<14,3> qtrim+qfilter",
    "fxg_kernel_rows_multi<20,2> qtrim+qfilter",
    "fxg_kernel_tiles<0,0> qtrim+qfilter",
    "fxg_kernel_tiles<0,1> ftrim",
    "fxg_kernel_tiles<0,2> revcomp[+ftrim]",
    "fxg_kernel_tiles<0,3> mask",
    "fxg_kernel_tiles<0,4> base census",
    "fxg_kernel_tiles<0,5> revcomp[+ftrim], dword-aligned windows",
]
TILES00 = "fxg_kernel_tiles<0,0> qtrim+qfilter"
FAMS = dict(lo.families(), hist=HIST)
ROWS_FAMS = [k for k, f in FAMS.items() if f.get("rows")]
ALL_KNOBS = CALL_KNOBS + ENGINE_KNOBS + ("FXG_CLIP_K_ONE_PASS", "FXG_NO_PACKED_CLIP", "FXG_QS_ROUND_ROBIN", "FXG_NO_SCAN_FALLBACK", "FXG_TEST_SCAN_TIMEOUT")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)


def _plan(monkeypatch, f, env=None, **kw):
    """the plan of family f's request under its call knobs and `env`"""
    for k, v in dict(f.get("env", {}), **(env or {})).items():
        monkeypatch.setenv(k, str(v))
    return emu.plan(f["stride"], oracle_params(f["pd"]), **kw)


def _quality(monkeypatch, stride, **env):
    """the instance of a compacting quality trim + filter over rows of `stride` bytes"""
    return _plan(monkeypatch, dict(stride=stride, pd=dict(stages=6, **QTF), env=env), n=513 * 64)["kernel"]


def test_the_instance_table_holds_the_names_the_tests_state():
    """The table is exactly the list above (four rows kernels, three with several reads per lane, six tile kernels; the table's order is the launch
    switch's and nothing relies on it)."""
    assert len(set(INSTANCE_NAMES)) == len(INSTANCE_NAMES) == 4 + 3 + 6
    assert sorted(emu.instance_names()) == sorted(INSTANCE_NAMES)
    # the clip instances: one packed and one general bucket, byte for byte; no name where the clip table has no instance
    assert emu.clip_instance_name(-13) == "fxg_kernel_tiles<-13,0> clip(packed)[+qtrim+qfilter]"
    assert emu.clip_instance_name(32) == "fxg_kernel_tiles<32,0> clip[+qtrim+qfilter]"
    assert emu.clip_instance_name(-17) is None and emu.clip_instance_name(0) is None


# ---- the choice, per family of the GPU tier ----
@pytest.mark.parametrize("fam", sorted(FAMS))
def test_every_family_plans_its_instance_and_tile(monkeypatch, fam):
    """Each family of tests/test_gpu_geometry.py (FAM, HIST) and tests/large_offsets.py (EXTRA) at 513 tiles under its own call knobs: the instance
    the GPU tier expects by name, and the tile size where the family states one."""
    f = FAMS[fam]
    T = f.get("T", 256)
    p = _plan(monkeypatch, f, n=513 * T, ragged=fam == "hist", hist=0 if fam == "hist" else None)
    assert p["kernel"].startswith(f["kernel"]), (fam, p)
    assert emu.instance_names().count(p["kernel"]) == (0 if f.get("clip") else 1), (fam, p)
    if "T" in f:
        assert p["tile"] == f["T"], (fam, p)
    assert p["block"] == (64 if f.get("rows") else 256), (fam, p)


def test_the_overrides_the_gpu_tier_relies_on(monkeypatch):
    for fam in ROWS_FAMS:                      # uncompacted launches never take a rows kernel: they need no output placement
        p = _plan(monkeypatch, FAMS[fam], n=513 * FAMS[fam]["T"], compact=False)
        assert p["kernel"] == TILES00 and p["block"] == 256, (fam, p)
    assert _plan(monkeypatch, FAMS["rows38"], n=513 * 64, compact=False)["tile"] == 128
    rev5 = FAMS["rev5"]
    assert _plan(monkeypatch, rev5, n=513 * 128)["kernel"].startswith("fxg_kernel_tiles<0,5> revcomp")
    assert _plan(monkeypatch, rev5, n=513 * 128, ragged=True)["kernel"] == "fxg_kernel_tiles<0,2> revcomp[+ftrim]"       # the dword form serves fixed-length batches only
    assert _plan(monkeypatch, rev5, env=dict(FXG_REV_DW="0"), n=513 * 128)["kernel"] == "fxg_kernel_tiles<0,2> revcomp[+ftrim]"
    monkeypatch.delenv("FXG_REV_DW")
    assert _plan(monkeypatch, rev5, env=dict(FXG_TILE="2"), n=513 * 2)["kernel"] == "fxg_kernel_tiles<0,2> revcomp[+ftrim]"  # ... in tiles of a multiple of four reads
    monkeypatch.delenv("FXG_TILE")
    for stride in range(1, 401):               # FXG_ROWS=0 never plans a rows kernel
        assert _quality(monkeypatch, stride, FXG_ROWS="0") == TILES00, stride
    p = _plan(monkeypatch, dict(stride=304, pd=dict(stages=6, **QTF)), env=dict(FXG_ROWS="2"), n=513 * 32)
    assert p["kernel"] == "fxg_kernel_rows<38,2> qtrim+qfilter" and p["tile"] == 32 and p["block"] == 64, p


# ---- the stride boundaries of the rows choice: compaction, stages = 6 (what the parent of the change that added this file planned) ----
ROWS_BY_STRIDE = [(27, TILES00), (28, "fxg_kernel_rows_multi<10,4>"), (40, "fxg_kernel_rows_multi<10,4>"), (41, "fxg_kernel_rows_multi<14,3>"),
                  (56, "fxg_kernel_rows_multi<14,3>"), (57, "fxg_kernel_rows_multi<20,2>"), (79, "fxg_kernel_rows_multi<20,2>"),
                  (80, "fxg_kernel_rows<26>"), (104, "fxg_kernel_rows<26>"), (105, "fxg_kernel_rows<38>"), (152, "fxg_kernel_rows<38>"),
                  (153, "fxg_kernel_rows<26,2>"), (208, "fxg_kernel_rows<26,2>"), (209, TILES00)]
ROWS2_BY_STRIDE = [(208, "fxg_kernel_rows<26,2>"), (209, "fxg_kernel_rows<38,2>"), (304, "fxg_kernel_rows<38,2>"), (305, TILES00)]


def test_rows_kernels_by_stride(monkeypatch):
    for stride, kernel in ROWS_BY_STRIDE:
        assert _quality(monkeypatch, stride) == (kernel if kernel == TILES00 else kernel + " qtrim+qfilter"), stride
    for stride, kernel in ROWS2_BY_STRIDE:
        assert _quality(monkeypatch, stride, FXG_ROWS="2") == (kernel if kernel == TILES00 else kernel + " qtrim+qfilter"), stride
    # the tile of a rows kernel: 64 lanes, R reads per lane, H lanes per read
    for stride, tile in ((36, 256), (50, 192), (76, 128), (100, 64), (150, 64), (200, 32)):
        assert _plan(monkeypatch, dict(stride=stride, pd=dict(stages=6, **QTF)), n=513 * tile)["tile"] == tile, stride
    # one stage of the two is enough; a clip stage, or no compaction, is not a rows request
    assert _plan(monkeypatch, dict(stride=100, pd=dict(stages=2, qt_threshold=20, qt_min_len=30)), n=64)["kernel"].startswith("fxg_kernel_rows<26>")
    assert _plan(monkeypatch, dict(stride=100, pd=dict(stages=4, qf_min_quality=20, qf_min_percent=80)), n=64)["kernel"].startswith("fxg_kernel_rows<26>")
    assert _plan(monkeypatch, FAMS["cfg5"], n=64)["kernel"].startswith("fxg_kernel_tiles<-13,0> clip(packed)")


# ---- the knob table ----
M = 2 ** 31 - 1
# variable -> (value when unset, {text: parsed value}): the tests' own statement of csrc/fxg_knobs.h, every row with a valid text, one outside the
# accepted range where there is one, and the empty string
KNOBS = {
    "request": {
        "FXG_TILE": (0, {"64": 64, "3": 3, "100000": 100000, "-4": -4, "": 0}),          # the raw number: the range depends on the instance (below)
        "FXG_ROWS": (1, {"0": 0, "1": 1, "2": 2, "7": 7, "-1": -1, "": 0}),
        "FXG_CLIP_GLOBAL": (-1, {"0": 0, "1": 1, "7": 1, "-1": 1, "": 0}),
        "FXG_REV_DW": (-1, {"0": 0, "1": 1, "7": 1, "-1": 1, "": 0}),
        "FXG_CLIP_K_ONE_PASS": (0, {"1": 1, "0": 1, "": 1}),                              # on when set at all
        "FXG_NO_PACKED_CLIP": (0, {"1": 1, "0": 1, "": 1}),
        "FXG_NO_SCAN_FALLBACK": (0, {"1": 1, "0": 1, "": 1}),
        "FXG_CLIP_DEPTH_RT": (0, {"2": 2, "3": 3, "4": 4, "1": 0, "5": 0, "-3": 0, "": 0}),
        "FXG_QS_ROUND_ROBIN": (1, {"0": 0, "1": 1, "3": 3, "0x3": 3, "010": 8, "-1": 2 ** 32 - 1, "": 0}),
    },
    "context": {
        "FXG_BLOCKS_PER_CU": (0, {"1": 1, "16": 16, "17": 0, "0": 0, "-2": 0, "": 0}),
        "FXG_WORKERS": (0, {"1": 1, "37": 37, str(M): M, "0": 0, "-2": 0, "": 0}),
        "FXG_NSCAN": (0, {"1": 1, "64": 64, "65": 0, "0": 0, "": 0}),
        "FXG_TEST_SCAN_TIMEOUT": (0, {"1": 1, "0": 0, "-1": 0, "": 0}),
        "FXG_TICKET_GROUPS": (0, {"1": 1, "3": 3, "8": 8, "9": 0, "0": 0, "": 0}),
    },
}


@pytest.mark.parametrize("scope", sorted(KNOBS))
def test_knob_parsing(monkeypatch, scope):
    unset = {k: v[0] for k, v in KNOBS[scope].items()}
    assert emu.knobs(scope) == unset                       # the table has these rows and no others
    for name, (_, texts) in KNOBS[scope].items():
        for text, value in texts.items():
            monkeypatch.setenv(name, text)
            assert emu.knobs(scope) == dict(unset, **{name: value}), (name, text)
            other = "context" if scope == "request" else "request"
            assert emu.knobs(other) == {k: v[0] for k, v in KNOBS[other].items()}
        monkeypatch.delenv(name)


def test_knobs_in_the_planned_result(monkeypatch):
    """What the parsed values do to a plan, where the plan is what accepts or ignores them."""
    t00 = FAMS["tiles00"]                                  # 150-byte rows, FXG_ROWS=0: tiles of 128 reads, 256 threads
    for text, tile in (("64", 64), ("1", 1), ("256", 256), ("3", 128), ("512", 128), ("0", 128), ("-4", 128), ("", 128)):
        assert _plan(monkeypatch, t00, env=dict(FXG_TILE=text), n=1000)["tile"] == tile, text
    monkeypatch.delenv("FXG_TILE")
    assert _quality(monkeypatch, 300, FXG_ROWS="-1") == TILES00 and _quality(monkeypatch, 300, FXG_ROWS="7").startswith("fxg_kernel_rows<38,2>")
    assert _quality(monkeypatch, 100, FXG_ROWS="") == TILES00          # the empty string is 0
    monkeypatch.delenv("FXG_ROWS")
    ad13, ad34 = b"AGATCGGAAGAGC", b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"
    clip = lambda stride, ad: dict(stride=stride, pd=dict(stages=1, adapter=ad, clip_min_len=5, clip_flags=4))
    for text, want in ((None, True), ("1", True), ("0", False), ("", False)):      # 188-byte rows: the plan's own choice is the DP over the batch
        env = {} if text is None else dict(FXG_CLIP_GLOBAL=text)
        assert _plan(monkeypatch, clip(188, ad13), env=env, n=300)["clip_global"] is want, text
    assert _plan(monkeypatch, clip(100, ad13), env=dict(FXG_CLIP_GLOBAL="1"), n=300)["clip_global"] is True
    monkeypatch.delenv("FXG_CLIP_GLOBAL")
    assert _plan(monkeypatch, clip(100, ad34), n=300)["two_pass"] is True
    assert _plan(monkeypatch, clip(100, ad34), env=dict(FXG_CLIP_K_ONE_PASS="0"), n=300)["two_pass"] is False
    monkeypatch.delenv("FXG_CLIP_K_ONE_PASS")
    p = _plan(monkeypatch, clip(100, ad13), env=dict(FXG_NO_PACKED_CLIP="0"), n=300)
    assert p["amax"] == 16 and p["kernel"] == "fxg_kernel_tiles<16,0> clip[+qtrim+qfilter]", p
    monkeypatch.delenv("FXG_NO_PACKED_CLIP")
    # FXG_CLIP_DEPTH_RT: fewer slots between decision and write-out are less LDS; a value outside 2..4 is no value
    lds = {text: _plan(monkeypatch, clip(100, ad13), env=dict(FXG_CLIP_DEPTH_RT=text) if text else {}, n=300)["lds"] for text in (None, "2", "3", "4", "5", "1")}
    assert lds["2"] < lds["3"] <= lds["4"] and lds["5"] == lds["1"] == lds[None] and lds[None] in (lds["3"], lds["4"]), lds
