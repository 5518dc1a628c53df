"""CPU half of tests/test_gpu_geometry_collapse.py and tests/test_gpu_large_offsets_collapse.py: the generators and closed forms of tests/collapse_shapes.py
against collapse_model on the same text at sizes Python parses, the Python form of the hash against the emulator's export, and what the GPU cases claim of
their own shapes -- which half of the old table the representatives hash to, which workgroups stage, what lies at an arena offset taken modulo 2^32."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import collapse_cases as CK
import collapse_model as M
import collapse_shapes as SH
import emu_py
from conftest import ROOT


def parsed(text):
    return M.collapse(M.records_of(text))


# ---- the hash ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_hash(tmp_path_factory):
    """fxg_emu_collapse_hash of emu/collapse_emu.cpp: fxg_cl_hash itself (tests/test_collapse_cpu.py holds it against std::hash<std::string>)"""
    d = str(tmp_path_factory.mktemp("shapes"))
    obj = os.path.join(d, "collapse_emu.o")
    subprocess.check_call(emu_py._CXX + ["-c", os.path.join(ROOT, "tests", "emu", "collapse_emu.cpp"), "-o", obj])
    subprocess.check_call(emu_py._LINK + [obj, "-o", os.path.join(d, "libcollapse_emu.so")])
    L = C.CDLL(os.path.join(d, "libcollapse_emu.so"))
    L.fxg_emu_collapse_hash.argtypes, L.fxg_emu_collapse_hash.restype = [C.c_void_p, C.c_uint32], C.c_uint64
    return L.fxg_emu_collapse_hash


def test_python_hash_is_the_engines(emu_hash):
    for n in list(range(0, 41)) + [150, 192, 250, 1000]:
        s = CK.seq(n * 31 + 5, n)
        buf = np.frombuffer(s + b"\0" * 8, dtype=np.uint8).copy()
        assert SH.std_hash(s) == emu_hash(buf.ctypes.data, n), n


# ---- templates and rows -----------------------------------------------------------------------------------------------------------------------------
def test_templates_differ_and_rows_parse():
    t = torch.arange(0, 3000, dtype=torch.int64)
    for L in (1, 11, 12, 13, 36, 97):
        b = SH.bases_of(torch, t[:4 ** min(L, 5)], L, 3)
        assert len({bytes(r.tolist()) for r in b}) == len(b), L           # distinct templates, distinct bases
        assert set(b.reshape(-1).tolist()) <= set(b"ACGT")
    b = SH.bases_of(torch, t, 36, 3)
    text = bytes(SH.rows(torch, t + 5, b).reshape(-1).tolist())
    recs = list(M.records_of(text))
    assert [n for n, _ in recs] == [b"%09d" % (i + 5) for i in range(3000)] and [s for _, s in recs] == [bytes(r.tolist()) for r in b]
    text = bytes(SH.rows(torch, t, b, counts=t * 7 + 1, cw=6).reshape(-1).tolist())
    assert [M.get_reads_count(n) for n, _ in M.records_of(text)] == [7 * i + 1 for i in range(3000)]
    assert len(text) == 3000 * SH.row_width(36, 6)
    assert SH.template_bytes(torch, 77, 36, 3) == bytes(b[77].tolist())


# ---- 1. slot launches in several trips ---------------------------------------------------------------------------------------------------------------
def test_trips_closed_form_is_the_model():
    table = SH.bases_of(torch, torch.arange(SH.TRIPS_NT), SH.TRIPS_L, SH.TRIPS_SEED)
    for n in (1, 5002, 5003, 5004, 12345):
        text = bytes(SH.trips_block(torch, 0, n, table, "cpu").reshape(-1).tolist())
        sums = parsed(text)
        counts = SH.trips_counts(n)
        assert sum(counts) == n
        assert sums == {bytes(table[t].tolist()): c for t, c in enumerate(counts) if c}
        assert sums == SH.sums_of(torch, SH.trips_templates(torch, 0, n), SH.TRIPS_L, SH.TRIPS_SEED)
    assert SH.trips_counts(SH.TRIPS_N) == torch.bincount(SH.trips_templates(torch, 0, SH.TRIPS_N), minlength=SH.TRIPS_NT).tolist()


def test_trips_shapes():
    """the table of 2^25 slots is initialised in two trips; 2 x (5 003 + 2^24 + 1) exceeds it, so the large block rebuilds it into 2^26 slots: the rebuild
    walks the old table in two trips, and representatives sit in both halves of it; init, mark and scatter walk the new one in four"""
    assert SH.SLOT_TRIP == 1 << 24 and SH.TRIPS_SLOTS == 2 * SH.SLOT_TRIP
    assert CK.slots_after(SH.TRIPS_SLOTS, [(0, SH.TRIPS_NT), (SH.TRIPS_NT, SH.TRIPS_N)]) == (1 << 26, 1)
    assert CK.slots_after(SH.TRIPS_SLOTS, [(0, SH.TRIPS_NT), (SH.TRIPS_NT, SH.TRIPS_N - 5004)]) == (1 << 25, 0)          # (the record count is at the threshold)
    table = SH.bases_of(torch, torch.arange(SH.TRIPS_NT), SH.TRIPS_L, SH.TRIPS_SEED)
    slot = [SH.std_hash(bytes(r.tolist())) & (SH.TRIPS_SLOTS - 1) for r in table]
    upper = sum(s >= SH.SLOT_TRIP for s in slot)
    assert 2000 < upper < 3003, upper
    assert len({s >> 24 for s in (SH.std_hash(bytes(r.tolist())) & ((1 << 26) - 1) for r in table)}) == 4               # and in every quarter of the new one
    assert len(set(slot)) > 5000                             # (hardly a collision: the rebuild's work is the walk, not the probing)


# ---- 2. the staging boundary ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead,first,again", [(16, 49152, 49168), (17, 49168, 49152), (31, 49168, 49152)])
def test_boundary_spans(lead, first, again):
    blocks = SH.boundary_case(lead)
    spans = SH.staged_spans([[len(b) for _, b in blk] for blk in blocks])
    assert [s for s, _ in spans[1]] == [first] and [s for s, _ in spans[3]] == [again]
    assert spans[1][0][1] == (first <= SH.STAGE_BYTES) and spans[3][0][1] == (again <= SH.STAGE_BYTES) and spans[1][0][1] != spans[3][0][1]
    assert lead % 16 == {16: 0, 17: 1, 31: 15}[lead]
    seen = {b for _, b in blocks[1]}
    dup = [b for _, b in blocks[3] if b in seen]
    assert len(dup) > 150 and len(blocks[3]) - len(dup) >= 40 and len(seen) == 200


def test_alternating_spans():
    (recs,) = SH.alternating_case()
    spans = SH.staged_spans([[len(b) for _, b in recs]])[0]
    assert [st for _, st in spans] == [True, False] * 3
    assert all(s <= SH.STAGE_BYTES - 1000 for s, st in spans if st) and all(s >= SH.STAGE_BYTES + 1000 for s, st in spans if not st)
    first = {}
    for r, (_, b) in enumerate(recs):
        first.setdefault(b, r // SH.WG)
    crossing = [(first[b], r // SH.WG) for r, (_, b) in enumerate(recs) if first[b] != r // SH.WG]
    assert sum(1 for a, g in crossing if (a - g) % 2) >= 25          # duplicates whose first occurrence lies in a workgroup of the other kind
    assert sum(1 for a, g in crossing if (a - g) % 2 == 0) >= 100    # and of the same kind


# ---- 3. contention ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,count", [(1 << 10, 4100), (1 << 12, (1 << 31) - 1), (40, 1)])
def test_contention_closed_form_is_the_model(n, count):
    text, sums = SH.contention_block(np, n, count)
    got = parsed(text)
    assert got == sums and list(got) == list(sums)
    assert len(set(sums.values())) == len(sums)


def test_contention_counts_pass_the_marks():
    singles = SH.CONT_SINGLES
    a = ((1 << 20) - singles) * 4100
    assert 1 << 32 < a < 1 << 33 and M.printed(a) == a - (1 << 32)                 # past 2^32: the printed int is the sum less 2^32
    b = ((1 << 20) - singles) * ((1 << 31) - 1)
    assert b > 1 << 50 and M.printed(b) < 0                                          # the largest count an id can carry: 2^51, printed negative
    # a sum past 2^64 needs 2^33 records (an id's count is below 2^31): no block reaches it, and no test of the suite takes a count sum there
    assert ((1 << 31) - 1) * (0xFFFFFFF0 // 4) < 1 << 64


# ---- 4. the arena -----------------------------------------------------------------------------------------------------------------------------------------
def arena_checks(A, least=8):
    t = A.templates(torch, 0, A.R)
    g = torch.arange(A.R)
    assert bool((t[t] == t).all()) and bool((t <= g).all())                          # a template's number is its first record's
    lo, mid, hi = g < A.G31, (g >= A.G31) & (g < A.G32), g >= A.G32
    assert (A.G31 - 1) * A.L < A.m31 <= A.G31 * A.L and (A.G32 - 1) * A.L < A.m32 <= A.G32 * A.L
    only_hi = hi & (t >= A.G32)
    assert int((only_hi & (t == g)).sum()) >= least and int((only_hi & (t != g)).sum()) >= least         # sequences that occur only above m32, some of them twice
    assert int((hi & (t < A.G31)).sum()) >= least                                        # first below m31, again above m32
    assert int((hi & (t >= A.G31) & (t < A.G32)).sum()) >= least                         # first between the marks, again above m32
    assert int((mid & (t < A.G31)).sum()) >= least                                       # first below m31, again between the marks
    assert int((lo & (t != g)).sum()) >= 2
    mine, a, b = A.aliases(torch)
    assert bool((mine != a).all()) and bool((mine != b).all())                       # a truncated offset reads another template's bytes
    ts, counts = A.counts(torch)
    assert int(counts.sum()) == A.R and int(counts.max()) <= 9                       # every printed count is one digit
    return t, ts, counts


def test_arena_small_is_the_model():
    A = SH.Arena(L=97, m31=1 << 14, m32=1 << 15)
    t, ts, counts = arena_checks(A, least=4)
    text = b"".join(bytes(A.text_rows(torch, g0, g1, "cpu").reshape(-1).tolist()) for g0, g1 in [(0, 100), (100, A.R)])
    sums = parsed(text)
    assert sums == SH.sums_of(torch, t, A.L, A.seed)
    assert len(sums) == len(ts) and sorted(sums.values()) == sorted(counts.tolist())
    assert M.out_bytes(sums) == M.out_bytes({SH.Seq(int(x), A.L): int(c) for x, c in zip(ts, counts)})


def test_arena_real_shape():
    A = SH.Arena()
    arena_checks(A)
    assert A.R == 182559 and A.R * A.L > (1 << 32) + (1 << 28) >= (A.R - 1) * A.L    # the fewest records of the longest line that pass the mark
    blocks = A.blocks()
    assert len(blocks) == 2 and blocks[0][0] == 0 and blocks[-1][1] == A.R and blocks[0][1] == blocks[1][0]
    assert all((g1 - g0) * SH.row_width(A.L) <= 0xFFFFFFF0 for g0, g1 in blocks)
