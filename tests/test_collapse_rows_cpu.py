"""fxg_collapse_add_rows and fastx_clip_collapser, CPU tier: the engine's host half and the two new kernel bodies through the CPU emulator
(tests/emu/collapse_rows_emu.cpp) -- every recorded collapser case added as packed rows gives the reference's bytes, rows and text alternate
within a set, the shapes at which the copy can go wrong, the zero-length rule, the counts through kept_index, the refusal table, every array
against guard pages at the ends of the memory contract; the tool over a stub that has the entry on every recorded answer of the reference
pipe (golden/clip_collapse), in 1 MB blocks and across a hand-over to the record API and back; a library without the entry; and the emulator
as a stand-alone program under ASan + UBSan."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import collapse_cases as K
import collapse_model as M
import collapse_rows_cases as RC
import emu_py
import test_collapse_cpu as T

EMU_DIR = T.EMU_DIR
NONE, IRR_BASE = RC.NONE, RC.IRR_BASE


@pytest.fixture(scope="module")
def rowsdir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("collapse_rows"))
    emu = T._obj(os.path.join(EMU_DIR, "collapse_rows_emu.cpp"), os.path.join(d, "collapse_rows_emu.o"))
    subprocess.check_call(emu_py._LINK + [emu, "-o", os.path.join(d, "libcollapse_emu.so")])      # (the name test_collapse_cpu's loader opens)
    return d


def _load(rowsdir):
    L = T._load(rowsdir)                                     # every export of collapse_emu.cpp is there too
    vp, u64 = C.c_void_p, C.c_uint64
    L.fxg_emu_collapse_add_rows.argtypes = [vp, vp, vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp, vp, u64, C.c_int, C.POINTER(T.Info), C.c_char_p, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def rlib(rowsdir):
    return _load(rowsdir)


class Rows:
    """a block of packed rows with its count source, every array at exactly its contracted size"""

    def __init__(self, records, fastq=False, guard=None, source=True, every=3):
        recs = RC.chomped(records)
        self.n = len(recs)
        bases, off, lens = RC.pack_rows([b for _, b in recs])
        tight = (lambda a: emu_py._tight(a, guard)) if guard else (lambda a: a)
        self.bases, self.off, self.len = tight(bases), tight(off), tight(lens)
        self.ix = self.kept = None
        if source:
            block, kept = RC.with_dropped(records, every)
            self.ix, self.kept = T.Indexed(block, fastq, guard), tight(kept)


class EmuRows(T.EmuSet):
    def add_rows(self, rows, n=None, bases=True, off=True, lens=True, kept=True, text=True, line=True, cap_lines=None, lpr=None, first=1, last=0):
        info = T.Info()
        p = lambda a, on: a.ctypes.data if (on and a is not None) else None
        ix = rows.ix
        rc = self.L.fxg_emu_collapse_add_rows(self.h, p(rows.bases, bases), p(rows.off, off), p(rows.len, lens), rows.n if n is None else n, first, last, p(rows.kept, kept),
                                              p(ix.d_text, text) if ix else None, p(ix.d_line, line) if ix else None,
                                              (ix.cap_lines if ix else 0) if cap_lines is None else cap_lines, (ix.lpr if ix else 0) if lpr is None else lpr,
                                              C.byref(info), self.err, 300)
        return rc, info


FIELDS = ("records", "reads", "uniques", "slots", "rebuilds", "first_bad", "out_reads", "out_bytes", "irregular")


def fields(info):
    return {k: getattr(info, k) for k in FIELDS}


def finish(S, windows=None, guard=None):
    rc, info = S.order()
    assert rc == 0, S.message
    out, rank = b"", 0
    while rank < info.uniques:
        rc, got, w = S.write(rank, windows or info.out_bytes, guard)
        assert rc == 0 and w.rank_end > rank, S.message
        out, rank = out + got, w.rank_end
    assert len(out) == info.out_bytes
    return out, info


def run_rows(S, blocks, fastq=False, initial=0, bits=0, guard=None, mixed=False, source=True):
    """begin, the blocks as rows (mixed: every second one as text), order, write.  Returns (out, info)."""
    assert S.begin(initial, bits) == 0, S.message
    for k, blk in enumerate(blocks):
        if mixed and k % 2 == 1:
            rc, info = S.add(T.Indexed(blk, fastq, guard))
        else:
            rc, info = S.add_rows(Rows(blk, fastq, guard, source))
        assert rc == 0 and info.irregular == 0 and info.first_bad == NONE, S.message
    return finish(S, guard=guard)


def run_text(S, blocks, fastq=False, initial=0, bits=0):
    assert S.begin(initial, bits) == 0, S.message
    for blk in blocks:
        rc, info = S.add(T.Indexed(blk, fastq))
        assert rc == 0 and not info.irregular, S.message
    return finish(S)


@pytest.mark.parametrize("name,records,fastq,ways,initial,bits", T._variants())
def test_rows_give_the_recorded_bytes(rlib, name, records, fastq, ways, initial, bits):
    """every recorded collapser case, its records as packed rows at every offset residue with the counts through kept_index: the reference's bytes
    and the info the model and the growth rule give"""
    S = EmuRows(rlib)
    try:
        blocks = K.split(records, ways)
        out, info = run_rows(S, blocks, fastq, initial, bits)
        K.assert_output(name, out)
        want = T.expected_info(blocks, fastq, initial)
        assert {k: getattr(info, k) for k in want} == want
        if ways > 1:
            out2, info2 = run_rows(S, blocks, fastq, initial, bits, mixed=True)
            assert out2 == out and fields(info2) == fields(info)
    finally:
        S.close()


def test_rows_equal_text_field_by_field_and_window_by_window(rlib):
    """set A from rows, set B from text: info equal in every field, bytes equal over windows that end after every record"""
    records = [c for c in K.abi_cases() if c[0] == "ties"][0][1] + RC.prefix_case() + RC.residue_case()
    for ways, mixed in ((1, False), (2, False), (5, False), (5, True)):
        A, B = EmuRows(rlib), EmuRows(rlib)
        blocks = K.split(records, ways)
        out_a, info_a = run_rows(A, blocks, mixed=mixed)
        out_b, info_b = run_text(B, blocks)
        assert fields(info_a) == fields(info_b) and out_a == out_b
        sizes = [len(M.record_text(r, c, b)) for r, c, b in M.parse_output(out_b)]
        for k in range(1, len(sizes) + 1):
            ga, gb = A.write(0, sum(sizes[:k])), B.write(0, sum(sizes[:k]))
            assert ga[0] == gb[0] == 0 and ga[1] == gb[1] and ga[2].rank_end == gb[2].rank_end == k
        A.close(), B.close()


@pytest.mark.parametrize("n", RC.RECORDS)
def test_rows_record_counts(rlib, n):
    records = [(K.ident(i, 1 + i % 3), K.seq(i % 200, 18)) for i in range(n)]
    A, B = EmuRows(rlib), EmuRows(rlib)
    good = [(b"g%d" % i, K.seq(1000 + i, 20)) for i in range(5)]
    out_a, info_a = run_rows(A, [good, records, good])          # (an empty block between two regular ones, for n = 0)
    out_b, info_b = run_text(B, [good, records, good] if n else [good, good])
    assert fields(info_a) == fields(info_b) and out_a == out_b
    A.close(), B.close()


def test_rows_without_a_count_source_count_one(rlib):
    records = [(K.ident(i, 5), K.seq(i % 7, 30)) for i in range(100)]
    A, B = EmuRows(rlib), EmuRows(rlib)
    out_a, info_a = run_rows(A, [records], source=False)
    out_b, info_b = run_text(B, [[(b"r%d" % i, b) for i, (_, b) in enumerate(records)]])
    assert info_a.reads == 100 and fields(info_a) == fields(info_b) and out_a == out_b
    out_q, info_q = run_rows(A, [records], fastq=True)           # a FASTQ count source counts 1 too
    assert out_q == out_a and info_q.reads == 100
    A.close(), B.close()


def test_counts_come_from_the_kept_records_own_id(rlib):
    """ids of every count form through kept_index, a dropped record with another count before every kept one"""
    ids = [b"x-5", b"x-", b"x-0", b"x-abc", b"1-2-3", b"nodash", b"x- 7", b"x--4", b"x-+9", b"a-2000000000", b"b-2000000000", b"c-4294967297"]
    records = [(n, K.seq(k % 5, 21)) for k, n in enumerate(ids * 2)]
    A, B = EmuRows(rlib), EmuRows(rlib)
    assert A.begin() == 0
    rc, info_a = A.add_rows(Rows(records, every=1))
    assert rc == 0 and info_a.reads == sum(M.get_reads_count(n, False) for n, _ in records) & M.M64
    out_a, info_a = finish(A)
    out_b, info_b = run_text(B, [records])
    assert fields(info_a) == fields(info_b) and out_a == out_b and info_a.reads > 1 << 32
    A.close(), B.close()


def trimmed(records, first, last):
    """what fastx_trimmer -f first -l last writes of the records (fastx_trimmer.c:122-134)"""
    out = []
    for name, b in records:
        b = b[:last] if last else b
        if first > 1:
            if len(b) < first:
                continue
            b = b[first - 1:]
        out.append((name, b))
    return out


@pytest.mark.parametrize("first,last", [(1, 0), (0, 0), (1, 20), (3, 0), (2, 19), (9, 9), (16, 17), (17, 40), (40, 0), (1, 1), (200, 0)])
def test_rows_window_is_the_trimmers(rlib, first, last):
    """every row cut to first .. last as the trimmer cuts it, rows that end before `first` left out with their counts; a window no row reaches
    adds nothing between two regular blocks"""
    records = RC.residue_case() + RC.prefix_case() + [(K.ident(i, 2 + i % 3), K.seq(i % 9, 8 + i % 40)) for i in range(300)]
    good = [(b"g%d" % i, K.seq(1000 + i, 50)) for i in range(5)]
    A, B = EmuRows(rlib), EmuRows(rlib)
    assert A.begin(4) == 0 and B.begin(4) == 0
    ib = T.Info()
    for blk in (good, records[:150], records[150:], good):
        rc, ia = A.add_rows(Rows(blk, guard=None), first=first, last=last)
        assert rc == 0 and not ia.irregular, A.message
        want = trimmed(blk, max(first, 1), last)
        if want:
            rc, ib = B.add(T.Indexed(want))
            assert rc == 0 and not ib.irregular
        assert (ia.records, ia.reads, ia.uniques) == (ib.records, ib.reads, ib.uniques)
    out_a, ia = finish(A)
    out_b, ib = finish(B)
    assert out_a == out_b and {k: v for k, v in fields(ia).items() if k not in ("slots", "rebuilds")} == {k: v for k, v in fields(ib).items() if k not in ("slots", "rebuilds")}
    A.close(), B.close()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_zero_length_row_leaves_the_set_as_it_was(rlib, where):
    good = [(K.ident(i), K.seq(i % 5, 33)) for i in range(300)]
    bad = [(K.ident(i), K.seq(i, 17)) for i in range(40)]
    at = {"first": 0, "middle": 17, "last": 39}[where]
    bad[at] = (b"bad", b"")
    if where == "middle":
        bad[29] = (b"bad2", b"")                              # first_bad is the smallest
    A, B = EmuRows(rlib), EmuRows(rlib)
    want, want_info = run_text(B, [good[:100], good[100:]])
    assert A.begin() == 0
    rc, info = A.add_rows(Rows(bad))                           # the first call on an empty set
    assert (rc, info.irregular, info.first_bad, info.records, info.uniques, info.reads) == (0, IRR_BASE, at, 0, 0, 0), A.message
    rc, info = A.add_rows(Rows(good[:100]))
    assert rc == 0 and info.irregular == 0 and info.records == 100
    before = fields(info)
    rc, info = A.add_rows(Rows(bad))
    assert (rc, info.irregular, info.first_bad) == (0, IRR_BASE, at)
    assert {k: v for k, v in fields(info).items() if k not in ("irregular", "first_bad")} == {k: v for k, v in before.items() if k not in ("irregular", "first_bad")}
    rc, info = A.add_rows(Rows(good[100:]))
    assert rc == 0 and info.irregular == 0
    out, info = finish(A)
    assert out == want and all(getattr(info, k) == getattr(want_info, k) for k in ("records", "reads", "uniques", "out_reads", "out_bytes"))
    A.close(), B.close()


REFUSALS = [
    ("rows_before_begin", "fxg_collapse_add_rows: no set; fxg_collapse_begin makes one"),
    ("null_bases", "fxg_collapse_add_rows: a null pointer with 10 records"),
    ("null_off", "fxg_collapse_add_rows: a null pointer with 10 records"),
    ("null_len", "fxg_collapse_add_rows: a null pointer with 10 records"),
    ("source_without_kept_index", "a count source is d_kept_index, d_text, d_line and cap_lines together"),
    ("source_without_text", "a count source is d_kept_index, d_text, d_line and cap_lines together"),
    ("source_without_line", "a count source is d_kept_index, d_text, d_line and cap_lines together"),
    ("source_without_cap_lines", "a count source is d_kept_index, d_text, d_line and cap_lines together"),
    ("lines_per_record_alone", "a count source is d_kept_index, d_text, d_line and cap_lines together"),
    ("lines_per_record_3", "fxg_collapse_add_rows: lines_per_record 3; 2 (FASTA) or 4 (FASTQ)"),
    ("lines_per_record_0", "fxg_collapse_add_rows: lines_per_record 0; 2 (FASTA) or 4 (FASTQ)"),
    ("last_before_first", "fxg_collapse_add_rows: last_base 3 is before first_base 4"),
    ("record_limit", "a set holds at most 2^40 - 2"),
    ("rows_after_order", "fxg_collapse_add_rows: the set is ordered and takes no more blocks"),
]


def refusal_calls(S, rows, plain):
    """the refusal table's calls on a begun set that holds rows once: {name: (rc, message, info)}.  Shared with the GPU tier, which gives S and
    the rows its own way."""
    said = {}

    def call(name, r, **kw):
        rc, info = S.add_rows(r, **kw)
        said[name] = (rc, S.message, info)
    call("null_bases", rows, bases=False)
    call("null_off", rows, off=False)
    call("null_len", rows, lens=False)
    call("source_without_kept_index", rows, kept=False)
    call("source_without_text", rows, text=False)
    call("source_without_line", rows, line=False)
    call("source_without_cap_lines", rows, cap_lines=0)
    call("lines_per_record_alone", plain, lpr=2)
    call("lines_per_record_3", rows, lpr=3)
    call("lines_per_record_0", rows, lpr=0)
    call("last_before_first", rows, first=4, last=3)
    call("record_limit", rows, n=(1 << 40) - 2 - 9)
    return said


def test_refusals(rlib):
    """the code and the text; the set's counts in info, and the set, as they were"""
    recs = [(K.ident(i, 2), K.seq(i, 20)) for i in range(10)]
    rows, plain = Rows(recs), Rows(recs, source=False)
    S = EmuRows(rlib)
    rc, info = S.add_rows(rows)
    said = {"rows_before_begin": (rc, S.message, info)}
    assert (info.records, info.first_bad) == (0, NONE)
    assert S.begin() == 0
    rc, info = S.add_rows(rows)
    assert rc == 0 and (info.records, info.reads) == (10, 20)
    said.update(refusal_calls(S, rows, plain))
    for name in said:
        if name != "rows_before_begin":
            i = said[name][2]
            assert (i.records, i.reads, i.uniques, i.irregular, i.first_bad) == (10, 20, 10, 0, NONE), name
    rc, info = S.add_rows(Rows([], source=False))             # records == 0: a valid call that changes nothing
    assert rc == 0 and (info.records, info.reads) == (10, 20)
    rc, info = S.add_rows(rows)
    assert rc == 0 and (info.records, info.reads, info.uniques) == (20, 40, 10)      # the refused calls left nothing behind
    rc, info = S.order()
    assert rc == 0
    rc, info = S.add_rows(rows)
    said["rows_after_order"] = (rc, S.message, info)
    for name, text in REFUSALS:
        rc, msg, _ = said[name]
        assert rc == -1 and text in msg, (name, rc, msg)
    assert set(said) == {n for n, _ in REFUSALS}
    S.close()


def _guard_child(where, rowsdir):
    try:
        L = _load(rowsdir)
        for name, records, fastq, ways, opts in K.abi_cases():
            if len(records) > 2000:
                continue
            S = EmuRows(L)
            out, _ = run_rows(S, K.split(records, ways[-1]), fastq, opts[-1][0], opts[-1][1], guard=where, mixed=True)
            K.assert_output(name, out)
            S.close()
        S = EmuRows(L)
        out, _ = run_rows(S, [RC.residue_case(), RC.prefix_case()], guard=where, source=False)
        for first, last in ((3, 0), (2, 19), (17, 40), (200, 0)):
            assert S.begin() == 0
            rc, info = S.add_rows(Rows(RC.residue_case(), guard=where), first=first, last=last)
            assert rc == 0 and not info.irregular
        bad = RC.residue_case()
        bad[-1] = (b"bad", b"")
        assert S.begin() == 0
        rc, info = S.add_rows(Rows(bad, guard=where))
        assert rc == 0 and info.irregular
        S.close()
        os._exit(0)
    except AssertionError:
        os._exit(3)
    except BaseException:
        os._exit(4)


@pytest.mark.parametrize("where", ["after", "before"])
def test_emulated_rows_kernels_within_bounds(rowsdir, where):
    """d_bases ends at the last record's last byte, d_off / d_len / d_kept_index hold exactly `records` entries, the text and the line index are
    at their contracted sizes: each against a PROT_NONE page, so a byte touched outside is a SIGSEGV of the child"""
    import multiprocessing as mp
    p = mp.get_context("fork").Process(target=_guard_child, args=(where, rowsdir))
    p.start()
    p.join(600)
    assert p.exitcode == 0, "child exit %s (-11: an access outside an array's contract, 3: a wrong result)" % p.exitcode


# ---- the tool over the stubs ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stock_stub():
    from fastx_toolkit_amd import build as b
    d = emu_py.build_stub()
    b.build_engine()
    b.build_host()
    return d


def _stub(rowsdir, stock_stub, src, emu, name):
    so = T._obj(os.path.join(EMU_DIR, src), os.path.join(rowsdir, src.replace(".cpp", ".o")))
    eo = T._obj(os.path.join(EMU_DIR, emu), os.path.join(rowsdir, emu.replace(".cpp", ".o")))
    d = os.path.join(rowsdir, name)
    os.makedirs(d, exist_ok=True)
    subprocess.check_call(emu_py._LINK + [os.path.join(stock_stub, "fxg_stub.o"), so, eo] + emu_py._emu_objects([]) + ["-o", os.path.join(d, "libfxg.so"), "-ldl"])
    return d


@pytest.fixture(scope="module")
def rows_stub(rowsdir, stock_stub):
    """a libfxg.so of the stub's own objects plus the five entries (collapse_rows_stub.cpp over collapse_rows_emu.cpp)"""
    return _stub(rowsdir, stock_stub, "collapse_rows_stub.cpp", "collapse_rows_emu.cpp", "stub")


@pytest.fixture(scope="module")
def old_stub(rowsdir, stock_stub):
    """one with the four entries of before (collapse_stub.cpp over collapse_emu.cpp)"""
    return _stub(rowsdir, stock_stub, "collapse_stub.cpp", "collapse_emu.cpp", "stub4")


def test_recorded_cases_hold_the_corners():
    by = {c["name"]: c for c in RC.golden_cases()}
    assert len(by) >= 20 and sum(len(c["stdin"]) for c in by.values()) < 600000
    assert any(c["trimmer"] for c in by.values()) and any(not c["trimmer"] for c in by.values())
    for flag in ("-c", "-C", "-n", "-M"):
        assert any(flag in c["clipper"] for c in by.values()), flag
    assert by["fasta_ids_c"]["stdin"].count(">x-5\n") and ">x-\n" in by["fasta_ids_c"]["stdin"] and ">x-0\n" in by["fasta_ids_c"]["stdin"]
    assert "representing 12000000587 reads" in by["fasta_ids_c"]["report"]
    assert by["all_dropped_c"]["exit"] == 1 and by["all_dropped_c"]["stderr"] == "fastx_collapser: Premature End-Of-File (filename ='-')\n"
    assert by["all_dropped_trim_v"]["stderr"].startswith("fastx_trimmer: Premature End-Of-File")
    counts = [int(ln.split("-")[1]) for ln in by["ties_c"]["stdout"].splitlines() if ln.startswith(">")]
    assert sum(1 for c in set(counts) if counts.count(c) > 1) >= 3            # ties at several counts


@pytest.mark.parametrize("case", RC.golden_cases(), ids=lambda c: c["name"])
def test_tool_on_recorded_cases(rows_stub, case):
    RC.assert_golden_case(rows_stub, case)
    RC.assert_golden_case(rows_stub, case, {"FXH_READ_BUFFER_MB": "1"})


def test_tool_in_1mb_blocks_and_across_the_record_api(rows_stub):
    """a FASTA input of several 1 MB blocks with collapsed ids, against this project's own clipper and collapser run one after the other over the
    same stub; then the same input with a block in the middle that the device calls irregular and the record API accepts (a NUL byte, where the
    reference's C strings end): it is rewritten and takes the device path with the same chain, and the blocks after it take it again"""
    import random
    rng = random.Random(5)
    ad = RC.golden()["adapter"].encode()
    pool = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(15, 28))) for _ in range(400)]
    recs = [(b"r%d-%d" % (i, 1 + i % 4), (rng.choice(pool) + (ad if i % 7 else b"") + b"ACGTACGTACGTACGTACGT")[:rng.randint(30, 44)]) for i in range(70000)]
    fa = lambda rs: b"".join(b">" + n + b"\n" + b + b"\n" for n, b in rs)
    argv = ["-a", ad.decode(), "-l", "15", "-c", "-f", "2", "-L", "24"]
    env = {"FXH_READ_BUFFER_MB": "1"}
    text = fa(recs)
    assert len(text) > 3 << 20
    code, report, err, out = RC.run_tool(rows_stub, argv, text, env)
    assert code == 0 and err == "", err
    bin_ = os.path.dirname(RC.TOOL)
    e = dict(os.environ, LD_LIBRARY_PATH=rows_stub + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""), **env)
    p1 = subprocess.run([os.path.join(bin_, "fastx_clipper"), "-v", "-a", ad.decode(), "-l", "15", "-c"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    p2 = subprocess.run([os.path.join(bin_, "fastx_trimmer"), "-v", "-f", "2", "-l", "24"], input=p1.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    p3 = subprocess.run([os.path.join(bin_, "fastx_collapser"), "-v"], input=p2.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
    assert (p1.returncode, p2.returncode, p3.returncode) == (0, 0, 0), (p1.stderr, p2.stderr, p3.stderr)
    assert out == p3.stdout and report == p1.stderr + p2.stderr + p3.stderr
    odd = fa(recs[:30000]) + b">odd\0-7\n" + pool[0] + ad + b"\0acgt\n" + fa(recs[30000:])
    for env2 in (env, {}):
        code, report2, err, out2 = RC.run_tool(rows_stub, argv, odd, env2)
        assert code == 0 and err == "", err
        got = {b: c for _, c, b in M.parse_output(out2)}
        want = {b: c for _, c, b in M.parse_output(out)}
        extra = pool[0][1:24]                                  # the odd record: kept up to its NUL, clipped, trimmed, counted once (its id ends at the NUL)
        want[extra] = want.get(extra, 0) + 1
        assert got == want
        assert report2.decode().splitlines()[3] == "Input: %d reads." % (sum(1 + i % 4 for i in range(70000)) + 1)


def test_tool_without_the_entry_says_so_and_the_collapser_still_runs(old_stub):
    code, report, err, out = RC.run_tool(old_stub, ["-a", "ACGT"], b">a\nACGTTTTTACGT\n")
    assert code == 1 and out is None and "no CPU fallback" in err and "fxg_collapse_add_rows" in err
    code, out, err, _ = K.run_tool(old_stub, ["-v"], b">a-3\nAC\n>b\nAC\n")
    assert (code, out) == (0, b">1-4\nAC\n") and "Input: 2 sequences (representing 4 reads)" in err


# ---- a stand-alone program under the sanitizers --------------------------------------------------------------------------------------------
@pytest.mark.sanitizers
def test_rows_emulator_under_sanitizers(tmp_path):
    """collapse_rows_san_main.cpp built with -fsanitize=address,undefined and run directly, nothing preloaded: the host half of the entry and
    the two kernel bodies on every FASTA case but the largest, rows alone, rows and text alternating, and rows without a count source"""
    exe = str(tmp_path / "collapse_rows_san_main")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wno-pass-failed", "-DFXG_HOST_EMULATION",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(EMU_DIR, "collapse_rows_san_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    src = tmp_path / "case.txt"
    checked = 0
    cases = [(n, r, w, o) for n, r, f, w, o in K.abi_cases() if len(r) <= 2000 and not f] + [("growth", K.growth_case()[0], (12,), ((4, 0),))]
    for name, records, ways, opts in cases:
        src.write_bytes(K.case_text(records))
        want = K.expected(name)
        modes = ["rows", "mixed"] + (["plain"] if name in ("all_unique", "records_257") else [])
        for w in ways:
            for initial, bits in opts:
                for mode in modes:
                    cap = max(max(len(b) for _, b in records) + 40, want["len"] // 2)
                    p = subprocess.run([exe, str(src), str(w), str(cap), str(initial), str(bits), mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
                    assert not any(m in p.stderr for m in T.REPORT) and p.returncode != 99, (name, p.stderr[-1500:])
                    assert p.returncode == 0 and hashlib.md5(p.stdout).hexdigest() == want["md5"], (name, w, initial, bits, mode, p.stderr[-300:])
                    checked += 1
    assert checked > 80
