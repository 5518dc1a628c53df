"""fasta_nucleotide_changer, CPU tier: the Python model (nucchange_model.py) against the recorded answers of the reference and, where the
reference tree is present, against the reference itself on seeded inputs; the kernel's body through the CPU emulator
(tests/emu/nucchange_emu.cpp) against the block model, with the text between guard pages; the tool over a stub variant that has the entry
(its device path) and over the stock stub (its record path); the reference's own tool source against host/fastx.h; and the emulator and the
record path as stand-alone programs under ASan + UBSan."""
import ctypes as C
import gzip
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest

import emu_py
import nucchange_model as M
from nucchange_cases import ROOT, assert_tool_case, block_cases, galaxy_pairs, golden_cases, message_of, regular_text, run_tool

REF = os.environ.get("FXG_REFERENCE", "/root/reference")
REF_SRC = os.path.join(REF, "src", "fasta_nucleotide_changer", "fasta_nucleotide_changer.c")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fastx_toolkit_amd", "csrc")
HOST = os.path.join(ROOT, "fastx_toolkit_amd", "host")
BLOCKS = block_cases()


# ---- the model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_model_matches_recorded(case):
    argv = [a for a in case["argv"] if a not in ("-o", "OUT")]
    out, report, status, msg = M.run_argv(argv, case["stdin"].encode("latin-1"))
    assert status == case["exit"]
    if out == M.USAGE:
        assert case["stdout"] == M.USAGE
        return
    if case["name"] == "unknown_option":
        return
    to_file = "-o" in case["argv"]
    assert out == (case["outfile"] if to_file else case["stdout"]).encode("latin-1")
    if status == 0:                         # the report goes to stdout once -o is given, to stderr otherwise
        assert (report or b"") == (case["stdout"] if to_file else case["stderr"]).encode("latin-1")
    elif msg.startswith(("Error: found", "Please", "RNA mode")):
        assert message_of(case["stderr"]) == msg          # the tool's own three messages, to the letter
    else:
        assert msg in case["stderr"], (msg, case["stderr"])           # the reader's messages: the model names their kind


def test_recorded_cases_hold_the_contract_corners():
    by = {c["name"]: c for c in golden_cases()}
    assert len(by) >= 45
    assert by["collapsed_ids_v"]["stderr"] == "Mode: DNA-to-RNA\nInput: 129 reads.\nOutput: 129 reads.\nNucleotides changed: 5\n"
    assert by["fastq_rna_to_dna_v"]["stdout"] == ">r1\nACGTT\n>r2 TU\nTNTGC\n"                  # FASTA out of FASTQ, ids untouched
    assert by["offender_two_records"]["stdout"] == ">a\nACGT\n" and "on line 4." in by["offender_two_records"]["stderr"]
    assert by["offender_fastq"]["stderr"].count("line 8") == 1 and by["offender_fastq"]["stdout"] == ">a\nACGT\n"
    assert by["offender_second_record"]["stderr"].count("\n") == 1                              # no report on the error path
    assert by["dna_to_rna_v_o"]["stdout"].startswith("Mode: DNA-to-RNA") and by["dna_to_rna_v_o"]["outfile"] == by["dna_to_rna"]["stdout"]
    assert all(c["exit"] == 1 for n, c in by.items() if n.startswith(("offender_", "error_")) or n in ("neither_mode", "both_modes", "unknown_option", "help"))
    assert sum(len(c["stdin"]) + len(c["stdout"]) for c in by.values()) < 100000


def test_model_galaxy_pairs():
    for mode, src, want in galaxy_pairs():
        assert M.change_whole(src, mode)[:3] == (want, 0, None)


def test_block_model_agrees_with_the_whole_model():
    """a regular block's text is a whole input: both forms of the model give the same bytes, counts and stopping place"""
    checked = 0
    for name, records, mode in BLOCKS:
        blk = M.Block(records, mode)
        if blk.irregular or b"\r" in blk.text.replace(b"\r\n", b"\n"):
            continue
        out, status, msg, rin, _, changed = M.change_whole(blk.text, mode)
        assert out == blk.out, name
        if blk.first_to == M.NONE:
            assert (status, changed) == (0, blk.changed), name
        else:
            assert (status, msg) == (1, M.offender_message(mode, blk.lpr * (blk.first_to + 1))), name
        checked += 1
    assert checked > 150


@pytest.fixture(scope="module")
def reference_exe(tmp_path_factory):
    if not os.path.exists(REF_SRC):
        pytest.skip("the reference sources exist in the build container only")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "nuc_changer"))
    import make_nuc_changer_golden as G
    return G.build(REF, str(tmp_path_factory.mktemp("ref_nuc_changer")))


def _random_input(rng, k, mode):
    frm, to, _ = M.MODES[mode]
    fastq = k % 3 == 1
    recs = []
    for i in range(rng.randint(1, 25)):
        alphabet = b"ACGN" + bytes([frm]) * 2 + (bytes([to]) if k % 9 == 4 and rng.random() < 0.2 else b"")
        bases = bytes(rng.choice(alphabet) for _ in range(rng.choice([1, 2, 16, 17, 33, rng.randint(1, 90)])))
        name = rng.choice([b"%d" % i, b"%d-%d" % (i, rng.randint(0, 40)), b"T U-x", b""])
        recs.append((name, bases, b"TU"[: i % 3], bytes(rng.randint(33, 73) for _ in bases)) if fastq else (name, bases))
    eol = b"\r\n" if k % 11 == 3 else b"\n"
    text = M.block_text(recs).replace(b"\n", eol)
    if k % 7 == 2:
        text = text[:-len(eol)]                              # no final newline
    if k % 13 == 5:                                          # something the reader refuses, somewhere
        lines = text.split(b"\n")
        at = rng.randrange(len(lines))
        lines[at] = rng.choice([b"", b"acgt", lines[at] + b"x", b">" + lines[at], b"@" + lines[at]])
        text = b"\n".join(lines)
    return text


def test_model_matches_reference_on_random_inputs(reference_exe):
    rng = random.Random(2026)
    for k in range(300):
        mode = "rd"[k % 2]
        text = _random_input(rng, k, mode)
        p = subprocess.run([reference_exe, "-v", "-" + mode], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        out, status, msg, rin, rout, changed = M.change_whole(text, mode)
        assert (p.returncode, p.stdout) == (status, out), (k, text[:200], p.stderr)
        if status == 0:
            assert p.stderr == M.report(mode, rin, rout, changed), k
        elif msg.startswith("Error: found"):
            assert message_of(p.stderr.decode("latin-1")) == msg, k


# ---- the kernel's body through the CPU emulator -----------------------------------------------------------------------------------------
class Info(C.Structure):
    _fields_ = [("changed", C.c_uint64), ("first_to_record", C.c_uint64), ("irregular", C.c_uint32)]


def _obj(src, out, flags=()):
    deps = [src, os.path.join(ROOT, "include", "fxg.h"), os.path.join(EMU_DIR, "fxg_stub_ctx.h"), os.path.join(EMU_DIR, "nucchange_emu.cpp")] + \
           [os.path.join(CSRC, f) for f in ("fxg_nucchange.h", "fxg_device.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(emu_py._CXX + list(flags) + ["-c", src, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


@pytest.fixture(scope="module")
def ncdir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("nucchange"))
    emu = _obj(os.path.join(EMU_DIR, "nucchange_emu.cpp"), os.path.join(d, "nucchange_emu.o"))
    subprocess.check_call(emu_py._LINK + [emu, "-o", os.path.join(d, "libnucchange_emu.so")])
    return d


def _load(ncdir):
    L = C.CDLL(os.path.join(ncdir, "libnucchange_emu.so"))
    L.fxg_emu_bases_change.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(Info), C.c_char_p, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def ncemu(ncdir):
    return _load(ncdir)


SENTINEL = 0x5A


class Indexed:
    """a block as fxg_fastq_index leaves it: the text plus 16 sentinel bytes and no more (with a guard: up against a PROT_NONE page, or
    starting behind one), lines_per_record * records + 1 line starts and as many chomped ends.  shift moves the text off the 16-byte boundary;
    against the page behind it the text starts wherever its length puts it."""

    def __init__(self, records, guard=None, shift=0):
        text = M.block_text(records)
        self.lpr = 4 if records and len(records[0]) == 4 else 2
        self.n, self.text_len, self.cap_lines = len(records), len(text), self.lpr * len(records) + 1
        if guard == "after":                             # the last of the 16 bytes is the byte before the PROT_NONE page
            span = (len(text) + 16 + 15) // 16 * 16
            self.d_text = emu_py._guarded(span, np.uint8, "after")[span - (len(text) + 16):]
        elif guard == "before":                          # the first byte of the text is the byte behind it
            self.d_text = emu_py._guarded(len(text) + 16, np.uint8, "before")[:len(text) + 16]
        else:
            self.d_text = emu_py._aligned(len(text) + 16 + shift)[shift:]
        self.d_text[:len(text)] = np.frombuffer(text, dtype=np.uint8)
        self.d_text[len(text):] = SENTINEL
        raw = np.frombuffer(text, dtype=np.uint8)
        nl = np.flatnonzero(raw == 10)
        starts = np.zeros(self.cap_lines, dtype=np.int64)
        starts[1:] = nl + 1
        ends = nl.copy()
        for j in np.flatnonzero(raw == 13):              # chomp: a line ends at its first CR
            i = int(np.searchsorted(nl, j))
            ends[i] = min(ends[i], j)
        self.d_line = emu_py._alloc(2 * self.cap_lines, np.uint32, guard)
        self.d_line[:self.cap_lines] = starts
        self.d_line[self.cap_lines:2 * self.cap_lines - 1] = ends


def emu_call(L, ix, mode, records=None, lpr=None, frm=None, to=None, text=True, line=True):
    f, t, _ = M.MODES[mode]
    info, err = Info(), C.create_string_buffer(300)
    rc = L.fxg_emu_bases_change(ix.d_text.ctypes.data if text else None, ix.text_len, ix.lpr if lpr is None else lpr, ix.d_line.ctypes.data if line else None, ix.cap_lines,
                                ix.n if records is None else records, f if frm is None else frm, t if to is None else to, C.byref(info), err, 300)
    return rc, info, err.value.decode()


def _check_block(L, name, records, mode, guard=None, shift=0):
    blk = M.Block(records, mode)
    ix = Indexed(records, guard, shift)
    rc, info, msg = emu_call(L, ix, mode)
    assert rc == 0, (name, msg)
    assert bytes(ix.d_text[:ix.text_len]) == blk.rewritten, name
    assert (ix.d_text[ix.text_len:] == SENTINEL).all(), name
    assert (info.first_to_record, info.irregular) == (blk.first_to, blk.irregular), name
    if blk.first_to == M.NONE:
        assert info.changed == blk.changed, name
    return blk, ix


@pytest.mark.parametrize("name,records,mode", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_emulated_kernel_blocks(ncemu, name, records, mode):
    _check_block(ncemu, name, records, mode, shift=len(name) % 16 if "idlen" not in name else 0)


def test_case_list_covers_every_start_offset_and_a_shared_piece():
    """what the case names promise: bases lines starting at every offset modulo 16, and aligned 16-byte pieces that hold bases of three records"""
    offsets, most = set(), 0
    for name, records, mode in BLOCKS:
        if name.startswith(("idlen_", "shared_")):
            text = M.block_text(records)
            starts = [0] + [i + 1 for i, c in enumerate(text) if c == 10]
            lpr = 4 if len(records[0]) == 4 else 2
            owners = {}
            for r in range(len(records)):
                s = starts[lpr * r + 1]
                offsets.add(s % 16)
                for p in range(s, s + len(M.chomp(records[r][1]))):
                    owners.setdefault(p // 16, set()).add(r)
            most = max(most, max(len(v) for v in owners.values()))
    assert offsets == set(range(16)) and most >= 3


def test_emulated_output_through_the_formatter(ncemu):
    """index, change, format with out_fasta = 1 over the emulated engine: the block's output as the model writes it, cut before the first offender"""
    for name, records, mode in BLOCKS:
        if not any(k in name for k in ("len_33_", "len_150_", "to_", "crlf", "full_of", "collapsed", "records_65_", "shared_mixed")):
            continue
        blk = M.Block(records, mode)
        ix = emu_py.fastq_index(blk.text, lpr=blk.lpr, cap_records=blk.n)
        assert ix["info"].records == blk.n and not ix["info"].irregular, name
        view = types.SimpleNamespace(d_text=ix["text"], d_line=ix["line"], text_len=ix["text_len"], lpr=blk.lpr, cap_lines=ix["cap_lines"], n=blk.n)
        rc, info, msg = emu_call(ncemu, view, mode)
        assert rc == 0 and info.first_to_record == blk.first_to, (name, msg)
        assert bytes(ix["text"][:ix["text_len"]]) == blk.rewritten, name
        n = blk.records_out
        if n:
            res = (1 << 16) | ix["lens"][:n].astype(np.uint32)
            assert emu_py.fastq_format(ix, n, res, out_fasta=True) == blk.out, name


def test_emulated_refusals_and_the_empty_call(ncemu):
    name, records, mode = next(b for b in BLOCKS if b[0] == "len_33_fasta_r")
    ix = Indexed(records)
    before = bytes(ix.d_text)
    for kw, frag in ((dict(frm=ord("T"), to=ord("T")), "'T' to 'U'"), (dict(frm=ord("A"), to=ord("U")), "'T' to 'U'"), (dict(frm=ord("u"), to=ord("t")), "'T' to 'U'"),
                     (dict(lpr=3), "lines_per_record 3"), (dict(lpr=0), "lines_per_record 0"), (dict(text=False), "null pointer"), (dict(line=False), "null pointer"),
                     (dict(records=ix.n + 1), "need more than"), (dict(records=ix.text_len), "more than")):
        rc, info, msg = emu_call(ncemu, ix, mode, **kw)
        assert rc == -1 and frag in msg, (kw, msg)
        assert (info.changed, info.first_to_record, info.irregular) == (0, M.NONE, 0) and bytes(ix.d_text) == before, kw
    for kw in (dict(records=0), dict(records=0, text=False, line=False)):
        rc, info, msg = emu_call(ncemu, ix, mode, **kw)
        assert rc == 0 and (info.changed, info.first_to_record, info.irregular) == (0, M.NONE, 0) and bytes(ix.d_text) == before, kw


def _guard_child(where, ncdir):
    try:
        L = _load(ncdir)
        for name, records, mode in BLOCKS:
            if "24997" in name and "fastq" in name:
                continue
            _check_block(L, name, records, mode, guard=where)
        os._exit(0)
    except AssertionError:
        os._exit(3)
    except BaseException:
        os._exit(4)


@pytest.mark.parametrize("where", ["after", "before"])
def test_emulated_kernel_within_bounds(ncdir, where):
    """the text at exactly text_len + 16 bytes against a PROT_NONE page (behind it, or in front of it): a byte touched outside is a SIGSEGV of the child"""
    import multiprocessing as mp
    p = mp.get_context("fork").Process(target=_guard_child, args=(where, ncdir))
    p.start()
    p.join(600)
    assert p.exitcode == 0, "child exit %s (-11: an access outside the text's contract, 3: a wrong result)" % p.exitcode


# ---- the tool over the stubs ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stock_stub():
    from fastx_toolkit_amd import build as b
    d = emu_py.build_stub()
    b.build_engine()
    b.build_host()
    return d


@pytest.fixture(scope="module")
def nucchange_stub(ncdir, stock_stub):
    """a libfxg.so of the stub's own objects plus fxg_bases_change (nucchange_stub.cpp over nucchange_emu.cpp)"""
    so = _obj(os.path.join(EMU_DIR, "nucchange_stub.cpp"), os.path.join(ncdir, "nucchange_stub.o"))
    d = os.path.join(ncdir, "stub")
    os.makedirs(d, exist_ok=True)
    subprocess.check_call(emu_py._LINK + [os.path.join(stock_stub, "fxg_stub.o"), so, os.path.join(ncdir, "nucchange_emu.o")] + emu_py._emu_objects([]) +
                          ["-o", os.path.join(d, "libfxg.so"), "-ldl"])
    return d


ONE_MB = {"FXH_READ_BUFFER_MB": "1"}


def _tool_on_everything(lib):
    for case in golden_cases():
        assert_tool_case(lib, case, ONE_MB)
    for mode, src, want in galaxy_pairs():
        assert run_tool(lib, ["-" + mode], src)[:2] == (0, want)
        code, out, err, outfile = run_tool(lib, ["-v", "-" + mode], src, files=True)
        assert (code, outfile, err) == (0, want, ""), mode
        assert out == M.report(mode, *M.change_whole(src, mode)[3:])


def test_tool_on_recorded_cases_device_path(nucchange_stub):
    _tool_on_everything(nucchange_stub)


def test_tool_on_recorded_cases_record_path(stock_stub):
    """the stock stub has no fxg_bases_change: every input goes through the record loop, and gives the same bytes"""
    _tool_on_everything(stock_stub)


def test_tool_takes_the_device_path_over_the_stub_with_the_entry(nucchange_stub, stock_stub):
    """the two stubs differ in the one symbol, so the two tool tests above run two paths"""
    has = C.CDLL(os.path.join(nucchange_stub, "libfxg.so"))
    lacks = C.CDLL(os.path.join(stock_stub, "libfxg.so"))
    assert hasattr(has, "fxg_bases_change") and not hasattr(lacks, "fxg_bases_change")


@pytest.fixture(scope="module")
def two_mb():
    return {(mode, fmt): regular_text(2 << 20, mode, fmt) for mode in "rd" for fmt in ("fasta", "fastq")}


def test_tool_many_blocks(nucchange_stub, stock_stub, two_mb):
    """2 MB in 1 MB blocks, FASTA and FASTQ, both modes: the device path and the record path equal the model, report included; -z gives a gzip stream of the same bytes"""
    for (mode, fmt), text in two_mb.items():
        want, status, _, rin, rout, changed = M.change_whole(text, mode)
        assert status == 0 and changed > 100000
        for lib, files in ((nucchange_stub, False), (nucchange_stub, True), (stock_stub, True)):
            code, out, err, outfile = run_tool(lib, ["-v", "-" + mode], text, ONE_MB, files=files)
            assert code == 0, err
            assert (outfile if files else out) == want, (mode, fmt, lib, files)
            assert (out if files else err.encode()) == M.report(mode, rin, rout, changed)
    text = two_mb[("r", "fasta")]
    code, out, err, _ = run_tool(nucchange_stub, ["-r", "-z"], text, ONE_MB)
    assert code == 0 and gzip.decompress(out) == M.change_whole(text, "r")[0]


def test_tool_offender_in_a_later_block(nucchange_stub, stock_stub, two_mb):
    """an offender in the second (and in the third) block: everything before it is written, the message carries the line number of the whole input"""
    for (mode, fmt), text in two_mb.items():
        to = bytes([M.MODES[mode][1]])
        for at in (len(text) * 3 // 5, len(text) - 200):
            cut = text.rfind(b"\n>" if fmt == "fasta" else b"\n@", 0, at) + 1
            tail = (b">bad\nAC" + to + b"G\n>after\nAC\n") if fmt == "fasta" else (b"@bad\nAC" + to + b"G\n+\nIIII\n@after\nAC\n+\nII\n")
            bad = text[:cut] + tail + text[cut:]
            want, status, msg, _, _, _ = M.change_whole(bad, mode)
            assert status == 1 and want == M.change_whole(text[:cut], mode)[0]
            assert msg == M.offender_message(mode, text[:cut].count(b"\n") + (2 if fmt == "fasta" else 4))
            for lib in (nucchange_stub, stock_stub):
                code, out, err, _ = run_tool(lib, ["-v", "-" + mode], bad, ONE_MB)
                assert (code, out) == (1, want), (mode, fmt, at)
                assert message_of(err) == msg and err.count("\n") == 1


def test_tool_offender_with_gzip_output(nucchange_stub, two_mb):
    text = two_mb[("r", "fasta")]
    cut = text.rfind(b"\n>", 0, len(text) * 3 // 4) + 1
    bad = text[:cut] + b">bad\nUU\n" + text[cut:]
    code, out, err, _ = run_tool(nucchange_stub, ["-r", "-z"], bad, ONE_MB)
    assert code == 1 and gzip.decompress(out) == M.change_whole(text[:cut], "r")[0]
    assert message_of(err) == M.offender_message("r", text[:cut].count(b"\n") + 2)


def test_tool_leaves_the_device_path_at_an_irregular_block(nucchange_stub, two_mb):
    """a lower-case record in the third block: the blocks before it go through the device path, the record API takes over with the change count,
    the tallies and the line number carried over, writes what precedes the bad record and owns the message; an irregular block followed by
    regular records ends well, with the whole input's report"""
    text = two_mb[("r", "fasta")]
    cut = text.rfind(b"\n>", 0, len(text) - 1000) + 1
    head = text[:cut]
    want, status, _, _, _, _ = M.change_whole(head, "r")
    code, out, err, _ = run_tool(nucchange_stub, ["-r"], head + b">x-3\nacgt\n>y-2\nAC\n", ONE_MB)
    assert code == 1 and out == want
    assert "found invalid nucleotide sequence (acgt) on line %d" % (head.count(b"\n") + 2) in err
    # a read of 24 998 bases is one more than fxg_fastq_index takes and one the record API still reads: its block ends the device path, and the
    # input ends well, with the whole input's report
    long_read = b">long-5\n" + (b"ACGTT" * 5000)[:24998] + b"\n"
    whole = head + long_read + text[cut:]
    want, status, _, rin, rout, changed = M.change_whole(whole, "r")
    assert status == 0
    code, out, err, _ = run_tool(nucchange_stub, ["-r", "-v"], whole, ONE_MB)
    assert (code, out) == (0, want), err
    assert err.encode() == M.report("r", rin, rout, changed)
    # ... and an offender behind the hand-over still gets the whole input's line number
    bad = whole + b">late\nACGU\n"
    code, out, err, _ = run_tool(nucchange_stub, ["-r"], bad, ONE_MB)
    assert (code, out) == (1, want) and message_of(err) == M.offender_message("r", bad.count(b"\n"))


# ---- the reference's own tool source against host/fastx.h --------------------------------------------------------------------------------
def test_reference_tool_source_compiles_unchanged_and_reproduces_its_galaxy_pairs(stock_stub, tmp_path):
    if not os.path.exists(REF_SRC):
        pytest.skip("the reference sources exist in the build container only")
    (tmp_path / "config.h").write_text("")                    # (PACKAGE_STRING is all the tool takes from it)
    exe = str(tmp_path / "fasta_nucleotide_changer")
    cmd = ["gcc", "-O1", "-std=gnu11", "-DPACKAGE_STRING=\"FASTX Toolkit 0.0.14\"", "-I", str(tmp_path), "-I", HOST, REF_SRC, os.path.join(HOST, "bin", "libfastx_amd.a"),
           "-L", os.path.join(ROOT, "fastx_toolkit_amd"), "-lfxg", "-lpthread", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "fastx_toolkit_amd"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, "the reference's fasta_nucleotide_changer.c no longer compiles against host/fastx.h + fastx_args.h:\n%s" % p.stdout[-3000:]
    for mode, src, want in galaxy_pairs():
        (tmp_path / "in.fa").write_bytes(src)
        r = subprocess.run([exe, "-" + mode, "-i", str(tmp_path / "in.fa"), "-o", str(tmp_path / "out.fa")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 0, r.stderr[-500:]
        assert (tmp_path / "out.fa").read_bytes() == want, mode


# ---- stand-alone programs under the sanitizers -----------------------------------------------------------------------------------------
REPORT = (b"ERROR: AddressSanitizer", b"runtime error:", b"ERROR: LeakSanitizer", b"SUMMARY: UndefinedBehaviorSanitizer")


@pytest.mark.sanitizers
def test_emulator_and_record_path_under_sanitizers(tmp_path, stock_stub):
    """two programs with a main of their own, built with -fsanitize=address,undefined and run directly, nothing preloaded: the emulated kernel
    over one block (nucchange_san_main.cpp), and the tool on its record path (the instrumented host build over the stock stub)"""
    exe = str(tmp_path / "nucchange_san_main")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wno-pass-failed", "-DFXG_HOST_EMULATION",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(EMU_DIR, "nucchange_san_main.cpp"), "-o", exe])
    subprocess.check_call(["make", "-s", "-C", HOST, "SAN=address,undefined"])
    tool = os.path.join(HOST, "bin_san_address_undefined", "fasta_nucleotide_changer")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    for case in golden_cases():             # the record path: every recorded input through the instrumented tool
        if "-o" in case["argv"]:
            continue
        p = subprocess.run([tool] + case["argv"], input=case["stdin"].encode("latin-1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                           env=dict(env, LD_LIBRARY_PATH=stock_stub))
        assert not any(m in p.stderr for m in REPORT) and p.returncode != 99, (case["name"], p.stderr[-1500:])
        assert p.returncode == case["exit"], case["name"]
        if case["stdout"] != M.USAGE:
            assert p.stdout == case["stdout"].encode("latin-1"), case["name"]
    src = tmp_path / "block.fx"
    checked = 0
    for name, records, mode in BLOCKS:      # the emulator: the block the device would get
        if "records_32" in name or "records_65" in name or "second_trip" in name or ("24997" in name and "fastq" in name):
            continue
        blk = M.Block(records, mode)
        src.write_bytes(blk.text)
        p = subprocess.run([exe, str(src), mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        assert not any(m in p.stderr for m in REPORT) and p.returncode != 99, (name, p.stderr[-1500:])
        rc, changed, first, irr = (int(x) for x in p.stderr.split()[:4])
        assert (p.returncode, rc, first, irr, p.stdout) == (0, 0, blk.first_to, blk.irregular, blk.rewritten), name
        if blk.first_to == M.NONE:
            assert changed == blk.changed, name
        checked += 1
    assert checked > 190
