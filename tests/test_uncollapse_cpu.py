"""fastx_uncollapser, CPU tier: the Python model (uncollapse_model.py) against the recorded answers of the reference and, where the reference
tree is present, against the reference itself on seeded random inputs; the kernels' bodies through the CPU emulator
(tests/emu/uncollapse_emu.cpp) against the block model, with every array against a guard page; the tool over a stub variant that has the
entry (its device path) and over the stock stub (its record path); and the emulator and the record path as stand-alone programs under
ASan + UBSan."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import emu_py
import uncollapse_model as M
from uncollapse_cases import (ROOT, TEXT_MAX, abi_blocks, assert_tool_case, collapsed_text, galaxy_pair, golden_cases, ordinal_blocks, rec, run_tool,
                              two_level_block, window_block)

REF = os.environ.get("FXG_REFERENCE", "/root/reference")
REF_SRC = os.path.join(REF, "src", "fastx_uncollapser", "fastx_uncollapser.cpp")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fastx_toolkit_amd", "csrc")
HOST = os.path.join(ROOT, "fastx_toolkit_amd", "host")


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _model_answer(case):
    argv = [a for a in case["argv"] if a not in ("-o", "OUT")]
    return M.run_argv(argv, case["stdin"].encode("latin-1"))


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_model_matches_recorded(case):
    out, report, status = _model_answer(case)
    assert status == case["exit"]
    if out == M.USAGE:
        assert case["stdout"] == M.USAGE
        return
    to_file = "-o" in case["argv"]
    assert out == (case["outfile"] if to_file else case["stdout"]).encode("latin-1")
    if status == 0:                         # the report goes to stdout once -o is given, to stderr otherwise
        assert (report or b"") == (case["stdout"] if to_file else case["stderr"]).encode("latin-1")


def test_recorded_cases_hold_the_contract_corners():
    by = {c["name"]: c for c in golden_cases()}
    assert len(by) >= 40
    assert by["ids_of_the_issue"]["stdout"] == ">1\nAC\n>2\nAC\n>3\nA\n>4\nN\n>5\nN\n>6\nN\n>7\nAC\n>8\nAC\n>9\nA\n>10\nT\n"
    assert by["ids_of_the_issue_v"]["stderr"] == "Input: 6 sequences (representing 10 reads)\nOutput: 10 sequences (representing 10 reads)\n"
    assert by["plain_v_o"]["stdout"].startswith("Input: 3 sequences (representing 6 reads)") and by["plain_v_o"]["outfile"] == by["plain"]["stdout"]
    assert by["crlf"]["stdout"] == ">1\nACGT\n>2\nACGT\n>3\nGG\n" and by["no_final_newline"]["stdout"].endswith(">5\nGG\n")
    assert [by[n]["exit"] for n in ("error_fastq_input", "error_lower_case", "error_empty_bases", "help", "unknown_option")] == [1] * 5
    assert by["error_lower_case"]["stdout"] == ">1\nACGT\n>2\nACGT\n"          # what came before the bad record is written
    assert sum(len(c["stdin"]) + len(c["stdout"]) for c in by.values()) < 100000


def test_model_galaxy_pair():
    src, want = galaxy_pair()
    assert M.uncollapse_whole(src)[:2] == (want, 0)


def test_block_model_windows_chain_to_the_whole_model():
    records, base = window_block()
    blk = M.Block(records, base)
    whole = M.uncollapse_whole(M.block_text(records))[0]
    assert blk.whole() == whole and 250 < blk.copies < 400
    for cap in (19, 20, 57, 200, 10 ** 6):
        got, g = b"", 0
        while g < blk.copies:
            g2, out = blk.window(g, cap)
            assert g2 > g and len(out) <= cap
            got, g = got + out, g2
        assert got == whole
    assert blk.window(blk.copies, 0) == (blk.copies, b"") and blk.window(0, 3) is None and blk.window(blk.copies + 1, 100) is None


@pytest.fixture(scope="module")
def reference_exe(tmp_path_factory):
    if not os.path.exists(REF_SRC):
        pytest.skip("the reference sources exist in the build container only")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "uncollapse"))
    import make_uncollapse_golden as G
    return G.build(REF, str(tmp_path_factory.mktemp("ref_uncollapser")))


def _random_input(rng, k):
    recs = []
    for i in range(rng.randint(1, 30)):
        shape = rng.random()
        if shape < 0.5:
            name = b"%d-%d" % (i, rng.choice([1, 1, 1, 2, 3, 16, 17, rng.randint(1, 300)]))
        elif shape < 0.7:
            name = bytes(rng.choice(b"ab1 -+\t_9") for _ in range(rng.randint(0, 12)))
        else:
            name = bytes(rng.choice(b"xyz-") for _ in range(rng.randint(0, 4))) + b"-" + bytes(rng.choice(b"0123456789 +-x") for _ in range(rng.randint(0, 3)))
        recs.append((name, bytes(rng.choice(b"ACGTN") for _ in range(rng.choice([1, 2, 16, 30, rng.randint(1, 80)])))))
    eol = b"\r\n" if k % 11 == 3 else b"\n"
    text = b"".join(b">" + n + eol + b + eol for n, b in recs)
    if k % 7 == 2:
        text = text[:-len(eol)]                              # no final newline
    if k % 13 == 5:                                          # something the reader refuses, somewhere
        lines = text.split(b"\n")
        at = rng.randrange(len(lines))
        lines[at] = rng.choice([b"", b"acgt", lines[at] + b"x", b"@" + lines[at]])
        text = b"\n".join(lines)
    return text


def test_model_matches_reference_on_random_inputs(reference_exe):
    rng = random.Random(2025)
    for k in range(300):
        text = _random_input(rng, k)
        p = subprocess.run([reference_exe, "-v"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        out, status, seqs, reads = M.uncollapse_whole(text)
        assert (p.returncode, p.stdout) == (status, out), (k, text[:200])
        if status == 0:
            assert p.stderr == M.report(seqs, reads), k


# ---- the kernels' bodies through the CPU emulator ---------------------------------------------------------------------------------------
class Opts(C.Structure):
    _fields_ = [("ordinal_base", C.c_uint64), ("copy_begin", C.c_uint64), ("out_cap", C.c_uint64)]


class Info(C.Structure):
    _fields_ = [("copies", C.c_uint64), ("copy_end", C.c_uint64), ("out_bytes", C.c_uint64)]


def _obj(src, out, flags=()):
    deps = [src, os.path.join(ROOT, "include", "fxg.h"), os.path.join(EMU_DIR, "fxg_stub_ctx.h"), os.path.join(EMU_DIR, "uncollapse_emu.cpp")] + \
           [os.path.join(CSRC, f) for f in ("fxg_uncollapse.h", "fxg_text.h", "fxg_barcode.h", "fxg_device.h", "fxg_kernels.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(emu_py._CXX + list(flags) + ["-c", src, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


@pytest.fixture(scope="module")
def ucdir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("uncollapse"))
    emu = _obj(os.path.join(EMU_DIR, "uncollapse_emu.cpp"), os.path.join(d, "uncollapse_emu.o"))
    subprocess.check_call(emu_py._LINK + [emu, "-o", os.path.join(d, "libuncollapse_emu.so")])
    return d


def _load(ucdir):
    L = C.CDLL(os.path.join(ucdir, "libuncollapse_emu.so"))
    L.fxg_emu_fasta_uncollapse.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(Opts), C.c_void_p, C.POINTER(Info),
                                           C.c_char_p, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def ucemu(ucdir):
    return _load(ucdir)


@pytest.fixture(scope="module")
def ucemu_side(tmp_path_factory):
    """the emulator built with the copy kernels' other lane mapping (csrc/fxg_uncollapse.h: FXG_UC_SIDE_BY_SIDE), which the product does not ship"""
    d = str(tmp_path_factory.mktemp("uncollapse_side"))
    emu = _obj(os.path.join(EMU_DIR, "uncollapse_emu.cpp"), os.path.join(d, "uncollapse_emu.o"), ["-DFXG_UC_SIDE_BY_SIDE=1"])
    subprocess.check_call(emu_py._LINK + [emu, "-o", os.path.join(d, "libuncollapse_emu.so")])
    return _load(d)


class Indexed:
    """a block of records as fxg_fastq_index leaves it, every array at its contracted size (include/fxg.h): the text plus its 16 bytes of slack,
    2 * records + 1 line starts and as many chomped ends, records lengths"""

    def __init__(self, records, guard=None):
        text = M.block_text(records)
        self.n, self.text_len, self.cap_lines = len(records), len(text), 2 * len(records) + 1
        self.d_text = emu_py._alloc(len(text) + 16, np.uint8, guard)
        self.d_text[:len(text)] = np.frombuffer(text, dtype=np.uint8)
        starts = np.zeros(self.cap_lines, dtype=np.int64)
        nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
        starts[1:] = nl + 1
        ends = nl.copy()
        for j in np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 13):      # chomp: a line ends at its first CR
            i = int(np.searchsorted(nl, j))
            ends[i] = min(ends[i], j)
        self.d_line = emu_py._alloc(2 * self.cap_lines, np.uint32, guard)
        self.d_line[:self.cap_lines] = starts
        self.d_line[self.cap_lines:2 * self.cap_lines - 1] = ends
        self.d_len = emu_py._alloc(max(self.n, 1), np.uint16, guard)
        self.d_len[:self.n] = np.minimum(ends[1::2] - starts[1:-1:2], 65535)


def emu_call(L, ix, base, copy_begin, out_cap, guard=None, text_len=None):
    """one emulated call with d_out of exactly out_cap bytes.  Returns (rc, bytes written, info, message)."""
    d_out = emu_py._tight(np.full(out_cap, 0xEE, dtype=np.uint8), guard) if guard else np.full(out_cap, 0xEE, dtype=np.uint8)
    o, info, err = Opts(base, copy_begin, out_cap), Info(), C.create_string_buffer(300)
    rc = L.fxg_emu_fasta_uncollapse(ix.d_text.ctypes.data, ix.text_len if text_len is None else text_len, ix.d_line.ctypes.data, ix.cap_lines, ix.n, ix.d_len.ctypes.data,
                                    C.byref(o), d_out.ctypes.data if out_cap else None, C.byref(info), err, 300)
    assert rc != 0 or (d_out[info.out_bytes:] == 0xEE).all()
    assert rc == 0 or (d_out == 0xEE).all(), "a refused call wrote to d_out"
    return rc, bytes(d_out[:info.out_bytes]), info, err.value.decode()


def _check_whole(L, records, base, guard=None, tag=None):
    """the block in one call into exactly its bytes, then once more in windows of a third of them"""
    blk = M.Block(records, base)
    want = blk.whole()
    ix = Indexed(records, guard)
    rc, out, info, msg = emu_call(L, ix, base, 0, len(want), guard)
    assert rc == 0, (tag, msg)
    assert (info.copies, info.copy_end, info.out_bytes) == (blk.copies, blk.copies, len(want)), tag
    assert out == want, tag
    cap = max(len(want) // 3, max(len(b) for b in blk.bases) + 24)
    got, g = b"", 0
    while g < blk.copies:
        rc, out, info, msg = emu_call(L, ix, base, g, cap, guard)
        assert rc == 0 and info.copy_end > g, (tag, msg)
        got, g = got + out, info.copy_end
    assert got == want, tag


@pytest.mark.parametrize("name,records,base", abi_blocks(), ids=[b[0] for b in abi_blocks()])
def test_emulated_kernels_blocks(ucemu, name, records, base):
    _check_whole(ucemu, records, base, tag=name)


def test_emulated_kernels_two_scan_levels(ucemu):
    records, base = two_level_block()
    blk = M.Block(records, base)
    want = blk.whole()
    ix = Indexed(records)
    rc, out, info, msg = emu_call(ucemu, ix, base, 0, len(want))
    assert rc == 0 and info.copies == blk.copies and out == want, msg


@pytest.mark.parametrize("name,records,base", ordinal_blocks(), ids=[b[0] for b in ordinal_blocks()])
def test_emulated_kernels_ordinals(ucemu, name, records, base):
    _check_whole(ucemu, records, base, tag=name)


def test_emulated_windows_every_capacity(ucemu):
    """out_cap of exactly the largest copy, one byte more, and every size up to 200: copy_end and out_bytes as the model says, the windows
    concatenated equal the one-call output"""
    records, base = window_block()
    blk = M.Block(records, base)
    whole = blk.whole()
    ix = Indexed(records)
    largest = max(len(blk.copy_of(g)) for g in range(blk.copies))
    assert largest == 19
    for cap in range(largest, 201):
        got, g = b"", 0
        while g < blk.copies:
            rc, out, info, msg = emu_call(ucemu, ix, base, g, cap)
            assert rc == 0, msg
            assert (info.copy_end, out) == blk.window(g, cap), (cap, g)
            got, g = got + out, info.copy_end
        assert got == whole, cap


def test_emulated_side_by_side_mapping(ucemu_side):
    """the lane mapping kept for measurement gives the same bytes: every block, every ordinal block, windows of a few capacities"""
    for name, records, base in abi_blocks() + ordinal_blocks():
        _check_whole(ucemu_side, records, base, tag=name)
    records, base = window_block()
    blk, ix = M.Block(records, base), Indexed(records)
    for cap in (19, 20, 33, 64, 199):
        g = 0
        while g < blk.copies:
            rc, out, info, msg = emu_call(ucemu_side, ix, base, g, cap)
            assert rc == 0 and (info.copy_end, out) == blk.window(g, cap), (cap, g, msg)
            g = info.copy_end


def test_emulated_large_count(ucemu):
    """one record with count 2^31 - 1, written only through a window of a few copies at copy 2 000 000 000: its byte offset is above 2^35"""
    records = [rec(0, 3, 5), (b"big-2147483647", b"ACGTNACGTN"), rec(2, 2, 4)]
    blk = M.Block(records, 0)
    assert blk.copies == 3 + 2147483647 + 2
    ix = Indexed(records)
    for g0, cap in ((2000000000, 100), (0, 200), (blk.copies - 4, 1000), (3 + 2147483647 - 1, 50)):
        rc, out, info, msg = emu_call(ucemu, ix, 0, g0, cap)
        assert rc == 0, msg
        assert (info.copies, info.copy_end, out) == (blk.copies,) + blk.window(g0, cap), g0


def test_emulated_refusals(ucemu):
    records, base = window_block()
    blk = M.Block(records, base)
    ix = Indexed(records)
    first = len(blk.copy_of(0))
    rc, _, _, msg = emu_call(ucemu, ix, base, 0, first - 1)
    assert rc == -1 and "needs %d bytes" % first in msg and "takes %d" % (first - 1) in msg
    rc, out, info, _ = emu_call(ucemu, ix, base, 0, first)
    assert rc == 0 and (info.copy_end, out) == (1, blk.copy_of(0))
    rc, _, _, msg = emu_call(ucemu, ix, base, blk.copies + 1, 100)
    assert rc == -1 and "copy_begin" in msg
    rc, _, _, msg = emu_call(ucemu, ix, (1 << 64) - blk.copies, 0, 100)
    assert rc == -1 and "2^64" in msg
    rc, out, info, msg = emu_call(ucemu, ix, (1 << 64) - 1 - blk.copies, blk.copies - 1, 100)          # the last number is 2^64 - 1
    assert rc == 0 and out == b">18446744073709551615\n" + blk.bases[-1] + b"\n", msg
    rc, _, _, msg = emu_call(ucemu, ix, base, 0, 100, text_len=TEXT_MAX + 1)
    assert rc == -1 and "at most" in msg
    rc, out, info, _ = emu_call(ucemu, ix, base, blk.copies, 0)                                          # the empty call
    assert rc == 0 and (info.copies, info.copy_end, info.out_bytes, out) == (blk.copies, blk.copies, 0, b"")


def _guard_child(where, ucdir):
    try:
        L = _load(ucdir)
        for name, records, base in abi_blocks():
            if "65535" not in name:
                _check_whole(L, records, base, guard=where, tag=name)
        for name, records, base in ordinal_blocks()[::5]:
            _check_whole(L, records, base, guard=where, tag=name)
        records, base = window_block()
        blk, ix = M.Block(records, base), Indexed(records, where)
        for cap in (19, 20, 33, 64, 199):
            g = 0
            while g < blk.copies:
                rc, out, info, _ = emu_call(L, ix, base, g, cap, where)
                assert rc == 0 and (info.copy_end, out) == blk.window(g, cap)
                g = info.copy_end
        os._exit(0)
    except AssertionError:
        os._exit(3)
    except BaseException:
        os._exit(4)


@pytest.mark.parametrize("where", ["after", "before"])
def test_emulated_kernels_within_bounds(ucdir, where):
    """every array of the call at exactly its contracted size against a PROT_NONE page: a byte touched outside it is a SIGSEGV of the child"""
    import multiprocessing as mp
    p = mp.get_context("fork").Process(target=_guard_child, args=(where, ucdir))
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


@pytest.fixture(scope="module")
def uncollapse_stub(ucdir, stock_stub):
    """a libfxg.so of the stub's own objects plus fxg_fasta_uncollapse (uncollapse_stub.cpp over uncollapse_emu.cpp)"""
    so = _obj(os.path.join(EMU_DIR, "uncollapse_stub.cpp"), os.path.join(ucdir, "uncollapse_stub.o"))
    d = os.path.join(ucdir, "stub")
    os.makedirs(d, exist_ok=True)
    subprocess.check_call(emu_py._LINK + [os.path.join(stock_stub, "fxg_stub.o"), so, os.path.join(ucdir, "uncollapse_emu.o")] + emu_py._emu_objects([]) +
                          ["-o", os.path.join(d, "libfxg.so"), "-ldl"])
    return d


def _tool_on_everything(lib):
    for case in golden_cases():
        assert_tool_case(lib, case)
    src, want = galaxy_pair()
    assert run_tool(lib, [], src)[:2] == (0, want)
    code, out, err, outfile = run_tool(lib, ["-v"], src, files=True)
    assert (code, outfile, err) == (0, want, "") and out == M.report(12, 42)


def test_tool_on_recorded_cases_device_path(uncollapse_stub):
    _tool_on_everything(uncollapse_stub)


def test_tool_on_recorded_cases_record_path(stock_stub):
    """the stock stub has no fxg_fasta_uncollapse: every input goes through the record loop, and gives the same bytes"""
    _tool_on_everything(stock_stub)


def test_tool_answers_c_with_one_line(stock_stub):
    code, out, err, _ = run_tool(stock_stub, ["-c", "2"], b"a\t1-2\n")
    assert code == 1 and out == b"" and err.count("\n") == 1 and "not supported" in err


@pytest.fixture(scope="module")
def two_mb():
    return collapsed_text(2 << 20)


def test_tool_many_blocks(uncollapse_stub, stock_stub, two_mb):
    """2 MB of collapsed text in 1 MB blocks and 1 MB windows: the device path and the record path equal the model, report included"""
    want, status, seqs, reads = M.uncollapse_whole(two_mb)
    assert status == 0 and len(want) > 8 << 20
    env = {"FXH_READ_BUFFER_MB": "1"}
    for lib, files in ((uncollapse_stub, False), (uncollapse_stub, True), (stock_stub, True)):
        code, out, err, outfile = run_tool(lib, ["-v"], two_mb, env, files=files)
        assert code == 0, err
        assert (outfile if files else out) == want, (lib, files)
        assert (out if files else err.encode()) == M.report(seqs, reads)


def test_tool_leaves_the_device_path_at_a_bad_block(uncollapse_stub, two_mb):
    """a lower-case record in the third block: the blocks before it go through the device path, the record API takes over with the right
    running number and line number, writes what precedes the bad record and owns the message"""
    cut = two_mb.rfind(b"\n>", 0, len(two_mb) - 1000) + 1
    head, tail = two_mb[:cut], b">x-3\nacgt\n>y-2\nAC\n"
    want, status, _, _ = M.uncollapse_whole(head + tail)
    assert status == 1
    code, out, err, _ = run_tool(uncollapse_stub, [], head + tail, {"FXH_READ_BUFFER_MB": "1"})
    assert code == 1 and out == want
    assert "found invalid nucleotide sequence (acgt) on line %d" % (head.count(b"\n") + 2) in err
    code, out, err, _ = run_tool(uncollapse_stub, ["-v"], head + b">x-3\nAC\r\n>y\nNN", {"FXH_READ_BUFFER_MB": "1"})      # CRLF and no final newline stay on the device
    assert code == 0 and out == M.uncollapse_whole(head + b">x-3\nAC\n>y\nNN\n")[0]


# ---- stand-alone programs under the sanitizers -----------------------------------------------------------------------------------------
REPORT = (b"ERROR: AddressSanitizer", b"runtime error:", b"ERROR: LeakSanitizer", b"SUMMARY: UndefinedBehaviorSanitizer")


@pytest.mark.sanitizers
def test_emulator_and_record_path_under_sanitizers(tmp_path, stock_stub):
    """two programs with a main of their own, built with -fsanitize=address,undefined and run directly, nothing preloaded: the emulated kernels
    over one block, window by window (uncollapse_san_main.cpp), and the tool on its record path (the instrumented host build over the stock stub)"""
    exe = str(tmp_path / "uncollapse_san_main")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wno-pass-failed", "-DFXG_HOST_EMULATION",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(EMU_DIR, "uncollapse_san_main.cpp"), "-o", exe])
    subprocess.check_call(["make", "-s", "-C", HOST, "SAN=address,undefined"])
    tool = os.path.join(HOST, "bin_san_address_undefined", "fastx_uncollapser")
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
    src = tmp_path / "block.fa"
    checked = 0
    blocks = [b for b in abi_blocks() if "65535" not in b[0] and "records_1" not in b[0]] + ordinal_blocks()[::3] + [("windows",) + window_block()]
    for name, records, base in blocks:      # the emulator: the block the device would get, in windows of three sizes
        blk = M.Block(records, base)
        want = blk.whole()
        src.write_bytes(M.block_text(records))
        largest = max(len(b) for b in blk.bases) + 24
        for cap in (largest, largest + 37, len(want) + 5):
            p = subprocess.run([exe, str(src), str(base), str(cap)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
            assert not any(m in p.stderr for m in REPORT) and p.returncode != 99, (name, p.stderr[-1500:])
            rc, copies = p.stderr.split()[:2]
            assert (p.returncode, int(rc), int(copies), p.stdout) == (0, 0, blk.copies, want), (name, cap)
            checked += 1
    assert checked > 100
