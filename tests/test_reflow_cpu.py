"""fasta_formatter, CPU tier: the Python model (reflow_model.py) against the recorded answers of the reference and, where the reference
tree is present, against the reference itself on seeded random inputs; the kernels' bodies through the CPU emulator
(tests/emu/reflow_emu.cpp) against the block model, with every array against a guard page; the tool over the emulation stub (its device
path) and over the stock stub (its host path); and the emulator and the host path as stand-alone programs under ASan + UBSan."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import emu_py
import reflow_model as M
from reflow_cases import (GRID, PIECE, ROOT, WIDTHS, argv_of, assert_tool_case, expected_status, galaxy_pairs, geometry_texts, golden_cases,
                          open_in_values, random_text, run_tool)

REF = os.environ.get("FXG_REFERENCE", "/root/reference")
REF_SRC = os.path.join(REF, "src", "fasta_formatter", "fasta_formatter.cpp")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fastx_toolkit_amd", "csrc")
HOST = os.path.join(ROOT, "fastx_toolkit_amd", "host")


# ---- the model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_model_matches_recorded(case):
    out, status = M.run_argv(case["argv"], case["stdin"].encode("latin-1"))
    assert status == expected_status(case)
    if case["exit"] != 134:             # (what the reference had written before it aborted is not part of the contract)
        assert out == (M.USAGE if case["stdout"] == M.USAGE else case["stdout"].encode("latin-1"))


def test_recorded_cases_hold_the_contract_corners():
    by = {c["name"]: c for c in golden_cases()}
    assert len(by) >= 40
    assert by["example_default"]["stdout"] == ">a\nACGT\rAC\n>c\nAAA\n" and by["example_e"]["stdout"] == ">a\nACGT\rAC\n>b\n>c\nAAA\n"
    assert by["example_t_e"]["stdout"] == "a\tACGT\rAC\nb\nc\tAAA\n" and by["example_w3"]["stdout"] == ">a\nACG\nT\rA\nC\n>c\nAAA\n"
    assert by["exact_multiple_w3"]["stdout"] == ">a\nACG\nTAC\n" and by["no_header_w0"]["stdout"] == "\nACGTAC\n"
    assert (by["empty_input"]["stdout"], by["empty_input_e"]["stdout"], by["empty_input_t"]["exit"]) == ("", "\n", 0)
    assert by["no_header_t"]["exit"] == 134 and by["empty_input_t_e"]["exit"] == 134 and by["negative_width"]["exit"] == 1 and by["unknown_option"]["exit"] == 1


def test_model_galaxy_pairs():
    for src, argv, want in galaxy_pairs():
        assert M.run_argv(argv, src) == (want, 0)


def test_block_model_chains_to_the_whole_model():
    """a text cut into two blocks at every byte: the chained blocks give the whole input's output, whatever the options"""
    rng = random.Random(11)
    text = random_text(rng, records=9, max_lines=4, max_line=30)[:600]
    text = b">s\n" + text
    for w, t, e in [(0, False, False), (3, False, True), (16, False, False), (60, True, True), (1, False, True)]:
        whole = M.format_whole(text, w, t, e)[0]
        for cut in range(len(text) + 1):
            assert M.reflow_chain(text, [cut], w, t, e) == whole, (w, t, e, cut)


@pytest.fixture(scope="module")
def reference_exe(tmp_path_factory):
    if not os.path.exists(REF_SRC):
        pytest.skip("the reference sources exist in the build container only")
    d = tmp_path_factory.mktemp("ref_formatter")
    (d / "config.h").write_text("")
    exe = str(d / "fasta_formatter")
    p = subprocess.run(["g++", "-O1", "-DPACKAGE_STRING=\"FASTX Toolkit 0.0.14\"", "-I", str(d), "-I", os.path.join(ROOT, "tests", "compat"), REF_SRC, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, "the reference's fasta_formatter.cpp no longer compiles against tests/compat/gtextutils:\n" + p.stdout[-3000:]
    return exe


def test_model_matches_reference_on_random_inputs(reference_exe):
    rng = random.Random(2024)
    for k in range(300):
        w, t, e = rng.choice(GRID)
        text = random_text(rng, long_lines=1 if k % 25 == 0 else 0, orphans=k % 10 == 3)
        if k % 40 == 7:
            text = b"".join(l for l in text.split(b"\n") if not l.startswith(b">"))      # no header at all
        p = subprocess.run([reference_exe] + argv_of(w, t, e), input=text, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        out, status = M.format_whole(text, w, t, e)
        if p.returncode == -6:
            assert status == 1, k
        else:
            assert (p.returncode, p.stdout) == (status, out), (k, w, t, e)


# ---- the kernels' bodies through the CPU emulator ---------------------------------------------------------------------------------------
class Opts(C.Structure):
    _fields_ = [("width", C.c_uint32), ("tabular", C.c_uint32), ("keep_empty", C.c_uint32), ("out_cap", C.c_uint64)]


class Info(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("headers", C.c_uint64), ("consumed", C.c_uint64), ("out_bytes", C.c_uint64), ("open_bases", C.c_uint64)]


def _obj(src, out, flags=()):
    deps = [src, os.path.join(ROOT, "include", "fxg.h"), os.path.join(EMU_DIR, "fxg_stub_ctx.h"), os.path.join(EMU_DIR, "reflow_emu.cpp")] + \
           [os.path.join(CSRC, f) for f in ("fxg_reflow.h", "fxg_barcode.h", "fxg_device.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(emu_py._CXX + list(flags) + ["-c", src, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


@pytest.fixture(scope="module")
def rfdir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("reflow"))
    emu = _obj(os.path.join(EMU_DIR, "reflow_emu.cpp"), os.path.join(d, "reflow_emu.o"))
    subprocess.check_call(emu_py._LINK + [emu, "-o", os.path.join(d, "libreflow_emu.so")])
    return d


def _load(rfdir):
    L = C.CDLL(os.path.join(rfdir, "libreflow_emu.so"))
    L.fxg_emu_fasta_reflow.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(Opts), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(Info),
                                       C.c_char_p, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def rfemu(rfdir):
    return _load(rfdir)


def emu_reflow(L, text, at_eof, open_in, w, t, e, guard=None, out_cap=None):
    """the emulated call with every array at its contracted size: the text plus its 16 bytes of slack, lines + 1 line starts (and as many
    ends), an output of exactly the bytes the model expects (or out_cap).  Returns (rc, out, consumed, open_bases, message)."""
    n, lines = len(text), text.count(b"\n")
    try:
        want = len(M.reflow_block(text, at_eof, open_in, w, t, e)[0])
    except M.Refused:
        want = 0
    cap = want if out_cap is None else out_cap
    d_text = emu_py._alloc(n + 16, np.uint8, guard)
    d_text[:n] = np.frombuffer(text, dtype=np.uint8)
    d_line = emu_py._alloc(2 * (lines + 1), np.uint32, guard)
    d_out = emu_py._tight(np.full(cap, 0xEE, dtype=np.uint8), guard) if guard else np.full(cap, 0xEE, dtype=np.uint8)
    o, info, err = Opts(w, int(t), int(e), cap), Info(), C.create_string_buffer(300)
    rc = L.fxg_emu_fasta_reflow(d_text.ctypes.data, n, int(at_eof), open_in, C.byref(o), d_line.ctypes.data, lines + 1,
                                d_out.ctypes.data if cap else None, C.byref(info), err, 300)
    return rc, bytes(d_out[:info.out_bytes]), info.consumed, info.open_bases, err.value.decode()


def _random_block(rng, k):
    w, t, e = GRID[k % len(GRID)]
    text = random_text(rng, long_lines=1 if k % 9 == 0 else 0, limit=50000)
    if text and not text.endswith(b"\n"):
        text += b"\n"
    at_eof = k % 2 == 0
    if not at_eof and text:
        text = text[:rng.randint(0, len(text))]
    return text, at_eof, rng.choice(open_in_values(w)), w, t, e


def _check_block(L, text, at_eof, open_in, w, t, e, guard=None, tag=None):
    try:
        want = M.reflow_block(text, at_eof, open_in, w, t, e)
    except M.Refused:
        rc, _, _, _, msg = emu_reflow(L, text, at_eof, open_in, w, t, e, guard)
        assert rc == -1 and "no record open" in msg, tag
        return
    rc, out, consumed, open_bases, msg = emu_reflow(L, text, at_eof, open_in, w, t, e, guard)
    assert rc == 0, (tag, msg)
    assert (out, consumed, open_bases) == want, (tag, w, t, e, at_eof, open_in)


@pytest.mark.parametrize("seed", range(4))
def test_emulated_kernels_match_block_model(rfemu, seed):
    rng = random.Random(100 + seed)
    for k in range(len(GRID)):
        _check_block(rfemu, *_random_block(rng, k + seed), tag=(seed, k))


def test_emulated_kernels_geometry(rfemu):
    for name, text in geometry_texts():
        for w, t, e in ((0, False, False), (3, False, True), (60, True, True)):
            _check_block(rfemu, text, True, 0, w, t, e, tag=name)
            _check_block(rfemu, text, False, 7, w, t, e, tag=name)
    line = b">one\n" + bytes(b"ACGT"[i % 4] for i in range((1 << 20) + 1)) + b"\n"          # piece boundaries: a line of 1 MiB + 1 bytes
    for w in (0, 60, PIECE):
        _check_block(rfemu, line, True, 0, w, False, False, tag=("long", w))
        _check_block(rfemu, line[5:], False, PIECE - 1, w, False, False, tag=("long_open", w))


def test_emulated_refusals(rfemu):
    text = b">a\nACGT\nAC\n>b\nGG\n"
    want = M.reflow_block(text, True, 0, 3, False, False)[0]
    rc, _, _, _, msg = emu_reflow(rfemu, text, True, 0, 3, False, False, out_cap=len(want) - 1)
    assert rc == -1 and "needs %d bytes" % len(want) in msg
    rc, out, consumed, open_bases, _ = emu_reflow(rfemu, b"", True, 5, 0, False, False)
    assert (rc, out, consumed, open_bases) == (0, b"\n", 0, 0)
    rc, out, _, _, _ = emu_reflow(rfemu, b"", True, 6, 3, False, False)
    assert (rc, out) == (0, b"")                                         # six bases at width 3: the last line is already ended
    rc, _, _, _, msg = emu_reflow(rfemu, b"ACGT\n>a\n", True, 0, 0, False, False)
    assert rc == -1 and "no record open" in msg


def _guard_child(where, rfdir):
    try:
        L = _load(rfdir)
        rng = random.Random(7 if where == "after" else 8)
        for k in range(len(GRID)):
            _check_block(L, *_random_block(rng, k), guard=where, tag=k)
        for name, text in geometry_texts()[:6]:
            _check_block(L, text, True, 0, 17, False, True, guard=where, tag=name)
        os._exit(0)
    except AssertionError:
        os._exit(3)
    except BaseException:
        os._exit(4)


@pytest.mark.parametrize("where", ["after", "before"])
def test_emulated_kernels_within_bounds(rfdir, where):
    """every array of the call at exactly its contracted size against a PROT_NONE page: a byte touched outside it is a SIGSEGV of the child"""
    import multiprocessing as mp
    p = mp.get_context("fork").Process(target=_guard_child, args=(where, rfdir))
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
def reflow_stub(rfdir, stock_stub):
    """a libfxg.so of the stub's own objects plus fxg_fasta_reflow (reflow_stub.cpp over reflow_emu.cpp)"""
    so = _obj(os.path.join(EMU_DIR, "reflow_stub.cpp"), os.path.join(rfdir, "reflow_stub.o"))
    d = os.path.join(rfdir, "stub")
    os.makedirs(d, exist_ok=True)
    subprocess.check_call(emu_py._LINK + [os.path.join(stock_stub, "fxg_stub.o"), so, os.path.join(rfdir, "reflow_emu.o")] + emu_py._emu_objects([]) +
                          ["-o", os.path.join(d, "libfxg.so"), "-ldl"])
    return d


@pytest.mark.parametrize("files", [False, True], ids=["stdin_stdout", "i_o"])
def test_tool_on_recorded_cases_device_path(reflow_stub, files):
    for case in golden_cases():
        assert_tool_case(reflow_stub, case, files=files)
    for src, argv, want in galaxy_pairs():
        assert run_tool(reflow_stub, argv, src, files=files)[:2] == (0, want)


@pytest.mark.parametrize("files", [False, True], ids=["stdin_stdout", "i_o"])
def test_tool_on_recorded_cases_host_path(stock_stub, files):
    """the stock stub has no fxg_fasta_reflow: every input takes the host path, and gives the same bytes"""
    for case in golden_cases():
        assert_tool_case(stock_stub, case, files=files)
    for src, argv, want in galaxy_pairs():
        assert run_tool(stock_stub, argv, src, files=files)[:2] == (0, want)


@pytest.fixture(scope="module")
def five_mb():
    rng = random.Random(77)
    parts = [random_text(rng, records=40, long_lines=2) for _ in range(60)]
    text = b">first\n" + b"".join(p if p.endswith(b"\n") else p + b"\n" for p in parts)
    while len(text) < 5 << 20:
        text += text[:1 << 20]
        text = text[:text.rfind(b"\n") + 1]
    return text


@pytest.mark.parametrize("opts", [(0, False, False), (60, False, True), (7, False, False), (0, True, True)], ids=str)
def test_tool_many_blocks(reflow_stub, stock_stub, five_mb, opts):
    """a 5 MB file in 1 MB blocks, lines longer than what a block carries over among them: the device path and the host path equal the model"""
    want = M.format_whole(five_mb, *opts)[0]
    env = {"FXH_READ_BUFFER_MB": "1"}
    for lib, files in ((reflow_stub, False), (reflow_stub, True), (stock_stub, True)):
        code, out, err = run_tool(lib, argv_of(*opts), five_mb, env, files=files)
        assert code == 0, err
        assert out == want, (lib, files, len(out), len(want))


def test_tool_line_longer_than_a_block(reflow_stub):
    """a 3 MB line with 1 MB blocks: the block grows until the line fits"""
    text = b">a\nAC\n>long\n" + b"ACGTTGCA" * (3 << 17) + b"\nGG\n>z\nTT\n"
    for opts in ((0, False, False), (60, False, False)):
        code, out, err = run_tool(reflow_stub, argv_of(*opts), text, {"FXH_READ_BUFFER_MB": "1"})
        assert code == 0, err
        assert out == M.format_whole(text, *opts)[0]


def test_tool_options(stock_stub):
    assert run_tool(stock_stub, ["-w", "-3"], b">a\nAC\n")[0] == 1
    assert run_tool(stock_stub, ["-Q", "33"], b">a\nAC\n")[0] == 1
    code, out, err = run_tool(stock_stub, ["-i", "/nonexistent/in.fa"], b"")
    assert code == 1 and out == b"" and "nonexistent" in err


# ---- stand-alone programs under the sanitizers -----------------------------------------------------------------------------------------
REPORT = (b"ERROR: AddressSanitizer", b"runtime error:", b"ERROR: LeakSanitizer", b"SUMMARY: UndefinedBehaviorSanitizer")


def _corner_corpus():
    corpus = [c["stdin"].encode("latin-1") for c in golden_cases()]
    corpus += [b">x\n" + b"ACGTN" * 1700 + b"\n>y\n\n\nAC\n", b">h\n" * 300, b"\n" * 50 + b">a\nA\n"]
    return corpus


@pytest.mark.sanitizers
def test_emulator_and_host_path_under_sanitizers(tmp_path, stock_stub):
    """two programs with a main of their own, built with -fsanitize=address,undefined and run directly: the emulated kernels over one block
    (reflow_san_main.cpp) and the tool on its host path (the instrumented host build over the stock stub)"""
    exe = str(tmp_path / "reflow_san_main")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wno-pass-failed", "-DFXG_HOST_EMULATION",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(EMU_DIR, "reflow_san_main.cpp"), "-o", exe])
    subprocess.check_call(["make", "-s", "-C", HOST, "SAN=address,undefined"])
    tool = os.path.join(HOST, "bin_san_address_undefined", "fasta_formatter")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    src = tmp_path / "block.fa"
    checked = 0
    for i, text in enumerate(_corner_corpus()):
        for w, t, e in ((0, False, False), (3, False, True), (16, True, True), (61, False, False)):
            # the host path: the whole input through the instrumented tool
            p = subprocess.run([tool] + argv_of(w, t, e), input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                               env=dict(env, LD_LIBRARY_PATH=stock_stub))
            assert not any(m in p.stderr for m in REPORT) and p.returncode != 99, (i, p.stderr[-1500:])
            assert (p.stdout, p.returncode) == M.format_whole(text, w, t, e), i
            # the emulator: the block the device would get (every line ended), at the end of input and not
            block = text if not text or text.endswith(b"\n") else text + b"\n"
            src.write_bytes(block)
            for at_eof, open_in in ((1, 0), (0, 0), (1, w + 1), (0, (1 << 32) + 5)):
                p = subprocess.run([exe, str(src), str(w), str(int(t)), str(int(e)), str(at_eof), str(open_in)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                   timeout=120, env=env)
                assert not any(m in p.stderr for m in REPORT) and p.returncode != 99, (i, p.stderr[-1500:])
                try:
                    want = M.reflow_block(block, bool(at_eof), open_in, w, t, e)
                except M.Refused:
                    assert p.returncode == 1 and b"no record open" in p.stderr, i
                    continue
                rc, consumed, open_bases = p.stderr.split()[:3]
                assert (p.returncode, int(rc), p.stdout, int(consumed), int(open_bases)) == (0, 0) + want, (i, w, t, e, at_eof, open_in)
                checked += 1
    assert checked > 300
