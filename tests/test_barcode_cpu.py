"""fastx_barcode_splitter, CPU tier: the Python model (bcsplit_model.py) against the recorded goldens, and against the reference script on
seeded random cases where perl and the reference tree are present."""
import ctypes as C
import os
import random
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import bcsplit_model as M
import emu_py
from bcsplit_cases import assert_tool_case, exit_class, golden_cases, line_starts, make_block, make_table, model_run, run_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SCRIPT = os.path.join(os.environ.get("FXG_REFERENCE", "/root/reference"), "scripts", "fastx_barcode_splitter.pl")     # (the tree oracle/Makefile builds from)


def assert_same(o, exit_code, stdout, stderr, files, P="/o/"):
    assert o.exit == exit_class(exit_code), (o.exit, exit_code, o.stderr, stderr)
    if stdout != "(usage)":
        assert o.stdout == stdout.replace("{P}", P).encode("latin-1")
    errs = [l for l in stderr if l.startswith("Error:")]
    assert o.error_line() == (errs[0].replace("{P}", P).replace("{B}", "/b.txt").encode("latin-1") if errs else None)
    assert {k[len(P):].decode("latin-1"): v.decode("latin-1") for k, v in o.files.items()} == files


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_model_matches_goldens(case):
    o = model_run(case["argv"], case["barcodes"], case["stdin"])
    assert_same(o, case["exit"], case["stdout"], case["stderr"], case["files"])
    if case["exit"] in (0, 255) or case["stderr"]:
        assert [l.replace(b"/o/", b"{P}").replace(b"/b.txt", b"{B}").decode("latin-1") for l in o.stderr] == case["stderr"]


def test_galaxy_counts():
    c = next(c for c in golden_cases() if c["name"] == "galaxy")
    o = model_run(c["argv"], c["barcodes"], c["stdin"])
    assert o.stdout.decode().splitlines()[1:] == ["BC1\t11\t/o/BC1", "BC2\t12\t/o/BC2", "BC3\t9\t/o/BC3", "BC4\t1\t/o/BC4",
                                                  "unmatched\t9\t/o/unmatched", "total\t42"]


# ---- random cases against the reference script ---------------------------------------------------------------------------------------
def random_case(rng):
    BL = rng.randint(1, 12)
    eol = rng.random() < 0.5
    mm = rng.randint(0, 3)
    nid = rng.randint(0, 40)
    pool = ["BC%d" % k for k in range(max(1, nid // 2 + 1))] + ["unmatched", "s_1", "Z"]
    lines, bcs = [], []
    for _ in range(nid):
        bc = "".join(rng.choice("ACGT") for _ in range(BL))
        bcs.append(bc)
        ident = rng.choice(pool)
        sep = rng.choice(["\t", " ", "  ", "\t \t"])
        lines.append(ident + sep + (bc.lower() if rng.random() < 0.1 else bc) + (rng.choice(["", "\r", " extra"]) if rng.random() < 0.2 else ""))
        if rng.random() < 0.1:
            lines.append("# comment")
    bad = rng.random()
    if bad < 0.03:
        lines.insert(rng.randint(0, len(lines)), "")
    elif bad < 0.06:
        lines.append("X " + "ACGN"[:BL])
    elif bad < 0.08:
        lines.append("A" * BL + "-x " + "A" * BL)
    elif bad < 0.10 and BL > 1:
        lines.append("Q " + "A" * (BL - 1))
    bcfile = "\n".join(lines) + ("\n" if rng.random() < 0.9 else "")
    fastq = rng.random() < 0.6
    recs = []
    for k in range(rng.randint(0, 30)):
        if bcs and rng.random() < 0.7:
            core = list(rng.choice(bcs))
            for _ in range(rng.randint(0, 3)):
                if core:
                    core[rng.randrange(len(core))] = rng.choice("ACGTN")
            if rng.random() < 0.2 and core:
                del core[0 if not eol else -1]
            flank = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 8)))
            seq = ("".join(core) + flank) if not eol else (flank + "".join(core))
        else:
            seq = "".join(rng.choice("ACGTN") for _ in range(rng.randint(0, 14)))
        r = rng.random()
        if r < 0.05:
            seq += "\r"
        elif r < 0.08 and seq:
            i = rng.randrange(len(seq))
            seq = seq[:i] + rng.choice(["\x00", "a", "c", "\x00\x00"]) + seq[i + 1:]
        name = "r%d" % k
        recs.append(("@%s\n%s\n+\n%s\n" % (name, seq, "I" * len(seq))) if fastq else (">%s\n%s\n" % (name, seq)))
    data = "".join(recs)
    r = rng.random()
    if r < 0.1 and data:
        data = data[:-1]
    elif r < 0.15 and data:
        data = data[:rng.randint(0, len(data) - 1)]
    elif r < 0.17:
        data = "ACGT\n" + data
    argv = []
    spell = lambda full: rng.choice(["--" + full, "-" + full, "--" + full[:max(3, len(full) - rng.randint(0, 3))], "--" + full.upper()])
    argv += [spell("bcfile"), "{B}"] if rng.random() < 0.5 else [spell("bcfile") + "={B}"]
    argv += [spell("prefix"), "{P}"]
    if rng.random() < 0.5:
        argv += [spell("suffix"), rng.choice([".fq", ".txt", "_x"])]
    argv.append(spell("eol" if eol else "bol"))
    if rng.random() < 0.8:
        argv += [spell("mismatches"), str(mm)]
    else:
        mm = 1
    if rng.random() < 0.1:
        argv.append(spell("exact"))
        mm = 0
    if rng.random() < 0.3:
        argv += [spell("partial"), str(rng.randint(0, mm))]
    if rng.random() < 0.05:
        argv.append("--quiet")
    if rng.random() < 0.03:
        argv.append(rng.choice(["--nosuch", "--partial=x", "--mismatches=-1", "--partial", "--eol"]))
    return argv, bcfile, data


def run_reference(argv, bc, stdin):
    with tempfile.TemporaryDirectory() as d:
        P = os.path.join(d, "o") + "/"
        os.makedirs(P)
        B = os.path.join(d, "b.txt")
        open(B, "wb").write(bc.encode("latin-1"))
        args = [a.replace("{B}", B).replace("{P}", P) for a in argv]
        p = subprocess.run(["perl", REF_SCRIPT] + args, input=stdin.encode("latin-1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        files = {f: open(os.path.join(P, f), "rb").read().decode("latin-1") for f in os.listdir(P)}
        sub = lambda s: s.decode("latin-1").replace(P, "{P}").replace(B, "{B}")
        return p.returncode, sub(p.stdout), [l for l in sub(p.stderr).split("\n") if l.startswith("Error:")], files


@pytest.mark.skipif(not (os.path.exists(REF_SCRIPT) and shutil.which("perl")), reason="needs perl and the reference tree")
@pytest.mark.parametrize("chunk", range(6))
def test_model_matches_reference_random(chunk):
    rng = random.Random(1000 + chunk)
    for i in range(60):
        argv, bc, data = random_case(rng)
        code, out, errs, files = run_reference(argv, bc, data)
        o = model_run(argv, bc, data, B="/b.txt")
        ctx = (chunk, i, argv, bc, data)
        assert o.exit == exit_class(code), ctx
        assert o.stdout == out.replace("{P}", "/o/").encode("latin-1"), ctx
        assert o.error_line() == (errs[0].replace("{P}", "/o/").replace("{B}", "/b.txt").encode("latin-1") if errs else None), ctx
        assert {k[3:].decode("latin-1"): v.decode("latin-1") for k, v in o.files.items()} == files, ctx


def test_classify_vectorised_equals_scalar():
    rng = random.Random(7)
    for _ in range(50):
        BL = rng.randint(1, 20)
        eol = rng.random() < 0.5
        mm = rng.randint(0, min(3, BL - 1))
        entries = []
        for k in range(rng.randint(0, 12)):
            b = bytes(rng.choice(b"ACGT") for _ in range(BL))
            entries.append((b"I%d" % rng.randint(0, 4), b))
            for p in range(rng.randint(0, mm)):
                b = b[:-1] if eol else b[1:]
                entries.append((entries[-1][0], b))
        seqs = [bytes(rng.choice(b"ACGTN\x00\rg") for _ in range(rng.randint(0, BL + 4))) for _ in range(40)]
        names = M.bins_of(entries)
        win = np.zeros((len(seqs), BL), dtype=np.uint8)
        F = []
        for r, s in enumerate(seqs):
            f = M.window(s, BL, eol)
            win[r, :len(f)] = np.frombuffer(f, dtype=np.uint8)
            F.append(len(f))
        tab = np.zeros((max(len(entries), 1), BL), dtype=np.uint8)
        for k, (_, b) in enumerate(entries):
            tab[k, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        got = M.classify(win, F, tab, [len(b) for _, b in entries], [names.index(i) if i != b"unmatched" else len(names) - 1 for i, _ in entries],
                         BL, mm, len(names) - 1)
        want = [names.index(M.match(s, entries, BL, mm, eol)) for s in seqs]
        assert list(got) == want


# ---- the kernels' bodies through the CPU emulator (tests/emu/bcsplit_emu.cpp) ---------------------------------------------------------
EMU_DIR = os.path.join(ROOT, "tests", "emu")
FXG_H = os.path.join(ROOT, "include", "fxg.h")
BC_H = os.path.join(ROOT, "fastx_toolkit_amd", "csrc", "fxg_barcode.h")


class BarcodeSet(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("len", C.c_void_p), ("bin", C.c_void_p), ("entries", C.c_uint32), ("barcode_len", C.c_uint32),
                ("mismatches", C.c_uint32), ("eol", C.c_uint32), ("bins", C.c_uint32)]


def _obj(src, out):
    deps = [src, FXG_H, BC_H, os.path.join(EMU_DIR, "fxg_stub_ctx.h"), os.path.join(ROOT, "fastx_toolkit_amd", "csrc", "fxg_device.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(emu_py._CXX + ["-c", src, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


@pytest.fixture(scope="module")
def bcdir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bcsplit"))
    emu = _obj(os.path.join(EMU_DIR, "bcsplit_emu.cpp"), os.path.join(d, "bcsplit_emu.o"))
    subprocess.check_call(emu_py._LINK + [emu, "-o", os.path.join(d, "libbcsplit_emu.so")])
    return d


@pytest.fixture(scope="module")
def bcemu(bcdir):
    L = C.CDLL(os.path.join(bcdir, "libbcsplit_emu.so"))
    L.fxg_emu_bc_prepare.restype = C.c_void_p
    L.fxg_emu_bc_prepare.argtypes = [C.POINTER(BarcodeSet), C.c_void_p, C.c_char_p, C.c_size_t]
    L.fxg_emu_bc_free.argtypes = [C.c_void_p]
    L.fxg_emu_bc_split.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    return L


def emu_split(L, data, lpr, ents, BL, mm, eol, bins, guard=None):
    E = len(ents)
    bases = np.zeros((max(E, 1), 64), dtype=np.uint8)
    lens = np.zeros(max(E, 1), dtype=np.uint32)
    binv = np.zeros(max(E, 1), dtype=np.uint32)
    for k, (b, j) in enumerate(ents):
        bases[k, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        lens[k], binv[k] = len(b), j
    st = BarcodeSet(bases.ctypes.data, lens.ctypes.data, binv.ctypes.data, E, BL, mm, int(eol), bins)
    t = L.fxg_emu_bc_prepare(C.byref(st), None, None, 0)
    assert t
    ls_all = line_starts(data)
    n = (len(ls_all) - 1) // lpr
    text = emu_py._alloc(len(data), np.uint8, guard)
    text[:] = np.frombuffer(data, dtype=np.uint8)
    ls = emu_py._alloc(lpr * n + 1, np.uint32, guard)
    ls[:] = ls_all[:lpr * n + 1]
    total = int(ls_all[lpr * n])
    rb = emu_py._alloc(n, np.uint16, guard)
    out = emu_py._alloc(total, np.uint8, guard)
    bb, br = np.zeros(bins, dtype=np.uint64), np.zeros(bins, dtype=np.uint64)
    rc = L.fxg_emu_bc_split(t, text.ctypes.data if len(data) else None, len(data), lpr, ls.ctypes.data, lpr * n + 1, n,
                            rb.ctypes.data if n else None, out.ctypes.data if total else None, bb.ctypes.data, br.ctypes.data, None, 0)
    L.fxg_emu_bc_free(t)
    assert rc == 0
    return rb.astype(np.int64), bb, br, out.tobytes()


@pytest.mark.parametrize("seed", range(8))
def test_emulated_kernels_match_model(bcemu, seed):
    rng = random.Random(seed)
    for n in (1, 255, 256, 257, 700):
        BL = rng.choice([1, 2, 5, 8, 12, 31, 32, 33, 63, 64])
        eol = rng.random() < 0.5
        mm = rng.randint(0, min(3, BL - 1))
        partial = rng.randint(0, mm)
        bins = rng.choice([1, 2, 5, 97])
        lpr = rng.choice([2, 4])
        ents = make_table(rng, BL, bins, partial, eol)
        data = make_block(rng, n, lpr, BL, ents)
        want = M.split_block(data, lpr, [b for b, _ in ents], [j for _, j in ents], BL, mm, eol, bins)
        got = emu_split(bcemu, data, lpr, ents, BL, mm, eol, bins)
        assert list(got[0]) == list(want[0]), (seed, n)
        assert list(got[1]) == list(want[1]) and list(got[2]) == list(want[2]) and got[3] == want[3], (seed, n)


def _guard_child(where, q):
    try:
        L = C.CDLL(os.path.join(q, "libbcsplit_emu.so"))
        L.fxg_emu_bc_prepare.restype = C.c_void_p
        L.fxg_emu_bc_prepare.argtypes = [C.POINTER(BarcodeSet), C.c_void_p, C.c_char_p, C.c_size_t]
        L.fxg_emu_bc_free.argtypes = [C.c_void_p]
        L.fxg_emu_bc_split.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        rng = random.Random(hash(where) & 0xFFFF)
        for k in range(12):
            BL = rng.choice([1, 7, 16, 64])
            eol = k % 2 == 1
            lpr = rng.choice([2, 4])
            ents = make_table(rng, BL, 3, 0, eol)
            data = make_block(rng, rng.choice([1, 17, 256, 300]), lpr, BL, ents, long_every=97 if k == 0 else 0)
            want = M.split_block(data, lpr, [b for b, _ in ents], [j for _, j in ents], BL, min(1, BL - 1), eol, 3)
            got = emu_split(L, data, lpr, ents, BL, min(1, BL - 1), eol, 3, guard=where)
            if got[3] != want[3] or list(got[0]) != list(want[0]):
                os._exit(3)
        os._exit(0)
    except BaseException:
        os._exit(4)


@pytest.mark.parametrize("where", ["after", "before"])
def test_emulated_kernels_within_bounds(bcdir, where):
    """every array of the split at exactly its contracted size against a guard page: a byte touched outside it is a SIGSEGV of the child"""
    import multiprocessing as mp
    ctx = mp.get_context("fork")
    p = ctx.Process(target=_guard_child, args=(where, bcdir))
    p.start()
    p.join(600)
    assert p.exitcode == 0, "child exit %s (-11: an access outside an array's contract)" % p.exitcode


# ---- the tool end to end over the emulation stub ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stubdir(bcdir):
    """a libfxg.so of the stub's own objects plus the splitter's two entry points (bcsplit_stub.cpp over bcsplit_emu.cpp)"""
    from fastx_toolkit_amd import build as b
    stub = emu_py.build_stub()
    b.build_engine()
    b.build_host()
    objs = emu_py._emu_objects([])
    so = _obj(os.path.join(EMU_DIR, "bcsplit_stub.cpp"), os.path.join(bcdir, "bcsplit_stub.o"))
    d = os.path.join(bcdir, "stub")
    os.makedirs(d, exist_ok=True)
    subprocess.check_call(emu_py._LINK + [os.path.join(stub, "fxg_stub.o"), so, os.path.join(bcdir, "bcsplit_emu.o")] + objs +
                          ["-o", os.path.join(d, "libfxg.so"), "-ldl"])
    return d


STUB_ENVS = [{}, {"FXH_LANES": "1"}, {"FXH_LANES": "3"}, {"FXG_EMU_DEVICES": "2", "FXG_DEVICES": "0,1"}, {"FXH_READ_BUFFER_MB": "1", "FXH_LANES": "3"}]


@pytest.mark.parametrize("env", STUB_ENVS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
def test_tool_on_goldens_over_stub(stubdir, env):
    for case in golden_cases():
        assert_tool_case(run_tool(stubdir, case["argv"], case["barcodes"], case["stdin"], env), case)


def test_tool_many_blocks_over_stub(stubdir):
    """1 MB blocks over ~3 MB of input, long records among them, one and three lanes, two fake devices: the files equal the model's"""
    rng = random.Random(5)
    ents = make_table(rng, 8, 6, 1, False)
    bc = "".join("id%d %s\n" % (j, b.decode()) for b, j in ents[::2])
    data = make_block(rng, 9000, 4, 8, ents, long_every=2999).decode("latin-1")
    o = model_run(["--bcfile", "{B}", "--prefix", "{P}", "--bol", "--partial", "1"], bc, data)
    for env in ({"FXH_READ_BUFFER_MB": "1", "FXH_LANES": "1"}, {"FXH_READ_BUFFER_MB": "1", "FXH_LANES": "3", "FXG_EMU_DEVICES": "2", "FXG_DEVICES": "0,1"}):
        code, out, err, files = run_tool(stubdir, ["--bcfile", "{B}", "--prefix", "{P}", "--bol", "--partial", "1"], bc, data, env)
        assert code == 0, err
        assert out == o.stdout.decode("latin-1").replace("/o/", "{P}")
        assert files == {k[3:].decode(): v.decode("latin-1") for k, v in o.files.items()}


def test_tool_limits_over_stub(stubdir):
    long_bc = "A %s\n" % ("ACGT" * 17)
    code, _, err, files = run_tool(stubdir, ["--bcfile", "{B}", "--prefix", "{P}", "--bol"], long_bc, ">a\nACGT\n")
    assert code != 0 and err[-1].startswith("Error: barcode ") and "longer than 64" in err[-1] and files == {}
    many = "".join("i%d %s\n" % (k, "ACGTACGT") for k in range(4096))
    code, _, err, files = run_tool(stubdir, ["--bcfile", "{B}", "--prefix", "{P}", "--bol"], many, ">a\nACGT\n")
    assert code != 0 and "at most 4095" in err[-1] and files == {}
    ok = "".join("i%d %s\n" % (k, "ACGTACGT") for k in range(4095))
    code, out, err, files = run_tool(stubdir, ["--bcfile", "{B}", "--prefix", "{P}", "--bol", "--quiet"], ok, ">a\nACGTACGT\n")
    assert code == 0 and len(files) == 4096 and files["i0"] == ">a\nACGTACGT\n"


# ---- refused requests: the table of tests/request_cases.py through the stub, whose checks are the engine's own ---------------------------
@pytest.fixture(scope="module")
def stub_session(stubdir):
    import request_cases as rq
    s = rq.Session(os.path.join(stubdir, "libfxg.so"))
    yield s
    s.close()


def _case_ids():
    import request_cases as rq
    return [c[0] for c in rq.CASES]


@pytest.mark.parametrize("k", range(len(_case_ids())), ids=_case_ids())
def test_refused_requests_over_stub(stub_session, k):
    import request_cases as rq
    rq.refuse(stub_session, rq.CASES[k])


def test_accepted_requests_over_stub(stub_session):
    """one request per entry point of the table that goes through: checks that refused everything would pass the table"""
    s, L = stub_session, stub_session.lib
    fq = b"@a\nACGT\n+\nIIII\n"

    def arr(n, dtype=np.uint8, fill=None):
        a = emu_py._aligned(n, dtype)
        if fill is not None:
            a[:len(fill)] = np.frombuffer(fill, dtype=np.uint8)
        return a
    text, line, lens, flags = arr(len(fq) + 16, fill=fq), arr(10, np.uint32), arr(1, np.uint16), arr(1)
    assert L.fxg_fastq_index(s.ctx, text.ctypes.data, len(fq), 1, 4, line.ctypes.data, 5, lens.ctypes.data, flags.ctypes.data, C.byref(s.info)) == 0
    assert (s.info.records, s.info.consumed, s.info.irregular, lens[0]) == (1, len(fq), 0, 4)
    two, line2 = arr(2 * len(fq) + 16, fill=fq + fq), arr(10, np.uint32)      # a line array with room for one record of the two: the index stops there
    assert L.fxg_fastq_index(s.ctx, two.ctypes.data, 2 * len(fq), 0, 4, line2.ctypes.data, 5, lens.ctypes.data, flags.ctypes.data, C.byref(s.info)) == 0
    assert (s.info.lines, s.info.records, s.info.consumed, s.info.irregular) == (8, 1, len(fq), 0)
    bases, qual = arr(16), arr(16)
    assert L.fxg_fastq_pack(s.ctx, text.ctypes.data, len(fq), 4, line.ctypes.data, 5, flags.ctypes.data, 1, 16, 33, bases.ctypes.data, qual.ctypes.data, C.byref(s.word)) == 0
    assert bases[:4].tobytes() == b"ACGT" and qual[:4].tobytes() == b"IIII" and s.word.value == 0
    res, out = arr(1, np.uint32), arr(len(fq) + 1 + 16)
    res[0] = (1 << 16) | 4
    assert L.fxg_fastq_format(s.ctx, text.ctypes.data, 4, line.ctypes.data, 5, flags.ctypes.data, 1, res.ctypes.data, 0, 0, None, None, None, qual.ctypes.data, 16, 33, 0,
                              out.ctypes.data, C.byref(s.bytes_out)) == 0
    assert out[:s.bytes_out.value].tobytes() == fq
    hist = arr(16 * 5 * 128, np.uint64)
    assert L.fxg_run_quality_stats(s.ctx, C.byref(rq_batch(bases, qual, 4, 16, 1)), hist.ctypes.data, 16) == 0
    assert int(hist.sum()) == 4
    assert L.fxg_barcode_prepare(s.ctx, s.barcodes([(b"ACGT", 0)])) == 0
    bb, br, rb = (C.c_uint64 * 2)(), (C.c_uint64 * 2)(), arr(1, np.uint16)
    assert L.fxg_barcode_split(s.ctx, text.ctypes.data, len(fq), 4, line.ctypes.data, 5, 1, rb.ctypes.data, out.ctypes.data, bb, br) == 0
    assert list(br) == [1, 0] and list(bb) == [len(fq), 0] and out[:len(fq)].tobytes() == fq
    p = s.params(0x02)                  # fastq_quality_trimmer -t 0: the one read stays whole
    res[0] = 0
    assert L.fxg_run_pipeline(s.ctx, C.byref(rq_batch(bases, qual, 4, 16, 1)), C.addressof(p), C.byref(rq_out(res))) == 0, s.last_error()
    assert (int(res[0]) & 0xFFFF, (int(res[0]) >> 16) & 1) == (4, 1)


def rq_batch(bases, qual, fixed_len, stride, n):
    from fastx_toolkit_amd.engine import FxgBatch
    return FxgBatch(bases.ctypes.data, qual.ctypes.data, None, fixed_len, stride, n)


def rq_out(res):
    from fastx_toolkit_amd.engine import FxgOut
    return FxgOut(res=res.ctypes.data)
