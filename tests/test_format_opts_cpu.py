"""CPU tier: the output modes of the device formatter (ids, quality encoding), fastx_renamer, fastq_quality_converter and fastq_to_fasta -r on the
device text path -- through the emulation stub with fxg_fastq_format_opts behind it (tests/emu/fmtopts_stub.cpp runs the FXG_HD bodies of
csrc/fxg_text.h serially), and, as the fallback, over the stock stub library, which has no such entry.  The engine-level checks are those of
tests/format_opts_cases.py, the same ones tests/test_gpu_format_opts.py runs on the GPU."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import emu_py
import format_opts_cases as F
from conftest import ROOT
from fastx_toolkit_amd import engine as E
from oracle import fxoracle_py as fo

HOST = os.path.join(ROOT, "fastx_toolkit_amd", "host")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
GAL = os.path.join(ROOT, "tests", "golden", "galaxy")
REF_SRC = "/root/reference/src"
GALAXY = [      # argv, input, expected output (the reference's Galaxy test pairs)
    (["fastx_renamer", "-n", "SEQ", "-Q", "33"], "fastx_renamer1.fastq", "fastx_renamer1.out"),
    (["fastx_renamer", "-n", "SEQ", "-Q", "64"], "fastx_renamer1.fastq", "fastx_renamer1.out"),
    (["fastq_quality_converter", "-n", "-Q", "64"], "fastq_qual_conv1.fastq", "fastq_qual_conv1.out"),
    (["fastq_quality_converter", "-a", "-Q", "64"], "fastq_qual_conv1.fastq", "fastq_qual_conv1a.out"),
    (["fastq_quality_converter", "-a", "-Q", "64"], "fastq_qual_conv2.fastq", "fastq_qual_conv2.out"),
    (["fastq_quality_converter", "-n", "-Q", "64"], "fastq_qual_conv2.fastq", "fastq_qual_conv2n.out"),
]


@pytest.fixture(scope="module")
def stubdir():
    """a libfxg.so of the stub's own objects plus fxg_fastq_format_opts (emu_py.build_fmtopts)"""
    from fastx_toolkit_amd import build as b
    b.build_engine()          # the tools link against the real library's soname; a stub replaces it at run time only
    b.build_host()
    return emu_py.build_fmtopts()


@pytest.fixture(scope="module")
def eng(stubdir):
    e = F.StubEngine(os.path.join(stubdir, "libfxg.so"))
    yield e
    e.close()


def tool(libdir, argv, data=b"", env=None, timeout=120):
    e = dict(os.environ, LD_LIBRARY_PATH=libdir, FXH_THREADS="4", FXH_TIMING="1")
    e.update(env or {})
    p = subprocess.run([os.path.join(HOST, "bin", argv[0])] + argv[1:], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=timeout)
    err = b"".join(l for l in p.stderr.splitlines(True) if not l.startswith(b"fxh timing"))
    return p.returncode, p.stdout, err, p.stderr


def on_device(timing):
    return b"device parse" in timing and b" 0 host-parsed blocks" in timing


# ---- the closed form under the ordinal ids ---------------------------------------------------------------------------------------------
def test_decimal_width_sum_against_a_plain_loop(stubdir):
    """D(a, a + span): a at every power of ten +- 2 from 1 to 10^19 and at 2^64 - 300, spans 0..300"""
    L = C.CDLL(os.path.join(stubdir, "libfxg.so"))
    L.fxg_emu_dec_width_sum.restype, L.fxg_emu_dec_width_sum.argtypes = C.c_uint64, [C.c_uint64, C.c_uint64]
    starts = sorted({10 ** k + d for k in range(20) for d in range(-2, 3) if 10 ** k + d >= 0} | {2 ** 64 - 300})
    for a in starts:
        want = 0
        for span in range(301):
            if a + span > 2 ** 64:
                break
            assert L.fxg_emu_dec_width_sum(a, span) == want, (a, span)
            want += len(str(a + span))


# ---- the emulated entry: the GPU tier's cases, inputs and expectations -------------------------------------------------------------------
@pytest.mark.parametrize("n", F.RECORD_COUNTS)
def test_ordinal_ids(eng, n):
    F.check_ordinals(eng, n)


def test_ordinal_ids_on_packed_reversed_output(eng):
    F.check_ordinals_packed_reversed(eng)


def test_sequence_ids(eng):
    F.check_sequence_ids(eng)


@pytest.mark.parametrize("qoffset", [33, 64])
def test_quality_modes(eng, qoffset):
    F.check_quality_modes(eng, qoffset)


def test_requests(eng):
    F.check_requests(eng)


def test_engine_method(eng):
    F.check_engine_method(eng)


@pytest.mark.parametrize("numeric", ["none", "all", "alternating"])
def test_source_mode_matrix(eng, numeric):
    F.check_matrix(eng, numeric)


def test_numeric_writer_beside_other_groups_of_a_wave(eng):
    F.check_wave_mix(eng)


@pytest.mark.parametrize("numeric", ["none", "all", "alternating"])
def test_matrix_model_against_the_reference_tools(numeric):
    """the model behind the matrix (expected over the oracle's trimmed, masked and reversed records) against pipes of the real libfastx's tools"""
    F.check_matrix_model(numeric)


def test_numeric_writer_lanes_in_lock_step(stubdir):
    """fxg_text_write_numeric's host form: the 16 lanes of a group together -- every lane's share and sum, the four-step scan over the group's 16
    values, every lane's write, the last lane's LF -- against "%d" joined by blanks.  Every length from 0 to 70 and around 256, 4 096, the longest
    read and 65 535; values cycling through -15..93 with three strides; the codes and the line each between two PROT_NONE pages, so a lane that
    reads past its share or writes past the line's LF faults."""
    L = C.CDLL(os.path.join(stubdir, "libfxg.so"))
    L.fxg_emu_write_numeric.restype, L.fxg_emu_write_numeric.argtypes = None, [C.c_void_p, C.c_void_p, C.c_uint32]
    span = list(range(-15, 94))
    for n in list(range(71)) + [255, 256, 257, 4095, 4096, 4097, 24999, 65535]:
        for stride in (1, 7, 40):
            vals = [span[(n + j * stride) % len(span)] for j in range(n)]
            want = b" ".join(b"%d" % v for v in vals) + b"\n"
            for where in ("after", "before"):
                # (_guarded rounds a range up to the 16-byte granule: the arrays end exactly at the page when their size is a multiple of 16,
                # so the line is padded in FRONT to one -- the LF is then the byte before the guard page)
                pad = (-len(want)) % 16 if where == "after" else 0
                buf = emu_py._guarded(len(want) + pad, np.uint8, where)
                spad = (-n) % 16 if where == "after" else 0
                sbuf = emu_py._guarded(n + spad, np.uint8, where)
                sbuf[spad:] = np.array(vals, np.int64) + 33
                buf[:] = 0xA5
                L.fxg_emu_write_numeric(buf.ctypes.data + pad, sbuf.ctypes.data + spad, n)
                assert buf[pad:].tobytes() == want and (buf[:pad] == 0xA5).all(), (n, stride, where)


# ---- the model against the reference's own sources ---------------------------------------------------------------------------------------
def tool_inputs():
    """name -> (data, fasta, qoffset): the random inputs of the tool tests of both tiers"""
    rng = np.random.default_rng(2024)
    return {"fastq": (F.make_block(rng, 3000, lmax=90), False, 33), "crlf": (F.make_block(rng, 1500, lmax=90, crlf=True), False, 33),
            "numeric": (F.make_block(rng, 1500, lmax=90, numeric="all", qoffset=64), False, 64), "mixed": (F.make_block(rng, 1500, lmax=90, numeric="alternating"), False, 33),
            "fasta_collapsed": (F.make_block(rng, 2000, lmax=90, fasta=True, collapsed=True), True, 33)}


def tool_jobs():
    """(argv, input name, what the model says), for every tool and input of the tool tests"""
    jobs = []
    for name, (data, fasta, q) in tool_inputs().items():
        for how in ("COUNT", "SEQ"):
            jobs.append((["fastx_renamer", "-n", how, "-Q", str(q)], name, F.model_rename(data, how, fasta, q)))
        if not fasta:
            for flag in ("-a", "-n"):
                jobs.append((["fastq_quality_converter", flag, "-Q", str(q)], name, F.model_convert(data, flag == "-n", q)))
    return jobs


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="the reference sources exist in the build container only")
def test_model_equals_the_references_own_tools(tmp_path):
    """fastx_renamer.c and fastq_quality_converter.c compiled unchanged against host/fastx.h (as tests/test_source_compat.py does: an empty
    config.h): the record API alone, no GPU library behind it"""
    from fastx_toolkit_amd import build as b
    b.build_all()
    (tmp_path / "config.h").write_text("")
    exe = {}
    for t in ("fastx_renamer", "fastq_quality_converter"):
        exe[t] = str(tmp_path / t)
        subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-DPACKAGE_STRING=\"FASTX Toolkit 0.0.14\"", "-I", str(tmp_path), "-I", HOST, os.path.join(REF_SRC, t, t + ".c"),
                               os.path.join(HOST, "bin", "libfastx_amd.a"), "-L", os.path.join(ROOT, "fastx_toolkit_amd"), "-lfxg", "-lpthread", "-lz",
                               "-Wl,-rpath," + os.path.join(ROOT, "fastx_toolkit_amd"), "-o", exe[t]])
    inputs = tool_inputs()
    for argv, name, want in tool_jobs():
        p = subprocess.run([exe[argv[0]]] + argv[1:], input=inputs[name][0], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                           env=dict(os.environ, LD_LIBRARY_PATH=os.path.join(EMU_DIR, "stub")))
        assert p.returncode == 0 and p.stdout == want, (argv, name, p.stderr[-300:])
    for argv, inp, exp in GALAXY:
        data, fasta = open(os.path.join(GAL, inp), "rb").read(), False
        q = int(argv[-1])
        want = F.model_rename(data, "SEQ", fasta, q) if argv[0] == "fastx_renamer" else F.model_convert(data, "-n" in argv, q)
        assert want == open(os.path.join(GAL, exp), "rb").read(), argv


# ---- the tools through the stub library with the entry, and over the stock one without it ---------------------------------------------
def test_galaxy_pairs(stubdir):
    for libdir, device in ((stubdir, True), (os.path.join(EMU_DIR, "stub"), False)):
        for argv, inp, exp in GALAXY:
            rc, out, err, timing = tool(libdir, argv + ["-i", os.path.join(GAL, inp)])
            assert rc == 0 and out == open(os.path.join(GAL, exp), "rb").read(), (argv, device, err)
            assert on_device(timing) == device, (argv, device, timing)


def test_tools_equal_the_model(stubdir, tmp_path):
    inputs = tool_inputs()
    for argv, name, want in tool_jobs():
        data = inputs[name][0]
        for env in ({}, {"FXH_READ_BUFFER_MB": "1", "FXH_LANES": "3"}):
            rc, out, err, timing = tool(stubdir, argv, data, env)
            assert rc == 0 and out == want and on_device(timing), (argv, name, env, err, timing[-300:])
        rc, out, err, timing = tool(os.path.join(EMU_DIR, "stub"), argv, data)          # no entry in the library: the record path
        assert rc == 0 and out == want and b"device parse" not in timing, (argv, name, err)
    data, want = inputs["fasta_collapsed"][0], F.model_rename(inputs["fasta_collapsed"][0], "COUNT", True)
    reads = sum(1 + i % 5 for i in range(2000))
    for libdir in (stubdir, os.path.join(EMU_DIR, "stub")):
        rc, out, err, _ = tool(libdir, ["fastx_renamer", "-n", "COUNT", "-v"], data)
        assert rc == 0 and out == want and err == b"Renamed: %d reads.\n" % reads, err
    data, want = inputs["mixed"][0], F.model_convert(inputs["mixed"][0], True)
    z = tmp_path / "o.gz"
    rc, out, err, _ = tool(stubdir, ["fastq_quality_converter", "-n", "-z", "-v", "-o", str(z)], data)
    assert rc == 0 and gzip.decompress(z.read_bytes()) == want and out == b"Input: 1500 reads.\nOutput: 1500 reads.\n", err


def test_renamer_command_line(stubdir):
    rec = b"@a\nACGT\n+\nIIII\n"
    for libdir in (stubdir, os.path.join(EMU_DIR, "stub")):
        assert tool(libdir, ["fastx_renamer"], rec)[1] == b"@ACGT\nACGT\n+ACGT\nIIII\n"                 # no -n: SEQ
        assert tool(libdir, ["fastx_renamer", "-n", "SEQUENCE"], rec)[1] == b"@ACGT\nACGT\n+ACGT\nIIII\n"      # strncmp: a prefix with trailing junk
        assert tool(libdir, ["fastx_renamer", "-n", "COUNTER"], rec)[1] == b"@1\nACGT\n+1\nIIII\n"
        rc, out, err, _ = tool(libdir, ["fastx_renamer", "-n", "count"], rec)
        assert rc == 1 and out == b"" and err == b"fastx_renamer: Uknown rename type [-n]: 'count'\n"
        rc, out, err, _ = tool(libdir, ["fastq_quality_converter"], b">a\nACGT\n")
        assert rc == 1 and out == b""


def fq_reads(n, L=60, seed=9):
    return fo.synth_fastq(seed, 0, n, L, False)


@pytest.mark.parametrize("lanes", ["1", "2", "4"])
def test_fastq_to_fasta_rename_on_the_device_path(stubdir, lanes):
    """fastq_to_fasta -r / -n -r against the reference: 1 MB blocks, several per lane over two devices, ids that pass 9 -> 10 and 99 999 -> 100 000
    inside the run; no block goes to the host parser"""
    data = fq_reads(150000)
    assert len(data) > 16 << 20
    for argv in (["fastq_to_fasta", "-r", "-v"], ["fastq_to_fasta", "-n", "-r", "-v"]):
        rc, out, err, timing = tool(stubdir, argv, data, {"FXH_READ_BUFFER_MB": "1", "FXH_LANES": lanes, "FXG_EMU_DEVICES": "2", "FXG_DEVICES": "0,1"})
        rrc, rout, rerr = F.reference(argv, data)
        assert (rc, err) == (rrc, rerr) and rout == out, (argv, err, rerr)
        assert on_device(timing) and out.count(b">") > 100000, timing[-400:]


def test_fastq_to_fasta_rename_without_the_entry_is_host_parsed(stubdir):
    data = fq_reads(20000)
    argv = ["fastq_to_fasta", "-r"]
    rc, out, err, timing = tool(os.path.join(EMU_DIR, "stub"), argv, data, {"FXH_READ_BUFFER_MB": "1"})
    assert rc == 0 and b"host parse" in timing and out == tool(stubdir, argv, data, {"FXH_READ_BUFFER_MB": "1"})[1]


def test_malformed_record_in_the_middle_block(stubdir):
    """five blocks of 1 MB, a bad base in the third: the reference's message, exit code and partial output, the ids right across the host-parsed
    block; the timeout fails a chain of counts that got stuck"""
    data = fq_reads(34000, seed=13)
    assert 4 << 20 < len(data) < 5 << 20
    at = data.index(b"\n@", int(len(data) * 0.5)) + 1
    seq = data.index(b"\n", at) + 1
    bad = data[:seq] + b"X" + data[seq + 1:]
    env = {"FXH_READ_BUFFER_MB": "1", "FXH_LANES": "2"}
    argv = ["fastq_to_fasta", "-n", "-r"]
    rc, out, err, timing = tool(stubdir, argv, bad, env, timeout=60)
    rrc, rout, rerr = F.reference(argv, bad)
    assert rc == 1 and (rc, out) == (rrc, rout) and err.split(b": ", 1)[-1] == rerr.split(b": ", 1)[-1], (err, rerr)
    assert b" 1 host-parsed blocks" in timing or b"host-parsed" not in timing, timing[-300:]      # (an error run prints no totals line)
    rc, out, err, _ = tool(stubdir, ["fastx_renamer", "-n", "COUNT"], bad, env, timeout=60)
    good = F.model_rename(data[:at], "COUNT")
    assert rc == 1 and out == good and err.endswith(rerr.split(b": ", 1)[-1]), err
    # a block the device hands back without an error (a read too long for the device path) goes through the host parser, and the ids go on
    rng = np.random.default_rng(1)
    longrec = b"@long\n" + rng.choice(np.frombuffer(b"ACGT", np.uint8), size=24998).tobytes() + b"\n+\n" + b"I" * 24998 + b"\n"
    mixed = data[:at] + longrec + data[at:]
    for argv, want in ((["fastx_renamer", "-n", "COUNT"], F.model_rename(mixed, "COUNT")), (["fastq_to_fasta", "-n", "-r"], F.expected(mixed, 4, out_fasta=True, id_mode=E.ID_ORDINAL))):
        rc, out, err, timing = tool(stubdir, argv, mixed, env, timeout=60)
        assert rc == 0 and out == want and b" 1 host-parsed blocks" in timing, (argv, err, timing[-300:])


def test_sequence_ids_and_quality_modes_in_parts(stubdir, tmp_path):
    """FXH_PARTS=3: cat of the parts is the one-stream output, three device-path parts"""
    data = fq_reads(90000, L=100, seed=21)
    inp = tmp_path / "in.fq"
    inp.write_bytes(data)
    for argv in (["fastx_renamer", "-n", "SEQ"], ["fastq_quality_converter", "-n"]):
        single = tmp_path / "single.fq"
        rc = tool(stubdir, argv + ["-i", str(inp), "-o", str(single)], env={"FXH_READ_BUFFER_MB": "1"})[0]
        pat = str(tmp_path / (argv[0] + ".%r.fq"))
        grc, _, err, timing = tool(stubdir, argv + ["-i", str(inp), "-o", pat], env={"FXH_READ_BUFFER_MB": "1", "FXH_PARTS": "3"})
        assert (rc, grc) == (0, 0) and timing.count(b"fxh timing part") == 3 and timing.count(b"device parse") == 3 and b"host parse" not in timing, (err, timing[-500:])
        assert b"".join(open(pat.replace("%r", str(r)), "rb").read() for r in range(3)) == single.read_bytes(), argv
        assert single.read_bytes() == (F.model_rename(data, "SEQ") if argv[0] == "fastx_renamer" else F.model_convert(data, True))
        assert len(open(pat.replace("%r", "parts")).read().splitlines()) == 4
    rc, _, err, timing = tool(stubdir, ["fastx_renamer", "-n", "COUNT", "-i", str(inp), "-o", str(tmp_path / "c.%r.fq")], env={"FXH_READ_BUFFER_MB": "1", "FXH_PARTS": "3"})
    assert rc == 0 and timing.count(b"fxh timing part") == 1 and open(str(tmp_path / "c.0.fq"), "rb").read() == F.model_rename(data, "COUNT")      # ordinal ids: one stream


def test_renamer_counter_wrap_decision(tmp_path):
    """the block in which the renamer's unsigned int would pass 2^32 - 1 is the host parser's; the count goes on modulo 2^32"""
    src = tmp_path / "wrap.c"
    src.write_text('#include "fxh_priv.h"\nint main(int c, char **v) { unsigned long long b = strtoull(v[1], 0, 10), k = strtoull(v[2], 0, 10); int w = atoi(v[3]);\n'
                   '    printf("%d %llu\\n", fxh_ord_on_device(b, k, w), (unsigned long long)fxh_ord_next_base(b, k, w)); return c != 4; }\n')
    exe = str(tmp_path / "wrap")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", HOST, str(src), "-o", exe])
    M = 2 ** 32
    for base, kept, wrap, want in ((0, 10, 1, (1, 10)), (M - 11, 10, 1, (1, M - 1)), (M - 10, 10, 1, (0, 0)), (M - 1, 1, 1, (0, 0)), (M - 1, 0, 1, (1, M - 1)),
                                   (M - 5, 100, 1, (0, 95)), (M - 10, 10, 0, (1, M)), (M + 5, 7, 0, (1, M + 12)), (0, M - 1, 1, (1, M - 1)), (0, M, 1, (0, 0))):
        got = subprocess.run([exe, str(base), str(kept), str(wrap)], stdout=subprocess.PIPE, check=True).stdout.split()
        assert (int(got[0]), int(got[1])) == want, (base, kept, wrap, got)
