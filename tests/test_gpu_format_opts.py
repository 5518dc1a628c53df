"""GPU tier (-m gpu): the output modes of the device formatter (fxg_fastq_format_opts: ordinal and sequence ids, forced quality encodings) on the
real engine, and the tools built on them -- fastq_to_fasta -r, fastx_renamer, fastq_quality_converter -- on the device text path.  The engine-level
checks are those of tests/format_opts_cases.py (the CPU tier runs the same ones through the emulator): exact bytes plus out_bytes, every output
between two 4 KiB canaries."""
import gzip
import os
import subprocess

import pytest

import format_opts_cases as F
from conftest import ROOT
from oracle import fxoracle_py as fo

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "fastx_toolkit_amd", "host")
GAL = os.path.join(ROOT, "tests", "golden", "galaxy")


@pytest.mark.parametrize("n", F.RECORD_COUNTS)
def test_ordinal_ids(engine, n):
    F.check_ordinals(engine, n)


def test_ordinal_ids_on_packed_reversed_output(engine):
    F.check_ordinals_packed_reversed(engine)


def test_sequence_ids(engine):
    F.check_sequence_ids(engine)


@pytest.mark.parametrize("qoffset", [33, 64])
def test_quality_modes(engine, qoffset):
    before = engine.scan_recoveries()
    F.check_quality_modes(engine, qoffset)
    assert engine.scan_recoveries() == before


def test_requests(engine):
    F.check_requests(engine)


def test_engine_method(engine):
    F.check_engine_method(engine)


@pytest.mark.parametrize("numeric", ["none", "all", "alternating"])
def test_source_mode_matrix(engine, numeric):
    before = engine.scan_recoveries()
    F.check_matrix(engine, numeric)
    assert engine.scan_recoveries() == before


def test_numeric_writer_beside_other_groups_of_a_wave(engine):
    before = engine.scan_recoveries()
    F.check_wave_mix(engine)
    assert engine.scan_recoveries() == before


# ---- the tools on the real engine ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "bin")


def tool(tools, argv, data=b"", env=None):
    e = dict(os.environ, FXH_TIMING="1")
    e.update(env or {})
    p = subprocess.run([os.path.join(tools, argv[0])] + argv[1:], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=120)      # a hang must fail fast
    err = b"".join(l for l in p.stderr.splitlines(True) if not l.startswith(b"fxh timing") and b"amdgpu.ids" not in l)
    return p.returncode, p.stdout, err, p.stderr


def on_device(timing):
    return b"device parse" in timing and b" 0 host-parsed blocks" in timing


def test_galaxy_pairs(tools):
    from test_format_opts_cpu import GALAXY
    for argv, inp, exp in GALAXY:
        rc, out, err, timing = tool(tools, argv + ["-i", os.path.join(GAL, inp)])
        assert rc == 0 and out == open(os.path.join(GAL, exp), "rb").read() and on_device(timing), (argv, err, timing[-300:])


@pytest.mark.parametrize("lanes", ["1", "3"])
def test_fastq_to_fasta_rename_against_the_reference(tools, lanes):
    data = fo.synth_fastq(9, 0, 200000, 100, False)
    for argv in (["fastq_to_fasta", "-r", "-v"], ["fastq_to_fasta", "-n", "-r", "-v"]):
        rc, out, err, timing = tool(tools, argv, data, {"FXH_READ_BUFFER_MB": "1", "FXH_LANES": lanes})
        rrc, rout, rerr = F.reference(argv, data)
        assert (rc, err) == (rrc, rerr) and rout == out, (argv, err, rerr)
        assert on_device(timing), timing[-400:]


def test_renamer_and_converter_against_the_model(tools, tmp_path):
    from test_format_opts_cpu import tool_inputs, tool_jobs
    inputs = tool_inputs()
    for argv, name, want in tool_jobs():
        rc, out, err, timing = tool(tools, argv, inputs[name][0], {"FXH_READ_BUFFER_MB": "1"})
        assert rc == 0 and out == want and on_device(timing), (argv, name, err, timing[-300:])
    data = inputs["fasta_collapsed"][0]
    rc, out, err, _ = tool(tools, ["fastx_renamer", "-n", "COUNT", "-v"], data)
    assert rc == 0 and out == F.model_rename(data, "COUNT", True) and err == b"Renamed: %d reads.\n" % sum(1 + i % 5 for i in range(2000)), err
    data = inputs["mixed"][0]
    for argv, want in ((["fastq_quality_converter", "-n"], F.model_convert(data, True)), (["fastx_renamer", "-n", "COUNT"], F.model_rename(data, "COUNT"))):
        z = tmp_path / (argv[0] + ".gz")
        rc, out, err, _ = tool(tools, argv + ["-z", "-o", str(z)], data)
        assert rc == 0 and gzip.decompress(z.read_bytes()) == want, (argv, err)


def test_sequence_ids_and_converter_in_parts(tools, tmp_path):
    data = fo.synth_fastq(21, 0, 90000, 100, False)
    inp = tmp_path / "in.fq"
    inp.write_bytes(data)
    for argv, want in ((["fastx_renamer", "-n", "SEQ"], F.model_rename(data, "SEQ")), (["fastq_quality_converter", "-n"], F.model_convert(data, True))):
        pat = str(tmp_path / (argv[0] + ".%r.fq"))
        rc, _, err, timing = tool(tools, argv + ["-i", str(inp), "-o", pat], env={"FXH_READ_BUFFER_MB": "1", "FXH_PARTS": "2"})
        assert rc == 0 and timing.count(b"fxh timing part") == 2 and timing.count(b"device parse") == 2 and b"host parse" not in timing, (err, timing[-500:])
        assert b"".join(open(pat.replace("%r", str(r)), "rb").read() for r in range(2)) == want, argv
