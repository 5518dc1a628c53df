"""Shared by the barcode splitter's tests (CPU and GPU tier): the recorded goldens, random tables and blocks, and running the tool.
Reads tests/golden only."""
import json
import os
import subprocess
import tempfile

import numpy as np

import bcsplit_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "barcode")


def golden_cases():
    cases = json.load(open(os.path.join(GOLD, "cases.json")))
    for c in cases:
        for k in ("barcodes", "stdin"):
            if c[k] is not None and c[k].startswith("file:"):
                c[k] = open(os.path.join(GOLD, c[k][5:]), encoding="latin-1").read()
    return cases


def exit_class(code):
    return "ok" if code == 0 else ("usage" if code == 1 else "error")


def model_run(argv, bc, stdin, P="/o/", B="/b.txt"):
    args = [a.replace("{B}", B).replace("{P}", P).encode("latin-1") for a in argv]
    read = lambda name: bc.encode("latin-1") if (bc is not None and name == B.encode()) else None
    return M.run(args, stdin.encode("latin-1"), read)


def make_table(rng, BL, nbins, partial, eol):
    """entries [(bases, bin)] in table order over nbins bins (the last is unmatched, which an entry may name too)"""
    ents = []
    for k in range(rng.randint(0, 3 * nbins)):
        b = bytes(rng.choice(b"ACGT") for _ in range(BL))
        j = rng.randrange(nbins)
        ents.append((b, j))
        for p in range(partial):
            b = b[:-1] if eol else b[1:]
            ents.append((b, j))
    return ents


def make_block(rng, n, lpr, BL, ents, long_every=0):
    recs = []
    for r in range(n):
        if ents and rng.random() < 0.6:
            core = bytearray(rng.choice(ents)[0])
            for _ in range(rng.randint(0, 2)):
                if core:
                    core[rng.randrange(len(core))] = rng.choice(b"ACGTN")
            seq = bytes(core) + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 20)))
        else:
            seq = bytes(rng.choice(b"ACGTN\r\x00a") for _ in range(rng.randint(0, BL + 10)))
        if long_every and r % long_every == 0:
            seq = bytes(rng.choice(b"ACGT") for _ in range(100000))
        seq = seq.replace(b"\n", b"N")
        recs.append((b"@r%d\n" % r + seq + b"\n+\n" + b"I" * len(seq) + b"\n") if lpr == 4 else (b">r%d\n" % r + seq + b"\n"))
    return b"".join(recs)


def line_starts(data):
    nl = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)
    return np.concatenate([[0], nl + 1]).astype(np.uint32)


TOOL = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fastx_barcode_splitter")


def run_tool(libdir, argv, bc, stdin, env=None, tool=TOOL):
    with tempfile.TemporaryDirectory() as d:
        P = os.path.join(d, "o") + "/"
        os.makedirs(P)
        B = os.path.join(d, "b.txt")
        if bc is not None:
            open(B, "wb").write(bc.encode("latin-1"))
        args = [a.replace("{B}", B).replace("{P}", P) for a in argv]
        e = dict(os.environ, **(env or {}))
        if libdir:
            e["LD_LIBRARY_PATH"] = libdir
        p = subprocess.run([tool] + args, input=stdin.encode("latin-1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=300)
        files = {f: open(os.path.join(P, f), "rb").read().decode("latin-1") for f in os.listdir(P)}
        sub = lambda s: s.decode("latin-1").replace(P, "{P}").replace(B, "{B}")
        return p.returncode, sub(p.stdout), [l for l in sub(p.stderr).split("\n") if l], files


def assert_tool_case(got, case):
    code, out, err, files = got
    assert exit_class(code) == exit_class(case["exit"]), (case["name"], code, err)
    if case["stdout"] != "(usage)":
        assert out == case["stdout"], case["name"]
    want_err = [l for l in case["stderr"] if l.startswith("Error:")]
    assert [l for l in err if l.startswith("Error:")][:1] == want_err[:1], (case["name"], err)
    assert files == case["files"], case["name"]
    if case["name"] == "debug":
        assert err == case["stderr"]


