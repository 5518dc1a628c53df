"""fastx_uncollapser: the case generators and checks that the CPU tier (test_uncollapse_cpu.py) and the GPU tier (test_gpu_uncollapse.py) share."""
import functools
import json
import os
import random
import subprocess
import tempfile

import uncollapse_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "uncollapse")
TOOL = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fastx_uncollapser")

PIECE = 16                  # FXG_UC_PIECE
TEXT_MAX = 1 << 28          # FXG_UC_TEXT_MAX
COUNTS = [1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257]          # each side of the piece marks
RECORDS = [1, 255, 256, 257, 1023, 1024, 1025]                  # each side of the launch tile and the scan block
BASES = [1, 13, 16, 17, 150, 65535]
SEQ = b"ACGTNTGCAAGCTNNACGTAGGCTA"


def golden_cases():
    return json.load(open(os.path.join(GOLDEN, "cases.json")))["cases"]


def galaxy_pair():
    """(input, expected) of the reference's Galaxy test"""
    return open(os.path.join(GOLDEN, "fasta_uncollapser1.fasta"), "rb").read(), open(os.path.join(GOLDEN, "fasta_uncollapser1.out"), "rb").read()


def bases_of(n, salt=0):
    return bytes(SEQ[(i * 7 + salt + i // 25) % len(SEQ)] for i in range(n)) if n < 4096 else (SEQ * (n // len(SEQ) + 1))[salt % 7:][:n]


def rec(i, count, nbases, dash=True):
    """record i: an id that says `count` (count 1 with or without a dash) and nbases bases"""
    name = b"%d-%d" % (i, count) if dash or count != 1 else b"read%d" % i
    return name, bases_of(nbases, i)


@functools.lru_cache(maxsize=None)
def abi_blocks():
    """(name, records, ordinal_base): the blocks both tiers put through the entry in one call and compare with the model"""
    out = []
    for c in COUNTS:
        out.append(("count_%d_alone" % c, [rec(0, c, 9)], 0))
        out.append(("count_%d_mixed" % c, [rec(i, c if i in (2, 6, 7) else 1, 5 + i % 4, dash=i % 2 == 0) for i in range(11)], 95))
    for n in RECORDS:
        out.append(("records_%d" % n, [rec(i, 17 if i % 97 == 5 else 2 if i % 13 == 0 else 1, 1 + i % 23, dash=i % 3 != 0) for i in range(n)], 990))
    for b in BASES:
        out.append(("bases_%d" % b, [rec(0, 1, b), rec(1, 18, b), rec(2, 2, max(b // 2, 1))], 7))
    out.append(("ids_of_the_issue", [(b"a-4294967298", b"AC"), (b"b--5", b"A"), (b"c- +3", b"N"), (b"d-2x", b"AC"), (b"e-", b"A"), (b"no dash", b"T")], 0))
    out.append(("crlf", [(b"1-3\r", b"ACGT\r"), (b"2\r-9", b"GG\r"), (b"3-2", b"T")], 0))
    return out


@functools.lru_cache(maxsize=None)
def two_level_block():
    """enough records for two levels of the scan (more than 1024 * 1024): minimal records, a few of them counted"""
    n = 1024 * 1024 + 1500
    return [((b"-40" if i % 50021 == 7 else b"-3" if i % 1001 == 0 else b""), b"ACGTN"[i % 5:i % 5 + 1]) for i in range(n)], 99990


def ordinal_blocks():
    """(name, records, ordinal_base): the ids cross 10^k - 1 -> 10^k, k = 1 .. 19, between two records, inside a record's first piece and inside a
    further piece"""
    out = []
    for k in range(1, 20):
        p = 10 ** k
        out.append(("k%d_between" % k, [rec(0, 5, 7), rec(1, 3, 4)], p - 6))
        out.append(("k%d_inside_head" % k, [rec(0, 5, 7), rec(1, 1, 3)], p - 3))
        if p >= 100:
            out.append(("k%d_inside_tail" % k, [rec(0, 1, 3), rec(1, 40, 6), rec(2, 1, 2)], p - 20))
    return out


def window_block():
    """about 300 copies of at most 19 bytes each (ids 1 .. 3 digits wide, 1 .. 13 bases)"""
    rng = random.Random(5)
    counts = [1, 1, 35, 1, 2, 16, 1, 1, 17, 64, 1, 3, 1, 1, 100, 1, 1, 33, 1, 20]
    return [rec(i, c, rng.randint(1, 13), dash=c != 1 or i % 2 == 0) for i, c in enumerate(counts)], 0


def collapsed_text(nbytes, seed=3):
    """seeded collapsed FASTA of about nbytes bytes: 22 .. 30 bases, most counts 1, a heavy tail up to a few hundred"""
    rng = random.Random(seed)
    out, size, i = [], 0, 1
    while size < nbytes:
        u = rng.random()
        count = 1 if u < 0.8 else rng.randint(2, 9) if u < 0.97 else rng.randint(10, 400)
        r = b">%d-%d\n%s\n" % (i, count, bytes(rng.choice(b"ACGTN") for _ in range(rng.randint(22, 30))))
        out.append(r)
        size += len(r)
        i += 1
    return b"".join(out)


def run_tool(libdir, argv, stdin, env=None, files=False, timeout=300):
    """host/bin/fastx_uncollapser with `libdir` first on the library path (None: the product's own libfxg.so).  files: through -i / -o instead of
    stdin / stdout; "OUT" in argv names the output file.  Returns (status, stdout bytes, stderr text, output file bytes or None)."""
    e = dict(os.environ)
    if libdir:
        e["LD_LIBRARY_PATH"] = libdir + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    e.update(env or {})
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.fa"), os.path.join(d, "out.fa")
        argv = [dst if a == "OUT" else a for a in argv]
        if files:
            open(src, "wb").write(stdin)
            argv = argv + ["-i", src] + ([] if dst in argv else ["-o", dst])
        p = subprocess.run([TOOL] + argv, input=None if files else stdin, stdin=subprocess.DEVNULL if files else None, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=e, timeout=timeout)
        return p.returncode, p.stdout, p.stderr.decode("latin-1"), (open(dst, "rb").read() if os.path.exists(dst) else None)


def assert_tool_case(libdir, case, env=None):
    """the tool's bytes, -v report and status against the reference's recorded answer"""
    code, out, err, outfile = run_tool(libdir, case["argv"], case["stdin"].encode("latin-1"), env)
    name = case["name"]
    assert code == case["exit"], (name, code, err)
    if case["stdout"] == M.USAGE:
        assert out.startswith(b"usage: fastx_uncollapser") and not err, name
        return
    assert out == case["stdout"].encode("latin-1"), (name, out, err)
    if "outfile" in case:
        assert outfile == case["outfile"].encode("latin-1"), name
    if code == 0:
        assert err == case["stderr"], (name, err)          # the -v report, or nothing
    else:
        assert err.strip(), name
        if name.startswith("error_"):                       # the record API owns the reference's messages
            assert err.replace("(filename ='-')", "").split(": ", 1)[1].split("\n")[0] == case["stderr"].replace("(filename ='-')", "").split(": ", 1)[1].split("\n")[0], (name, err)
