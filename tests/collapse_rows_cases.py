"""fxg_collapse_add_rows and fastx_clip_collapser: what the CPU tier (test_collapse_rows_cpu.py) and the GPU tier (test_gpu_collapse_rows.py)
share.  The entry is checked against the text entry: the same records added as packed rows and as indexed text must give the same info and the
same bytes, and for the recorded cases of collapse_cases.py those are the reference's.  The tool is checked against the recorded answers of the
reference pipe (golden/clip_collapse/cases.json)."""
import functools
import json
import os
import subprocess
import tempfile

import numpy as np

import collapse_cases as K
import collapse_model as M

ROOT = K.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_collapse")
TOOL = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fastx_clip_collapser")
NONE = (1 << 64) - 1
IRR_BASE = 0x10
PACK_LONGEST = K.LONGEST                # the longest read the pack takes: the longest line the index accepts
LENGTHS = [1, 7, 8, 9, 15, 16, 17, 31, 33, 150, PACK_LONGEST]
RECORDS = [0, 1, 15, 16, 17, 255, 256, 257, K.TRIP - 1, K.TRIP, K.TRIP + 1]      # the insert's workgroup; one either side of the copy launch's trip


def pack_rows(seqs, gap=lambda k: (5 * k + 3) % 16, lead=0):
    """the sequences as packed rows with gaps between them, so that d_off runs through every residue modulo 16 (gap(k) bytes of 'x' before
    record k, lower case: a byte that would be irregular if it were ever copied).  Returns (bases, off, len): bases ends at the last record's last byte."""
    off, at = [], lead
    for k, s in enumerate(seqs):
        at += gap(k)
        off.append(at)
        at += len(s)
    bases = np.full(at, ord("x"), dtype=np.uint8)
    for o, s in zip(off, seqs):
        bases[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    return bases, np.array(off, dtype=np.uint64), np.array([len(s) for s in seqs], dtype=np.uint16)


def with_dropped(records, every=3):
    """the records as the kept ones of a larger FASTA block: a record the chain dropped, with a count of its own in its id, before every
    `every`-th one and after the last.  Returns (block records, kept_index)."""
    block, kept = [], []
    for k, (name, bases) in enumerate(records):
        if k % every == 0:
            block.append((b"dropped%d-%d" % (k, 1000 + k), b"ACGTN"))
        kept.append(len(block))
        block.append((name, bases))
    block.append((b"tail-77", b"GG"))
    return block, np.array(kept, dtype=np.uint32)


def chomped(records):
    return [(M.chomp(n), M.chomp(b)) for n, b in records]


def residue_case():
    """48 records whose offsets take every residue modulo 16 three times over, lengths from the list above (but the longest)"""
    return [(K.ident(k, 1 + k % 4), K.seq(k % 11, LENGTHS[k % (len(LENGTHS) - 1)])) for k in range(48)]


def prefix_case():
    """one read a proper prefix of another, both ways round, next to each other and apart"""
    a = K.seq(3, 40)
    return [(b"a", a), (b"b", a[:39]), (b"c", a[:20]), (b"d", a), (b"e", K.seq(4, 40)), (b"f", a[:39]), (b"g", a[:1])]


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(os.path.join(GOLDEN, "cases.json")))


def golden_cases():
    """the recorded runs, each with its input under "stdin" (cases.json stores an input once, under a key)"""
    g = golden()
    return [dict(c, stdin=g["inputs"][c["input"]]) for c in g["cases"]]


def run_tool(libdir, argv, stdin, env=None, tool=TOOL, timeout=600):
    """the tool through files, -v and -o given: the report then goes to stdout and stderr holds messages only.  Returns (status, report bytes,
    stderr text, output file bytes or None)."""
    e = dict(os.environ)
    if libdir:
        e["LD_LIBRARY_PATH"] = libdir + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    e.update(env or {})
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.fx"), os.path.join(d, "out.fa")
        open(src, "wb").write(stdin)
        p = subprocess.run([tool] + list(argv) + ["-v", "-i", src, "-o", dst], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=timeout)
        return p.returncode, p.stdout, p.stderr.decode("latin-1"), (open(dst, "rb").read() if os.path.exists(dst) else None)


def assert_golden_case(libdir, case, env=None):
    """bytes, -v text, status and -- where the pipe's last tools met an empty input -- their messages and no output file"""
    import hashlib
    code, report, err, outfile = run_tool(libdir, case["tool"], case["stdin"].encode("latin-1"), env)
    name = case["name"]
    assert code == case["exit"], (name, code, err)
    assert report == case["report"].encode("latin-1"), (name, report, err)
    assert err == case["stderr"], (name, err)
    if code != 0:
        assert outfile is None, name
        return
    assert len(outfile) == case["len"] and hashlib.md5(outfile).hexdigest() == case["md5"], name
    if "stdout" in case:
        assert outfile == case["stdout"].encode("latin-1"), name


def seeded_clip_input(reads=300000, seed=7):
    """about 300 000 FASTQ reads of 36 bases: an insert from a skewed pool, the adapter, filler; a tenth without the adapter"""
    import random
    rng = random.Random(seed)
    ad = golden()["adapter"].encode()
    letters = b"ACGT"
    pool = [bytes(letters[(b >> (2 * k)) & 3] for k in range(15 + b % 12)) for b in (rng.getrandbits(64) for _ in range(30000))]
    filler = bytes(letters[(b >> (2 * k)) & 3] for b in (rng.getrandbits(80),) for k in range(40))
    out = []
    for i in range(reads):
        ins = pool[int(len(pool) * rng.random() ** 5)]
        b = ((ins + ad) if i % 10 else (ins + filler[:17])) + filler
        out.append(b"@s%d\n%s\n+\n%s\n" % (i, b[:36], b"I" * 36))
    return b"".join(out), ["-a", ad.decode(), "-l", "15", "-c"]
