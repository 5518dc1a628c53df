"""fastx_collapser: the case generators and checks that the CPU tier (test_collapse_cpu.py), the GPU tier (test_gpu_collapse.py) and the recorder
of the reference's answers (golden/collapser/make_collapser_golden.py) share.  A case is a list of (name, bases) records; its expected output
is what the reference wrote for its text -- stored whole in cases.json when small, as md5 and length otherwise -- because the order of equal
counts is libstdc++'s and nothing here restates it."""
import functools
import hashlib
import json
import os
import random
import subprocess
import tempfile

import collapse_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "collapser")
TOOL = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fastx_collapser")

WG = 256                    # records a workgroup of the insert launch takes (FXG_BLOCK)
TRIP = 2048 * 16            # records a trip of the copy launch takes (FXG_CL_GRID_MAX workgroups of 16 groups)
LONGEST = 24997             # bases: the longest line fxg_fastq_index accepts
LENGTHS = [1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 150, 255, 256, LONGEST]          # every len & 7 tail of the hash, every piece boundary of the compare
REHASH = [13, 14, 29, 30, 59, 60, 127, 128, 257, 258, 541, 542, 1109, 1110]    # distinct sequences each side of libstdc++'s rehash sizes
STORE_WHOLE = 700           # outputs up to this many bytes are recorded whole
DEFAULT_SLOTS = 1 << 16


def seq(i, n):
    """sequence number i of length n: distinct for distinct i as long as 4^n > i (the first bases spell i in base 4), the rest a fixed mix with N"""
    out = bytearray(n)
    for k in range(n):
        if k < 12:
            out[k] = b"ACGT"[(i >> (2 * k)) & 3]
        else:
            out[k] = b"ACGTNTGCAAGCTNNACGTAGGCTA"[(k * 7 + i + k // 25) % 25]
    return bytes(out)


def ident(i, count=None):
    """an id whose width runs through 1 .. 16 and more, so that bases lines start at every offset modulo 16"""
    name = b"r" * (i % 17) + b"%d" % i
    return name if count is None else name + b"-%d" % count


def _lengths_case(L):
    a = seq(5, L)
    first = (b"C" if a[:1] != b"C" else b"G") + a[1:]
    last = a[:-1] + (b"C" if a[-1:] != b"C" else b"G")
    seqs = [a, first, last, a, last, a]
    if L > 1:
        seqs += [a[:-1], a[:-1]]                     # a proper prefix, twice
    return [(ident(k, [None, 3, 1, 7][k % 4]), s) for k, s in enumerate(seqs)]


def _dups_case():
    """1 500 records of 36 bases: equal reads in neighbouring lanes, within a wave, across the waves of a workgroup, across workgroups, and --
    added as 2 or 5 blocks -- across blocks"""
    recs = []
    for i in range(1500):
        key = i // 2 if i < 200 else (i - 200) % 50 if i < 600 else i % 257 if i < 1200 else i
        recs.append((ident(i, 1 + i % 3 if i % 5 == 0 else None), seq(key, 36)))
    return recs


def _counts_case():
    ids = [b"x-5", b"x-", b"x-0", b"x-abc", b"1-2-3", b"nodash", b"x- 7", b"x--4", b"x-+9"]
    recs = [(n, seq(k % 4, 20)) for k, n in enumerate(ids)]
    recs += [(b"a-2000000000", seq(100, 21))] * 2                       # passes 2^31: prints -294967296
    recs += [(b"b-1073741824", seq(101, 22))] * 4                       # equals 2^32: prints 0
    recs += [(b"c-1073741824", seq(102, 23))] * 5                       # passes 2^32: prints 1073741824
    recs += [(b"w-%d" % c, seq(200 + k, 24)) for k, c in enumerate([5, 50, 500, 5000, 50000, 500000, 5000000, 50000000, 500000000, 2000000000])]
    return recs


def _ties_case():
    recs, k = [], 0
    for count, members in ((9, 4), (5, 3), (2, 5), (1, 6)):
        for _ in range(members):
            recs += [(ident(k), seq(k, 30))] * count
            k += 1
    rng = random.Random(11)
    order = sorted(range(len(recs)), key=lambda _: rng.random())
    return [recs[j] for j in order]


def _growth_blocks():
    """block sizes that double the distinct sequences: from 4 slots the table reaches 4 096 through ten rebuilds (8, 16, ... 4 096)"""
    return [1, 1] + [1 << k for k in range(1, 11)]


@functools.lru_cache(maxsize=None)
def seeded_text(reads=300000, templates=40000, seed=2026):
    """a small-RNA-like mix: reads of 36 to 50 bases drawn from `templates` templates with a skewed draw (a few carry most reads)"""
    rng = random.Random(seed)
    pool = []
    for t in range(templates):
        n = 36 + int(rng.random() * 15)
        bits = rng.getrandbits(2 * n)
        pool.append(bytes(b"ACGT"[(bits >> (2 * k)) & 3] for k in range(n)))
    out = []
    for i in range(reads):
        u = rng.random()
        t = int(templates * u ** 6)                  # u^6: a tenth of the templates carries two thirds of the reads
        out.append(b">%d\n%s\n" % (i + 1, pool[t]))
    return b"".join(out)


@functools.lru_cache(maxsize=None)
def abi_cases():
    """[(name, records, fastq, ways, opts)]: `ways` the block counts the case is added in, opts (initial_slots, hash_bits) variants"""
    plain = ((0, 0),)
    out = []
    for L in LENGTHS:
        out.append(("len_%d" % L, _lengths_case(L), False, (1,), plain))
    out.append(("dups", _dups_case(), False, (1, 2, 5), ((0, 0), (0, 1), (0, 4), (4, 0))))
    out.append(("all_identical", [(ident(i), seq(7, 36)) for i in range(3 * WG + 1)], False, (1, 2), ((0, 0), (0, 1))))
    out.append(("all_unique", [(ident(i), seq(i, 36)) for i in range(1000)], False, (1, 5), ((0, 0), (0, 4))))
    for n in (WG - 1, WG, WG + 1):
        out.append(("records_%d" % n, [(ident(i), seq(i % 200, 18)) for i in range(n)], False, (1,), plain))
    for n in (TRIP - 1, TRIP, TRIP + 1):
        out.append(("records_%d" % n, [(b"%d" % i, seq(i % 5003, 36)) for i in range(n)], False, (1,), plain))
    out.append(("counts", _counts_case(), False, (1, 2), plain))
    out.append(("fastq", [(b"q%d-9" % i, seq(i % 7, 25 + i % 3)) for i in range(40)], True, (1, 2), plain))
    out.append(("ties", _ties_case(), False, (1, 5), ((0, 0), (0, 1))))
    for U in REHASH:
        out.append(("uniq_%d" % U, [(ident(i), seq(i * 2654435761 % (1 << 24), 22)) for i in range(U)], False, (1,), plain))
    out.append(("crlf", [(b"1-3\r", b"ACGT\r"), (b"2\r-9", b"GG\r"), (b"3-2", b"ACGT")], False, (1,), plain))
    return out


def growth_case():
    """(records, block sizes): 2 048 distinct sequences added in doubling blocks to a table that begins with 4 slots"""
    sizes = _growth_blocks()
    return [(ident(i), seq(i, 24)) for i in range(sum(sizes))], sizes


def threshold_cases(initial=64):
    """[(name, records, block sizes)]: the distinct sequences of the first block at the growth threshold of `initial` slots and one either side"""
    return [("threshold_%d" % n, [(ident(i), seq(i, 24)) for i in range(n + 3)], [n, 3]) for n in (initial // 2 - 1, initial // 2, initial // 2 + 1)]


def slots_after(initial, uniques_before_and_sizes):
    """the documented growth rule (include/fxg.h): before a block of n records goes in, the table holds at least 2 x (uniques so far + n) slots,
    reached by doubling.  [(uniques before the block, n)] -> (slots, rebuilds)"""
    slots, rebuilds = max(4, initial or DEFAULT_SLOTS), 0
    while slots & (slots - 1):
        slots += 1
    for u, n in uniques_before_and_sizes:
        if n and slots < 2 * (u + n):
            while slots < 2 * (u + n):
                slots *= 2
            rebuilds += 1
    return slots, rebuilds


def split(records, ways):
    """the records in `ways` consecutive blocks of nearly equal size (no empty one)"""
    ways = min(ways, len(records))
    return [records[len(records) * k // ways:len(records) * (k + 1) // ways] for k in range(ways)]


def split_sizes(records, sizes):
    out, at = [], 0
    for n in sizes:
        out.append(records[at:at + n])
        at += n
    assert at == len(records)
    return out


def case_text(records, fastq=False):
    return M.block_text(records, fastq)


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(os.path.join(GOLDEN, "cases.json")))


def golden_cli():
    return golden()["cli"]


def expected(name):
    """the reference's recorded answer for an ABI case: {"md5", "len"} and "stdout" when it is small"""
    return golden()["abi"][name]


def assert_output(name, out):
    want = expected(name)
    assert len(out) == want["len"], (name, len(out), want["len"])
    if "stdout" in want:
        assert out == want["stdout"].encode("latin-1"), name
    assert hashlib.md5(out).hexdigest() == want["md5"], name


def galaxy_pair():
    """(input, expected) of the reference's Galaxy test"""
    return open(os.path.join(GOLDEN, "fasta_collapser1.fasta"), "rb").read(), open(os.path.join(GOLDEN, "fasta_collapser1.out"), "rb").read()


def irregular_blocks():
    """[(name, records)]: blocks fxg_collapse_add must leave out of the set whole, each with regular records around the bad one"""
    good = [(ident(i), seq(i % 3, 30)) for i in range(40)]
    return [("lower_case", good[:17] + [(b"bad", b"ACGTacgt")] + good[17:]),
            ("lower_case_last_byte", good[:5] + [(b"bad", seq(1, 33)[:-1] + b"t")] + good[5:]),
            ("outside_alphabet", good[:30] + [(b"bad", b"ACGTXACGT")] + good[30:]),
            ("high_byte", good + [(b"bad", b"AC\xe9T")]),
            ("u_is_not_dna", [(b"bad", b"ACGU")] + good),
            ("empty_bases", good[:9] + [(b"bad", b"")] + good[9:])]


# C-ABI refusals: (name, the call, what the message holds).  The calls are made by the tiers' own drivers.
REFUSALS = [
    ("add_before_begin", "no set; fxg_collapse_begin makes one"),
    ("order_before_begin", "no set; fxg_collapse_begin makes one"),
    ("write_before_begin", "no set; fxg_collapse_begin makes one"),
    ("write_before_order", "the set is not ordered; fxg_collapse_order comes first"),
    ("add_after_order", "the set is ordered and takes no more blocks"),
    ("order_after_order", "the set is ordered already"),
    ("lines_per_record_3", "lines_per_record 3; 2 (FASTA) or 4 (FASTQ)"),
    ("null_text", "a null pointer with"),
    ("too_many_lines", "records need more than"),
    ("text_too_long", "text block too large"),
    ("records_do_not_fit", "records do not fit"),
    ("rank_begin_past_end", "rank_begin"),
    ("out_cap_too_small", "needs %d bytes, d_out takes %d"),
    ("hash_bits_65", "hash_bits 65"),
]


def run_tool(libdir, argv, stdin, env=None, files=False, timeout=300):
    """host/bin/fastx_collapser with `libdir` first on the library path (None: the product's own libfxg.so).  files: through -i / -o instead of
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
    """the tool's bytes, -v report, message and status against the reference's recorded answer"""
    code, out, err, outfile = run_tool(libdir, case["argv"], case["stdin"].encode("latin-1"), env)
    name = case["name"]
    assert code == case["exit"], (name, code, err)
    if case["stdout"] == M.USAGE:
        assert out.startswith(b"usage: fastx_collapser") and not err, name
        return
    assert out == case["stdout"].encode("latin-1"), (name, out, err)
    if "outfile" in case:
        # empty after a bad record: the reference opens it before it reads; None: the run ended before that (an empty input)
        assert outfile == (None if case["outfile"] is None else case["outfile"].encode("latin-1")), name
    if code == 0:
        assert err == case["stderr"], (name, err)          # the -v report, or nothing
    else:
        assert err.strip(), name
        if name.startswith("error_"):                       # the record API owns the reference's messages
            first = lambda s: s.replace("(filename ='-')", "").split(": ", 1)[1].split("\n")[0]
            assert first(err) == first(case["stderr"]), (name, err)
