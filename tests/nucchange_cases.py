"""fasta_nucleotide_changer: the case generators and checks that the CPU tier (test_nucchange_cpu.py) and the GPU tier (test_gpu_nucchange.py)
share.  A block case is (name, records, mode): records as nucchange_model.block_text takes them, mode "r" (T -> U) or "d" (U -> T).  The
generators write bases over the letters A C G N plus F (the mode's `from` letter) and O (its `to` letter); both modes run every shape."""
import functools
import json
import os
import random
import subprocess
import tempfile

import nucchange_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nuc_changer")
TOOL = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fasta_nucleotide_changer")

LANES = 16                  # FXG_NC_LANES: lanes that share a record
GROUP_RECORDS = 256 // 16   # records a workgroup takes at a time (FXG_BLOCK / FXG_NC_LANES)
TRIP_RECORDS = 2048 * GROUP_RECORDS      # records the whole launch takes a trip (FXG_NC_GRID_MAX workgroups)
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 24997]      # 24 997: the longest read fxg_fastq_index does not flag
RECORDS = [1, 3, 4, 5, 63, 64, 65, GROUP_RECORDS - 1, GROUP_RECORDS, GROUP_RECORDS + 1, 16 * GROUP_RECORDS - 1, 16 * GROUP_RECORDS, 16 * GROUP_RECORDS + 1,
           TRIP_RECORDS - 1, TRIP_RECORDS, TRIP_RECORDS + 1, 2 * TRIP_RECORDS + 1]      # ... of the whole grid (the last one's groups take a second trip, one of them a third)
PLAIN = b"ACGNFGCAFFNACGFAGGCFA"


def golden_cases():
    return json.load(open(os.path.join(GOLDEN, "cases.json")))["cases"]


def galaxy_pairs():
    """(mode, input, expected) of the reference's two Galaxy tests"""
    return [(mode, open(os.path.join(GOLDEN, stem + ".fasta"), "rb").read(), open(os.path.join(GOLDEN, stem + ".out"), "rb").read())
            for stem, mode in (("fasta_nuc_changer1", "r"), ("fasta_nuc_changer2", "d"))]


def letters(pattern, mode):
    """a pattern over A C G N F O as bases of the mode"""
    frm, to, _ = M.MODES[mode]
    return pattern.replace(b"F", bytes([frm])).replace(b"O", bytes([to]))


def pattern_of(n, salt=0):
    return bytes(PLAIN[(i * 7 + salt + i // 21) % len(PLAIN)] for i in range(n)) if n < 4096 else (PLAIN * (n // len(PLAIN) + 1))[salt % 7:][:n]


def fasta(patterns, mode, name=lambda i: b"%d" % i):
    return [(name(i), letters(p, mode)) for i, p in enumerate(patterns)]


def fastq(patterns, mode, name=lambda i: b"q%d" % i, name2=lambda i: b"", qual=lambda i, n: bytes(33 + (i * 5 + k) % 41 for k in range(n))):
    return [(name(i), letters(p, mode), name2(i), qual(i, len(p))) for i, p in enumerate(patterns)]


@functools.lru_cache(maxsize=None)
def block_cases():
    out = []
    for mode in "rd":
        def add(name, records):
            out.append(("%s_%s" % (name, mode), records, mode))
        # read lengths
        for n in LENGTHS:
            pats = [pattern_of(n, 0), b"F" * n, pattern_of(n, 3), b"A" * n, pattern_of(max(n // 2, 1), 5)]
            add("len_%d_fasta" % n, fasta(pats, mode))
            add("len_%d_fastq" % n, fastq(pats, mode))
        # alignment: the first bases line starts at id length + 2, the later ones wherever 37 and 21 bases put them -- every offset modulo 16
        for idlen in range(1, 17):
            add("idlen_%d" % idlen, fasta([pattern_of(37, idlen), b"F" * 21, pattern_of(40, 2)], mode, name=lambda i, k=idlen: (b"%d" % i) * k))
        # shared pieces: one-character ids, 1 to 4 bases, so that up to three records' bases lie in one aligned 16-byte piece
        add("shared_all_from", fasta([b"F" * (1 + i % 4) for i in range(40)], mode, name=lambda i: b"%d" % (i % 10)))
        add("shared_mixed", fasta([(b"FAFC", b"F", b"GF", b"FFN")[i % 4] for i in range(41)], mode, name=lambda i: b"%d" % (i % 10)))
        add("shared_two_bases", fasta([b"FF"] * 37, mode, name=lambda i: b"x"))
        add("shared_fastq", fastq([b"F" * (1 + i % 3) for i in range(23)], mode, name=lambda i: b"", qual=lambda i, n: b"U" * n))
        # record counts each side of the group of a workgroup and of many workgroups
        big = pattern_of(4000)
        for n in RECORDS:
            add("records_%d" % n, fasta([big[(i * 13) % 3900:][:1 + (i * 11) % 45] for i in range(n)], mode))
        add("records_4097_fastq", fastq([pattern_of(1 + (i * 7) % 38, i) for i in range(4097)], mode))
        # where the `from` bytes are
        for n in (1, 5, 16, 17, 33, 150):
            add("all_from_%d" % n, fasta([b"F" * n] * 7, mode))
            add("no_from_%d" % n, fasta([pattern_of(n, 1).replace(b"F", b"C")] * 7, mode))
            add("from_first_only_%d" % n, fasta([b"F" + b"G" * (n - 1)] * 7, mode))
            add("from_last_only_%d" % n, fasta([b"G" * (n - 1) + b"F"] * 7, mode))
        # what must stay: ids, '+' lines and quality lines full of T and U, carriage returns
        add("ids_full_of_t_and_u", fasta([pattern_of(19, i) for i in range(9)], mode, name=lambda i: b"TTUUTUTU"[: 1 + i]))
        add("fastq_lines_full_of_t_and_u", fastq([pattern_of(18 + i, i) for i in range(9)], mode, name=lambda i: b"UTTU" * (1 + i % 3), name2=lambda i: b"TUUT" * (i % 4),
                                                 qual=lambda i, n: (b"TU" * n)[:n]))
        add("crlf_fasta", [(n + b"\r", b + b"\r") for n, b in fasta([pattern_of(15 + i, i) for i in range(8)], mode)])
        add("crlf_fastq", [(n + b"\r", b + b"\r", n2 + b"\r", q + b"\r") for n, b, n2, q in fastq([b"F" * (14 + i) for i in range(8)], mode, name2=lambda i: b"TU")])
        add("cr_then_letters", [(b"a", letters(b"FAF\rFOF", mode)), (b"b", letters(b"GF", mode))])      # chomp cuts at the first CR: what follows it is no base
        # the `to` byte
        base = [pattern_of(20 + i, i) for i in range(6)]
        def with_to(at, pos):
            p = list(base)
            for r in at:
                b = p[r].replace(b"O", b"C")
                k = (0 if pos == "first" else len(b) - 1 if pos == "last" else len(b) // 2)
                p[r] = b[:k] + b"O" + b[k + 1:]
            return p
        add("to_in_record_0", fasta(with_to([0], "mid"), mode))
        add("to_in_last_record", fasta(with_to([5], "mid"), mode))
        add("to_in_two_records", fasta(with_to([4, 2], "mid"), mode))
        add("to_first_position", fasta(with_to([3], "first"), mode))
        add("to_last_position", fasta(with_to([3], "last"), mode))
        add("to_among_all_from", fasta([b"F" * 30, b"F" * 17, b"F" * 9 + b"O" + b"F" * 23, b"F" * 5], mode))
        add("to_fastq", fastq(with_to([1, 4], "last"), mode))
        add("to_in_many_groups", fasta([pattern_of(9, i).replace(b"F", b"C") + (b"O" if i >= 700 else b"A") for i in range(1000)], mode))
        add("to_on_a_second_trip", fasta([b"GFC" if i not in (TRIP_RECORDS + 5, TRIP_RECORDS + 40) else b"GOC" for i in range(TRIP_RECORDS + 100)], mode))
        add("collapsed_ids", fasta([pattern_of(12, i) for i in range(6)], mode, name=lambda i: (b"7-120", b"2-3", b"x", b"9-0", b"a-b-4", b"5- 17")[i]))
        # irregular blocks: a lower-case letter, an X and a byte of 0x80 or above at the first and at the last position of a line
        for tag, byte in (("lower", bytes([M.MODES[mode][0] | 0x20])), ("x", b"X"), ("high", b"\xd4"), ("lower_u", b"u"), ("nul_like", b"\x7f")):
            add("irregular_%s_first" % tag, fasta([b"ACGF" * 5, byte + b"CGF" * 6, b"FF"], mode))
            add("irregular_%s_last" % tag, fasta([b"ACGF" * 5, b"CGF" * 11 + byte, b"FF"], mode))
        add("irregular_fastq", fastq([b"ACGF" * 5, b"CGF" * 6 + b"X", b"FF"], mode))
    return out


def regular_text(nbytes, mode, fmt="fasta", seed=7, collapsed=True):
    """seeded regular input of about nbytes bytes for the mode (no `to` letter): reads of 20 to 60 bases, some ids collapsed"""
    rng = random.Random(seed)
    frm = bytes([M.MODES[mode][0]])
    alphabet = b"ACGN" + frm * 2
    out, size, i = [], 0, 1
    while size < nbytes:
        bases = bytes(rng.choice(alphabet) for _ in range(rng.randint(20, 60)))
        if fmt == "fasta":
            r = b">%d%s\n%s\n" % (i, b"-%d" % rng.randint(1, 30) if collapsed and i % 5 == 0 else b"", bases)
        else:
            r = b"@%d\n%s\n+\n%s\n" % (i, bases, bytes(rng.randint(35, 73) for _ in bases))
        out.append(r)
        size += len(r)
        i += 1
    return b"".join(out)


def run_tool(libdir, argv, stdin, env=None, files=False, timeout=300, tool=TOOL):
    """host/bin/fasta_nucleotide_changer with `libdir` first on the library path (None: the product's own libfxg.so).  files: through -i / -o instead
    of stdin / stdout; "OUT" in argv names the output file.  Returns (status, stdout bytes, stderr text, output file bytes or None)."""
    e = dict(os.environ)
    e.pop("FXH_HOST_PARSE", None)                        # (it would send every input through the record path, which gives the same bytes)
    if libdir:
        e["LD_LIBRARY_PATH"] = libdir + os.pathsep + e.get("LD_LIBRARY_PATH", "")
    e.update(env or {})
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.fa"), os.path.join(d, "out.fa")
        argv = [dst if a == "OUT" else a for a in argv]
        if files:
            open(src, "wb").write(stdin)
            argv = argv + ["-i", src] + ([] if dst in argv else ["-o", dst])
        p = subprocess.run([tool] + argv, input=None if files else stdin, stdin=subprocess.DEVNULL if files else None, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=e, timeout=timeout)
        return p.returncode, p.stdout, p.stderr.decode("latin-1"), (open(dst, "rb").read() if os.path.exists(dst) else None)


def message_of(stderr):
    """the first line of a message on stderr without the program-name prefix and the input's file name"""
    line = stderr.replace("(filename ='-')", "").split("\n")[0]
    return line.split(": ", 1)[1] if ": " in line else line


def assert_tool_case(libdir, case, env=None, tool=TOOL):
    """the tool's bytes, -v report, message and status against the reference's recorded answer"""
    code, out, err, outfile = run_tool(libdir, case["argv"], case["stdin"].encode("latin-1"), env, tool=tool)
    name = case["name"]
    assert code == case["exit"], (name, code, err)
    if case["stdout"] == M.USAGE:
        assert out.startswith(b"usage: fasta_nucleotide_changer") and not err, name
        return
    assert out == case["stdout"].encode("latin-1"), (name, out, err)
    if "outfile" in case:
        assert outfile == case["outfile"].encode("latin-1"), name
    if code == 0:
        assert err == case["stderr"], (name, err)          # the -v report, or nothing
    elif name == "unknown_option":
        assert "invalid option -- 'x'" in err, err
    else:
        assert message_of(err) == message_of(case["stderr"]), (name, err)
