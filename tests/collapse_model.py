"""fastx_collapser's contract in Python (reference src/fastx_collapser/fastx_collapser.cpp:112-135 over src/libfastx/fastx.c:314-404, 475-495).
Written from the reference's observable behaviour; tests/golden/collapser/cases.json holds the reference's recorded answers.

The model knows everything but the order of equal counts: that is what libstdc++'s unordered_map gives and is not restated anywhere -- the
recorded outputs carry it, and same_up_to_ties() compares two outputs without it."""

USAGE = "(usage)"
BASES = frozenset(b"ACGTN")
SPACE = frozenset(b" \t\n\v\f\r")
M64 = (1 << 64) - 1


def chomp(line):
    """a line as the reference holds it: a C string cut at its first CR or LF (chomp.c:36-41), so a NUL ends it too"""
    for i, c in enumerate(line):
        if c in (0, 10, 13):
            return line[:i]
    return line


def get_reads_count(name, fastq=False):
    """get_reads_count (fastx.c:475-495): 1 for a FASTQ record; for a FASTA id atoi of what follows its first '-', 1 if there is no dash or the
    number is not positive.  atoi is (int)strtol: blanks, one sign, digits; the long lands in an int."""
    at = name.find(b"-")
    if fastq or at < 0:
        return 1
    s, p = name[at + 1:], 0
    while p < len(s) and s[p] in SPACE:
        p += 1
    neg = False
    if p < len(s) and s[p] in b"+-":
        neg = s[p] == ord("-")
        p += 1
    v, k = 0, 0
    while p < len(s) and 48 <= s[p] <= 57 and k < 23:
        v = (v * 10 + s[p] - 48) & M64
        p += 1
        k += 1
    v &= 0xFFFFFFFF
    if v >= 1 << 31:
        v -= 1 << 32
    if neg:
        v = -v
    return v if 0 < v < (1 << 31) else 1


class InputError(Exception):
    """the reference's errx: a message on stderr, status 1 and -- all output being written after the last read -- nothing on stdout"""


def records_of(text, qoffset=33):
    """the records of a whole input as the reference's reader takes them, (name, bases) at a time; raises InputError where it exits"""
    if not text:
        raise InputError("Premature End-Of-File")
    if text[:1] not in (b">", b"@"):
        raise InputError("unknown file format")
    fastq = text[:1] == b"@"
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()                                  # (fgets sees no line behind the last newline)
    i, lpr = 0, 4 if fastq else 2
    while i < len(lines):
        if lines[i][:1] != (b"@" if fastq else b">"):
            raise InputError("expecting prefix character")
        name = chomp(lines[i][1:])
        if i + 1 >= len(lines):
            raise InputError("missing 2nd line (nucleotides)")
        bases = chomp(lines[i + 1])
        if not bases:
            raise InputError("found empty nucleotide sequence")
        if any(c not in BASES for c in bases):
            raise InputError("found invalid nucleotide sequence")
        if fastq:
            if i + 3 >= len(lines):
                raise InputError("missing 3rd or 4th line")
            qual = chomp(lines[i + 3])
            if len(qual) != len(bases):
                raise InputError("number of quality values doesn't match number of nucleotides")
            if any(not -15 <= c - qoffset <= 93 for c in qual):
                raise InputError("Invalid quality score value")
        yield name, bases
        i += lpr


def is_fastq(text):
    return text[:1] == b"@"


def collapse(records, fastq=False):
    """the multiset: {bases: sum of counts modulo 2^64}, keys in first-occurrence order"""
    sums = {}
    for name, bases in records:
        sums[bases] = (sums.get(bases, 0) + get_reads_count(name, fastq)) & M64
    return sums


def printed(count):
    """a count as the reference prints it: the size_t truncated to int (the printer takes each pair as pair<string,int>)"""
    v = count & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def out_reads(sums):
    """the second number of the -v report's Output line: the printed ints added into a size_t"""
    return sum(printed(c) for c in sums.values()) & M64


def record_text(rank, count, bases):
    return b">%d-%d\n%s\n" % (rank, printed(count), bases)


def output_in_order(sums, order):
    """the output for the sequences in `order` (every key of sums once)"""
    return b"".join(record_text(k + 1, sums[b], b) for k, b in enumerate(order))


def out_bytes(sums):
    """bytes of the whole output: the order does not change them (ranks are 1 .. U whatever it is, and counts go with their sequences...) --
    but a count's width goes with its rank's, so sum both over the sorted counts, which is order-free"""
    counts = sorted(sums.values(), reverse=True)
    by = {}
    for b, c in sums.items():
        by.setdefault(c, []).append(len(b))
    total, rank = 0, 1
    for c in sorted(by, reverse=True):
        for n in by[c]:
            total += 4 + len(str(rank)) + len(str(printed(c))) + n
            rank += 1
    assert len(counts) == rank - 1
    return total


def report(seqs, reads, sums):
    return ("Input: %d sequences (representing %d reads)\nOutput: %d sequences (representing %d reads)\n" % (seqs, reads & M64, len(sums), out_reads(sums))).encode()


def parse_output(out):
    """[(rank, printed count, bases)] of a collapser output"""
    lines = out.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 2 == 1, "not whole two-line records"
    recs = []
    for i in range(0, len(lines) - 1, 2):
        assert lines[i][:1] == b">"
        rank, count = lines[i][1:].split(b"-", 1)
        recs.append((int(rank), int(count), lines[i + 1]))
    return recs


def same_up_to_ties(got, want):
    """the order-free comparison: equal (rank, count) record by record, and within every run of equal counts the same set of sequences"""
    g, w = parse_output(got), parse_output(want)
    if [(r, c) for r, c, _ in g] != [(r, c) for r, c, _ in w]:
        return False
    i = 0
    while i < len(g):
        j = i
        while j < len(g) and g[j][1] == g[i][1]:
            j += 1
        if sorted(b for _, _, b in g[i:j]) != sorted(b for _, _, b in w[i:j]):
            return False
        i = j
    return True


def check_against(text, out, true_counts=True):
    """an output `out` for the input `text` against the model, order of ties aside: ranks 1 .. U, every sequence once with its printed count,
    counts descending by their untruncated sums"""
    sums = collapse(records_of(text), is_fastq(text))
    recs = parse_output(out)
    assert [r for r, _, _ in recs] == list(range(1, len(sums) + 1))
    assert sorted(b for _, _, b in recs) == sorted(sums)
    assert all(c == printed(sums[b]) for _, c, b in recs)
    if true_counts:
        full = [sums[b] for _, _, b in recs]
        assert full == sorted(full, reverse=True)
    assert len(out) == out_bytes(sums)
    return sums


def run_argv(argv, stdin):
    """the tool on argv (without -i / -o) and stdin: (status, input sequences, input reads, sums) -- sums None where the run fails.  -h: USAGE."""
    if "-h" in argv:
        return USAGE
    if any(a not in ("-v", "-z", "-Q", "33", "64") for a in argv):
        return 1, 0, 0, None
    q = int(argv[argv.index("-Q") + 1]) if "-Q" in argv else 33
    try:
        recs = list(records_of(stdin, q))
    except InputError:
        return 1, 0, 0, None
    fq = is_fastq(stdin)
    return 0, len(recs), sum(get_reads_count(n, fq) for n, _ in recs), collapse(recs, fq)


# ---- the block form: what fxg_collapse_add is given ----------------------------------------------------------------------------------------
def block_text(records, fastq=False):
    """the text of a block of (name, bases) records; FASTQ gets a '+' line and a quality line of 'I's"""
    if fastq:
        return b"".join(b"@" + n + b"\n" + b + b"\n+\n" + b"I" * len(chomp(b)) + b"\n" for n, b in records)
    return b"".join(b">" + n + b"\n" + b + b"\n" for n, b in records)


def block_irregular(records):
    """the smallest record of a block that fxg_collapse_add refuses (an empty bases line, a byte outside upper-case A C G T N), or None"""
    for r, (_, b) in enumerate(records):
        b = chomp(b)
        if not b or any(c not in BASES for c in b):
            return r
    return None
