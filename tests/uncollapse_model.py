"""fastx_uncollapser's contract in Python (reference src/fastx_uncollapser/fastx_uncollapser.cpp:73-98 over src/libfastx/fastx.c:314-404,
440-495), in two forms: the whole input as the tool sees it (run_argv, uncollapse_whole), and a block of records window by window as
fxg_fasta_uncollapse sees it (Block).  Written from the reference's observable behaviour; tests/golden/uncollapse/cases.json
holds the reference's recorded answers it is checked against."""
import bisect

USAGE = "(usage)"
BASES = frozenset(b"ACGTN")
SPACE = frozenset(b" \t\n\v\f\r")


def chomp(line):
    """a line as the reference holds it: a C string cut at its first CR or LF (chomp.c:36-41), so a NUL ends it too"""
    for i, c in enumerate(line):
        if c in (0, 10, 13):
            return line[:i]
    return line


def reads_count(name):
    """get_reads_count (fastx.c:475-495): atoi of what follows the first '-' of the id, 1 if there is no dash or the number is not positive.  atoi
    is (int)strtol: blanks, one sign, digits; the long lands in an int, so 4294967298 is 2 (csrc/fxg_text.h: fxg_reads_count keeps 23 digits in
    64 bits and takes the low 32, which is the same number for every input that fits a long)."""
    at = name.find(b"-")
    if at < 0:
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
        v = (v * 10 + s[p] - 48) & 0xFFFFFFFFFFFFFFFF
        p += 1
        k += 1
    v &= 0xFFFFFFFF
    if v >= 1 << 31:
        v -= 1 << 32
    if neg:
        v = -v
    return v if 0 < v < (1 << 31) else 1


def copy_bytes(number, bases):
    return b">%d\n%s\n" % (number, bases)


class InputError(Exception):
    """the reference's errx: a message on stderr and status 1, after what was written before it"""


def records_of(text):
    """the records of a whole input as the reference's reader takes them, one (name, bases) at a time; raises InputError where it exits"""
    if not text:
        raise InputError("Premature End-Of-File")
    if text[:1] == b"@":
        raise InputError("input file is FASTQ, but only FASTA input is allowed")
    if text[:1] != b">":
        raise InputError("unknown file format")
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()                                  # (fgets sees no line behind the last newline)
    i = 0
    while i < len(lines):
        if lines[i][:1] != b">":
            raise InputError("expecting FASTA prefix character '>'")
        name = chomp(lines[i][1:])
        if i + 1 >= len(lines):
            raise InputError("missing 2nd line (nucleotides)")
        bases = chomp(lines[i + 1])
        if not bases:
            raise InputError("found empty nucleotide sequence")
        if any(c not in BASES for c in bases):
            raise InputError("found invalid nucleotide sequence")
        yield name, bases
        i += 2


def uncollapse_whole(text):
    """(stdout bytes, status, input sequences, reads): every record `count` times under a running number from 1 on"""
    out, number, seqs = [], 1, 0
    try:
        for name, bases in records_of(text):
            seqs += 1
            for _ in range(reads_count(name)):
                out.append(copy_bytes(number, bases))
                number += 1
    except InputError:
        return b"".join(out), 1, seqs, number - 1
    return b"".join(out), 0, seqs, number - 1


def report(seqs, reads):
    return ("Input: %d sequences (representing %d reads)\nOutput: %d sequences (representing %d reads)\n" % (seqs, reads, reads, reads)).encode()


def run_argv(argv, stdin):
    """the tool on argv (without -i / -o) and stdin: (stdout, report or None, status).  stdout is USAGE for -h; -c is answered with status 1."""
    if "-h" in argv:
        return USAGE, None, 1
    if any(a.startswith("-c") for a in argv):
        return b"", None, 1
    if any(a not in ("-v",) for a in argv):
        return b"use '-h' for usage information.\n", None, 1        # fastx_args.c's answer to a letter it does not know
    out, status, seqs, reads = uncollapse_whole(stdin)
    return out, (report(seqs, reads) if "-v" in argv and status == 0 else None), status


# ---- the block / window form -----------------------------------------------------------------------------------------------------------
def block_text(records):
    """the text of a block of (name, bases) records"""
    return b"".join(b">" + n + b"\n" + b + b"\n" for n, b in records)


def block_counts(records):
    return [reads_count(chomp(n)) for n, _ in records]


class Block:
    """a block's copies without writing them all out: copy g is copy_of(g); sizes come in closed form, so a count of 2^31 - 1 costs nothing"""

    def __init__(self, records, ordinal_base=0):
        self.bases = [chomp(b) for _, b in records]
        self.counts = block_counts(records)
        self.base = ordinal_base
        self.first = [0]                             # C[r]
        for c in self.counts:
            self.first.append(self.first[-1] + c)
        self.copies = self.first[-1]

    def record_of(self, g):
        return bisect.bisect_right(self.first, g) - 1

    def copy_of(self, g):
        return copy_bytes(self.base + g + 1, self.bases[self.record_of(g)])

    def window(self, copy_begin, out_cap):
        """(copy_end, bytes) of the call: the longest run of whole copies from copy_begin on that fits out_cap; None where the call is refused"""
        if copy_begin > self.copies or self.base + self.copies > (1 << 64) - 1:
            return None
        out, used, g = [], 0, copy_begin
        while g < self.copies:
            c = self.copy_of(g)
            if used + len(c) > out_cap:
                break
            out.append(c)
            used += len(c)
            g += 1
        if g == copy_begin and copy_begin < self.copies:
            return None
        return g, b"".join(out)

    def whole(self):
        out, number = [], self.base + 1
        for bases, count in zip(self.bases, self.counts):
            for _ in range(count):
                out.append(copy_bytes(number, bases))
                number += 1
        return b"".join(out)
