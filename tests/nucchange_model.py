"""fasta_nucleotide_changer's contract in Python (reference src/fasta_nucleotide_changer/fasta_nucleotide_changer.c over
src/libfastx/fastx.c:314-404, 440-495), in two forms: the whole input as the tool sees it (run_argv, change_whole), and a block of records as
fxg_bases_change and the formatter behind it see it (Block).  Written from the reference's observable behaviour;
tests/golden/nuc_changer/cases.json holds the reference's recorded answers it is checked against."""
from uncollapse_model import chomp, reads_count

USAGE = "(usage)"
ALPHABET = frozenset(b"ACGTNU")
MODES = {"r": (ord("T"), ord("U"), "DNA-to-RNA"), "d": (ord("U"), ord("T"), "RNA-to-DNA")}
NONE = (1 << 64) - 1
IRR_BASE = 0x10             # FXG_TEXT_IRR_BASE
NEITHER = "Please specify either RNA mode (-r) or DNA mode (-d)"
BOTH = "RNA mode (-r) and DNA mode (-d) can not be used together."


class InputError(Exception):
    """the reference's errx: a message on stderr and status 1, after what was written before it"""


def offender_message(mode, line):
    _, to, name = MODES[mode]
    return "Error: found '%c' nucleotide on line %d. (input should not contain '%c' nucleotides in %s mode)" % (to, line, to, name)


def _quality_ok(qual, nbases, qoffset):
    if len(qual) == nbases:                              # as many characters as bases: ASCII (fastx.c:382-390)
        return all(-15 <= c - qoffset <= 93 for c in qual)
    toks = qual.split()
    if len(toks) != nbases:
        return False
    for t in toks:
        try:
            v = int(t)
        except ValueError:
            return False
        if not -15 <= v <= 93:
            return False
    return True


def records_of(text, qoffset=33):
    """the records of a whole input as the reference's reader takes them (FASTA or FASTQ, upper case, N and U allowed): (name, bases, line number
    after the record) one at a time; raises InputError with a fragment of the reader's message where it exits"""
    if not text:
        raise InputError("Premature End-Of-File")
    fastq = text[:1] == b"@"
    if not fastq and text[:1] != b">":
        raise InputError("unknown file format")
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()                                      # (fgets sees no line behind the last newline)
    lpr, i = (4 if fastq else 2), 0
    while i < len(lines):
        if lines[i][:1] != (b"@" if fastq else b">"):
            raise InputError("Invalid input")           # (the wrong prefix character, or what looks like multi-line FASTA)
        name = chomp(lines[i][1:])
        if i + 1 >= len(lines):
            raise InputError("missing 2nd line (nucleotides)")
        bases = chomp(lines[i + 1])
        if not bases:
            raise InputError("found empty nucleotide sequence")
        if any(c not in ALPHABET for c in bases):
            raise InputError("found invalid nucleotide sequence")
        if fastq:
            if i + 2 >= len(lines):
                raise InputError("missing 3rd line (name-2)")
            if i + 3 >= len(lines):
                raise InputError("missing 4th line (quality)")
            if not _quality_ok(chomp(lines[i + 3]), len(bases), qoffset):
                raise InputError("quality")
        i += lpr
        yield name, bases, i, fastq


def change_whole(text, mode, qoffset=33):
    """(stdout bytes, status, stderr line or fragment or None, input reads, output reads, nucleotides changed)"""
    frm, to, _ = MODES[mode]
    out, reads, changed = [], 0, 0
    try:
        for name, bases, line, fastq in records_of(text, qoffset):
            if to in bases:
                return b"".join(out), 1, offender_message(mode, line), reads, reads, changed
            changed += bases.count(bytes([frm]))
            reads += 1 if fastq else reads_count(name)
            out.append(b">" + name + b"\n" + bases.replace(bytes([frm]), bytes([to])) + b"\n")
    except InputError as e:
        return b"".join(out), 1, str(e), reads, reads, changed
    return b"".join(out), 0, None, reads, reads, changed


def report(mode, reads_in, reads_out, changed):
    return ("Mode: %s\nInput: %d reads.\nOutput: %d reads.\nNucleotides changed: %d\n" % (MODES[mode][2], reads_in, reads_out, changed)).encode()


def run_argv(argv, stdin):
    """the tool on argv (without -i / -o / -z) and stdin: (stdout, report or None, status, stderr line or None).  stdout is USAGE for -h."""
    if "-h" in argv:
        return USAGE, None, 1, None
    qoffset, flags, args = 33, "", list(argv)
    while args:
        a = args.pop(0)
        if a == "-Q":
            qoffset = int(args.pop(0))
        else:
            flags += a[1:]
    if any(c not in "vrd" for c in flags):
        return b"", None, 1, None                        # fastx_args.c's answer to a letter it does not know
    r, d = "r" in flags, "d" in flags
    if not r and not d:
        return b"", None, 1, NEITHER
    if r and d:
        return b"", None, 1, BOTH
    mode = "r" if r else "d"
    out, status, msg, rin, rout, changed = change_whole(stdin, mode, qoffset)
    return out, (report(mode, rin, rout, changed) if "v" in flags and status == 0 else None), status, msg


# ---- the block form ------------------------------------------------------------------------------------------------------------------------
def block_text(records):
    """the text of a block: (name, bases) records are FASTA, (name, bases, name2, quality) records FASTQ; every field is written as it is (a
    trailing CR included) in front of its newline"""
    if records and len(records[0]) == 4:
        return b"".join(b"@" + n + b"\n" + b + b"\n+" + n2 + b"\n" + q + b"\n" for n, b, n2, q in records)
    return b"".join(b">" + n + b"\n" + b + b"\n" for n, b in records)


class Block:
    """what fxg_bases_change leaves of a block and what fxg_fastq_format(out_fasta = 1) then writes"""

    def __init__(self, records, mode):
        frm, to, _ = MODES[mode]
        self.lpr = 4 if records and len(records[0]) == 4 else 2
        self.n = len(records)
        self.changed, self.first_to, self.irregular = 0, NONE, 0
        new, outs = [], []
        for r, rec in enumerate(records):
            bases = chomp(rec[1])
            rest = rec[1][len(bases):]                   # (a CR and what follows it stay as they are)
            self.changed += bases.count(bytes([frm]))
            if to in bases and self.first_to == NONE:
                self.first_to = r
            if any(c not in ALPHABET for c in bases):
                self.irregular = IRR_BASE
            nb = bases.replace(bytes([frm]), bytes([to]))
            new.append(rec[:1] + (nb + rest,) + rec[2:])
            outs.append(b">" + chomp(rec[0]) + b"\n" + nb + b"\n")
        self.text = block_text(records)
        self.rewritten = block_text(new)                 # every `from` byte of every bases line, whatever else the block holds
        self.records_out = self.n if self.first_to == NONE else self.first_to
        self.out = b"".join(outs[:self.records_out])
        self.total_bases = sum(len(chomp(rec[1])) for rec in records)
