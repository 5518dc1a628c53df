"""The barcode splitter's contract restated in Python (no GPU, no reference needed): command line, barcode table, input format, matching,
partition into files and the summary.  tests/test_barcode_cpu.py holds it against the reference script and the recorded goldens; the GPU tier
holds the engine and the tool against it.  classify() is the vectorised form of the matching for large inputs."""
import re

import numpy as np

OPTIONS = [("bcfile", "s"), ("eol", ""), ("bol", ""), ("exact", ""), ("prefix", "s"), ("suffix", "s"), ("quiet", ""), ("partial", "i"),
           ("debug", ""), ("mismatches", "i"), ("help", "")]
_INT = re.compile(rb"^[-+]?_*[0-9][0-9_]*$")


class Outcome:
    """What one run leaves: exit ("ok" = 0, "usage" = 1 with the usage text on stdout, "error" = non-zero), stdout, the stderr lines, the
    output files by name (only when the run got to create them)."""

    def __init__(self):
        self.exit, self.stdout, self.stderr, self.files = "ok", b"", [], {}

    def error_line(self):
        return next((l for l in self.stderr if l.startswith(b"Error:")), None)


def parse_options(argv):
    """Getopt::Long with its default configuration over OPTIONS: '-' or '--', any unique prefix in any letter case, '=value' or the next
    argument.  Returns (values, warnings, ok)."""
    vals, warns, ok = {}, [], True
    args = [a if isinstance(a, bytes) else a.encode() for a in argv]
    i = 0
    while i < len(args):
        a = args[i]
        i += 1
        if a == b"--":
            break
        if not a.startswith(b"-") or a == b"-":
            continue                                        # (non-option arguments stay in @ARGV; the script ignores them)
        body = a[2:] if a.startswith(b"--") else a[1:]
        name, eq, optarg = body.partition(b"=")
        lname = name.lower().decode("latin-1")
        hits = [o for o in OPTIONS if o[0] == lname] or [o for o in OPTIONS if o[0].startswith(lname)]
        if len(hits) != 1:
            if hits:
                warns.append(("Option %s is ambiguous (%s)" % (lname, ", ".join(sorted(h[0] for h in hits)))).encode())
            else:
                warns.append(("Unknown option: %s" % lname).encode())
            ok = False
            continue
        opt, typ = hits[0]
        if not typ:
            if eq:
                warns.append(("Option %s does not take an argument" % opt).encode())
                ok = False
                continue
            vals[opt] = 1
            continue
        if eq:
            arg = optarg
            if arg == b"":
                warns.append(("Option %s requires an argument" % opt).encode())
                ok = False
                continue
        else:
            if i >= len(args):
                warns.append(("Option %s requires an argument" % opt).encode())
                ok = False
                continue
            arg = args[i]
            i += 1
        if typ == "i":
            if not _INT.match(arg):
                warns.append(b'Value "' + arg + (b'" invalid for option %s (number expected)' % opt.encode()))
                ok = False
                if not eq:
                    i -= 1                                  # (pushed back: it is a non-option argument then)
                continue
            vals[opt] = int(arg.replace(b"_", b""))
        else:
            vals[opt] = arg
    return vals, warns, ok


def check_options(vals):
    """The script's own checks, in its order: None or the error line."""
    if "bcfile" not in vals:
        return b"Error: barcode file not specified (use '--bcfile [FILENAME]')"
    if "prefix" not in vals:
        return b"Error: prefix path/filename not specified (use '--prefix [PATH]')"
    bol, eol = vals.get("bol", 0), vals.get("eol", 0)
    if bol == eol:
        return b"Error: can't specify both --eol & --bol" if eol else b"Error: must specify either --eol or --bol"
    if vals.get("partial", 0) < 0:
        return b"Error: invalid for value partial matches (valid values are 0 or greater)"
    mm = 0 if vals.get("exact") else vals.get("mismatches", 1)
    if mm < 0:
        return b"Error: invalid value for mismatches (valid values are 0 or more)"
    p = vals.get("partial", 0)
    if p > mm:
        return b"Error: partial overlap value (%d) bigger than max. allowed mismatches (%d)" % (p, mm)
    return None


def load_table(text, fname, mismatches, partial, eol):
    """Barcode file contents -> (entries [(ident, bases)], BL) or the error line."""
    entries, BL = [], None
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for no, line in enumerate(lines, 1):
        if line.startswith(b"#"):
            continue
        f = line.split()                        # (Perl's split ' ': bytes.split() knows the same six whitespace bytes)
        ident = f[0] if f else None
        bc = f[1].upper() if len(f) > 1 else b""
        if not re.fullmatch(rb"[AGCT]+", bc):
            return b"Error: bad barcode value (" + bc + b") at barcode file (" + fname + b") line %d" % no
        if not re.fullmatch(rb"[A-Za-z0-9_]+", ident):
            return b"Error: bad identifier value (" + ident + b") at barcode file (" + fname + b") line %d (must be alphanumeric)" % no
        if len(bc) <= mismatches:
            return (b"Error: badcode(" + ident + b", " + bc + b") is shorter or equal to maximum number of mismatches (%d). "
                    b"This makes no sense. Specify fewer  mismatches." % mismatches)
        if BL is None:
            BL = len(bc)
        if len(bc) != BL:
            return b"Error: found barcodes in different lengths. this feature is not supported yet."
        entries.append((ident, bc))
        for _ in range(partial):
            bc = bc[:-1] if eol else bc[1:]
            entries.append((ident, bc))
    return entries, (BL or 0)


def mismatches_of(frag, bases, BL):
    """The reference's count for one window and one entry (the XOR of two strings counts NUL bytes)."""
    F = len(frag)
    eq = sum(1 for i in range(min(F, len(bases))) if frag[i] == bases[i])
    nul = sum(1 for i in range(len(bases), F) if frag[i] == 0)
    return F - eq - nul + (BL - len(bases))


def window(seq, BL, eol):
    F = min(BL, len(seq))
    return seq[len(seq) - F:] if eol else seq[:F]


def match(seq, entries, BL, mismatches, eol):
    """ident of the entry the bases line `seq` (without its '\\n') goes to, or b'unmatched'."""
    frag = window(seq, BL, eol)
    best, ident = BL, None
    for e_ident, bases in entries:
        mm = mismatches_of(frag, bases, BL)
        if mm < best:
            best, ident = mm, e_ident
    return ident if ident is not None and best <= mismatches else b"unmatched"


def bins_of(entries):
    """Bin numbering of the engine: distinct identifiers in order of first appearance, `unmatched` last (an identifier spelled so shares it)."""
    names = []
    for ident, _ in entries:
        if ident != b"unmatched" and ident not in names:
            names.append(ident)
    names.append(b"unmatched")
    return names


def records(data, lpr):
    """(complete records as lists of lines with their '\\n', error line or None)"""
    lines = data.split(b"\n")
    tail = lines.pop()                          # b"" when the data ends in '\n'
    lines = [l + b"\n" for l in lines] + ([tail] if tail else [])
    n = len(lines) // lpr
    recs = [lines[lpr * k:lpr * k + lpr] for k in range(n)]
    extra = len(lines) - lpr * n
    err = None
    if extra:
        err = [None, b"Error: bad input file, expecting line with sequences", b"Error: bad input file, expecting line with sequence name2",
               b"Error: bad input file, expecting line with quality scores"][extra]
    return recs, err


def run(argv, stdin, read_file):
    """One run of the tool.  read_file(name) -> bytes or None (cannot be opened).  Output file names are the prefix + ident + suffix bytes."""
    o = Outcome()
    if not argv:
        o.exit = "usage"
        return o
    vals, warns, ok = parse_options(argv)
    o.stderr += warns
    if vals.get("help"):
        o.exit = "usage"
        return o
    err = check_options(vals)
    if err:
        o.stderr.append(err)
        o.exit = "error"
        return o
    if not ok:
        return o
    mm = 0 if vals.get("exact") else vals.get("mismatches", 1)
    partial, eol = vals.get("partial", 0), bool(vals.get("eol"))
    text = read_file(vals["bcfile"])
    if text is None:
        o.stderr.append(b"Error: failed to open barcode file (" + vals["bcfile"] + b")")
        o.exit = "error"
        return o
    t = load_table(text, vals["bcfile"], mm, partial, eol)
    if isinstance(t, bytes):
        o.stderr.append(t)
        o.exit = "error"
        return o
    entries, BL = t
    debug = bool(vals.get("debug"))
    if debug:
        o.stderr.append(b"barcode\tsequence")
        o.stderr += [i + b"\t" + b for i, b in entries]
    first = stdin[:1]
    if first not in (b">", b"@"):
        o.stderr.append(b"Error: unknown file format. First character = '" + first + b"' (expecting > or @)")
        o.exit = "error"
        return o
    fastq = first == b"@"
    if debug:
        o.stderr.append(b"Detected FASTQ format" if fastq else b"Detected FASTA format")
    prefix, suffix = vals["prefix"], vals.get("suffix", b"")
    names = bins_of(entries)
    fname = {n: prefix + n + suffix for n in names}
    counts = {n: 0 for n in names}
    o.files = {fname[n]: b"" for n in names}
    out = {n: [] for n in names}
    recs, err = records(stdin, 4 if fastq else 2)
    for rec in recs:
        seq = rec[1][:-1] if rec[1].endswith(b"\n") else rec[1]
        ident = match(seq, entries, BL, mm, eol)
        if debug:
            o.stderr.append(b"sequence " + seq + b": ")
            o.stderr.append(b"sequence " + seq + b" matched barcode: " + ident)
        counts[ident] += 1
        out[ident].append(rec[0] + seq + b"\n" + b"".join(rec[2:]))
    for n in names:
        o.files[fname[n]] = b"".join(out[n])
    if err:
        o.stderr.append(err)
        o.exit = "error"
        return o
    if not vals.get("quiet"):
        lines = [b"Barcode\tCount\tLocation\n"]
        lines += [n + b"\t%d\t" % counts[n] + fname[n] + b"\n" for n in sorted(names)]
        lines.append(b"total\t%d\n" % sum(counts.values()))
        o.stdout = b"".join(lines)
    return o


# ---- the vectorised matching (numpy) -------------------------------------------------------------------------------------------------
def classify(win, F, tab, tab_len, tab_bin, BL, mismatches, unmatched):
    """Bins of many windows at once.  win: uint8 (n, W >= BL) with window r in win[r, :F[r]]; tab: uint8 (E, >= BL) entry bases, tab_len
    their lengths, tab_bin their bins.  The reference's choice: first entry with the fewest mismatches, if fewer than BL and <= mismatches."""
    n = win.shape[0]
    F = np.asarray(F, dtype=np.int64)
    pos = np.arange(BL)[None, :]
    inF = pos < F[:, None]
    w = win[:, :BL]
    isnul = (w == 0) & inF
    best = np.full(n, BL, dtype=np.int64)
    out = np.full(n, unmatched, dtype=np.int64)
    for k in range(len(tab_len)):
        Le = int(tab_len[k])
        eq = ((w[:, :Le] == tab[k, :Le][None, :]) & inF[:, :Le]).sum(1)
        nul = isnul[:, Le:].sum(1)
        mm = F - eq - nul + (BL - Le)
        upd = mm < best
        best[upd] = mm[upd]
        out[upd] = tab_bin[k]
    out[best > mismatches] = unmatched
    return out


def split_block(data, lpr, tab_bases, tab_bin, BL, mismatches, eol, bins):
    """What fxg_barcode_split returns for a block of complete records (each line '\\n'-terminated): (rec_bin, bin_bytes, bin_records, out)."""
    recs, err = records(data, lpr)
    assert err is None
    n = len(recs)
    W = max(BL, 1)
    win = np.zeros((n, W), dtype=np.uint8)
    F = np.zeros(n, dtype=np.int64)
    for r, rec in enumerate(recs):
        f = window(rec[1][:-1], BL, eol)
        F[r] = len(f)
        win[r, :len(f)] = np.frombuffer(f, dtype=np.uint8)
    E = len(tab_bases)
    tab = np.zeros((max(E, 1), W), dtype=np.uint8)
    tl = np.zeros(max(E, 1), dtype=np.int64)
    for k, b in enumerate(tab_bases):
        tab[k, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        tl[k] = len(b)
    rb = classify(win, F, tab, tl[:E], np.asarray(tab_bin, dtype=np.int64), BL, mismatches, bins - 1) if n else np.zeros(0, dtype=np.int64)
    parts = [[] for _ in range(bins)]
    for r, rec in enumerate(recs):
        parts[rb[r]].append(b"".join(rec))
    bb = np.array([sum(len(x) for x in p) for p in parts], dtype=np.uint64)
    br = np.array([len(p) for p in parts], dtype=np.uint64)
    return rb, bb, br, b"".join(b"".join(p) for p in parts)
