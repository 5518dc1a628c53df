"""fasta_formatter in Python: the contract of the tool for whole inputs (the reference's loop and its four writers,
src/fasta_formatter/fasta_formatter.cpp:136-201, sequence_writers.h:31-109), and the block form of the engine's fxg_fasta_reflow
(include/fxg.h), which carries one integer from block to block.  Bytes in, bytes out; nothing here reads the reference."""

USAGE = "(usage)"


class Refused(Exception):
    """the block form's precondition: a sequence line with no record open"""


def _wrap(bases, c, w):
    """`bases` of a record whose first c bases are already out, with a '\\n' after every w-th base of the record (w > 0)"""
    out = bytearray()
    p = 0
    while p < len(bases):
        take = min(len(bases) - p, w - (c + p) % w)
        out += bases[p:p + take]
        p += take
        if (c + p) % w == 0:
            out += b"\n"
    return bytes(out)


def write_record(ident, bases, width=0, tabular=False, keep_empty=False):
    """one record through the writer the options pick; None: the reference aborts (substr(1) of an empty id)"""
    if not bases and not keep_empty:
        return b""
    if tabular:
        if not ident:
            return None
        return ident[1:] + (b"\t" + bases if bases else b"") + b"\n"
    out = ident + b"\n"
    if bases:
        if width == 0:
            out += bases + b"\n"
        else:
            out += _wrap(bases, 0, width)
            if len(bases) % width:
                out += b"\n"
    return out


def format_whole(data, width=0, tabular=False, keep_empty=False):
    """(stdout, status): the whole tool on one input.  Status 1 with the output so far where the reference aborts (-t without any header)."""
    out = bytearray()
    ident, bases, first = b"", bytearray(), True
    for line in data.split(b"\n"):
        if not line:
            continue
        if line[:1] == b">":
            if first:
                first = False
            else:
                out += write_record(ident, bytes(bases), width, tabular, keep_empty)
            ident, bases = line, bytearray()
        else:
            bases += line
    last = write_record(ident, bytes(bases), width, tabular, keep_empty)
    if last is None:
        return bytes(out), 1
    return bytes(out + last), 0


def run_argv(argv, stdin):
    """the command line (getopt "i:o:hw:te", files not modelled): (stdout or USAGE, status)"""
    width, tab, keep = 0, False, False
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "--":
            break
        if not a.startswith("-") or a == "-":
            break
        k = 1
        while k < len(a):
            ch = a[k]
            if ch == "h":
                return USAGE, 0
            if ch in "te":
                tab, keep = tab or ch == "t", keep or ch == "e"
                k += 1
                continue
            if ch in "iow":
                if k + 1 < len(a):
                    val = a[k + 1:]
                else:
                    i += 1
                    if i >= len(argv):
                        return b"", 1
                    val = argv[i]
                if ch == "w":
                    width = _atoi(val)
                    if width < 0:
                        return b"", 1
                break
            return b"", 1
        i += 1
    return format_whole(stdin, width, tab, keep)


def _atoi(s):
    s = s.lstrip(" \t\n\v\f\r")
    sign, k = 1, 0
    if s[:1] in ("-", "+"):
        sign, k = (-1 if s[0] == "-" else 1), 1
    v = 0
    while k < len(s) and s[k].isdigit() and s[k].isascii():
        v = v * 10 + int(s[k])
        k += 1
    return sign * v


def reflow_block(text, at_eof, open_in, width=0, tabular=False, keep_empty=False):
    """fxg_fasta_reflow on one block: (out, consumed, open_bases).  Only complete lines count.  open_in: bases already written for the
    record open at the block's start (0: none is open).  A record's terminating '\\n' (or, for an empty record with keep_empty, its whole
    id line) is written when the next header line or the end of input closes it.  Not at end of input, the last header line is not
    consumed while no non-empty sequence line follows it: it closes the record before it and is read again with the next block."""
    nl = text.rfind(b"\n")
    lines = text[:nl + 1].split(b"\n")[:-1] if nl >= 0 else []
    starts, p = [], 0
    for ln in lines:
        starts.append(p)
        p += len(ln) + 1
    consumed = p
    withheld = -1
    if not at_eof:
        for i in range(len(lines) - 1, -1, -1):
            if lines[i][:1] == b">":
                withheld = i
                break
            if lines[i]:
                break
    out = bytearray()
    is_open, c, hdr = open_in > 0, open_in, None

    def close():
        if not is_open:
            return
        if c > 0:
            if width == 0 or tabular or c % width:
                out.extend(b"\n")
        elif keep_empty:
            out.extend((hdr[1:] if tabular else hdr) + b"\n")

    for i, ln in enumerate(lines):
        if not ln:
            continue
        if ln[:1] == b">":
            close()
            if i == withheld:
                return bytes(out), starts[i], 0
            is_open, c, hdr = True, 0, ln
        else:
            if not is_open:
                raise Refused("line %d: a sequence line with no record open" % i)
            if c == 0:
                out.extend((hdr[1:] + b"\t") if tabular else (hdr + b"\n"))
            out.extend(ln if (width == 0 or tabular) else _wrap(ln, c, width))
            c += len(ln)
    if at_eof:
        close()
        return bytes(out), consumed, 0
    return bytes(out), consumed, (c if is_open else 0)


def reflow_chain(data, cuts, width=0, tabular=False, keep_empty=False):
    """the blocks data[0:cuts[0]], ... as a host would chain them: every block starts where the one before was consumed up to"""
    if data and not data.endswith(b"\n"):
        data += b"\n"
    out, pos, carry = bytearray(), 0, 0
    for end in list(cuts) + [len(data)]:
        eof = end == len(data)
        if end <= pos and not eof:
            continue
        o, used, carry = reflow_block(data[pos:end], eof, carry, width, tabular, keep_empty)
        out += o
        pos += used
    return bytes(out)
