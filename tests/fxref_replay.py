"""Stand-in for oracle/_ref/fxref (the driver around the real reference libfastx) where it cannot be built: the reference's sources are not
part of this repository, so a clean checkout has no fxref.  answer(argv, stdin) gives what the real driver gave for the same command line
and input -- exit code, stdout, stderr and the `-o` file -- from tests/golden/fxref_answers.xz.  A request that was never recorded fails
the test; nothing is guessed.

Outputs up to INLINE bytes are stored whole.  A longer stdout is stored as its length and SHA-256 and comes back as a Recorded value: a
bytes object that compares equal exactly to bytes of that length and digest, and that can itself be the input of a further request
(requests are keyed by the digest of their input).

    FXREF_RECORD=<dir> python -m pytest tests ...      # where oracle/_ref/fxref exists: run the real driver and keep every answer in <dir>
    python tests/fxref_replay.py <dir> [<dir> ...]      # rewrite tests/golden/fxref_answers.xz from the recorded directories
"""
import hashlib
import json
import lzma
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STORE = os.path.join(HERE, "golden", "fxref_answers.xz")
REAL = os.path.join(ROOT, "oracle", "_ref", "fxref")
INLINE = 4 << 10


class Recorded(bytes):
    """A recorded reference output kept as (length, SHA-256) only."""

    def __new__(cls, n, sha):
        self = super().__new__(cls)
        self.n, self.sha = n, sha
        return self

    def __eq__(self, other):
        if isinstance(other, Recorded):
            return (self.n, self.sha) == (other.n, other.sha)
        if isinstance(other, (bytes, bytearray, memoryview)):
            return len(other) == self.n and hashlib.sha256(other).hexdigest() == self.sha
        return NotImplemented

    def __ne__(self, other):
        eq = self.__eq__(other)
        return eq if eq is NotImplemented else not eq

    __hash__ = None

    def __len__(self):
        return self.n

    def __repr__(self):
        return "<reference output: %d bytes, sha256 %s>" % (self.n, self.sha)

    __str__ = __repr__


def _digest(data):
    return data.sha if isinstance(data, Recorded) else hashlib.sha256(data).hexdigest()


def _key(argv, data):
    """The request: arguments (the -o path replaced, its content is part of the answer) and the digest of the bytes on stdin."""
    args = ["<out>" if i > 0 and argv[i - 1] == "-o" else a for i, a in enumerate(argv)]
    return hashlib.sha256((json.dumps(args) + "\0" + _digest(data)).encode()).hexdigest()[:32]


def _out_path(argv):
    return argv[argv.index("-o") + 1] if "-o" in argv[:-1] else None


def _encode(rc, out, err, ofile):
    inline = len(out) <= INLINE and not isinstance(out, Recorded)
    head = dict(rc=rc, out=len(out), sha=None if inline else _digest(out), err=len(err), ofile=None if ofile is None else len(ofile))
    return json.dumps(head).encode() + b"\n" + (out if inline else b"") + err + (ofile or b"")


def _decode(blob):
    head, body = blob.split(b"\n", 1)
    h = json.loads(head)
    if h["sha"] is None:
        out, body = body[:h["out"]], body[h["out"]:]
    else:
        out = Recorded(h["out"], h["sha"])
    err, ofile = body[:h["err"]], (None if h["ofile"] is None else body[h["err"]:])
    return h["rc"], out, err, ofile


def _record(argv, data, where):
    p = subprocess.run([REAL] + argv, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    o = _out_path(argv)
    ofile = open(o, "rb").read() if o and os.path.exists(o) else None
    os.makedirs(where, exist_ok=True)
    k = _key(argv, data)
    tmp = os.path.join(where, ".%s.%d" % (k, os.getpid()))
    with open(tmp, "wb") as f:
        f.write(_encode(p.returncode, p.stdout, p.stderr, ofile))
    os.replace(tmp, os.path.join(where, k))
    return p.returncode, p.stdout, p.stderr


_answers = None


def _load():
    """The store: one xz stream of records `<key> <length>\n<answer>`."""
    d, raw, i = {}, lzma.decompress(open(STORE, "rb").read()), 0
    while i < len(raw):
        j = raw.index(b"\n", i)
        k, n = raw[i:j].split()
        d[k.decode()] = raw[j + 1:j + 1 + int(n)]
        i = j + 1 + int(n)
    return d


def answer(argv, data=b""):
    """(exit code, stdout, stderr) of `fxref argv` with `data` on stdin; the -o file, if any, is written as the reference wrote it."""
    global _answers
    where = os.environ.get("FXREF_RECORD")
    if where:
        return _record(argv, data, where)
    if _answers is None:
        _answers = _load()
    try:
        blob = _answers[_key(argv, data)]
    except KeyError:
        raise AssertionError("no recorded reference answer for %r with %d bytes on stdin in %s: record it where oracle/_ref/fxref can be "
                             "built (tests/fxref_replay.py)" % (argv, len(data), os.path.relpath(STORE, ROOT))) from None
    rc, out, err, ofile = _decode(blob)
    o = _out_path(argv)
    if o and ofile is not None:
        with open(o, "wb") as f:
            f.write(ofile)
    return rc, out, err


def pack(dirs):
    entries = {}
    for d in dirs:
        for k in os.listdir(d):
            if not k.startswith("."):
                entries[k] = open(os.path.join(d, k), "rb").read()
    raw = []
    for k in sorted(entries):                            # sorted, and re-encoded with this file's INLINE: the same answers make the same file
        blob = _encode(*_decode(entries[k]))
        raw.append(b"%s %d\n%s" % (k.encode(), len(blob), blob))
    tmp = STORE + ".new"
    with open(tmp, "wb") as f:
        f.write(lzma.compress(b"".join(raw), preset=9))
    os.replace(tmp, STORE)
    print("%s: %d answers, %d bytes" % (os.path.relpath(STORE, ROOT), len(entries), os.path.getsize(STORE)))


if __name__ == "__main__":
    pack(sys.argv[1:])
