"""Records tests/golden/clip_collapse/cases.json from the reference pipe that fastx_clip_collapser replaces:

    fastx_clipper -a A -l N [-n] [-c|-C] [-M N] [-Q N] | [fastx_trimmer -f F -l L |] fastx_collapser

    python tests/golden/clip_collapse/make_clip_collapse_golden.py [REFERENCE_TREE]

The clipper and the trimmer are oracle/_ref/fxref (the reference's libfastx behind the restated tool loops, `make -C oracle ref`); the collapser is
the reference's own fastx_collapser.cpp compiled with -DHAVE_CXX11=1 into a temporary directory, as tests/golden/collapser/make_collapser_golden.py
does it.  The three run one after the other, each on its predecessor's stdout, all with -v.  Nothing compiled from the reference is kept.
Per case: the input (stored once under a key when cases share it), the three command lines, the fused tool's arguments, md5 and length of the pipe's output (the bytes themselves when small),
the -v texts of the tools that ran to their end joined in pipe order, the last tool's exit status, and the stderr of the tools that met an
empty input (the collapser, and the trimmer before it, when nothing survives the stage before), under the tools' own names.
The inputs are made here from fixed seeds; the variable-length case is searched for until the one-aligner rule (the aligner's query
buffer keeps the tail of a longer read before) changes what the clipper writes against clipping every read in a process of its own."""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "collapser"))
import make_collapser_golden as G  # noqa: E402

FXREF = os.path.join(ROOT, "oracle", "_ref", "fxref")
AD = "CTGTAGGCACCATCAAT"
STORE_WHOLE = 1200


def seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def fastq(recs, q="I"):
    return "".join("@%s\n%s\n+\n%s\n" % (n, b, q * len(b)) for n, b in recs)


def fasta(recs):
    return "".join(">%s\n%s\n" % (n, b) for n, b in recs)


def small_rna(rng, reads, length, inserts, with_n=0.0, ragged=False):
    """reads of `length` bases: an insert from a pool (so that sequences repeat), the adapter, filler; some without the adapter, some with a
    damaged one, some (with_n) holding an N; ragged: cut to a random length afterwards"""
    pool = [seq(rng, rng.randint(14, 30)) for _ in range(inserts)]
    out = []
    for i in range(reads):
        ins = rng.choice(pool)
        kind = rng.random()
        if kind < 0.70:
            b = ins + AD
        elif kind < 0.80:
            a = list(AD)
            a[rng.randrange(len(a))] = rng.choice("ACGT")
            b = ins + "".join(a)
        elif kind < 0.88:
            b = ins + AD[:rng.randint(3, 10)]
        else:
            b = ins + seq(rng, 12)
        b = (b + seq(rng, length))[:length]
        if ragged:
            b = b[:rng.randint(8, length)]
        if rng.random() < with_n:
            k = rng.randrange(len(b))
            b = b[:k] + "N" + b[k + 1:]
        out.append(("r%d" % i, b))
    return out


def ties_input(rng):
    """distinct inserts that end up with counts 1, 2, 3 and 5, several at each, in shuffled order"""
    recs = []
    for count in (1, 2, 3, 5):
        for _ in range(7):
            ins = seq(rng, rng.randint(16, 26))
            recs += [ins + AD + seq(rng, 40)] * count
    rng.shuffle(recs)
    return [("t%d" % i, b[:44]) for i, b in enumerate(recs)]


def ids_input(rng):
    """collapsed FASTA ids of every form, dropped records between the kept ones: the count must be the kept record's own"""
    ins = [seq(rng, 18) for _ in range(4)]
    forms = ["x-5", "x-", "x-0", "x", "7-3", "a-b-4", "x-2000000000", "y-2000000000", "z- 12", "w--3", "v-+6", "x-abc", "1-2-3", "q-4294967297"]
    recs = []
    for k, name in enumerate(forms * 3):
        recs.append((name, ins[k % 4] + AD + seq(rng, 6)))
        if k % 2 == 0:
            recs.append(("drop%d-%d" % (k, 100 + k), seq(rng, 30)))          # no adapter: -c drops it, its count must not leak to a neighbour
        if k % 5 == 0:
            recs.append(("short%d-9" % k, "ACG" + AD))                       # too short after clipping
    return recs


def run(cmd, data):
    p = subprocess.run(cmd, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return p.returncode, p.stdout, p.stderr


def pipe(collapser, clip, trim, q, data):
    """the pipe, tool after tool.  Returns (exit of the last, its stdout, the -v texts of the tools that ran to their end joined, the stderr of
    those that did not -- a tool that meets an empty input -- joined, under the tools' own names)."""
    qa = ["-Q", str(q)] if q != 33 else []
    rc, out, err = run([FXREF, "fastx_clipper", "-v"] + clip + qa, data)
    assert rc == 0, err
    report, failed = err, b""
    if trim is not None:
        rc, out, err = run([FXREF, "fastx_trimmer", "-v"] + trim + qa, out)
        if rc == 0:
            report += err
        else:
            assert out == b"" and err.startswith(b"fxref: Premature End-Of-File"), err
            failed += err.replace(b"fxref:", b"fastx_trimmer:", 1)
    rc, out, err = run([collapser, "-v"] + qa, out)
    if rc == 0:
        report += err
    else:
        failed += err
    return rc, out, report, failed


def n3_input(collapser):
    """a ragged input on which one aligner over the whole run writes something else than an aligner per read"""
    for seed in range(1, 2000):
        rng = random.Random(seed)
        recs = small_rna(rng, 48, 40, 8, ragged=True)
        clip = ["-a", AD, "-l", "5"]
        whole = run([FXREF, "fastx_clipper"] + clip, fastq(recs).encode())[1]
        alone = b"".join(run([FXREF, "fastx_clipper"] + clip, fastq([r]).encode())[1] for r in recs)
        if whole != alone:
            return recs
    raise AssertionError("no seed shows the stale-tail rule")


def cases(collapser):
    R = random.Random
    fixed = small_rna(R(11), 72, 36, 9)
    with_n = small_rna(R(12), 60, 36, 8, with_n=0.2)
    ragged = n3_input(collapser)
    ids = ids_input(R(13))
    ties = ties_input(R(14))
    c = ["-a", AD, "-l", "15", "-c"]
    yield "fastq_c", fastq(fixed), c, None, 33
    yield "fastq_c_trim_1_27", fastq(fixed), c, ["-f", "1", "-l", "27"], 33
    yield "fastq_trim_f3", fastq(fixed), ["-a", AD, "-l", "10"], ["-f", "3"], 33
    yield "fastq_trim_l20", fastq(fixed), ["-a", AD, "-l", "10"], ["-l", "20"], 33
    yield "fasta_c", fasta(fixed), c, None, 33
    yield "fasta_default_adapter", fasta(fixed), [], None, 33
    yield "fastq_C", fastq(fixed), ["-a", AD, "-l", "15", "-C"], None, 33
    yield "fastq_n", fastq(with_n), ["-a", AD, "-l", "15", "-n"], None, 33
    yield "fastq_discards_n", fastq(with_n), ["-a", AD, "-l", "15"], None, 33
    yield "fastq_M8", fastq(fixed), ["-a", AD, "-l", "15", "-M", "8"], None, 33
    yield "fastq_M8_c_trim", fastq(fixed), ["-a", AD, "-l", "15", "-M", "8", "-c"], ["-f", "2", "-l", "22"], 33
    yield "fastq_Q64", fastq(fixed[:30], "h"), c, None, 64
    yield "ragged_n3_fastq", fastq(ragged), ["-a", AD, "-l", "5"], None, 33
    yield "ragged_n3_fasta_trim", fasta(ragged), ["-a", AD, "-l", "5", "-n"], ["-f", "2", "-l", "19"], 33
    yield "fasta_ids_c", fasta(ids), ["-a", AD, "-l", "5", "-c"], None, 33
    yield "fasta_ids_trim", fasta(ids), ["-a", AD, "-l", "5"], ["-f", "1", "-l", "12"], 33
    yield "ties_c", fastq(ties), c, None, 33
    yield "ties_fasta_trim", fasta(ties), c, ["-f", "1", "-l", "16"], 33
    yield "crlf_fasta", fasta(fixed[:24]).replace("\n", "\r\n"), c, None, 33
    yield "all_dropped_c", fastq([("n%d" % i, seq(R(15 + i), 36)) for i in range(12)]), ["-a", AD, "-l", "15", "-c", "-M", "12"], None, 33
    yield "all_dropped_trim_v", fasta([("n%d-3" % i, seq(R(70 + i), 30)) for i in range(8)]), ["-a", AD, "-l", "40"], ["-f", "1", "-l", "10"], 33


def tool_argv(clip, trim, q):
    out = list(clip)
    if trim is not None:
        out += ["-L" if a == "-l" else a for a in trim]
    return out + (["-Q", str(q)] if q != 33 else [])


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FXG_REFERENCE", "/root/reference")
    assert os.path.exists(FXREF), "make -C oracle ref first"
    recorded, inputs = [], {}
    with tempfile.TemporaryDirectory() as d:
        collapser = G.build(ref, d)
        for name, text, clip, trim, q in cases(collapser):
            key = hashlib.md5(text.encode("latin-1")).hexdigest()[:8]          # several cases share an input: it is stored once
            inputs[key] = text
            rc, out, report, err = pipe(collapser, clip, trim, q, text.encode("latin-1"))
            case = dict(name=name, input=key, clipper=clip, trimmer=trim, q=q, tool=tool_argv(clip, trim, q), exit=rc, md5=hashlib.md5(out).hexdigest(), len=len(out),
                        report=report.decode("latin-1"), stderr=err.decode("latin-1"))
            if len(out) <= STORE_WHOLE:
                case["stdout"] = out.decode("latin-1")
            recorded.append(case)
    with open(os.path.join(HERE, "cases.json"), "w") as f:
        json.dump(dict(adapter=AD, inputs=inputs, cases=recorded), f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d bytes of input" % (len(recorded), sum(len(t) for t in inputs.values())))


if __name__ == "__main__":
    main()
