"""Records tests/golden/collapser/cases.json from the reference's fastx_collapser.

    python tests/golden/collapser/make_collapser_golden.py [REFERENCE_TREE]

The reference's fastx_collapser.cpp and the three C files of its libfastx are compiled where they lie, into a temporary directory, with
-DHAVE_CXX11=1 (its std::unordered_map branch, what its own configure picks on every compiler of the last decade) by this machine's g++: the
order of equal counts in the recorded outputs is that libstdc++'s.  Nothing compiled from the reference is kept.
  "cli"   every case below through the binary with its input on stdin: argv, stdin, stdout, stderr, the exit status and -- where the case
          names an output file with -o -- that file's bytes.  "OUT" in an argv stands for the output file's path; the usage screen is
          recorded as "(usage)".
  "abi"   every case of tests/collapse_cases.py (abi_cases, the growth and threshold cases, the seeded case): md5 and length of the
          reference's output for the case's text, and the output itself when it is small."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import collapse_cases as K  # noqa: E402

PLAIN = ">a\nACGT\n>b\nGG\n>c\nACGT\n>d\nTTN\n>e\nACGT\n>f\nGG\n"
COLLAPSED = ">1-3\nACGT\n>2-2\nGG\n>3-1\nTTN\n>x-5\nGG\n"
FASTQ = "@r1-7\nACGT\n+\nIIII\n@r2\nGG\n+r2\nII\n@r3\nACGT\n+\nhhhh\n"
BIG = ">a-2000000000\nAC\n>b-2000000000\nAC\n>c\nGT\n>d\nN\n"
CASES = [
    ("plain", [], PLAIN),
    ("plain_v", ["-v"], PLAIN),
    ("plain_v_o", ["-v", "-o", "OUT"], PLAIN),
    ("plain_o", ["-o", "OUT"], PLAIN),
    ("z_is_ignored", ["-z", "-v"], PLAIN),
    ("collapsed_input_counts", ["-v"], COLLAPSED),
    ("ids_of_the_issue", ["-v"], ">x-5\nA\n>x-\nC\n>x-0\nG\n>x-abc\nT\n>1-2-3\nN\n"),
    ("count_passes_int", ["-v"], BIG),
    ("count_equals_2_32", ["-v"], ">a-2147483647\nAC\n>b-2147483647\nAC\n>c-2\nAC\n>d\nGT\n"),
    ("fastq", ["-v"], FASTQ),
    ("fastq_Q64", ["-v", "-Q", "64"], "@r1\nACGT\n+\nhhhh\n@r2\nACGT\n+\nhhhh\n"),
    ("crlf", ["-v"], ">1\r\nACGT\r\n>2\r\nGG\r\n>3\r\nACGT\r\n"),
    ("no_final_newline", ["-v"], ">1\nACGT\n>2\nGG"),
    ("one_record", ["-v"], ">only\nACGT\n"),
    ("n_bases", [], ">1\nNNNN\n>2\nANCNGNT\n>3\nNNNN\n"),
    ("ties_of_three", [], "".join(">%d\n%s\n" % (i, s) for i, s in enumerate(["AAC", "CCG", "GGT", "AAC", "CCG", "GGT", "TTA", "ACA", "TTA"]))),
    ("bases_150", [], (">r\n" + "ACGTN" * 30 + "\n") * 3 + ">s\n" + "ACGTN" * 29 + "ACGTA\n"),
    ("error_lower_case", ["-v"], ">1\nACGT\n>2\nacgt\n>3\nGG\n"),
    ("error_lower_case_o", ["-o", "OUT"], ">1\nACGT\n>2\nacgt\n>3\nGG\n"),
    ("error_empty_bases", [], ">1\nACGT\n>2\n\n>3\nAC\n"),
    ("error_missing_second_line", [], ">1\nACGT\n>2\n"),
    ("error_blank_line_between_records", [], ">1\nACGT\n\n>2\nGG\n"),
    ("error_multi_line_fasta", [], ">1\nACGT\nACGT\n"),
    ("error_bad_base", [], ">1\nACXT\n"),
    ("error_fastq_quality_length", [], "@r\nACGT\n+\nIII\n"),
    ("error_fastq_quality_value", ["-Q", "64"], "@r\nACGT\n+\nIII!\n"),
    ("error_not_fasta", [], "hello\n"),
    ("error_empty_input", [], ""),
    ("error_empty_input_o", ["-o", "OUT"], ""),
    ("unknown_option", ["-x"], PLAIN),
    ("help", ["-h"], PLAIN),
]
USAGE = "(usage)"


def build(ref, d):
    open(os.path.join(d, "config.h"), "w").close()
    lib = os.path.join(ref, "src", "libfastx")
    defs = ["-DPACKAGE_STRING=\"FASTX Toolkit 0.0.14\"", "-DVERSION=\"0.0.14\"", "-DHAVE_CXX11=1"]
    objs = []
    for f in ("fastx", "fastx_args", "chomp"):
        objs.append(os.path.join(d, f + ".o"))
        subprocess.check_call(["gcc", "-O1", "-w"] + defs + ["-I", d, "-I", lib, "-c", os.path.join(lib, f + ".c"), "-o", objs[-1]])
    exe = os.path.join(d, "fastx_collapser")
    subprocess.check_call(["g++", "-O1", "-w", "-std=c++11"] + defs + ["-I", d, "-I", lib, os.path.join(ref, "src", "fastx_collapser", "fastx_collapser.cpp")] + objs + ["-o", exe])
    return exe


def record_abi(exe, name, text):
    p = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (name, p.stderr)
    ans = dict(md5=hashlib.md5(p.stdout).hexdigest(), len=len(p.stdout))
    if len(p.stdout) <= K.STORE_WHOLE:
        ans["stdout"] = p.stdout.decode("latin-1")
    return ans


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FXG_REFERENCE", "/root/reference")
    with tempfile.TemporaryDirectory() as d:
        exe = build(ref, d)
        cli = []
        for name, argv, stdin in CASES:
            dst = os.path.join(d, "out.fa")
            if os.path.exists(dst):
                os.unlink(dst)
            p = subprocess.run([exe] + [dst if a == "OUT" else a for a in argv], input=stdin.encode("latin-1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            code = p.returncode if p.returncode >= 0 else 128 - p.returncode
            case = dict(name=name, argv=argv, stdin=stdin, stdout=USAGE if "-h" in argv else p.stdout.decode("latin-1"), stderr=p.stderr.decode("latin-1").replace(d, "TMP"), exit=code)
            if "OUT" in argv:
                case["outfile"] = open(dst, "rb").read().decode("latin-1") if os.path.exists(dst) else None      # (None: the run ended before the file was opened)
            cli.append(case)
        abi = {}
        for name, records, fastq, _, _ in K.abi_cases():
            abi[name] = record_abi(exe, name, K.case_text(records, fastq))
        abi["growth"] = record_abi(exe, "growth", K.case_text(K.growth_case()[0]))
        for name, records, _ in K.threshold_cases():
            abi[name] = record_abi(exe, name, K.case_text(records))
        abi["seeded"] = record_abi(exe, "seeded", K.seeded_text())
        # the Galaxy pair: this build reproduces everything but the order of its equal counts (neither does a build with HAVE_CXX11 == 0)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import collapse_model as M
        got = subprocess.run([exe, "-i", os.path.join(HERE, "fasta_collapser1.fasta")], stdout=subprocess.PIPE, check=True).stdout
        assert M.same_up_to_ties(got, open(os.path.join(HERE, "fasta_collapser1.out"), "rb").read()), "the Galaxy pair"
        abi["galaxy"] = record_abi(exe, "galaxy", open(os.path.join(HERE, "fasta_collapser1.fasta"), "rb").read())
    with open(os.path.join(HERE, "cases.json"), "w") as f:
        json.dump(dict(cli=cli, abi=abi), f, indent=1)
        f.write("\n")
    print("%d cli cases, %d abi cases" % (len(cli), len(abi)))


if __name__ == "__main__":
    main()
