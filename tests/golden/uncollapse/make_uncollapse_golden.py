"""Records tests/golden/uncollapse/cases.json from the reference's fastx_uncollapser.

    python tests/golden/uncollapse/make_uncollapse_golden.py [REFERENCE_TREE]

The reference's fastx_uncollapser.cpp and the three C files of its libfastx are compiled where they lie, into a temporary directory, against
the stand-in headers of tests/compat/uncollapser/gtextutils/ (its FASTA mode uses none of libgtextutils; the stand-ins only have to compile).
Every case below is run through the binary with its input on stdin; argv, stdin, stdout, stderr, the exit status and -- where the case
names an output file with -o -- that file's bytes are written down.  "OUT" in an argv stands for the output file's path.  The usage screen
is recorded as "(usage)": its wording is the reference's own and stays there.  No case gives atoi a number beyond a long, and none runs
the tabular mode (-c), whose tokenizer is libgtextutils'."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))

IDS = ">a-4294967298\nAC\n>b--5\nA\n>c- +3\nN\n>d-2x\nAC\n>e-\nA\n>nodash\nT\n"
PLAIN = ">1-3\nACGT\n>2-1\nGG\n>3-2\nTTN\n"
CASES = [
    ("ids_of_the_issue", [], IDS),
    ("ids_of_the_issue_v", ["-v"], IDS),
    ("plain", [], PLAIN),
    ("plain_v", ["-v"], PLAIN),
    ("plain_v_o", ["-v", "-o", "OUT"], PLAIN),
    ("plain_o", ["-o", "OUT"], PLAIN),
    ("crlf", ["-v"], ">1-2\r\nACGT\r\n>2-1\r\nGG\r\n"),
    ("cr_inside_id_hides_the_count", [], ">a\r-5\nAC\n>b-2\rx\nGT\n"),
    ("no_final_newline", ["-v"], ">1-2\nACGT\n>2-3\nGG"),
    ("n_bases", [], ">1-2\nNNNN\n>2-1\nANCNGNT\n"),
    ("one_base", ["-v"], ">1-3\nA\n"),
    ("one_record_count_1", [], ">only\nACGT\n"),
    ("count_zero", ["-v"], ">a-0\nAC\n>b-00\nGT\n"),
    ("count_negative", ["-v"], ">a--3\nAC\n>b- -2\nGT\n"),
    ("count_plus", [], ">a-+4\nAC\n"),
    ("count_leading_zeros", [], ">a-007\nAC\n"),
    ("count_blanks_and_tabs", [], ">a- \t 2\nAC\n>b-\t3 x\nG\n"),
    ("two_dashes", [], ">1-2-9\nAC\n>x-y-3\nGT\n"),
    ("dash_last", [], ">abc-\nAC\n"),
    ("dash_first", [], ">-3\nAC\n"),
    ("empty_id", ["-v"], ">\nAC\n>\nGT\n"),
    ("id_with_blanks", [], ">read one-2 tail-9\nAC\n"),
    ("digits_then_letters", [], ">a-12abc\nA\n"),
    ("letters_then_digits", [], ">a-x12\nAC\n"),
    ("count_2147483648_wraps_to_1", [], ">a-2147483648\nAC\n"),
    ("count_4294967297_is_1", [], ">a-4294967297\nAC\n"),
    ("ordinal_crosses_9_10_inside_a_record", [], ">a-8\nAC\n>b-4\nGT\n"),
    ("ordinal_crosses_99_100", ["-v"], ">a-98\nA\n>b-3\nC\n>c-1\nG\n"),
    ("count_257", ["-v"], ">a-257\nT\n"),
    ("bases_150", [], ">r-3\n" + "ACGTN" * 30 + "\n"),
    ("mixed_counts", ["-v"], "".join(">%d-%d\n%s\n" % (i, c, "ACGTTGCA"[: 1 + i % 8]) for i, c in enumerate([1, 1, 17, 1, 2, 1, 1, 16, 33, 1, 1, 15]))),
    ("error_fastq_input", [], "@r\nACGT\n+\nIIII\n"),
    ("error_lower_case", ["-v"], ">1-2\nACGT\n>2-2\nacgt\n"),
    ("error_empty_bases", [], ">1-2\nACGT\n>2-2\n\n>3-1\nAC\n"),
    ("error_missing_second_line", [], ">1-2\nACGT\n>2-2\n"),
    ("error_blank_line_between_records", [], ">1-2\nACGT\n\n>2-2\nGG\n"),
    ("error_multi_line_fasta", [], ">1-2\nACGT\nACGT\n"),
    ("error_bad_base", [], ">1-1\nACXT\n"),
    ("error_not_fasta", [], "hello\n"),
    ("error_empty_input", [], ""),
    ("unknown_option", ["-x"], PLAIN),
    ("help", ["-h"], PLAIN),
]


def build(ref, d):
    open(os.path.join(d, "config.h"), "w").close()
    lib = os.path.join(ref, "src", "libfastx")
    defs = ["-DPACKAGE_STRING=\"FASTX Toolkit 0.0.14\"", "-DVERSION=\"0.0.14\""]
    objs = []
    for f in ("fastx", "fastx_args", "chomp"):
        objs.append(os.path.join(d, f + ".o"))
        subprocess.check_call(["gcc", "-O1", "-w"] + defs + ["-I", d, "-I", lib, "-c", os.path.join(lib, f + ".c"), "-o", objs[-1]])
    exe = os.path.join(d, "fastx_uncollapser")
    subprocess.check_call(["g++", "-O1", "-w"] + defs + ["-I", d, "-I", lib, "-I", os.path.join(ROOT, "tests", "compat", "uncollapser"),
                           os.path.join(ref, "src", "fastx_uncollapser", "fastx_uncollapser.cpp")] + objs + ["-o", exe])
    return exe


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FXG_REFERENCE", "/root/reference")
    with tempfile.TemporaryDirectory() as d:
        exe = build(ref, d)
        out = []
        for name, argv, stdin in CASES:
            dst = os.path.join(d, "out.fa")
            if os.path.exists(dst):
                os.unlink(dst)
            p = subprocess.run([exe] + [dst if a == "OUT" else a for a in argv], input=stdin.encode("latin-1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            code = p.returncode if p.returncode >= 0 else 128 - p.returncode
            case = dict(name=name, argv=argv, stdin=stdin, stdout=USAGE if "-h" in argv else p.stdout.decode("latin-1"), stderr=p.stderr.decode("latin-1").replace(d, "TMP"), exit=code)
            if "OUT" in argv:
                case["outfile"] = open(dst, "rb").read().decode("latin-1")
            out.append(case)
        src = os.path.join(HERE, "fasta_uncollapser1.fasta")
        got = subprocess.run([exe, "-i", src], stdout=subprocess.PIPE, check=True).stdout
        assert got == open(os.path.join(HERE, "fasta_uncollapser1.out"), "rb").read(), "the Galaxy pair"
    with open(os.path.join(HERE, "cases.json"), "w") as f:
        json.dump(dict(cases=out), f, indent=1)
        f.write("\n")
    print("%d cases" % len(out))


USAGE = "(usage)"

if __name__ == "__main__":
    main()
