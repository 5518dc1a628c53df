"""Records tests/golden/reflow/cases.json from the reference's fasta_formatter.

    python tests/golden/reflow/make_reflow_golden.py [REFERENCE_TREE]

The reference's fasta_formatter.cpp is compiled where it lies, into a temporary directory, against the stand-in headers of
tests/compat/gtextutils/ (as tests/test_reflow_cpu.py does); every case below is run through it and its stdout and exit status are
written down.  A status of 134 is the reference's abort (tabular output without any header).  The usage screen is recorded as
"(usage)": its wording is the reference's own and stays there."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))

EXAMPLE = "orph\n>a\nACGT\r\nAC\n\n>b\n>c\nAAA"
CASES = [
    ("example_default", [], EXAMPLE),
    ("example_e", ["-e"], EXAMPLE),
    ("example_t_e", ["-t", "-e"], EXAMPLE),
    ("example_te_joined", ["-te"], EXAMPLE),
    ("example_t", ["-t"], EXAMPLE),
    ("example_w3", ["-w", "3"], EXAMPLE),
    ("example_w3_e", ["-w3", "-e"], EXAMPLE),
    ("example_w0", ["-w", "0"], EXAMPLE),
    ("example_w1", ["-w", "1"], EXAMPLE),
    ("example_t_wins_over_w", ["-w", "2", "-t"], EXAMPLE),
    ("exact_multiple_w3", ["-w", "3"], ">a\nACGTAC\n"),
    ("exact_multiple_w6", ["-w", "6"], ">a\nACGTAC\n>b\nACG\nTAC\nAA\n"),
    ("wider_than_any", ["-w", "100000"], ">a\nACGTAC\nGT\n"),
    ("no_header_w0", ["-w", "0"], "ACGT\nAC\n"),
    ("no_header_w4", ["-w", "4"], "ACGT\nAC\n"),
    ("no_header_e", ["-e"], "ACGT\nAC"),
    ("no_header_t", ["-t"], "ACGT\nAC\n"),
    ("no_header_t_e", ["-t", "-e"], "ACGT\n"),
    ("empty_input", [], ""),
    ("empty_input_e", ["-e"], ""),
    ("empty_input_t", ["-t"], ""),
    ("empty_input_t_e", ["-t", "-e"], ""),
    ("only_newlines", [], "\n\n\n"),
    ("only_newlines_e", ["-e"], "\n\n\n"),
    ("only_headers", [], ">a\n>b\n>c\n"),
    ("only_headers_e", ["-e"], ">a\n>b\n>c"),
    ("only_headers_t_e", ["-t", "-e"], ">a\n>b\n>\n"),
    ("bare_prefix_id", [], ">\nAC\n>\n>\nGT\n"),
    ("crlf", [], ">a\r\nAC\r\nGT\r\n"),
    ("crlf_w2", ["-w", "2"], ">a\r\nAC\r\nGT\r\n"),
    ("lone_cr_line", ["-e"], ">a\n\r\n>b\n"),
    ("nul_and_blanks", ["-w", "4"], ">a b\tc\nAC\x00G T\n\x00\n>z\nac gt\n"),
    ("nul_first_byte", [], ">a\n\x00>x\nAC\n"),
    ("prefix_inside_line", [], ">a\nAC>b\n >c\nGT\n"),
    ("last_line_unterminated", ["-w", "2"], ">a\nACG\n>b\nT"),
    ("orphans_then_header", ["-e"], "AC\nGT\n\n>a\n"),
    ("empty_lines_in_record", ["-w", "5"], ">a\n\nACG\n\n\nTAC\n\nGTA\n"),
    ("negative_width", ["-w", "-1"], ">a\nAC\n"),
    ("width_not_a_number", ["-w", "x"], ">a\nACGT\n"),
    ("width_with_tail", ["-w", "2x"], ">a\nACGT\n"),
    ("unknown_option", ["-v"], ">a\nAC\n"),
    ("help", ["-h"], ">a\nAC\n"),
]


def build(ref, d):
    open(os.path.join(d, "config.h"), "w").close()
    exe = os.path.join(d, "fasta_formatter")
    subprocess.check_call(["g++", "-O1", "-DPACKAGE_STRING=\"FASTX Toolkit 0.0.14\"", "-I", d, "-I", os.path.join(ROOT, "tests", "compat"),
                           os.path.join(ref, "src", "fasta_formatter", "fasta_formatter.cpp"), "-o", exe])
    return exe


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FXG_REFERENCE", "/root/reference")
    with tempfile.TemporaryDirectory() as d:
        exe = build(ref, d)
        out = []
        for name, argv, stdin in CASES:
            p = subprocess.run([exe] + argv, input=stdin.encode("latin-1"), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
            code = p.returncode if p.returncode >= 0 else 128 - p.returncode
            out.append(dict(name=name, argv=argv, stdin=stdin, stdout="(usage)" if "-h" in argv else p.stdout.decode("latin-1"), exit=code))
        for src, argv, want in (("fasta_formatter1.fasta", ["-w", "0"], "fasta_formatter1.out"), ("fasta_formatter1.fasta", ["-w", "60"], "fasta_formatter2.out")):
            got = subprocess.run([exe] + argv + ["-i", os.path.join(HERE, src)], stdout=subprocess.PIPE, check=True).stdout
            assert got == open(os.path.join(HERE, want), "rb").read(), want
    with open(os.path.join(HERE, "cases.json"), "w") as f:
        json.dump(dict(cases=out), f, indent=1)
        f.write("\n")
    print("%d cases" % len(out))


if __name__ == "__main__":
    main()
