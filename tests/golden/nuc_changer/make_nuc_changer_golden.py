"""Records tests/golden/nuc_changer/cases.json from the reference's fasta_nucleotide_changer.

    python tests/golden/nuc_changer/make_nuc_changer_golden.py [REFERENCE_TREE]

The reference's fasta_nucleotide_changer.c and the three C files of its libfastx are compiled where they lie, into a temporary directory.
Every case below is run through the binary with its input on stdin; argv, stdin, stdout, stderr, the exit status and -- where the case
names an output file with -o -- that file's bytes are written down.  "OUT" in an argv stands for the output file's path.  The usage screen
is recorded as "(usage)": its wording is the reference's own and stays there.  The program-name prefix of a message on stderr is whatever
the binary was called; the tests compare what follows it.  The two Galaxy pairs (fasta_nuc_changer1/2) are copied beside the cases and
checked against the binary here."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))

DNA = ">s1\nACGTTGCA\n>s2\nTTTT\n>s3\nGGNCC\n"
RNA = ">s1\nACGUUGCA\n>s2\nUUUU\n>s3\nGGNCC\n"
DNAQ = "@r1\nACGTT\n+r1\nIIIII\n@r2 TU\nTNTGC\n+TU\nTUTUT\n"
RNAQ = "@r1\nACGUU\n+r1\nIIIII\n@r2 TU\nUNUGC\n+TU\nTUTUT\n"
COLLAPSED = ">1-120\nACGT\n>2-7\nTT\n>3\nGGT\n>x-0\nT\n"
LONG = ">long\n" + "ACGTN" * 30 + "\n>long2\n" + "T" * 33 + "\n"
CASES = [
    ("dna_to_rna", ["-r"], DNA),
    ("dna_to_rna_v", ["-r", "-v"], DNA),
    ("rna_to_dna", ["-d"], RNA),
    ("rna_to_dna_v", ["-d", "-v"], RNA),
    ("dna_to_rna_v_o", ["-r", "-v", "-o", "OUT"], DNA),
    ("rna_to_dna_o", ["-d", "-o", "OUT"], RNA),
    ("fastq_dna_to_rna_v", ["-r", "-v"], DNAQ),
    ("fastq_rna_to_dna_v", ["-d", "-v"], RNAQ),
    ("fastq_numeric_quality", ["-r", "-v"], "@n\nACGT\n+\n40 40 30 2\n@m\nTT\n+\n-5 93\n"),
    ("fastq_q64", ["-r", "-Q", "64"], "@n\nACGT\n+\nhhhh\n"),
    ("collapsed_ids_v", ["-r", "-v"], COLLAPSED),
    ("collapsed_ids_rna_v", ["-d", "-v"], COLLAPSED.replace("T", "U")),
    ("nothing_to_change_v", ["-r", "-v"], ">a\nACGN\n>b\nGGCC\n"),
    ("every_base_changes_v", ["-d", "-v"], ">a\nUUUU\n>b\nU\n"),
    ("ids_full_of_t_and_u", ["-r"], ">TTUUTU T U\nACGT\n>UUU\nTT\n"),
    ("crlf", ["-r", "-v"], ">a\r\nACGT\r\n>b\r\nTT\r\n"),
    ("crlf_fastq", ["-d"], "@a\r\nACGU\r\n+\r\nIIII\r\n"),
    ("no_final_newline", ["-r", "-v"], ">a\nACGT\n>b\nTT"),
    ("one_base", ["-r", "-v"], ">a\nT\n"),
    ("bases_150", ["-r", "-v"], LONG),
    ("n_bases", ["-d"], ">a\nNNNN\n>b\nNUN\n"),
    ("offender_first_record", ["-r"], ">a\nACGU\n>b\nTT\n"),
    ("offender_second_record", ["-r", "-v"], ">a\nACGT\n>b\nTUT\n>c\nAC\n"),
    ("offender_last_record", ["-d"], ">a\nACGU\n>b\nUU\n>c\nACT\n"),
    ("offender_two_records", ["-d"], ">a\nACGU\n>b\nT\n>c\nACT\n"),
    ("offender_first_position", ["-r"], ">a\nTTT\n>b\nUACG\n"),
    ("offender_last_position", ["-r"], ">a\nTTT\n>b\nACGU\n"),
    ("offender_among_from", ["-d"], ">a\nUU\n>b\nUUUTUUU\n>c\nUU\n"),
    ("offender_fastq", ["-d", "-v"], "@a\nACGU\n+\nIIII\n@b\nACGT\n+\nIIII\n"),
    ("offender_fastq_rna", ["-r"], "@a\nACGT\n+\nIIII\n@b\nACGU\n+\nIIII\n@c\nAC\n+\nII\n"),
    ("offender_o", ["-r", "-o", "OUT"], ">a\nACGT\n>b\nTUT\n"),
    ("error_lower_case", ["-r", "-v"], ">a\nACGT\n>b\nacgt\n"),
    ("error_lower_case_t_last", ["-d"], ">a\nACGU\n>b\nACGt\n"),
    ("error_bad_base_first", ["-r"], ">a\nACGT\n>b\nXCGT\n"),
    ("error_bad_base_last", ["-d"], ">a\nACGU\n>b\nACGX\n"),
    ("error_high_byte", ["-r"], ">a\nACGT\n>b\nAC\xe9T\n"),
    ("error_empty_bases", ["-r"], ">a\nACGT\n>b\n\n>c\nAC\n"),
    ("error_missing_second_line", ["-r"], ">a\nACGT\n>b\n"),
    ("error_multi_line_fasta", ["-r"], ">a\nACGT\nACGT\n"),
    ("error_blank_line", ["-d"], ">a\nACGU\n\n>b\nGG\n"),
    ("error_fastq_bad_quality", ["-r"], "@a\nACGT\n+\nIIII\n@b\nACGT\n+\nII\x01I\n"),
    ("error_fastq_short_quality", ["-r"], "@a\nACGT\n+\nIIII\n@b\nACGT\n+\nIII\n"),
    ("error_fastq_wrong_prefix", ["-d"], "@a\nACGU\n+\nIIII\n>b\nACGU\n"),
    ("error_not_fastx", ["-r"], "hello\n"),
    ("error_empty_input", ["-r"], ""),
    ("neither_mode", [], DNA),
    ("both_modes", ["-r", "-d"], DNA),
    ("unknown_option", ["-r", "-x"], DNA),
    ("help", ["-h"], DNA),
]
GALAXY = [("fasta_nuc_changer1", ["-r"]), ("fasta_nuc_changer2", ["-d"])]


def build(ref, d):
    open(os.path.join(d, "config.h"), "w").close()
    lib = os.path.join(ref, "src", "libfastx")
    defs = ["-DPACKAGE_STRING=\"FASTX Toolkit 0.0.14\"", "-DVERSION=\"0.0.14\""]
    srcs = [os.path.join(lib, f + ".c") for f in ("fastx", "fastx_args", "chomp")]
    exe = os.path.join(d, "fasta_nucleotide_changer")
    subprocess.check_call(["gcc", "-O1", "-w"] + defs + ["-I", d, "-I", lib, os.path.join(ref, "src", "fasta_nucleotide_changer", "fasta_nucleotide_changer.c")] + srcs + ["-o", exe])
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
                case["outfile"] = open(dst, "rb").read().decode("latin-1") if os.path.exists(dst) else ""
            out.append(case)
        for stem, argv in GALAXY:
            for ext in (".fasta", ".out"):
                shutil.copyfile(os.path.join(ref, "galaxy", "test-data", stem + ext), os.path.join(HERE, stem + ext))
                os.chmod(os.path.join(HERE, stem + ext), 0o644)
            got = subprocess.run([exe] + argv + ["-i", os.path.join(HERE, stem + ".fasta")], stdout=subprocess.PIPE, check=True).stdout
            assert got == open(os.path.join(HERE, stem + ".out"), "rb").read(), stem
    with open(os.path.join(HERE, "cases.json"), "w") as f:
        json.dump(dict(cases=out), f, indent=1)
        f.write("\n")
    print("%d cases" % len(out))


USAGE = "(usage)"

if __name__ == "__main__":
    main()
