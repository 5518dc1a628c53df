"""Records tests/golden/barcode/cases.json: the reference script's answers (exit status, stdout, stderr, every output file) for the cases
below.  Needs perl and the reference tree; the tests only read the JSON.  Run:  python make_barcode_golden.py REFERENCE_ROOT
Bytes are stored as latin-1 strings; "{P}" stands for the output prefix (a directory of the run's own) and "{B}" for the barcode file; "file:NAME" stands for the contents of a file beside it."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
BC4 = "BC1\tGATCT\nBC2\tATCGT\nBC3\tGTGAT\nBC4 TGTCT\n"
FQ = "@r1\nGATCTAAAA\n+\nIIIIIIIII\n@r2\nATCGTCCCC\n+r2\nIIIIIIIII\n@r3\nTTTTTTTTT\n+\nIIIIIIIII\n@r4\nAAAAGTGAT\n+\n#########\n"
FA = ">r1\nGATCTAAAA\n>r2\nATCGTCCCC\n>r3\nTTTTTTTTT\n>r4\nAAAATGTCT\n"
STD = ["--bcfile", "{B}", "--prefix", "{P}", "--suffix", ".txt"]

CASES = [
    ("fastq_bol", STD + ["--bol"], BC4, FQ),
    ("fastq_eol", STD + ["--eol"], BC4, FQ),
    ("fasta_bol_mm0", STD + ["--bol", "--mismatches", "0"], BC4, FA),
    ("fasta_eol_exact", STD + ["--eol", "--exact"], BC4, FA),
    ("crlf_reads_eol", STD + ["--eol", "--mismatches", "1"], BC4, ">a\r\nCCCCGTGAT\r\n>b\r\nCCCCGTGA\r\n"),
    ("crlf_reads_bol", STD + ["--bol"], BC4, "@a\r\nGATCTAC\r\n+\r\nIIIIIII\r\n"),
    ("crlf_barcode_file", STD + ["--bol"], BC4.replace("\n", "\r\n"), FQ),
    ("nul_bytes_partial", STD + ["--bol", "--partial", "1", "--mismatches", "1"], BC4, ">a\nATCT\x00GG\n>b\nGATC\x00\n>c\n\x00\x00\x00\x00\x00\n"),
    ("short_reads", STD + ["--bol", "--mismatches", "0"], BC4, ">a\nGA\n>b\nG\n>c\nAT\n"),
    ("empty_read", STD + ["--bol"], BC4, "@e\n\n+\n\n@f\nGATCT\n+\nIIIII\n"),
    ("partial_eol_start", STD + ["--eol", "--partial", "1", "--mismatches", "1"], "BC1 GATCT\n", ">a\nCCCCCGATC\n>b\nCCCCGATCT\n>c\nCCCCATCT\n"),
    ("partial_bol", STD + ["--bol", "--partial", "2", "--mismatches", "2"], BC4, ">a\nTCTAAAA\n>b\nCGTCCCC\n>c\nGGGGGGG\n"),
    ("repeated_and_unmatched_ident", STD + ["--bol"], "X AAAAA\nY CCCCC\nX GGGGG\nunmatched TTTTT\n", ">a\nGGGGG\n>b\nTTTTT\n>c\nCCCCC\n>d\nACGTA\n"),
    ("lowercase", STD + ["--bol"], "lo gatct\n", ">a\ngatct\n>b\nGATCT\n>c\nGAtCT\n"),
    ("fasta_no_final_newline", STD + ["--bol"], BC4, ">a\nGATCT\n>b\nATCGT"),
    ("fastq_no_final_newline", STD + ["--bol"], BC4, "@a\nGATCT\n+\nIIIII\n@b\nATCGT\n+\nIIIII"),
    ("incomplete_sequence", STD + ["--bol"], BC4, ">a\nGATCT\n>b\n"),
    ("incomplete_name2", STD + ["--bol"], BC4, "@a\nGATCT\n+\nIIIII\n@b\nATCGT\n"),
    ("incomplete_quality", STD + ["--bol"], BC4, "@a\nGATCT\n+\nIIIII\n@b\nATCGT\n+\n"),
    ("empty_table", STD + ["--bol"], "# nothing\n#at all\n", FQ),
    ("quiet", STD + ["--bol", "--quiet"], BC4, FQ),
    ("debug", STD + ["--bol", "--debug"], BC4, FA),
    ("spellings", ["-BCF={B}", "-pre", "{P}", "--EOL", "--mism=2", "--part", "1"], BC4, FQ),
    ("err_blank_line", STD + ["--bol"], "BC1 GATCT\n\nBC2 ATCGT\n", FQ),
    ("err_one_field", STD + ["--bol"], "BC1\n", FQ),
    ("err_bad_base", STD + ["--bol"], "BC1 GATNT\n", FQ),
    ("err_bad_ident", STD + ["--bol"], "BC-1 GATCT\n", FQ),
    ("err_barcode_too_short", STD + ["--bol", "--mismatches", "2"], "A GA\n", FQ),
    ("err_lengths", STD + ["--bol"], "A GATC\nB GATCT\n", FQ),
    ("err_open_bcfile", ["--bcfile", "{P}missing.txt", "--prefix", "{P}", "--bol"], None, FQ),
    ("err_no_bcfile", ["--prefix", "{P}", "--bol"], BC4, FQ),
    ("err_no_prefix", ["--bcfile", "{B}", "--bol"], BC4, FQ),
    ("err_eol_and_bol", STD + ["--bol", "--eol"], BC4, FQ),
    ("err_neither", STD, BC4, FQ),
    ("err_partial_negative", STD + ["--bol", "--partial", "-1"], BC4, FQ),
    ("err_mismatches_negative", STD + ["--bol", "--mismatches", "-2"], BC4, FQ),
    ("err_partial_too_big", STD + ["--bol", "--partial", "2"], BC4, FQ),
    ("err_format", STD + ["--bol"], BC4, "ACGT\n"),
    ("err_empty_input", STD + ["--bol"], BC4, ""),
    ("getopt_unknown", STD + ["--bol", "--frobnicate"], BC4, FQ),
    ("getopt_ambiguous", ["--bcfile", "{B}", "--p", "{P}", "--bol"], BC4, FQ),
    ("getopt_missing_argument", STD + ["--bol", "--mismatches"], BC4, FQ),
    ("getopt_not_a_number", STD + ["--bol", "--mismatches", "two"], BC4, FQ),
    ("usage_no_arguments", [], BC4, FQ),
    ("usage_help", STD + ["--bol", "--help"], BC4, FQ),
]


def record(ref, name, argv, bc, stdin):
    script = os.path.join(ref, "scripts", "fastx_barcode_splitter.pl")
    with tempfile.TemporaryDirectory() as d:
        P = os.path.join(d, "out") + "/"
        os.makedirs(P)
        B = os.path.join(d, "barcodes.txt")
        if bc is not None:
            open(B, "wb").write(bc.encode("latin-1"))
        args = [a.replace("{B}", B).replace("{P}", P) for a in argv]
        p = subprocess.run(["perl", script] + args, input=stdin.encode("latin-1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        sub = lambda b: b.decode("latin-1").replace(P, "{P}").replace(B, "{B}")
        files = {f: open(os.path.join(P, f), "rb").read().decode("latin-1") for f in sorted(os.listdir(P))}
        lines = [l for l in sub(p.stderr).split("\n") if l]
        stdout = sub(p.stdout)
        if p.returncode == 1 and not stdout.startswith("Barcode\t"):
            stdout = "(usage)"                      # (the usage text itself is not recorded: the tools print their own)
        return {"name": name, "argv": argv, "barcodes": bc, "stdin": stdin, "exit": p.returncode, "stdout": stdout,
                "stderr": [l for l in lines if not l.startswith("Use of uninitialized") and " line " not in l or l.startswith("Error:")],
                "files": files}


def main():
    ref = sys.argv[1]
    out = [record(ref, *c) for c in CASES]
    galaxy = open(os.path.join(HERE, "fastx_barcode_splitter1.txt"), encoding="latin-1").read()
    fq = open(os.path.join(HERE, "fastx_barcode_splitter1.fastq"), encoding="latin-1").read()
    g = record(ref, "galaxy", ["--bcfile", "{B}", "--prefix", "{P}", "--bol", "--mismatches", "2"], galaxy, fq)
    g["barcodes"], g["stdin"] = "file:fastx_barcode_splitter1.txt", "file:fastx_barcode_splitter1.fastq"
    out.append(g)
    json.dump(out, open(os.path.join(HERE, "cases.json"), "w"), indent=1, sort_keys=True)
    print("%d cases" % len(out))


if __name__ == "__main__":
    main()
