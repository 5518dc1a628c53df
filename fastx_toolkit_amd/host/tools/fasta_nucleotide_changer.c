/* fasta_nucleotide_changer -- command line, checks and -v report of the FASTX-Toolkit tool of that name (behaviour:
 * src/fasta_nucleotide_changer/fasta_nucleotide_changer.c).  The run itself: ../fxh_nucchange.c. */
#define _GNU_SOURCE
#include <err.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include "../fastx_args.h"
#include "../fxh_nucchange.h"

const char *usage =
    "usage: fasta_nucleotide_changer [-h] [-z] [-v] [-i INFILE] [-o OUTFILE] [-r] [-d]\n"
    "MI355X build of the FASTX-Toolkit nucleotide changer (same flags as FASTX Toolkit 0.0.14).\n\n"
    "   [-h]         = this help\n"
    "   [-z]         = compress the output with gzip\n"
    "   [-v]         = report the mode, the read counts and the nucleotides changed\n"
    "                  (to stdout if -o is given, else to stderr)\n"
    "   [-i INFILE]  = FASTA/Q input file. default is STDIN.\n"
    "   [-o OUTFILE] = FASTA output file. default is STDOUT.\n"
    "   [-r]         = DNA-to-RNA mode: T becomes U\n"
    "   [-d]         = RNA-to-DNA mode: U becomes T\n\n";

static int flag_dna_mode, flag_rna_mode;

static int parse_program_args(int optind_, int optc, char *optarg_)
{
    (void)optind_; (void)optarg_;
    switch (optc) {
    case 'd': flag_dna_mode = 1; break;
    case 'r': flag_rna_mode = 1; break;
    default: errx(1, __FILE__ ":%d: Unknown argument (%c)", __LINE__, optc);
    }
    return 1;
}

int main(int argc, char *argv[])
{
    static FASTX fastx;
    fxh_totals tot;
    size_t changed = 0;
    fastx_parse_cmdline(argc, argv, "rd", parse_program_args);
    if (!flag_dna_mode && !flag_rna_mode) errx(1, "Please specify either RNA mode (-r) or DNA mode (-d)");
    if (flag_dna_mode && flag_rna_mode) errx(1, "RNA mode (-r) and DNA mode (-d) can not be used together.");
    fastx_init_reader(&fastx, get_input_filename(), FASTA_OR_FASTQ, ALLOW_N | ALLOW_U, REQUIRE_UPPERCASE, get_fastq_ascii_quality_offset());
    fastx_init_writer(&fastx, get_output_filename(), OUTPUT_FASTA, compress_output_flag());
    fxh_nucchange_run(&fastx, flag_dna_mode, &tot, &changed);
    if (verbose_flag()) {
        fprintf(get_report_file(), "Mode: %s\n", flag_dna_mode ? "RNA-to-DNA" : "DNA-to-RNA");
        fprintf(get_report_file(), "Input: %zu reads.\n", tot.input_reads);
        fprintf(get_report_file(), "Output: %zu reads.\n", tot.output_reads);
        fprintf(get_report_file(), "Nucleotides changed: %zu\n", changed);
    }
    fastx_finish(&fastx);
    /* everything is written and flushed: skip the HIP runtime's exit handlers, as fxh_tool_main does (FXH_SLOW_EXIT=1 takes them, for leak checkers) */
    fflush(NULL);
    if (!getenv("FXH_SLOW_EXIT")) _exit(0);
    return 0;
}
