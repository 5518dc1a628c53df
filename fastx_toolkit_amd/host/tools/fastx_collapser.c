/* fastx_collapser -- command line, output and -v report of the FASTX-Toolkit tool of that name (behaviour: src/fastx_collapser/fastx_collapser.cpp
 * built with HAVE_CXX11 == 1).  The run itself: ../fxh_collapse.c.  The reference writes through an ostream, not through its record writer: -z is
 * accepted and does nothing, and FASTQ input gives FASTA output. */
#define _GNU_SOURCE
#include <err.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include "../fastx_args.h"
#include "../fxh_collapse.h"

const char *usage =
    "usage: fastx_collapser [-h] [-v] [-i INFILE] [-o OUTFILE]\n"
    "MI355X build of the FASTX-Toolkit collapser (same flags as FASTX Toolkit 0.0.14).\n\n"
    "   [-h]         = this help\n"
    "   [-v]         = report the input and output counts (to stdout if -o is given, else to stderr)\n"
    "   [-i INFILE]  = FASTA/Q input file. default is STDIN.\n"
    "   [-o OUTFILE] = FASTA output file. default is STDOUT.\n\n";

int main(int argc, char *argv[])
{
    static FASTX fastx;
    fxh_collapse_totals tot;
    fastx_parse_cmdline(argc, argv, "", NULL);
    fastx_init_reader(&fastx, get_input_filename(), FASTA_OR_FASTQ, ALLOW_N, REQUIRE_UPPERCASE, get_fastq_ascii_quality_offset());
    fastx_init_writer(&fastx, get_output_filename(), OUTPUT_FASTA, 0);
    fxh_collapse_run(&fastx, &tot);
    if (verbose_flag()) {
        fprintf(get_report_file(), "Input: %zu sequences (representing %zu reads)\n", tot.input_sequences, tot.input_reads);
        fprintf(get_report_file(), "Output: %zu sequences (representing %zu reads)\n", tot.output_sequences, tot.output_reads);
    }
    fastx_finish(&fastx);
    /* everything is written and flushed: skip the HIP runtime's exit handlers, as fxh_tool_main does (FXH_SLOW_EXIT=1 takes them, for leak checkers) */
    fflush(NULL);
    if (!getenv("FXH_SLOW_EXIT")) _exit(0);
    return 0;
}
