/* fastx_uncollapser -- command line, output and -v report of the FASTX-Toolkit tool of that name (behaviour: src/fastx_uncollapser/fastx_uncollapser.cpp,
 * its FASTA mode).  The run itself: ../fxh_uncollapse.c.  The tabular mode (-c N) is not built: its tokenizer is libgtextutils' (INTEGRATION.md section 1). */
#define _GNU_SOURCE
#include <err.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include "../fastx_args.h"
#include "../fxh_uncollapse.h"

const char *usage =
    "usage: fastx_uncollapser [-c N] [-h] [-v] [-i INFILE] [-o OUTFILE]\n"
    "MI355X build of the FASTX-Toolkit uncollapser (same flags as FASTX Toolkit 0.0.14; -c is not supported).\n\n"
    "   [-h]         = this help\n"
    "   [-v]         = report the input and output counts (to stdout if -o is given, else to stderr)\n"
    "   [-c N]       = tabular input with the collapsed identifier on column N: NOT SUPPORTED by this build\n"
    "   [-i INFILE]  = FASTA input file. default is STDIN.\n"
    "   [-o OUTFILE] = FASTA output file. default is STDOUT.\n\n";

static int parse_program_args(int optind_, int optc, char *optarg_)
{
    (void)optind_; (void)optarg_;
    if (optc == 'c') errx(1, "tabular input [-c N] is not supported by this build: only collapsed FASTA is uncollapsed");
    errx(1, "Internal error: unknown option '%c'", optc);
    return 1;
}

int main(int argc, char *argv[])
{
    static FASTX fastx;
    fxh_totals tot;
    fastx_parse_cmdline(argc, argv, "c:", parse_program_args);
    fastx_init_reader(&fastx, get_input_filename(), FASTA_ONLY, ALLOW_N, REQUIRE_UPPERCASE, get_fastq_ascii_quality_offset());
    fastx_init_writer(&fastx, get_output_filename(), OUTPUT_SAME_AS_INPUT, compress_output_flag());
    fxh_uncollapse_run(&fastx, &tot);
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
