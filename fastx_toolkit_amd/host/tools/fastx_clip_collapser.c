/* fastx_clip_collapser -- fastx_clipper | [fastx_trimmer |] fastx_collapser in one process, the reads staying on the device between the chain
 * and the set (the reference's own small-RNA example: clip the adapter, cut to a length, collapse).
 *
 * Not a FASTX-Toolkit program: the reference runs the tools as a shell pipe, the kept reads formatted, piped and parsed again once or twice.
 * Here the engine clips (FXG_STAGE_CLIP) and compacts the kept reads, and fxg_collapse_add_rows copies them into the collapser's set, cut to
 * the trimmer's first .. last base on the way (../fxh_collapse.c), so this tool writes exactly the bytes that
 *     fastx_clipper -a A -l N [-n] [-c|-C] [-M N] [-Q N] -i IN | [fastx_trimmer -f F -l L |] fastx_collapser -o OUT
 * writes (the collapser built with HAVE_CXX11 == 1, as ./fastx_collapser.c), and -v prints the tools' reports one after the other, as the pipe
 * would (each stage's input is its predecessor's output).  The trimmer's -l is spelled -L (the clipper owns -l); the trimmer stage is there
 * only if -f or -L is given.  The clipper's -k and -d and the trimmer's -t / -m are not offered.  Like fastx_clipper the run goes through one
 * aligner in input order.  When no read survives a stage the pipe's next tools meet an empty input: their messages, status 1
 * and no output file, which is what happens here. */
#define _GNU_SOURCE
#include <err.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../fastx_args.h"
#include "../fxh_collapse.h"

const char *usage =
    "usage: fastx_clip_collapser [-h] [-v] [-a ADAPTER] [-l N] [-n] [-c] [-C] [-M N] [-f N] [-L N] [-Q N] [-i INFILE] [-o OUTFILE]\n"
    "One-pass equivalent of  fastx_clipper -a A -l N | [fastx_trimmer -f N -l N |] fastx_collapser  on the MI355X engine.\n\n"
    "   -a ADAPTER  clipper: adapter string, default CCTTAAGG\n"
    "   -l N        clipper: discard sequences shorter than N nucleotides after clipping, default 5\n"
    "   -n          clipper: keep sequences with unknown (N) nucleotides\n"
    "   -c / -C     clipper: discard non-clipped / clipped sequences\n"
    "   -M N        clipper: require a minimum adapter alignment length of N\n"
    "   -f N        trimmer: first base to keep, default 1\n"
    "   -L N        trimmer: last base to keep (the trimmer's -l), default the entire read\n"
    "               (the trimmer stage is present only if -f or -L is given)\n"
    "   -i INFILE   FASTA/Q input, default stdin\n"
    "   -o OUTFILE  collapsed FASTA output, default stdout\n"
    "   -v          verbose report (to stdout if -o is given, else to stderr)\n"
    "   -Q N        ASCII quality offset, default 33\n"
    "Not offered: the clipper's -k and -d, the trimmer's -t and -m.\n\n";

#define MAXLEN (MAX_SEQ_LINE_LENGTH - 1)
static char adapter[100] = "CCTTAAGG";                       /* fastx_clipper.cpp:68 */
static unsigned int clip_min_length = 5;                     /* :69 */
static int keep_n = 0, only_clipped = 0, only_non_clipped = 0, min_adapter = 0;
static int trim_first = 1, trim_last = 0, trim_stage = 0;

static int parse_program_args(int optind_, int optc, char *optarg_)
{
    (void)optind_;
    switch (optc) {
    case 'n': keep_n = 1; return 1;
    case 'c': only_clipped = 1; return 1;
    case 'C': only_non_clipped = 1; return 1;
    default: break;
    }
    if (optarg_ == NULL) errx(1, "[-%c] parameter requires an argument value", optc);
    switch (optc) {
    case 'a': strncpy(adapter, optarg_, sizeof adapter - 1); break;
    case 'l': clip_min_length = (unsigned int)strtoul(optarg_, NULL, 10); break;
    case 'M':
        min_adapter = atoi(optarg_);
        if (min_adapter <= 0) errx(1, "Invalid minimum adapter length (-M %s)", optarg_);
        break;
    case 'f':
        trim_first = (int)strtoul(optarg_, NULL, 10);
        if (trim_first < 1 || trim_first > MAXLEN) errx(1, "Invalid number bases to keep (-f %s)", optarg_);      /* fastx_trimmer.c:66-72 */
        trim_stage = 1;
        break;
    case 'L':
        trim_last = (int)strtoul(optarg_, NULL, 10);
        if (trim_last < 1 || trim_last > MAXLEN) errx(1, "Invalid number bases to keep (-L %s)", optarg_);       /* :74-80 */
        trim_stage = 1;
        break;
    default: errx(1, "Unknown argument (%c)", optc);
    }
    return 1;
}

static void open_writer(FASTX *fx) { fastx_init_writer(fx, get_output_filename(), OUTPUT_FASTA, 0); }

int main(int argc, char *argv[])
{
    static FASTX fastx;
    fxh_collapse_totals tot;
    fxh_totals st;
    fxg_params p;
    fastx_parse_cmdline(argc, argv, "a:l:ncCM:f:L:", parse_program_args);
    fastx_init_reader(&fastx, get_input_filename(), FASTA_OR_FASTQ, ALLOW_N, REQUIRE_UPPERCASE, get_fastq_ascii_quality_offset());
    fxh_default_params(&p, get_fastq_ascii_quality_offset());
    p.stages = FXG_STAGE_CLIP | (trim_stage ? FXG_STAGE_FTRIM : 0u);
    memcpy(p.adapter, adapter, sizeof p.adapter);          /* both are char[100], NUL-terminated */
    p.clip_min_len = clip_min_length;
    p.clip_min_adapter_len = min_adapter;
    p.clip_flags = (only_clipped ? FXG_CLIP_DISCARD_NON_CLIPPED : 0u) | (only_non_clipped ? FXG_CLIP_DISCARD_CLIPPED : 0u) | (keep_n ? FXG_CLIP_KEEP_N : 0u);
    p.ft_first = trim_first;
    p.ft_last = trim_last;
    const int kept_any = fxh_collapse_run_chain(&fastx, &p, open_writer, &tot, &st);
    const int trim_ran = trim_stage && st.output_sequences > 0;      /* on an empty input the trimmer ends before its report, as the collapser does */
    if (verbose_flag()) {
        FILE *rf = get_report_file();
        const unsigned clip_out = st.clip_input - st.clip_too_short - st.clip_no_adapter - st.clip_adapter_found - st.clip_n - st.clip_adapter_only;
        fprintf(rf, "Clipping Adapter: %s\n", adapter);                       /* fastx_clipper.c's report table */
        fprintf(rf, "Min. Length: %d\n", (int)clip_min_length);
        if (only_non_clipped) fprintf(rf, "Clipped reads - discarded.\n");
        if (only_clipped) fprintf(rf, "Non-Clipped reads - discarded.\n");
        fprintf(rf, "Input: %u reads.\n", st.clip_input);
        fprintf(rf, "Output: %u reads.\n", clip_out);
        fprintf(rf, "discarded %u too-short reads.\n", st.clip_too_short);
        fprintf(rf, "discarded %u adapter-only reads.\n", st.clip_adapter_only);
        if (only_clipped) fprintf(rf, "discarded %u non-clipped reads.\n", st.clip_no_adapter);
        if (only_non_clipped) fprintf(rf, "discarded %u clipped reads.\n", st.clip_adapter_found);
        if (!keep_n) fprintf(rf, "discarded %u N reads.\n", st.clip_n);
        if (trim_ran) {                                                        /* fastx_trimmer.c's */
            if (trim_first != 1 || trim_last != 0) fprintf(rf, "Trimming: base %d to %d\n", trim_first, trim_last);
            fprintf(rf, "Input: %zu reads.\n", st.output_reads);
            fprintf(rf, "Output: %zu reads.\n", tot.input_reads);
        }
        if (kept_any) {                                                        /* fastx_collapser.c's */
            fprintf(rf, "Input: %zu sequences (representing %zu reads)\n", tot.input_sequences, tot.input_reads);
            fprintf(rf, "Output: %zu sequences (representing %zu reads)\n", tot.output_sequences, tot.output_reads);
        }
    }
    fflush(NULL);
    if (!kept_any) {       /* the pipe's tools on an empty input (fastx.c:226-228), under their own names */
        if (trim_stage && !trim_ran) fprintf(stderr, "fastx_trimmer: Premature End-Of-File (filename ='-')\n");
        fprintf(stderr, "fastx_collapser: Premature End-Of-File (filename ='-')\n");
        if (!getenv("FXH_SLOW_EXIT")) _exit(1);
        return 1;
    }
    fastx_finish(&fastx);
    /* everything is written and flushed: skip the HIP runtime's exit handlers, as fxh_tool_main does (FXH_SLOW_EXIT=1 takes them, for leak checkers) */
    fflush(NULL);
    if (!getenv("FXH_SLOW_EXIT")) _exit(0);
    return 0;
}
