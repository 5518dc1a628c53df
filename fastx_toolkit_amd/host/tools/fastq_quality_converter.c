/* fastq_quality_converter -- command line, output and -v report of the FASTX-Toolkit tool of that name (behaviour:
 * src/fastq_quality_converter/fastq_quality_converter.c).  No stage runs: the device formatter writes every record's quality line as
 * characters (-a) or as numbers (-n), whatever it came in as (include/fxg.h: fxg_format_opts). */
#include "../fxh_tool.h"

enum { NUMERIC };

static const fxh_option options[] = {
    {'a', FXH_K_FLAG, NUMERIC, 0, NULL, 0, 0, 0, NULL, -1, 0},
    {'n', FXH_K_FLAG, NUMERIC, 1, NULL, 0, 0, 0, NULL, -1, 0},
};
static const fxh_report_line report[] = {
    {FXH_W_ALWAYS, 0, 0, {{"Input: ", FXH_V_IN, 0}, {" reads.\n", FXH_V_NONE, 0}}},
    {FXH_W_ALWAYS, 0, 0, {{"Output: ", FXH_V_OUT, 0}, {" reads.\n", FXH_V_NONE, 0}}},
};
static void configure(const long *v, const char *s, fxg_params *p) { (void)v; (void)s; p->stages = 0; }
static int alt_run(const long *v, FASTX *fx, const fxg_params *p, fxh_totals *tot)
{
    (void)p;
    if (v[NUMERIC]) fx->write_fastq_ascii = 0;      /* the writer was opened as OUTPUT_FASTQ_ASCII_QUAL; -n makes it OUTPUT_FASTQ_NUMERIC_QUAL (the table has one output type per tool) */
    if (fxh_format_opts_available()) return 0;
    return fxh_tool_record_loop(fx, tot, NULL);
}
static const fxh_tool tool = {
    "usage: fastq_quality_converter [-h] [-a] [-n] [-z] [-v] [-i INFILE] [-o OUTFILE]\n"
    "MI355X build of the FASTX-Toolkit quality converter (same flags as FASTX Toolkit 0.0.14).\n\n"
    "   -h          this help\n"
    "   -a          output ASCII quality scores (default)\n"
    "   -n          output numeric quality scores\n"
    "   -z          compress output with gzip\n"
    "   -v          verbose report (to stdout if -o is given, else to stderr)\n"
    "   -i INFILE   FASTQ input, default stdin\n"
    "   -o OUTFILE  FASTQ output, default stdout\n\n",
    "an", options, 2, NULL, {0}, NULL, FASTQ_ONLY, OUTPUT_FASTQ_ASCII_QUAL, NULL, configure, report, 2, alt_run,
};
int main(int argc, char *argv[]) { return fxh_tool_main(&tool, argc, argv); }
