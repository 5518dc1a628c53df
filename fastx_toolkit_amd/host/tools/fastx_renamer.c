/* fastx_renamer -- command line, output and -v report of the FASTX-Toolkit tool of that name (behaviour: src/fastx_renamer/fastx_renamer.c).
 * No stage runs: the device formatter writes the records with their output bases (-n SEQ) or their running number (-n COUNT) on both
 * name lines (include/fxg.h: fxg_format_opts). */
#include <err.h>
#include <stdio.h>
#include <string.h>

#include "../fxh_tool.h"

static const fxh_option options[] = {
    {'n', FXH_K_STRING, 0, 0, "[-n] parameter requires an argument value", 0, 0, 0, NULL, -1, 0},
};
static const fxh_report_line report[] = {
    {FXH_W_ALWAYS, 0, 0, {{"Renamed: ", FXH_V_IN, 0}, {" reads.\n", FXH_V_NONE, 0}}},
};
/* strncmp, as the reference compares: "SEQUENCE" and "COUNTER" pass (fastx_renamer.c:87-105) */
static int by_count(const char *s) { return strncmp(s, "SEQ", 3) != 0; }
static void check(const long *v, const char *s)
{
    (void)v;
    if (strncmp(s, "SEQ", 3) != 0 && strncmp(s, "COUNT", 5) != 0) errx(1, "Uknown rename type [-n]: '%s'", s);
}
static int counting;
static unsigned int counter = 1;              /* (fastx_renamer.c:47) */
static void configure(const long *v, const char *s, fxg_params *p)
{
    (void)v;
    p->stages = 0;
    counting = by_count(s);
    fxh_set_output_ids(counting ? FXG_ID_ORDINAL : FXG_ID_SEQUENCE, 1, 1);
}
/* the reference's loop body, for the record path */
static void edit(FASTX *fx)
{
    if (counting) snprintf(fx->name, sizeof fx->name, "%u", counter++);
    else strncpy(fx->name, fx->nucleotides, sizeof fx->name);
    strncpy(fx->name2, fx->name, sizeof fx->name2);
}
static int alt_run(const long *v, FASTX *fx, const fxg_params *p, fxh_totals *tot)
{
    (void)v; (void)p;
    if (fxh_format_opts_available()) return 0;
    return fxh_tool_record_loop(fx, tot, edit);
}
static const fxh_tool tool = {
    "usage: fastx_renamer [-n TYPE] [-h] [-z] [-v] [-i INFILE] [-o OUTFILE]\n"
    "MI355X build of the FASTX-Toolkit sequence renamer (same flags as FASTX Toolkit 0.0.14).\n\n"
    "   -n TYPE     rename type:\n"
    "               SEQ - use the nucleotides sequence as the name (default)\n"
    "               COUNT - use simply counter as the name\n"
    "   -h          this help\n"
    "   -z          compress output with gzip\n"
    "   -v          verbose report (to stdout if -o is given, else to stderr)\n"
    "   -i INFILE   FASTA/Q input, default stdin\n"
    "   -o OUTFILE  FASTA/Q output, default stdout\n\n",
    "n:", options, 1, NULL, {0}, "SEQ", FASTA_OR_FASTQ, OUTPUT_SAME_AS_INPUT, check, configure, report, 1, alt_run,
};
int main(int argc, char *argv[]) { return fxh_tool_main(&tool, argc, argv); }
