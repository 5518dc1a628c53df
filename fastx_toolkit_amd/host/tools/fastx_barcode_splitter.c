/* fastx_barcode_splitter -- command line of the FASTX-Toolkit's scripts/fastx_barcode_splitter.pl (Getopt::Long with its default
 * configuration: '-' or '--', any unique prefix of an option in any letter case, '=value' or the value as the next argument; its complaints,
 * then the script's own checks in its order).  The run itself: ../fxh_split.c. */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include "../fxh_split.h"

static void usage(void)
{
    fputs("usage: fastx_barcode_splitter.pl --bcfile FILE --prefix PREFIX [--suffix SUFFIX] [--bol|--eol]\n"
          "         [--mismatches N] [--exact] [--partial N] [--help] [--quiet] [--debug]\n"
          "MI355X build of the FASTX-Toolkit barcode splitter (same options as FASTX Toolkit 0.0.14).\n"
          "Reads FASTA/FASTQ from stdin (the format is detected), writes the reads of each barcode identifier to\n"
          "PREFIX + identifier + SUFFIX (unmatched reads to PREFIX + 'unmatched' + SUFFIX) and a summary to stdout.\n\n"
          "--bcfile FILE    barcode file: lines 'identifier barcode'; lines starting with '#' are comments\n"
          "--prefix PREFIX  output file prefix (may name a directory)\n"
          "--suffix SUFFIX  output file suffix (default none)\n"
          "--bol            match the barcodes at the beginning of the reads (5' end)\n"
          "--eol            match the barcodes at the end of the reads (3' end); one of --bol / --eol is required\n"
          "--mismatches N   largest number of mismatches allowed, default 1\n"
          "--exact          same as --mismatches 0 (takes precedence)\n"
          "--partial N      also try the barcodes with up to N bases missing at the read's end, each counted as a mismatch (default 0)\n"
          "--quiet          no summary\n"
          "--debug          the barcode table and every read's match on stderr\n"
          "--help           this help\n", stdout);
    exit(1);
}

enum { O_BCFILE, O_EOL, O_BOL, O_EXACT, O_PREFIX, O_SUFFIX, O_QUIET, O_PARTIAL, O_DEBUG, O_MISMATCHES, O_HELP, O_N };
static const struct { const char *name; char type; } opts[O_N] = {
    {"bcfile", 's'}, {"eol", 0}, {"bol", 0}, {"exact", 0}, {"prefix", 's'}, {"suffix", 's'}, {"quiet", 0}, {"partial", 'i'}, {"debug", 0},
    {"mismatches", 'i'}, {"help", 0},
};

/* Getopt::Long's integer: [-+]?_*[0-9][0-9_]* (underscores dropped) */
static int parse_int(const char *s, long *v)
{
    const char *p = s;
    if (*p == '-' || *p == '+') ++p;
    while (*p == '_') ++p;
    if (*p < '0' || *p > '9') return 0;
    for (const char *q = p; *q; ++q) if (!((*q >= '0' && *q <= '9') || *q == '_')) return 0;
    long x = 0;
    for (const char *q = p; *q; ++q) if (*q != '_') { x = x * 10 + (*q - '0'); if (x > 2147483647L) x = 2147483647L; }
    *v = s[0] == '-' ? -x : x;
    return 1;
}

int main(int argc, char *argv[])
{
    if (argc < 2) usage();
    const char *sval[O_N] = {0};
    long ival[O_N] = {0};
    int set[O_N] = {0};
    int ok = 1;
    for (int i = 1; i < argc; ++i) {
        const char *a = argv[i];
        if (strcmp(a, "--") == 0) break;
        if (a[0] != '-' || a[1] == 0) continue;                  /* a non-option argument: left alone, as the script does */
        const char *body = a + (a[1] == '-' ? 2 : 1);
        const char *eq = strchr(body, '=');
        const size_t nlen = eq ? (size_t)(eq - body) : strlen(body);
        char name[256];
        size_t k;
        for (k = 0; k < nlen && k + 1 < sizeof name; ++k) name[k] = (char)((body[k] >= 'A' && body[k] <= 'Z') ? body[k] + 32 : body[k]);
        name[k] = 0;
        int hit = -1, nhit = 0;
        for (int o = 0; o < O_N; ++o) if (strcmp(opts[o].name, name) == 0) { hit = o; nhit = 1; }
        if (nhit == 0) for (int o = 0; o < O_N; ++o) if (strncmp(opts[o].name, name, k) == 0) { hit = o; ++nhit; }
        if (nhit != 1) {
            if (nhit == 0) fprintf(stderr, "Unknown option: %s\n", name);
            else {                                               /* the candidates in sorted order */
                const char *c[O_N];
                int m = 0;
                for (int o = 0; o < O_N; ++o) if (strncmp(opts[o].name, name, k) == 0) c[m++] = opts[o].name;
                for (int x = 0; x < m; ++x) for (int y = x + 1; y < m; ++y) if (strcmp(c[y], c[x]) < 0) { const char *t = c[x]; c[x] = c[y]; c[y] = t; }
                fprintf(stderr, "Option %s is ambiguous (", name);
                for (int x = 0; x < m; ++x) fprintf(stderr, "%s%s", x ? ", " : "", c[x]);
                fputs(")\n", stderr);
            }
            ok = 0;
            continue;
        }
        if (!opts[hit].type) {
            if (eq) { fprintf(stderr, "Option %s does not take an argument\n", opts[hit].name); ok = 0; continue; }
            set[hit] = 1; ival[hit] = 1;
            continue;
        }
        const char *arg;
        if (eq) {
            arg = eq + 1;
            if (!*arg) { fprintf(stderr, "Option %s requires an argument\n", opts[hit].name); ok = 0; continue; }
        } else {
            if (i + 1 >= argc) { fprintf(stderr, "Option %s requires an argument\n", opts[hit].name); ok = 0; continue; }
            arg = argv[++i];
        }
        if (opts[hit].type == 'i') {
            long v;
            if (!parse_int(arg, &v)) {
                fprintf(stderr, "Value \"%s\" invalid for option %s (number expected)\n", arg, opts[hit].name);
                ok = 0;
                if (!eq) --i;                                    /* pushed back: a non-option argument then */
                continue;
            }
            ival[hit] = v;
        } else sval[hit] = arg;
        set[hit] = 1;
    }
    if (set[O_HELP]) usage();
    if (!set[O_BCFILE]) fxh_split_die("Error: barcode file not specified (use '--bcfile [FILENAME]')");
    if (!set[O_PREFIX]) fxh_split_die("Error: prefix path/filename not specified (use '--prefix [PATH]')");
    if (set[O_BOL] == set[O_EOL]) {
        if (set[O_EOL]) fxh_split_die("Error: can't specify both --eol & --bol");
        fxh_split_die("Error: must specify either --eol or --bol");
    }
    const long partial = set[O_PARTIAL] ? ival[O_PARTIAL] : 0;
    if (partial < 0) fxh_split_die("Error: invalid for value partial matches (valid values are 0 or greater)");
    long mism = set[O_MISMATCHES] ? ival[O_MISMATCHES] : 1;
    if (set[O_EXACT]) mism = 0;
    if (mism < 0) fxh_split_die("Error: invalid value for mismatches (valid values are 0 or more)");
    if (partial > mism) fxh_split_die("Error: partial overlap value (%ld) bigger than max. allowed mismatches (%ld)", partial, mism);
    if (!ok) return 0;                                           /* the script: `exit unless $result` */
    fxh_split_opts o;
    memset(&o, 0, sizeof o);
    o.bcfile = sval[O_BCFILE]; o.prefix = sval[O_PREFIX]; o.suffix = set[O_SUFFIX] ? sval[O_SUFFIX] : "";
    o.eol = set[O_EOL]; o.mismatches = (int)mism; o.partial = (int)partial; o.quiet = set[O_QUIET]; o.debug = set[O_DEBUG];
    return fxh_split_run(&o);
}
