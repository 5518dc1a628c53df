/* fxh_split.h -- fastx_barcode_splitter: the run behind the command line (host/tools/fastx_barcode_splitter.c).  Behaviour: the reference's
 * scripts/fastx_barcode_splitter.pl (barcode table, input format, files, summary and messages); the matching and the partition run on the
 * device (csrc/fxg_barcode.h). */
#ifndef FXH_SPLIT_H
#define FXH_SPLIT_H

typedef struct fxh_split_opts {
    const char *bcfile, *prefix, *suffix;
    int eol;                  /* 0: --bol */
    int mismatches, partial;
    int quiet, debug;
} fxh_split_opts;

/* Reads stdin to its end; returns the exit status (0).  Every error ends the process with its message and status 255. */
int fxh_split_run(const fxh_split_opts *o);

/* "Error: ..." + '\n' on stderr, exit 255 (the script's die) */
void fxh_split_die(const char *fmt, ...) __attribute__((noreturn, format(printf, 1, 2)));
#endif
