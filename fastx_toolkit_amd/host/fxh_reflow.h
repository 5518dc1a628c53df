/* fxh_reflow.h -- fasta_formatter's run (fxh_reflow.c): multi-line FASTA reflowed block by block on the device, input that does not begin
 * with a header line on the host.  Behaviour: the reference's src/fasta_formatter/fasta_formatter.cpp and sequence_writers.h. */
#ifndef FXH_REFLOW_H
#define FXH_REFLOW_H
#include <stdint.h>

typedef struct fxh_reflow_opts {
    const char *in, *out;        /* -i / -o; NULL = stdin / stdout */
    uint32_t width;              /* -w */
    int tabular, keep_empty;     /* -t, -e */
} fxh_reflow_opts;

int fxh_reflow_run(const fxh_reflow_opts *o);      /* the tool's exit status */
#endif
