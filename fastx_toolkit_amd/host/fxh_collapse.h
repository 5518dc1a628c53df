/* fxh_collapse.h -- fastx_collapser's run (fxh_collapse.c): the reads of a FASTA or FASTQ input merged into a set on the device block by block,
 * ordered after the last block and written window by window.  Behaviour: the reference's src/fastx_collapser/fastx_collapser.cpp:112-135
 * built with HAVE_CXX11 == 1. */
#ifndef FXH_COLLAPSE_H
#define FXH_COLLAPSE_H
#include "fastx.h"

typedef struct fxh_collapse_totals {
    size_t input_sequences, input_reads;       /* the -v report's first line */
    size_t output_sequences, output_reads;     /* its second: the distinct sequences, and their counts as printed (truncated to int) added up */
} fxh_collapse_totals;

/* fx: reader and writer are open (FASTA_OR_FASTQ; OUTPUT_FASTA, not compressed).  Writes ">rank-count\nBASES\n" for every distinct sequence after
 * the last record has been read -- a bad record ends the run before anything is written -- and fills *tot for the -v report. */
void fxh_collapse_run(FASTX *fx, fxh_collapse_totals *tot);
#endif
