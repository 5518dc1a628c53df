/* fxh_uncollapse.h -- fastx_uncollapser's run (fxh_uncollapse.c): collapsed FASTA expanded block by block and window by window on the device,
 * anything the device path does not take through the record API from there on.  Behaviour: the reference's
 * src/fastx_uncollapser/fastx_uncollapser.cpp:73-98 (its FASTA mode). */
#ifndef FXH_UNCOLLAPSE_H
#define FXH_UNCOLLAPSE_H
#include "fastx.h"
#include "fxh_batch.h"

/* fx: reader and writer are open (FASTA_ONLY, OUTPUT_SAME_AS_INPUT).  Writes every record get_reads_count() times under a running number from 1
 * on and fills the four counts of *tot for the -v report. */
void fxh_uncollapse_run(FASTX *fx, fxh_totals *tot);
#endif
