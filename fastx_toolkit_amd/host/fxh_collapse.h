/* fxh_collapse.h -- fastx_collapser's run (fxh_collapse.c): the reads of a FASTA or FASTQ input merged into a set on the device block by block,
 * ordered after the last block and written window by window.  Behaviour: the reference's src/fastx_collapser/fastx_collapser.cpp:112-135
 * built with HAVE_CXX11 == 1. */
#ifndef FXH_COLLAPSE_H
#define FXH_COLLAPSE_H
#include "fastx.h"
#include "fxh_batch.h"

typedef struct fxh_collapse_totals {
    size_t input_sequences, input_reads;       /* the -v report's first line */
    size_t output_sequences, output_reads;     /* its second: the distinct sequences, and their counts as printed (truncated to int) added up */
} fxh_collapse_totals;

/* fx: reader and writer are open (FASTA_OR_FASTQ; OUTPUT_FASTA, not compressed).  Writes ">rank-count\nBASES\n" for every distinct sequence after
 * the last record has been read -- a bad record ends the run before anything is written -- and fills *tot for the -v report. */
void fxh_collapse_run(FASTX *fx, fxh_collapse_totals *tot);

/* The same run behind a stage chain (fastx_clip_collapser): chain->stages is FXG_STAGE_CLIP, with FXG_STAGE_FTRIM or without.  The clip stage runs
 * through fxg_run_pipeline, and what it keeps of every block goes into the set on the device (fxg_collapse_add_rows), cut to ft_first .. ft_last
 * on the way if the trim stage is there, counted by its FASTA id where the input is FASTA.  *stages gets the clip stage's totals as fxh_run_tool
 * would fill them: its output_sequences / output_reads are the trim stage's input, whose output is the set's input in *tot.  The writer is not open yet: open_writer is called after the last block, and only if a read
 * was kept -- the run then writes and returns 1.  If none was kept it returns 0 with nothing opened: the pipe's collapser meets an empty input.
 * With chain == NULL and open_writer == NULL this is fxh_collapse_run. */
int fxh_collapse_run_chain(FASTX *fx, const fxg_params *chain, void (*open_writer)(FASTX *), fxh_collapse_totals *tot, fxh_totals *stages);
#endif
