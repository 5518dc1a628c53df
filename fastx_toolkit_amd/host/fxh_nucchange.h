/* fxh_nucchange.h -- fasta_nucleotide_changer's run (fxh_nucchange.c): the bases of FASTA or FASTQ records rewritten T -> U or U -> T block by
 * block on the device and written as FASTA, anything the device path does not take through the record API from there on.  Behaviour: the
 * reference's src/fasta_nucleotide_changer/fasta_nucleotide_changer.c:101-115. */
#ifndef FXH_NUCCHANGE_H
#define FXH_NUCCHANGE_H
#include "fastx.h"
#include "fxh_batch.h"

/* fx: reader and writer are open (FASTA_OR_FASTQ with ALLOW_N | ALLOW_U, OUTPUT_FASTA).  rna_to_dna: -d (U becomes T), else -r (T becomes U).
 * Writes every record up to the first one that holds a byte of the mode's target letter and ends there as the reference does: the output
 * finished, its message, status 1.  Otherwise fills the four counts of *tot and *changed for the -v report. */
void fxh_nucchange_run(FASTX *fx, int rna_to_dna, fxh_totals *tot, size_t *changed);
#endif
