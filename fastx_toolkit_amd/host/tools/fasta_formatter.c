/* fasta_formatter -- command line of the FASTX-Toolkit's src/fasta_formatter/fasta_formatter.cpp:96-133 (its own getopt string, not the
 * other tools' shared parser: no -v, -z or -Q).  The run itself: ../fxh_reflow.c. */
#define _GNU_SOURCE
#include <err.h>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>

#include "../fxh_reflow.h"

static void usage(void)
{
    fputs("usage: fasta_formatter [-h] [-i INFILE] [-o OUTFILE] [-w N] [-t] [-e]\n"
          "MI355X build of the FASTX-Toolkit FASTA formatter (same options as FASTX Toolkit 0.0.14).\n"
          "Joins the sequence lines of every record of a multi-line FASTA file and writes them out again.\n\n"
          "   [-h]         = this help\n"
          "   [-i INFILE]  = FASTA input file, default stdin\n"
          "   [-o OUTFILE] = output file, default stdout\n"
          "   [-w N]       = sequence lines of at most N characters; 0 (the default): each record's\n"
          "                  sequence on one line\n"
          "   [-t]         = tabular output: identifier (without '>'), a tab, the sequence on one line\n"
          "   [-e]         = keep records that have an identifier line but no sequence (dropped by default)\n",
          stdout);
    exit(0);
}

int main(int argc, char *argv[])
{
    fxh_reflow_opts o = {0};
    int opt;
    while ((opt = getopt(argc, argv, "i:o:hw:te")) != -1) {
        switch (opt) {
        case 'h': usage(); break;
        case 'i': o.in = optarg; break;
        case 'o': o.out = optarg; break;
        case 'w': {
            const int v = atoi(optarg);
            if (v < 0) errx(1, "Invalid value (%s) for requested width [-w]", optarg);
            o.width = (uint32_t)v;
            break;
        }
        case 't': o.tabular = 1; break;
        case 'e': o.keep_empty = 1; break;
        default: exit(1);
        }
    }
    return fxh_reflow_run(&o);
}
