// nucchange_san_main.cpp -- TEST-ONLY stand-alone program: the emulated kernel of fxg_bases_change (nucchange_emu.cpp) over one block of two-line
// FASTA or four-line FASTQ, every array in a heap allocation of exactly its contracted size, so that a build with -fsanitize=address,undefined
// sees any access outside them.  The block is indexed here by a plain loop (lines cut at their first CR, as the index kernels chomp them).
//   nucchange_san_main FILE r|d     the block after the call on stdout; "rc changed first_to_record irregular" on stderr
// tests/test_nucchange_cpu.py builds it with the sanitizers and runs it directly.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nucchange_emu.cpp"

int main(int argc, char **argv)
{
    if (argc != 3 || (argv[2][0] != 'r' && argv[2][0] != 'd')) { fprintf(stderr, "usage: nucchange_san_main FILE r|d\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> data;
    uint8_t chunk[65536];
    size_t k;
    while ((k = fread(chunk, 1, sizeof chunk, f)) > 0) data.insert(data.end(), chunk, chunk + k);
    fclose(f);
    const uint64_t n = data.size();
    const int lpr = n && data[0] == '@' ? 4 : 2;
    uint64_t lines = 0;
    for (uint8_t c : data) lines += c == '\n';
    const uint64_t records = lines / lpr, cap_lines = lpr * records + 1;
    uint8_t *text = (uint8_t *)malloc(n + 16);                   // the contract: readable 16 bytes past the text
    if (n) memcpy(text, data.data(), n);
    memset(text + n, 0xA5, 16);
    uint32_t *line = (uint32_t *)malloc(2 * cap_lines * sizeof(uint32_t));
    uint64_t p = 0;
    for (uint64_t j = 0; j < lpr * records; ++j) {
        uint64_t e = p, cr;
        while (text[e] != '\n') ++e;
        for (cr = p; cr < e && text[cr] != '\r'; ++cr) {}
        line[j] = (uint32_t)p; line[cap_lines + j] = (uint32_t)cr;
        p = e + 1;
    }
    line[lpr * records] = (uint32_t)p;
    fxg_bases_change_info info;
    char err[256] = "";
    const int rna_to_dna = argv[2][0] == 'd';
    const int rc = fxg_emu_bases_change(text, p, lpr, line, cap_lines, records, rna_to_dna ? 'U' : 'T', rna_to_dna ? 'T' : 'U', &info, err, sizeof err);
    int bad = 0;
    for (int i = 0; i < 16; ++i) bad |= text[n + i] != 0xA5;     // the slack behind the text is read at the most
    fwrite(text, 1, n, stdout);
    fprintf(stderr, "%d %llu %llu %u %s\n", rc, (unsigned long long)info.changed, (unsigned long long)info.first_to_record, info.irregular, err);
    free(line); free(text);
    return rc == FXG_OK && !bad ? 0 : 1;
}
