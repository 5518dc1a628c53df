// reflow_san_main.cpp -- TEST-ONLY stand-alone program: the emulated kernels of fxg_fasta_reflow (reflow_emu.cpp) over one block, every array
// in a heap allocation of exactly its contracted size, so that a build with -fsanitize=address,undefined sees any access outside them.
//   reflow_san_main FILE WIDTH TABULAR KEEP_EMPTY AT_EOF OPEN_IN     the block's output on stdout, "rc consumed open_bases" on stderr
// tests/test_reflow_cpu.py builds it with the sanitizers and runs it directly over the corner corpus.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "reflow_emu.cpp"

int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: reflow_san_main FILE WIDTH TABULAR KEEP_EMPTY AT_EOF OPEN_IN\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> data;
    uint8_t chunk[65536];
    size_t k;
    while ((k = fread(chunk, 1, sizeof chunk, f)) > 0) data.insert(data.end(), chunk, chunk + k);
    fclose(f);
    const uint64_t n = data.size();
    uint64_t lines = 0;
    for (uint8_t c : data) lines += c == '\n';
    uint8_t *text = (uint8_t *)malloc(n + 16);                   // the contract: readable 16 bytes past the text
    if (n) memcpy(text, data.data(), n);
    memset(text + n, 0xA5, 16);
    uint32_t *line = (uint32_t *)malloc(2 * (lines + 1) * sizeof(uint32_t));
    fxg_reflow_opts o;
    o.width = (uint32_t)strtoul(argv[2], nullptr, 10); o.tabular = (uint32_t)atoi(argv[3]); o.keep_empty = (uint32_t)atoi(argv[4]);
    // first pass: an output array of the bound; second pass: one of exactly the bytes the block needs
    fxg_reflow_info info;
    char err[256] = "";
    o.out_cap = 2 * n + 2;
    uint8_t *big = (uint8_t *)malloc(o.out_cap);
    int rc = fxg_emu_fasta_reflow(text, n, atoi(argv[5]), strtoull(argv[6], nullptr, 10), &o, line, lines + 1, big, &info, err, sizeof err);
    if (rc == FXG_OK) {
        fxg_reflow_info again;
        o.out_cap = info.out_bytes;
        uint8_t *tight = (uint8_t *)malloc(info.out_bytes ? info.out_bytes : 1);
        rc = fxg_emu_fasta_reflow(text, n, atoi(argv[5]), strtoull(argv[6], nullptr, 10), &o, line, lines + 1, tight, &again, err, sizeof err);
        if (rc == FXG_OK && (again.out_bytes != info.out_bytes || memcmp(big, tight, info.out_bytes) != 0)) rc = 77;
        if (rc == FXG_OK) fwrite(tight, 1, info.out_bytes, stdout);
        free(tight);
    }
    fprintf(stderr, "%d %llu %llu %s\n", rc, (unsigned long long)info.consumed, (unsigned long long)info.open_bases, err);
    free(big); free(line); free(text);
    return rc == FXG_OK ? 0 : 1;
}
