// uncollapse_san_main.cpp -- TEST-ONLY stand-alone program: the emulated kernels of fxg_fasta_uncollapse (uncollapse_emu.cpp) over one block of
// two-line FASTA, every array in a heap allocation of exactly its contracted size, so that a build with -fsanitize=address,undefined sees any
// access outside them.  The block is indexed here by a plain loop (lines cut at their first CR, as the index kernels chomp them).
//   uncollapse_san_main FILE ORDINAL_BASE OUT_CAP     the windows' output, one after the other, on stdout; "rc copies windows" on stderr
// Every window is written into an allocation of exactly the bytes it is entitled to (min(OUT_CAP, what is left)), so a byte past a window is seen.
// tests/test_uncollapse_cpu.py builds it with the sanitizers and runs it directly.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uncollapse_emu.cpp"

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: uncollapse_san_main FILE ORDINAL_BASE OUT_CAP\n"); return 2; }
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
    const uint64_t records = lines / 2, cap_lines = 2 * records + 1;
    uint8_t *text = (uint8_t *)malloc(n + 16);                   // the contract: readable 16 bytes past the text
    if (n) memcpy(text, data.data(), n);
    memset(text + n, 0xA5, 16);
    uint32_t *line = (uint32_t *)malloc(2 * cap_lines * sizeof(uint32_t));
    uint16_t *len = (uint16_t *)malloc((records ? records : 1) * sizeof(uint16_t));
    uint64_t p = 0;
    for (uint64_t j = 0; j < 2 * records; ++j) {
        uint64_t e = p, cr;
        while (text[e] != '\n') ++e;
        for (cr = p; cr < e && text[cr] != '\r'; ++cr) {}
        line[j] = (uint32_t)p; line[cap_lines + j] = (uint32_t)cr;
        if (j & 1) len[j / 2] = (uint16_t)(cr - p);
        p = e + 1;
    }
    line[2 * records] = (uint32_t)p;
    fxg_uncollapse_opts o;
    o.ordinal_base = strtoull(argv[2], nullptr, 10); o.copy_begin = 0; o.out_cap = strtoull(argv[3], nullptr, 10);
    fxg_uncollapse_info info;
    char err[256] = "";
    int rc = FXG_OK;
    uint64_t windows = 0;
    memset(&info, 0, sizeof info);
    do {
        uint8_t *out = (uint8_t *)malloc(o.out_cap ? o.out_cap : 1);
        rc = fxg_emu_fasta_uncollapse(text, p, line, cap_lines, records, len, &o, out, &info, err, sizeof err);
        if (rc == FXG_OK) {
            uint8_t *tight = (uint8_t *)malloc(info.out_bytes ? info.out_bytes : 1);          // again, into exactly the bytes the window took
            fxg_uncollapse_opts to = o;
            fxg_uncollapse_info again;
            to.out_cap = info.out_bytes;
            rc = fxg_emu_fasta_uncollapse(text, p, line, cap_lines, records, len, &to, tight, &again, err, sizeof err);
            if (rc == FXG_OK && (again.out_bytes != info.out_bytes || again.copy_end != info.copy_end || memcmp(out, tight, info.out_bytes) != 0)) rc = 77;
            if (rc == FXG_OK) fwrite(tight, 1, info.out_bytes, stdout);
            free(tight);
            o.copy_begin = info.copy_end;
            ++windows;
        }
        free(out);
    } while (rc == FXG_OK && info.copy_end < info.copies);
    fprintf(stderr, "%d %llu %llu %s\n", rc, (unsigned long long)info.copies, (unsigned long long)windows, err);
    free(len); free(line); free(text);
    return rc == FXG_OK ? 0 : 1;
}
