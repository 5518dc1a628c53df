// collapse_rows_san_main.cpp -- TEST-ONLY stand-alone program over collapse_rows_emu.cpp, built by tests/test_collapse_rows_cpu.py with
// -fsanitize=address,undefined and run directly.
//   collapse_rows_san_main FILE BLOCKS OUT_CAP INITIAL_SLOTS HASH_BITS MODE
//       FILE: whole two-line FASTA records.  They are added in BLOCKS blocks of nearly equal record counts.  MODE rows: every block as packed
//       rows -- the bases of its records with gaps of 0 .. 15 bytes between them in a heap allocation that ends at the last record's last
//       byte, offsets, lengths and a kept_index in allocations of exactly records entries, the block's text (16 bytes of slack) and line index
//       as the count source.  MODE mixed: every second block through fxg_emu_collapse_add instead.  MODE plain: rows without a count source.
//       Then order and write, window by window into allocations of exactly min(OUT_CAP, what is left) bytes.  The output goes to stdout;
//       "rc records reads uniques slots rebuilds out_reads out_bytes message" to stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "collapse_rows_emu.cpp"

int main(int argc, char **argv)
{
    if (argc != 7) { fprintf(stderr, "usage: collapse_rows_san_main FILE BLOCKS OUT_CAP INITIAL_SLOTS HASH_BITS rows|mixed|plain\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> data;
    uint8_t chunk[65536];
    size_t k;
    while ((k = fread(chunk, 1, sizeof chunk, f)) > 0) data.insert(data.end(), chunk, chunk + k);
    fclose(f);
    const uint64_t blocks = strtoull(argv[2], nullptr, 10), out_cap = strtoull(argv[3], nullptr, 10);
    fxg_collapse_opts opts;
    opts.initial_slots = strtoull(argv[4], nullptr, 10); opts.hash_bits = (uint32_t)atoi(argv[5]);
    const bool mixed = !strcmp(argv[6], "mixed"), plain = !strcmp(argv[6], "plain");
    std::vector<uint64_t> nl;
    for (uint64_t i = 0; i < data.size(); ++i) if (data[i] == '\n') nl.push_back(i);
    const uint64_t records = nl.size() / 2;
    void *h = fxg_emu_collapse_new();
    char err[256] = "";
    fxg_collapse_info info;
    memset(&info, 0, sizeof info);
    int rc = fxg_emu_collapse_begin(h, &opts, err, sizeof err);
    for (uint64_t b = 0; b < blocks && rc == FXG_OK; ++b) {
        const uint64_t r0 = records * b / blocks, r1 = records * (b + 1) / blocks, n = r1 - r0, cap_lines = 2 * n + 1;
        const uint64_t t0 = r0 ? nl[2 * r0 - 1] + 1 : 0, t1 = r1 ? nl[2 * r1 - 1] + 1 : 0, len = t1 - t0;
        uint8_t *text = (uint8_t *)malloc(len + 16);
        if (len) memcpy(text, data.data() + t0, len);
        memset(text + len, 0xA5, 16);
        uint32_t *line = (uint32_t *)malloc(2 * cap_lines * sizeof(uint32_t));
        uint16_t *l16 = (uint16_t *)malloc((n ? n : 1) * sizeof(uint16_t));
        uint64_t p = 0, total = 0;
        for (uint64_t j = 0; j < 2 * n; ++j) {                   // lines cut at their first CR, as the index kernels chomp them
            uint64_t e = p, cr;
            while (text[e] != '\n') ++e;
            for (cr = p; cr < e && text[cr] != '\r'; ++cr) {}
            line[j] = (uint32_t)p; line[cap_lines + j] = (uint32_t)cr;
            if (j % 2 == 1) { l16[j / 2] = (uint16_t)(cr - p); total += (j / 2 * 5 + 3) % 16 + (cr - p); }
            p = e + 1;
        }
        line[2 * n] = (uint32_t)p;
        if (mixed && b % 2 == 1) rc = fxg_emu_collapse_add(h, text, len, 2, line, cap_lines, n, l16, &info, err, sizeof err);
        else {
            uint8_t *bases = (uint8_t *)malloc(total ? total : 1);
            uint64_t *off = (uint64_t *)malloc((n ? n : 1) * sizeof(uint64_t));
            uint32_t *kept = (uint32_t *)malloc((n ? n : 1) * sizeof(uint32_t));
            memset(bases, 'x', total ? total : 1);
            uint64_t at = 0;
            for (uint64_t r = 0; r < n; ++r) {
                at += (r * 5 + 3) % 16;
                off[r] = at; kept[r] = (uint32_t)r;
                memcpy(bases + at, text + line[2 * r + 1], l16[r]);
                at += l16[r];
            }
            if (plain) rc = fxg_emu_collapse_add_rows(h, bases, off, l16, n, 0, 0, nullptr, nullptr, nullptr, 0, 0, &info, err, sizeof err);
            else rc = fxg_emu_collapse_add_rows(h, bases, off, l16, n, 1, 0, kept, text, line, cap_lines, 2, &info, err, sizeof err);
            free(kept); free(off); free(bases);
        }
        if (rc == FXG_OK && info.irregular) { snprintf(err, sizeof err, "block %llu is irregular at record %llu", (unsigned long long)b, (unsigned long long)info.first_bad); rc = 78; }
        free(l16); free(line); free(text);
    }
    if (rc == FXG_OK) rc = fxg_emu_collapse_order(h, &info, err, sizeof err);
    uint64_t rank = 0, left = info.out_bytes;
    while (rc == FXG_OK && rank < info.uniques) {
        const uint64_t cap = out_cap < left ? out_cap : left;
        uint8_t *out = (uint8_t *)malloc(cap ? cap : 1);
        fxg_collapse_window w;
        rc = fxg_emu_collapse_write(h, rank, cap, out, &w, err, sizeof err);
        if (rc == FXG_OK) { fwrite(out, 1, w.out_bytes, stdout); rank = w.rank_end; left -= w.out_bytes; }
        free(out);
    }
    fprintf(stderr, "%d %llu %llu %llu %llu %llu %llu %llu %s\n", rc, (unsigned long long)info.records, (unsigned long long)info.reads, (unsigned long long)info.uniques,
            (unsigned long long)info.slots, (unsigned long long)info.rebuilds, (unsigned long long)info.out_reads, (unsigned long long)info.out_bytes, err);
    fxg_emu_collapse_free(h);
    return rc == FXG_OK ? 0 : 1;
}
