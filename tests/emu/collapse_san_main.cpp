// collapse_san_main.cpp -- TEST-ONLY stand-alone program over collapse_emu.cpp, built by tests/test_collapse_cpu.py (plainly for the hash pin,
// with -fsanitize=address,undefined for the kernels' bodies) and run directly.
//   collapse_san_main hash
//       fxg_cl_hash against std::hash<std::string> of the libstdc++ this program is built with, at every length 0 .. 64, a few long ones and
//       every alignment of the first byte; one line "len hash" per length on stdout, exit 1 at the first difference.  This is the pin that
//       says on which libstdc++ the order contract holds.
//   collapse_san_main FILE LPR BLOCKS OUT_CAP INITIAL_SLOTS HASH_BITS
//       FILE: whole records of LPR (2 or 4) lines.  They are added in BLOCKS blocks of nearly equal record counts, every block's arrays in heap
//       allocations of exactly their contracted sizes (the text has its 16 bytes of slack), then ordered and written window by window, every
//       window into an allocation of exactly min(OUT_CAP, what is left) bytes and once more into exactly the bytes it took.  The output goes
//       to stdout; "rc records reads uniques slots rebuilds out_reads out_bytes windows message" to stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "collapse_emu.cpp"

static int hash_pin()
{
    std::vector<uint32_t> lens;
    for (uint32_t n = 0; n <= 64; ++n) lens.push_back(n);
    for (uint32_t n : {150u, 255u, 256u, 1000u, 24997u}) lens.push_back(n);
    for (uint32_t n : lens) {
        std::string s(n, 'A');
        for (uint32_t i = 0; i < n; ++i) s[i] = "ACGTN"[(i * 7u + n + i / 5u) % 5u];
        const uint64_t want = (uint64_t)std::hash<std::string>()(s);
        for (uint32_t a = 0; a < 8; ++a) {
            std::vector<u64> pad(n / 8 + 3, 0x5A5A5A5A5A5A5A5Aull);
            uint8_t *p = (uint8_t *)pad.data() + a;
            if (n) memcpy(p, s.data(), n);
            const uint64_t got = fxg_cl_hash(p, n);
            if (got != want) { fprintf(stderr, "length %u at alignment %u: fxg_cl_hash %016llx, std::hash %016llx\n", n, a, (unsigned long long)got, (unsigned long long)want); return 1; }
        }
        printf("%u %016llx\n", n, (unsigned long long)want);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "hash")) return hash_pin();
    if (argc != 7) { fprintf(stderr, "usage: collapse_san_main hash | FILE LPR BLOCKS OUT_CAP INITIAL_SLOTS HASH_BITS\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> data;
    uint8_t chunk[65536];
    size_t k;
    while ((k = fread(chunk, 1, sizeof chunk, f)) > 0) data.insert(data.end(), chunk, chunk + k);
    fclose(f);
    const int lpr = atoi(argv[2]);
    const uint64_t blocks = strtoull(argv[3], nullptr, 10), out_cap = strtoull(argv[4], nullptr, 10);
    fxg_collapse_opts opts;
    opts.initial_slots = strtoull(argv[5], nullptr, 10); opts.hash_bits = (uint32_t)atoi(argv[6]);
    std::vector<uint64_t> nl;                                    // the newline behind every line
    for (uint64_t i = 0; i < data.size(); ++i) if (data[i] == '\n') nl.push_back(i);
    const uint64_t records = nl.size() / (uint64_t)lpr;
    void *h = fxg_emu_collapse_new();
    char err[256] = "";
    fxg_collapse_info info;
    memset(&info, 0, sizeof info);
    int rc = fxg_emu_collapse_begin(h, &opts, err, sizeof err);
    for (uint64_t b = 0; b < blocks && rc == FXG_OK; ++b) {
        const uint64_t r0 = records * b / blocks, r1 = records * (b + 1) / blocks, n = r1 - r0, cap_lines = (uint64_t)lpr * n + 1;
        const uint64_t t0 = r0 ? nl[(uint64_t)lpr * r0 - 1] + 1 : 0, t1 = r1 ? nl[(uint64_t)lpr * r1 - 1] + 1 : 0, len = t1 - t0;
        uint8_t *text = (uint8_t *)malloc(len + 16);             // the contract: readable 16 bytes past the text
        if (len) memcpy(text, data.data() + t0, len);
        memset(text + len, 0xA5, 16);
        uint32_t *line = (uint32_t *)malloc(2 * cap_lines * sizeof(uint32_t));
        uint16_t *l16 = (uint16_t *)malloc((n ? n : 1) * sizeof(uint16_t));
        uint64_t p = 0;
        for (uint64_t j = 0; j < (uint64_t)lpr * n; ++j) {       // lines cut at their first CR, as the index kernels chomp them
            uint64_t e = p, cr;
            while (text[e] != '\n') ++e;
            for (cr = p; cr < e && text[cr] != '\r'; ++cr) {}
            line[j] = (uint32_t)p; line[cap_lines + j] = (uint32_t)cr;
            if (j % (uint64_t)lpr == 1) l16[j / (uint64_t)lpr] = (uint16_t)(cr - p);
            p = e + 1;
        }
        line[(uint64_t)lpr * n] = (uint32_t)p;
        rc = fxg_emu_collapse_add(h, text, len, lpr, line, cap_lines, n, l16, &info, err, sizeof err);
        if (rc == FXG_OK && info.irregular) { snprintf(err, sizeof err, "block %llu is irregular at record %llu", (unsigned long long)b, (unsigned long long)info.first_bad); rc = 78; }
        free(l16); free(line); free(text);
    }
    if (rc == FXG_OK) rc = fxg_emu_collapse_order(h, &info, err, sizeof err);
    uint64_t windows = 0, rank = 0, left = info.out_bytes;
    while (rc == FXG_OK && rank < info.uniques) {
        const uint64_t cap = out_cap < left ? out_cap : left;
        uint8_t *out = (uint8_t *)malloc(cap ? cap : 1), *tight = nullptr;
        fxg_collapse_window w, again;
        rc = fxg_emu_collapse_write(h, rank, cap, out, &w, err, sizeof err);
        if (rc == FXG_OK) {
            tight = (uint8_t *)malloc(w.out_bytes ? w.out_bytes : 1);        // again, into exactly the bytes the window took
            rc = fxg_emu_collapse_write(h, rank, w.out_bytes, tight, &again, err, sizeof err);
            if (rc == FXG_OK && (again.out_bytes != w.out_bytes || again.rank_end != w.rank_end || memcmp(out, tight, w.out_bytes) != 0)) rc = 77;
            if (rc == FXG_OK) { fwrite(tight, 1, w.out_bytes, stdout); rank = w.rank_end; left -= w.out_bytes; ++windows; }
        }
        free(tight); free(out);
    }
    fprintf(stderr, "%d %llu %llu %llu %llu %llu %llu %llu %llu %s\n", rc, (unsigned long long)info.records, (unsigned long long)info.reads, (unsigned long long)info.uniques,
            (unsigned long long)info.slots, (unsigned long long)info.rebuilds, (unsigned long long)info.out_reads, (unsigned long long)info.out_bytes, (unsigned long long)windows, err);
    fxg_emu_collapse_free(h);
    return rc == FXG_OK ? 0 : 1;
}
