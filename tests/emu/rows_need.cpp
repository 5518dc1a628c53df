// rows_need.cpp -- TEST-ONLY host check of the sparse base fetch of the rows kernels (fxg_rows_need_mask, fxg_rows.h).
//
// Compiled for the HOST only (hipcc --cuda-host-only -DFXG_HOST_EMULATION) by tests/test_rows_need_cpu.py.  The same __host__ __device__
// predicate the kernels run, with ds_bpermute replaced by an index into the lanes' klen words (modulo 64, as the hardware takes the address),
// against brute-force overlap of every 16-byte chunk (and every tail byte) of a tile with the kept prefixes of its reads:
//   complete: every byte of a kept prefix lies in a chunk (or tail byte) whose bit is set;
//   exact:    no chunk (or tail byte) inside the tile that holds no kept-prefix byte has its bit set.
// Usage: rows_need <form> [seed]   form = h1_26 h1_38 h2_26 h2_38 r4_10 r3_14 r2_20 | div.  Exit status 0 and "ok ..." on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../fastx_toolkit_amd/csrc/fxg_rows.h"

static unsigned long long g_cases = 0, g_chunks = 0;

// one tile: klen[r] for r < nreads (the kernel's contract: reads past nreads have klen 0), the lanes' words laid out as the kernel lays them
template <int NW, int H, int R>
static bool check_tile(u32 stride, u32 nreads, const std::vector<u32> &klen, std::mt19937 &rng, const char *what)
{
    constexpr int NC = (NW * R * 4 + 15) / 16;
    constexpr u32 TR = FXG_ROWS_T * (u32)R / (u32)H;
    const u32 tbytes = nreads * stride, magic = fxg_rows_magic(stride);
    u32 words[64];
    for (u32 l = 0; l < 64; ++l) words[l] = H == 2 && (l & 1u) ? (u32)rng() : 0u;        // the odd lanes' words of H = 2 are never read
    for (u32 r = 0; r < TR; ++r) {
        const u32 k = r < nreads ? klen[r] : 0u;
        if (R > 1) words[r & 63u] |= k << (8u * (r / 64u));
        else words[r * (u32)H] = k;
    }
    std::vector<unsigned char> inpre(tbytes, 0);
    for (u32 r = 0; r < nreads; ++r)
        for (u32 i = 0; i < klen[r]; ++i) inpre[r * stride + i] = 1;
    const u32 whole = tbytes & ~3u;
    for (u32 lane = 0; lane < 64; ++lane) {
        const u32 m = fxg_rows_need_mask<NC, H, R>(lane, stride, magic, tbytes, [&](u32 l) { return words[l & 63u]; });
        for (int K = 0; K < NC; ++K) {
            const u32 b0 = 1024u * (u32)K + 16u * lane;
            if (b0 >= tbytes) continue;                 // past the tile: fxg_rows_fetch never loads it
            bool any = false;
            for (u32 b = b0; b < b0 + 16u && b < tbytes; ++b) any |= inpre[b] != 0;
            const bool got = (m >> K) & 1u;
            ++g_chunks;
            if (got != any) {
                std::printf("FAIL %s: NW %d H %d R %d stride %u nreads %u lane %u load %d (bytes %u..%u): predicate %d, overlap %d\n",
                            what, NW, H, R, stride, nreads, lane, K, b0, b0 + 15u, (int)got, (int)any);
                return false;
            }
        }
        if (whole + lane < tbytes) {                    // the tail bytes of a tile that ends inside a dword
            const bool any = inpre[whole + lane] != 0, got = (m & FXG_ROWS_TAIL_BIT) != 0u;
            if (got != any) {
                std::printf("FAIL %s: NW %d H %d R %d stride %u nreads %u tail byte %u: predicate %d, kept %d\n", what, NW, H, R, stride, nreads,
                            whole + lane, (int)got, (int)any);
                return false;
            }
        }
    }
    ++g_cases;
    return true;
}

// every case for one stride: kept lengths never exceed the row (a read is at most `stride` long)
template <int NW, int H, int R>
static bool check_stride(u32 stride, std::mt19937 &rng)
{
    constexpr u32 TR = FXG_ROWS_T * (u32)R / (u32)H;
    const u32 sizes[] = {TR, TR - 1u, 1u, 2u, TR / 2u + 1u, 1u + (u32)rng() % TR};
    std::vector<u32> k(TR);
    for (u32 nreads : sizes) {
        const auto run = [&](const char *what) { return check_tile<NW, H, R>(stride, nreads, k, rng, what); };
        for (u32 &x : k) x = 0;
        if (!run("every read dropped")) return false;
        for (u32 &x : k) x = stride;
        if (!run("every read kept whole")) return false;
        for (u32 v : {1u, 2u, 3u, 4u, 15u, 16u, 17u, stride - 1u}) {             // one value for every read, and every other read
            for (u32 r = 0; r < TR; ++r) k[r] = v;
            if (!run("every read one length")) return false;
            for (u32 r = 0; r < TR; ++r) k[r] = r & 1u ? v : 0u;
            if (!run("odd reads one length")) return false;
            for (u32 r = 0; r < TR; ++r) k[r] = r & 1u ? 0u : v;
            if (!run("even reads one length")) return false;
        }
        // prefix ends at every residue mod 128 (and so mod 16 and 64): read r ends at the smallest end >= its start with that residue
        for (u32 t = 0; t < 128u; ++t) {
            for (u32 r = 0; r < TR; ++r) {
                const u32 v = (t + 128u - (r * stride) % 128u) % 128u;
                k[r] = v <= stride ? v : (rng() & 1u ? stride : 0u);
            }
            if (!run("prefix ends at one residue mod 128")) return false;
        }
        for (int t = 0; t < 24; ++t) {                 // random: kept or dropped, lengths from the short end, the long end and anywhere
            const u32 pk = (u32)rng() % 5u;
            for (u32 r = 0; r < TR; ++r) {
                const u32 sel = (u32)rng() % 4u;
                const u32 v = sel == 0 ? (u32)rng() % 4u : sel == 1 ? stride - (u32)rng() % 4u : (u32)rng() % (stride + 1u);
                k[r] = (u32)rng() % 4u < pk ? (v <= stride ? v : stride) : 0u;
            }
            if (!run("random")) return false;
        }
    }
    return true;
}

template <int NW, int H, int R>
static bool check_form(u32 lo, u32 hi, std::mt19937 &rng)
{
    for (u32 s = lo; s <= hi; ++s)
        if (!check_stride<NW, H, R>(s, rng)) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: rows_need <form> [seed]\n"); return 2; }
    const char *f = argv[1];
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    bool ok;
    // every form over strides 28 .. the longest row it holds (4 NW bytes per piece, H pieces; R reads per lane hold rows of 4 NW)
    if (!std::strcmp(f, "div")) {                      // the multiply-high quotient, every tile offset the kernels use, every stride
        ok = true;
        for (u32 d = 28; d <= 304 && ok; ++d) {
            const u32 m = fxg_rows_magic(d);
            for (u32 x = 0; x < (1u << 14) && ok; ++x)
                if (fxg_rows_div(x, m) != x / d) { std::printf("FAIL div: %u / %u -> %u\n", x, d, fxg_rows_div(x, m)); ok = false; }
        }
    }
    else if (!std::strcmp(f, "h1_26")) ok = check_form<26, 1, 1>(28, 104, rng);
    else if (!std::strcmp(f, "h1_38")) ok = check_form<38, 1, 1>(28, 152, rng);
    else if (!std::strcmp(f, "h2_26")) ok = check_form<26, 2, 1>(28, 208, rng);
    else if (!std::strcmp(f, "h2_38")) ok = check_form<38, 2, 1>(28, 304, rng);
    else if (!std::strcmp(f, "r4_10")) ok = check_form<10, 1, 4>(28, 40, rng);
    else if (!std::strcmp(f, "r3_14")) ok = check_form<14, 1, 3>(28, 56, rng);
    else if (!std::strcmp(f, "r2_20")) ok = check_form<20, 1, 2>(28, 80, rng);
    else { std::fprintf(stderr, "unknown form %s\n", f); return 2; }
    if (!ok) return 1;
    if (!std::strcmp(f, "div")) std::printf("ok div: strides 28..304, offsets 0..16383\n");
    else std::printf("ok %s: %llu tiles, %llu chunks\n", f, g_cases, g_chunks);
    return 0;
}
