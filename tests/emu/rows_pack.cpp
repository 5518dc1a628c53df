// rows_pack.cpp -- TEST-ONLY host check of the unpredicated (`fast`) pack of the rows kernels (fxg_rows_pack_step, fxg_rows.h).
//
// Compiled for the HOST only (hipcc --cuda-host-only -DFXG_HOST_EMULATION) by tests/test_rows_pack_cpu.py, plainly and with
// -fsanitize=address,undefined.  The kernels' own __host__ __device__ write schedule -- for step S, the lane's LDS byte address, width and
// value -- is run for the 64 lanes of a wave against a byte array the size of the kernels' staging buffer (fxg_rows_lds, a heap block of
// exactly that size): step by step in instruction order, as the wave's LDS instructions execute, and with the lanes inside one step
// applied in a SHUFFLED order, so that a result that leans on the order inside an instruction shows.  The R sub-tiles of a rows_multi
// tile are packed one after the other, as the kernel does.  The bytes [0, totb) must then equal the concatenation of the kept prefixes.
// The rows hold random bytes past the kept length too (the kernels pack quality rows read whole), so a wrong winner of a shared dword shows.
// Usage: rows_pack <form> [seed]   form = nw10 nw14 nw20 nw26 nw38.  Exit status 0 and "ok ..." on success.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../fastx_toolkit_amd/csrc/fxg_rows.h"

static unsigned long long g_tiles = 0, g_stores = 0, g_al[4] = {0, 0, 0, 0};

struct Store { u32 addr, width, value; };

// step S of every kept lane of one sub-tile, applied in a shuffled lane order; then step S + 1
template <int NW, int S>
static bool run_steps(std::vector<unsigned char> &buf, const u32 (*rows)[NW], const u32 *D, const u32 *klen, std::mt19937 &rng)
{
    if constexpr (S < FXG_ROWS_PACK_STEPS(NW)) {
        Store st[64];
        u32 n = 0;
        for (u32 l = 0; l < 64; ++l) {
            if (!klen[l]) continue;                         // the kernel's `if (keep)`: a dropped lane stays out of every step
            const FxgPackStore s = fxg_rows_pack_step<NW, S>(D[l], rows[l]);
            if (s.width) st[n++] = {s.base + fxg_rows_pack_off<NW, S>(), s.width, s.value};
        }
        std::shuffle(st, st + n, rng);
        for (u32 i = 0; i < n; ++i) {
            if (st[i].width != 4u && st[i].width != 1u) { std::printf("FAIL step %d: width %u\n", S, st[i].width); return false; }
            if (st[i].width == 4u && (st[i].addr & 3u)) { std::printf("FAIL step %d: dword store at byte %u\n", S, st[i].addr); return false; }
            if ((size_t)st[i].addr + st[i].width > buf.size()) {
                std::printf("FAIL step %d: store of %u bytes at %u, the staging buffer has %zu\n", S, st[i].width, st[i].addr, buf.size());
                return false;
            }
            for (u32 k = 0; k < st[i].width; ++k) buf.data()[st[i].addr + k] = (unsigned char)(st[i].value >> (8u * k));
            ++g_stores;
        }
        return run_steps<NW, S + 1>(buf, rows, D, klen, rng);
    }
    return true;
}

// one tile of R sub-tiles: klen[j * 64 + l] = kept length of lane l's read in sub-tile j, 0 = dropped; every kept read has >= 4 bytes (`fast`)
template <int NW, int R>
static bool check_tile(const std::vector<u32> &klen, std::mt19937 &rng, const char *what)
{
    static u32 rows[R][64][NW];
    std::vector<unsigned char> want;
    u32 D[R][64];
    for (int j = 0; j < R; ++j)
        for (u32 l = 0; l < 64; ++l) {
            for (int k = 0; k < NW; ++k) rows[j][l][k] = (u32)rng();
            const u32 n = klen[(u32)j * 64u + l];
            D[j][l] = (u32)want.size();
            if (n) ++g_al[D[j][l] & 3u];
            for (u32 i = 0; i < n; ++i) want.push_back((unsigned char)(rows[j][l][i >> 2] >> (8u * (i & 3u))));
        }
    std::vector<unsigned char> buf(fxg_rows_lds(4u * (u32)NW, 1u, (u32)R));         // the longest row of the form: what the launch allocates at most
    for (auto &x : buf) x = (unsigned char)rng();
    for (int j = 0; j < R; ++j)
        if (!run_steps<NW, 0>(buf, rows[j], D[j], &klen[(u32)j * 64u], rng)) { std::printf("     in %s, NW %d R %d sub-tile %d\n", what, NW, R, j); return false; }
    for (size_t i = 0; i < want.size(); ++i)
        if (buf[i] != want[i]) {
            std::printf("FAIL %s: NW %d R %d: packed byte %zu of %zu is %02x, the kept prefixes have %02x\n", what, NW, R, i, want.size(), buf[i], want[i]);
            return false;
        }
    ++g_tiles;
    return true;
}

template <int NW, int R>
static bool check_form(std::mt19937 &rng)
{
    constexpr u32 T = 64u * (u32)R, FULL = 4u * (u32)NW;
    std::vector<u32> k(T);
    const auto run = [&](const char *what) { return check_tile<NW, R>(k, rng, what); };
    for (int rep = 0; rep < 4; ++rep) {                        // another shuffle and other row bytes every time
        for (u32 v : {4u, 5u, 6u, 7u, FULL}) {
            for (u32 &x : k) x = v;
            if (!run("every read one length")) return false;
        }
        for (u32 s = 0; s < 4; ++s) {                          // lengths 4..7 in turn: every D & 3 follows every other
            for (u32 r = 0; r < T; ++r) k[r] = 4u + (r + s) % 4u;
            if (!run("lengths 4..7 in turn")) return false;
            for (u32 r = 0; r < T; ++r) k[r] = 4u + (r * 3u + s) % 4u;
            if (!run("lengths 7..4 in turn")) return false;
        }
        for (u32 first = 0; first < T; first += 64u) {         // one long read, then reads of length 4: its overshoot covers dozens of them
            for (u32 r = 0; r < T; ++r) k[r] = r == first ? FULL : 4u;
            if (!run("one long read, then length 4")) return false;
            for (u32 r = 0; r < T; ++r) k[r] = r == first ? FULL - 1u - rep % 3u : 4u + (r & 1u);
            if (!run("one long read off a dword, then lengths 4 and 5")) return false;
        }
        for (u32 r = 0; r < T; ++r) k[r] = r & 1u ? 4u : FULL;
        if (!run("alternating full and 4")) return false;
        for (u32 r = 0; r < T; ++r) k[r] = r & 1u ? FULL : 4u;
        if (!run("alternating 4 and full")) return false;
        for (u32 r = 0; r < T; ++r) k[r] = FULL > 4u + r % (FULL - 3u) ? FULL - r % (FULL - 3u) : 4u;
        if (!run("descending by one")) return false;
        for (u32 r = 0; r < T; ++r) k[r] = r % 3u == 1u ? 0u : FULL > 4u + r % (FULL - 3u) ? FULL - r % (FULL - 3u) : 4u;
        if (!run("descending, every third read dropped")) return false;
        for (u32 r = 0; r < T; ++r) k[r] = r % 5u < 3u ? 0u : (r & 1u ? FULL : 4u + r % 4u);
        if (!run("runs of dropped reads in between")) return false;
        for (u32 r = 0; r < T; ++r) k[r] = r + 1u == T ? FULL : 0u;
        if (!run("only the last read kept")) return false;
        for (int t = 0; t < 40; ++t) {                         // random: kept or dropped, lengths from the short end, the long end and anywhere
            const u32 pk = 1u + (u32)rng() % 4u;
            for (u32 r = 0; r < T; ++r) {
                const u32 sel = (u32)rng() % 4u;
                const u32 v = sel == 0 ? 4u + (u32)rng() % 4u : sel == 1 ? FULL - (u32)rng() % 4u : 4u + (u32)rng() % (FULL - 3u);
                k[r] = (u32)rng() % 4u < pk ? v : 0u;
            }
            if (!run("random")) return false;
        }
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: rows_pack <form> [seed]\n"); return 2; }
    const char *f = argv[1];
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    bool ok;
    // the instances of the kernels: fxg_kernel_rows_multi<10,4> <14,3> <20,2>, fxg_kernel_rows<26,*> <38,*> (a piece of an H = 2 read is packed like a read)
    if (!std::strcmp(f, "nw10")) ok = check_form<10, 4>(rng);
    else if (!std::strcmp(f, "nw14")) ok = check_form<14, 3>(rng);
    else if (!std::strcmp(f, "nw20")) ok = check_form<20, 2>(rng);
    else if (!std::strcmp(f, "nw26")) ok = check_form<26, 1>(rng);
    else if (!std::strcmp(f, "nw38")) ok = check_form<38, 1>(rng);
    else { std::fprintf(stderr, "unknown form %s\n", f); return 2; }
    if (!ok) return 1;
    if (!g_al[0] || !g_al[1] || !g_al[2] || !g_al[3]) { std::printf("FAIL %s: not every D & 3 was covered\n", f); return 1; }
    std::printf("ok %s: %llu tiles, %llu stores, reads at D & 3 = 0..3: %llu %llu %llu %llu\n", f, g_tiles, g_stores, g_al[0], g_al[1], g_al[2], g_al[3]);
    return 0;
}
