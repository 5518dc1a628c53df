// fxg_nucchange.h -- fasta_nucleotide_changer on the device: the bases lines of an indexed block rewritten in place, T -> U (-r) or U -> T (-d)
// (reference src/fasta_nucleotide_changer/fasta_nucleotide_changer.c:101-115).
//
// The block has been through fxg_fastq_index: ls / le are its line starts and chomped line ends, record r's bases line is line lpr * r + 1.
// One launch of at most FXG_NC_GRID_MAX workgroups, nothing waits on another workgroup, no LDS.  A group of 16 lanes takes one record at a time,
// group g of G the records g, g + G, g + 2 G, ...; a record's bases [s, e) are dealt to the group's lanes as
// items: item 0 is the ragged head, the bytes before the first 16-byte aligned address of the line; items 1 .. full are the aligned 16-byte
// pieces that lie whole inside the line; item full + 1 is the ragged tail.  Lane l takes the items l, l + 16, ...  Every item is fetched by
// one 16-byte load (an unaligned one for the head), checked and counted by SWAR compares on its four dwords under a byte mask of the item's
// own bytes, and written back only if a byte of it changed: an aligned piece by one 16-byte store, a head or a tail byte by byte, only the
// bytes that changed.  So no lane ever stores a byte outside its own record's bases line -- two records whose lines share an aligned piece
// (">1\nAC\n>2\nTT\n") both reach it through their heads and tails, by bytes -- and nothing is written at or past a line's chomped end:
// a CR stays, ids, '+' lines and quality lines are never touched.  Loads end at most 15 bytes past e <= text_len, inside the 16 bytes of slack
// the text path guarantees behind the text.
// Results: a lane sums its `from` bytes over its trips, the wave sums its lanes, and one 64-bit atomic per wave adds that to one of
// FXG_NC_SLOTS counters a cache line apart; the host adds the slots up.  (A form with a group per record, no trips and one counter was 13.9
// times slower on 64 MB of 150-base FASTA; that its 104 000 atomics on one address were the reason is supposed, not measured.)
// The smallest record with a `to` byte goes into a 64-bit atomicMin after a minimum over the wave, the alphabet bit into an atomicOr, one of
// each per wave at the most and none on regular input.
// Every `from` byte of the block is rewritten whatever else the block holds: a caller that finds a `to` record or an irregular bit takes its
// text from elsewhere.
// The per-lane body is __host__ __device__ so that the CPU emulator runs the same code.
#pragma once
#include "fxg_device.h"

#define FXG_NC_LANES 16u              // lanes that share a record
#define FXG_NC_NONE (~0ull)           // first_to_record: no record holds a `to` byte

struct FxgNcArgs {
    uint8_t *text;
    const u32 *ls, *le;               // line starts and chomped ends
    u64 n;                            // records
    u32 lpr;                          // lines per record: 2 or 4
    u32 from, to;                     // 'T','U' or 'U','T'
    u64 *res;                         // FXG_NC_RES_* words, zeroed / set to FXG_NC_NONE before the launch
};
#define FXG_NC_GRID_MAX 2048u         // workgroups of the launch at most (eight per CU of an MI355X): 32 768 records a trip
#define FXG_NC_SLOTS 16u              // counters the waves' sums are spread over, by workgroup
#define FXG_NC_SLOT_WORDS 16u         // u64 words from one counter to the next: 128 bytes
enum { FXG_NC_RES_FIRST_TO = 0, FXG_NC_RES_IRREGULAR = 1, FXG_NC_RES_CHANGED = 16, FXG_NC_RES_WORDS = 16 + 16 * 16 };      // [CHANGED + SLOT_WORDS * slot]: the slots' sums
#define FXG_NC_HAS_TO 1u              // a lane's flags: one of its bytes is `to`
#define FXG_NC_BAD    2u              // ... is outside upper-case A C G T N U

// bit 7 of every byte of w that equals the byte replicated in c4
FXG_HD u32 fxg_nc_eq_flags(u32 w, u32 c4) { return fxg_nonzero_flags(w ^ c4) ^ 0x80808080u; }

// nonzero if any byte of w selected by m (0x00 / 0xFF per byte) is not one of upper-case A C G T N U
FXG_HD u32 fxg_nc_invalid4(u32 w, u32 m)
{
    const u32 x = w ^ 0x40404040u;                          // A=01 C=03 G=07 N=0E T=14 U=15; lower case keeps bit 5, bytes of 0x80 and above bit 7
    const u32 LUT = (1u << 0x01) | (1u << 0x03) | (1u << 0x07) | (1u << 0x0E) | (1u << 0x14) | (1u << 0x15);
    const u32 nb = (~(LUT >> (x & 31u)) & m) | (~(LUT >> ((x >> 8) & 31u)) & (m >> 8)) |
                   (~(LUT >> ((x >> 16) & 31u)) & (m >> 16)) | (~(LUT >> ((x >> 24) & 31u)) & (m >> 24));
    return (x & 0xE0E0E0E0u & m) | (nb & 1u);
}

// one item: the `cnt` bytes at p (1 .. 16; 16 with `aligned`: a whole aligned piece).  Returns its `from` bytes, ORs the lane's flags.
FXG_HD u32 fxg_nc_item(const FxgNcArgs &a, uint8_t *p, u32 cnt, bool aligned, u32 *flags)
{
    const u32x4 v = fxg_ld16(p);
    const u32x4 m = fxg_lowmask16((int)cnt);
    const u32 f4 = a.from * 0x01010101u, t4 = a.to * 0x01010101u;
    const u32 w[4] = {v.x, v.y, v.z, v.w}, mk[4] = {m.x, m.y, m.z, m.w};
    u32 hit[4], any_to = 0, bad = 0, cnt_from = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        hit[i] = fxg_nc_eq_flags(w[i], f4) & mk[i];         // bit 7 of every `from` byte of the item
        any_to |= fxg_nc_eq_flags(w[i], t4) & mk[i];
        bad |= fxg_nc_invalid4(w[i], mk[i]);
        cnt_from += (u32)__builtin_popcount(hit[i]);
    }
    if (any_to) *flags |= FXG_NC_HAS_TO;
    if (bad) *flags |= FXG_NC_BAD;
    if (!cnt_from) return 0u;
    const u32 d4 = (a.from ^ a.to) * 0x01010101u;
    if (aligned) {
        // (hit >> 7) * 0xFF: 0xFF in every `from` byte
        const u32x4 o = {w[0] ^ (((hit[0] >> 7) * 0xFFu) & d4), w[1] ^ (((hit[1] >> 7) * 0xFFu) & d4), w[2] ^ (((hit[2] >> 7) * 0xFFu) & d4), w[3] ^ (((hit[3] >> 7) * 0xFFu) & d4)};
        *reinterpret_cast<u32x4 *>(p) = o;
    } else {
        u32 bits = fxg_flags16(hit[0], hit[1], hit[2], hit[3]);
        while (bits) {
            const u32 b = (u32)__builtin_ctz(bits);
            bits &= bits - 1u;
            p[b] = (uint8_t)a.to;
        }
    }
    return cnt_from;
}

// record r by lane l of its group: the lane's share of the bases line.  Returns the `from` bytes it rewrote, ORs the lane's flags.
FXG_HD u32 fxg_nc_record(const FxgNcArgs &a, u64 r, u32 l, u32 *flags)
{
    const u64 li = (u64)a.lpr * r + 1ull;
    const u32 s = a.ls[li], e = a.le[li];
    if (e <= s) return 0u;                                   // (an empty bases line: the index pass has flagged the block)
    uint8_t *p = a.text + s;
    const u32 n = e - s;
    u32 head = (16u - (u32)((uintptr_t)p & 15u)) & 15u;
    if (head > n) head = n;
    const u32 full = (n - head) >> 4, tail = n - head - (full << 4);
    u32 changed = 0;
    for (u32 k = l; k < full + 2u; k += FXG_NC_LANES) {
        if (k == 0u) { if (head) changed += fxg_nc_item(a, p, head, false, flags); }
        else if (k <= full) changed += fxg_nc_item(a, p + head + ((k - 1u) << 4), 16u, true, flags);
        else if (tail) changed += fxg_nc_item(a, p + head + (full << 4), tail, false, flags);
    }
    return changed;
}

// ---- host side of fxg_bases_change, one copy for the engine and tests/emu ----
static inline int fxg_nc_check(const uint8_t *text, u64 text_len, int lpr, const u32 *line, u64 cap_lines, u64 n, int from, int to, fxg_bases_change_info *info, char *err, size_t cap)
{
    if (!info) FXG_PLAN_FAIL("fxg_bases_change: info is null");
    memset(info, 0, sizeof *info);
    info->first_to_record = FXG_NC_NONE;
    if (!((from == 'T' && to == 'U') || (from == 'U' && to == 'T'))) FXG_PLAN_FAIL("fxg_bases_change: from %d, to %d; 'T' to 'U' or 'U' to 'T'", from, to);
    if (!fxg_text_lpr_ok(lpr)) FXG_PLAN_FAIL("fxg_bases_change: lines_per_record %d; 2 (FASTA) or 4 (FASTQ)", lpr);
    if (n && (!text || !line)) FXG_PLAN_FAIL("fxg_bases_change: a null pointer with %llu records", (unsigned long long)n);
    if (fxg_text_check_len(text_len, err, cap) != FXG_OK) return FXG_E_INVALID;
    if (n && (u64)lpr * n + 1 > cap_lines) FXG_PLAN_FAIL("fxg_bases_change: %llu records need more than %llu lines", (unsigned long long)n, (unsigned long long)cap_lines);
    if (n > text_len / (2ull * (u64)lpr)) FXG_PLAN_FAIL("fxg_bases_change: %llu records do not fit %llu bytes of text", (unsigned long long)n, (unsigned long long)text_len);      // a line takes two bytes at least
    return FXG_OK;
}
static inline FxgNcArgs fxg_nc_args(uint8_t *text, int lpr, const u32 *line, u64 cap_lines, u64 n, int from, int to, u64 *res)
{
    FxgNcArgs a;
    a.text = text; a.ls = line; a.le = line + cap_lines; a.n = n; a.lpr = (u32)lpr; a.from = (u32)from; a.to = (u32)to; a.res = res;
    return a;
}
static inline void fxg_nc_res_init(u64 *res) { memset(res, 0, FXG_NC_RES_WORDS * sizeof(u64)); res[FXG_NC_RES_FIRST_TO] = FXG_NC_NONE; }
static inline void fxg_nc_results(const u64 *res, fxg_bases_change_info *info)
{
    info->changed = 0;
    for (u32 s = 0; s < FXG_NC_SLOTS; ++s) info->changed += res[FXG_NC_RES_CHANGED + FXG_NC_SLOT_WORDS * s];
    info->first_to_record = res[FXG_NC_RES_FIRST_TO];
    info->irregular = res[FXG_NC_RES_IRREGULAR] ? FXG_TEXT_IRR_BASE : 0u;
}
// workgroups of the launch: a group of FXG_NC_LANES lanes per record, FXG_NC_GRID_MAX workgroups at the most (the groups then take further trips)
static inline u64 fxg_nc_grid(u64 n) { const u64 g = (n * FXG_NC_LANES + FXG_BLOCK - 1) / FXG_BLOCK; return g < FXG_NC_GRID_MAX ? g : FXG_NC_GRID_MAX; }
// the counter of a workgroup's waves
FXG_HD u32 fxg_nc_slot(u64 workgroup) { return FXG_NC_RES_CHANGED + FXG_NC_SLOT_WORDS * (u32)(workgroup % FXG_NC_SLOTS); }
// group g of `groups`, lane l: its trips through the records.  Returns the `from` bytes the lane rewrote, ORs its flags, *first: its smallest record with a `to` byte
FXG_HD u64 fxg_nc_lane(const FxgNcArgs &a, u64 g, u64 groups, u32 l, u32 *flags, u64 *first)
{
    u64 changed = 0;
    for (u64 r = g; r < a.n; r += groups) {
        u32 f = 0;
        changed += fxg_nc_record(a, r, l, &f);
        if ((f & FXG_NC_HAS_TO) && *first == FXG_NC_NONE) *first = r;      // (r only grows)
        *flags |= f;
    }
    return changed;
}

#ifndef FXG_HOST_EMULATION
__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_bases_change(const FxgNcArgs a)
{
    const u64 g = ((u64)blockIdx.x * FXG_BLOCK + threadIdx.x) / FXG_NC_LANES, groups = (u64)gridDim.x * (FXG_BLOCK / FXG_NC_LANES);
    u32 flags = 0;
    u64 first = FXG_NC_NONE;
    u64 sum = fxg_nc_lane(a, g, groups, threadIdx.x & (FXG_NC_LANES - 1u), &flags, &first);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 lo = __shfl_down((u32)sum, d, 64), hi = __shfl_down((u32)(sum >> 32), d, 64);
        sum += ((u64)hi << 32) | lo;
    }
    if (fxg_lane() == 0 && sum) atomicAdd(a.res + fxg_nc_slot(blockIdx.x), sum);
    if (__ballot((flags & FXG_NC_HAS_TO) != 0u) != 0ull) {   // (wave-uniform, and rare: the run ends at that record)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const u64 o = ((u64)__shfl_xor((u32)(first >> 32), d, 64) << 32) | __shfl_xor((u32)first, d, 64);
            first = o < first ? o : first;
        }
        if (fxg_lane() == 0) atomicMin(a.res + FXG_NC_RES_FIRST_TO, first);
    }
    if (__ballot((flags & FXG_NC_BAD) != 0u) != 0ull && fxg_lane() == 0) atomicOr(a.res + FXG_NC_RES_IRREGULAR, 1ull);
}
#endif  // FXG_HOST_EMULATION
