// fxg_barcode.h -- fastx_barcode_splitter on the device: a stable (K+1)-way partition of the records of a block of text.
//
// The reference (scripts/fastx_barcode_splitter.pl) compares every read's barcode window with every entry of its barcode table and
// writes the record to the file of the first entry with the fewest mismatches.  Here that is three launches without any wait between
// workgroups:
//   classify  one lane per record: the window (<= 64 bytes at the start or the end of the bases line) as two bit planes of 2-bit
//             codes plus a mask of non-ACGT bytes and a mask of NUL bytes; per table entry XOR, fold, mask and popcount; the first
//             minimum wins.  Writes rec_bin[r], per tile of FXG_BC_TILE records the bytes that went to each bin, and adds the tile's
//             records and bytes per bin to the bins' totals;
//   scan      an exclusive scan of those per-(bin, tile) byte counts in bin-major order (fxg_scan_u64): the offset of each tile's
//             share of each bin in an output laid out as bin 0's slice, bin 1's slice, ...;
//   scatter   every record ranked inside its tile among the earlier records of its bin, then copied there by 16 lanes.
// The per-record bodies are __host__ __device__ so that the CPU emulator can run them.
#pragma once
#include "fxg_device.h"

#define FXG_BC_TILE 256u              // records per tile = threads per workgroup of classify and scatter
#define FXG_BC_STAGE 256u             // table entries staged in LDS at a time by classify (one per thread).  With a global load per entry
                                      // inside the entry loop, 192 entries took 67 us on a 64 MB block, from LDS 44 (96 entries: 36 either way)

struct FxgBcEntry {                   // one table entry, as the classify loop reads it (wave-uniform)
    u64 b0, b1;                       // bit planes of the 2-bit codes of its bases (A 0, C 1, G 2, T 3), bit i = base i
    u64 m;                            // its length as a mask: bits 0 .. len - 1
    u32 pen;                          // barcode length - len: the bases a shortened (--partial) entry lacks count as mismatches
    u32 bin;
};

struct FxgBcWin {                     // one record's window
    u64 f0, f1;                       // bit planes of its codes
    u64 ok;                           // bytes that are upper-case A, C, G or T
    u64 nul;                          // NUL bytes
    u32 F;                            // window length = min(barcode length, bases)
};

// A/C/G/T -> 0/1/2/3 (any other byte gets some code and is kept out of every match by the `ok` mask)
FXG_HD u32 fxg_bc_code(u32 c) { return ((c >> 1) ^ (c >> 2)) & 3u; }
FXG_HD u32 fxg_bc_is_acgt(u32 c) { return (c == 'A') | (c == 'C') | (c == 'G') | (c == 'T'); }
FXG_HD u64 fxg_bc_lowmask(u32 n) { return n >= 64u ? ~0ull : ((1ull << n) - 1ull); }

FXG_HD void fxg_bc_add_byte(FxgBcWin &w, u32 c, u32 i)
{
    const u32 code = fxg_bc_code(c);
    w.f0 |= (u64)(code & 1u) << i;
    w.f1 |= (u64)(code >> 1) << i;
    w.ok |= (u64)fxg_bc_is_acgt(c) << i;
    w.nul |= (u64)(c == 0u) << i;
}

// The window of the bases line text[s, e) (e: its '\n'): its first F bytes (bol) or its last F (eol), F = min(BL, e - s).  Read as
// dwords from the dword boundary at or below its start to the one that holds its last byte: never before a 4-byte aligned `text`,
// never past the line's '\n' + 3.
FXG_HD FxgBcWin fxg_bc_window(const uint8_t *text, u32 s, u32 e, u32 BL, u32 eol)
{
    FxgBcWin w;
    w.f0 = w.f1 = w.ok = w.nul = 0ull;
    const u32 L = e - s;
    const u32 F = L < BL ? L : BL;
    w.F = F;
    if (F == 0u) return w;
    const u32 ws = eol ? e - F : s;
    const u32 a = ws & ~3u;
    const u32 span = ws + F - a;                                 // bytes from the first dword's start to the window's end: 1 .. F + 3
#pragma unroll
    for (u32 k = 0; k < (FXG_MAX_BARCODE + 4u) / 4u; ++k) {      // (unrolled: no lane-divergent loop with live-out values)
        const u32 q = a + 4u * k;
        if (4u * k < span) {                                     // (not q < ws + F: in the last 64 bytes below 2^32 q wraps and would admit a load of the block's first dword)
            u32 d;
            __builtin_memcpy(&d, text + q, 4);
#pragma unroll
            for (u32 j = 0; j < 4u; ++j) {
                const u32 p = q + j;
                if (p >= ws && p < ws + F) fxg_bc_add_byte(w, (d >> (8u * j)) & 0xFFu, p - ws);
            }
        }
    }
    return w;
}

// one table entry from its bases (upper-case A/C/G/T, len <= BL <= 64); false if a base is anything else
FXG_HD bool fxg_bc_encode_entry(const uint8_t *bases, u32 len, u32 BL, u32 bin, FxgBcEntry &e)
{
    e.b0 = e.b1 = 0ull;
    for (u32 i = 0; i < len; ++i) {
        if (!fxg_bc_is_acgt(bases[i])) return false;
        const u32 code = fxg_bc_code(bases[i]);
        e.b0 |= (u64)(code & 1u) << i;
        e.b1 |= (u64)(code >> 1) << i;
    }
    e.m = fxg_bc_lowmask(len);
    e.pen = BL - len;
    e.bin = bin;
    return true;
}

// mismatches of the window against one entry: F - (window bytes equal to the entry's bases) - (NUL window bytes past the entry's end) +
// (bases the entry lacks).  The NUL term is the reference's: it counts the NUL bytes of a string XOR, whose tail past the shorter string
// is the longer one's own bytes.
FXG_HD u32 fxg_bc_mm(const FxgBcWin &w, const FxgBcEntry &e)
{
    const u64 eq = ~((w.f0 ^ e.b0) | (w.f1 ^ e.b1)) & w.ok & e.m;
    return w.F + e.pen - (u32)__builtin_popcountll(eq) - (u32)__builtin_popcountll(w.nul & ~e.m);
}

// The reference's choice: a running best that starts at BL and is replaced only by a strictly smaller count, then `unmatched` unless the
// best is within the allowed mismatches.
FXG_HD u32 fxg_bc_classify_one(const FxgBcWin &w, const FxgBcEntry *tab, u32 entries, u32 BL, u32 mismatches, u32 unmatched)
{
    u32 best = BL, bin = unmatched;
    for (u32 k = 0; k < entries && best != 0u; ++k) {
        const u32 mm = fxg_bc_mm(w, tab[k]);
        if (mm < best) { best = mm; bin = tab[k].bin; }
    }
    return best <= mismatches ? bin : unmatched;
}

// the bases line of record r is line LPR * r + 1; the record is text[ls[LPR * r], ls[LPR * (r + 1)])
FXG_HD u32 fxg_bc_record_bin(const uint8_t *text, const u32 *ls, u32 lpr, u64 r, const FxgBcEntry *tab, u32 entries, u32 BL, u32 mismatches,
                             u32 eol, u32 unmatched)
{
    const u32 s = ls[lpr * r + 1], e = ls[lpr * r + 2] - 1u;
    return fxg_bc_classify_one(fxg_bc_window(text, s, e, BL, eol), tab, entries, BL, mismatches, unmatched);
}

// n bytes from src (any alignment) to dst (any alignment) by `lanes` cooperating lanes: head bytes up to dst's next 16-byte boundary,
// aligned 16-byte stores, tail bytes.  Touches exactly dst[0, n) and src[0, n).
FXG_HD void fxg_bc_copy(uint8_t *dst, const uint8_t *src, u64 n, u32 l, u32 lanes)
{
    u64 head = (16u - (u32)((uintptr_t)dst & 15u)) & 15u;
    if (head > n) head = n;
    const u64 full = (n - head) >> 4;
    for (u64 i = l; i < head; i += lanes) dst[i] = src[i];
    for (u64 k = l; k < full; k += lanes) {
        const u32x4 v = fxg_ld16(src + head + (k << 4));
        *reinterpret_cast<u32x4 *>(dst + head + (k << 4)) = v;
    }
    for (u64 i = head + (full << 4) + l; i < n; i += lanes) dst[i] = src[i];
}

// byte offset of tile member i inside its bin's share of the tile: the sizes of the earlier members of the same bin
// (a loop of uniform length: every lane reads the same LDS word at the same time)
FXG_HD u32 fxg_bc_rank_bytes(const u32 *bin, const u32 *size, u32 i)
{
    const u32 mine = bin[i];
    u32 off = 0;
    for (u32 j = 0; j < FXG_BC_TILE; ++j) off += (j < i && bin[j] == mine) ? size[j] : 0u;
    return off;
}

struct FxgBcArgs {
    const uint8_t *text;
    const u32 *ls;                    // line starts (fxg_fastq_index's first half)
    u64 n;                            // records
    u32 lpr;
    u32 tiles;
    const FxgBcEntry *tab;
    u32 entries, BL, mismatches, eol, bins;   // unmatched = bins - 1
    uint16_t *rec_bin;
    u64 *hist_bytes;                  // [bins * tiles], bin-major; after the scan: the output offset of (bin, tile)
    uint8_t *out;
    u64 *totals;                      // [2 * bins], zeroed before classify: bytes per bin, then records per bin
};

// ---- host side of fxg_barcode_prepare / _split, one copy for the engine and tests/emu ----
static inline int fxg_bc_set_check(const fxg_barcode_set *set, char *err, size_t cap)
{
    const u32 E = set->entries, BL = set->barcode_len;
    if (set->bins < 1 || set->bins > FXG_MAX_BARCODE_BINS) FXG_PLAN_FAIL("barcode split: %u bins (1 .. %d)", set->bins, FXG_MAX_BARCODE_BINS);
    if (BL > FXG_MAX_BARCODE || (E > 0 && BL == 0)) FXG_PLAN_FAIL("barcode length %u (1 .. %d)", BL, FXG_MAX_BARCODE);
    if (E > 0 && (!set->bases || !set->len || !set->bin)) FXG_PLAN_FAIL("barcode table without bases / lengths / bins");
    return FXG_OK;
}
static inline int fxg_bc_set_encode(const fxg_barcode_set *set, FxgBcEntry *tab, char *err, size_t cap)      // the entries of a checked set into tab[set->entries]
{
    for (u32 k = 0; k < set->entries; ++k) {
        const u32 L = set->len[k];
        if (L > set->barcode_len || set->bin[k] >= set->bins) FXG_PLAN_FAIL("barcode entry %u: length %u, bin %u", k, L, set->bin[k]);
        if (!fxg_bc_encode_entry(set->bases + (size_t)k * FXG_MAX_BARCODE, L, set->barcode_len, set->bin[k], tab[k])) FXG_PLAN_FAIL("barcode entry %u: a base that is not A, C, G or T", k);
    }
    return FXG_OK;
}
// what a split needs (bins: of the prepared table, 0 = there is none), and the empty totals: the caller has nothing more to do for n == 0
static inline int fxg_bc_split_check(u32 bins, const uint8_t *text, u64 text_len, int lpr, const u32 *line, u64 cap_lines, u64 n, const uint8_t *out, uint64_t *bin_bytes, uint64_t *bin_records,
                                     char *err, size_t cap)
{
    if (!text || !line || !bin_bytes || !bin_records || !fxg_text_lpr_ok(lpr)) return FXG_E_INVALID;
    if (!bins) FXG_PLAN_FAIL("fxg_barcode_split: no table (fxg_barcode_prepare)");
    memset(bin_bytes, 0, bins * sizeof(uint64_t));
    memset(bin_records, 0, bins * sizeof(uint64_t));
    if (n == 0) return FXG_OK;
    if (!out) return FXG_E_INVALID;
    if (((uintptr_t)text & 3u) != 0) FXG_PLAN_FAIL("fxg_barcode_split: the text must be 4-byte aligned");
    if (fxg_text_check_len(text_len, err, cap) != FXG_OK) return FXG_E_INVALID;
    if ((u64)lpr * n + 1 > cap_lines) FXG_PLAN_FAIL("fxg_barcode_split: %llu records need more than %llu lines", (unsigned long long)n, (unsigned long long)cap_lines);
    return FXG_OK;
}

#ifndef FXG_HOST_EMULATION
// classify: one lane per record.  The table goes through LDS FXG_BC_STAGE entries at a time (every lane then reads the same entry: a
// broadcast); a wave skips the rest of the table once every lane has found an entry with no mismatch, after which no later entry can win.
__global__ __launch_bounds__(FXG_BC_TILE) void fxg_kernel_bc_classify(const FxgBcArgs a)
{
    extern __shared__ u32 bc_lds[];                // [bins] records, [bins] bytes
    __shared__ FxgBcEntry s_tab[FXG_BC_STAGE];
    u32 *h_recs = bc_lds, *h_bytes = bc_lds + a.bins;
    for (u32 b = threadIdx.x; b < a.bins; b += FXG_BC_TILE) { h_recs[b] = 0u; h_bytes[b] = 0u; }
    const u64 r = (u64)blockIdx.x * FXG_BC_TILE + threadIdx.x;
    const bool live = r < a.n;
    const u32 unmatched = a.bins - 1u;
    FxgBcWin w;
    w.f0 = w.f1 = w.ok = w.nul = 0ull; w.F = 0u;
    u32 size = 0u;
    if (live) {
        const u64 b0 = (u64)a.lpr * r;
        const u32 s = a.ls[b0 + 1], e = a.ls[b0 + 2] - 1u;
        size = a.ls[b0 + a.lpr] - a.ls[b0];
        w = fxg_bc_window(a.text, s, e, a.BL, a.eol);
    }
    u32 best = live ? a.BL : 0u, bin = unmatched;
    for (u32 k0 = 0; k0 < a.entries; k0 += FXG_BC_STAGE) {
        const u32 m = a.entries - k0 < FXG_BC_STAGE ? a.entries - k0 : FXG_BC_STAGE;
        __syncthreads();
        if (threadIdx.x < m) s_tab[threadIdx.x] = a.tab[k0 + threadIdx.x];
        __syncthreads();
        if (__all(best == 0u)) continue;
        for (u32 k = 0; k < m; ++k) {
            const FxgBcEntry e = s_tab[k];
            const u32 mm = fxg_bc_mm(w, e);
            if (mm < best) { best = mm; bin = e.bin; }
        }
    }
    if (best > a.mismatches) bin = unmatched;
    __syncthreads();
    if (live) {
        a.rec_bin[r] = (uint16_t)bin;
        atomicAdd(&h_recs[bin], 1u);
        atomicAdd(&h_bytes[bin], size);
    }
    __syncthreads();
    for (u32 b = threadIdx.x; b < a.bins; b += FXG_BC_TILE) {
        const u32 c = h_recs[b], y = h_bytes[b];
        a.hist_bytes[(u64)b * a.tiles + blockIdx.x] = y;
        if (c) { atomicAdd(&a.totals[b], (u64)y); atomicAdd(&a.totals[a.bins + b], (u64)c); }
    }
}

// scatter: each tile's records ranked within their bins (LDS, in input order), then copied by groups of 16 lanes
__global__ __launch_bounds__(FXG_BC_TILE) void fxg_kernel_bc_scatter(const FxgBcArgs a)
{
    __shared__ u32 s_bin[FXG_BC_TILE], s_size[FXG_BC_TILE], s_src[FXG_BC_TILE];
    __shared__ u64 s_dst[FXG_BC_TILE];
    const u64 r0 = (u64)blockIdx.x * FXG_BC_TILE;
    const u64 r = r0 + threadIdx.x;
    const u32 i = threadIdx.x;
    u32 bin = 0xFFFFFFFFu, size = 0u, src = 0u;
    if (r < a.n) {
        const u64 b0 = (u64)a.lpr * r;
        bin = a.rec_bin[r];
        src = a.ls[b0];
        size = a.ls[b0 + a.lpr] - src;
    }
    s_bin[i] = bin; s_size[i] = size; s_src[i] = src;
    __syncthreads();
    if (r < a.n) s_dst[i] = a.hist_bytes[(u64)bin * a.tiles + blockIdx.x] + fxg_bc_rank_bytes(s_bin, s_size, i);
    __syncthreads();
    const u64 live = a.n - r0 < FXG_BC_TILE ? a.n - r0 : FXG_BC_TILE;
    for (u32 k = i >> 4; k < live; k += FXG_BC_TILE / 16u)
        fxg_bc_copy(a.out + s_dst[k], a.text + s_src[k], s_size[k], i & 15u, 16u);
}
#endif  // FXG_HOST_EMULATION
