// fxg_uncollapse.h -- fastx_uncollapser on the device: collapsed FASTA (">id-count\nBASES\n") expanded, every record written `count` times
// under a running number (reference src/fastx_uncollapser/fastx_uncollapser.cpp:73-98, src/libfastx/fastx.c:440-495).
//
// The block has been through fxg_fastq_index with two lines per record: ls / le are its line starts and chomped line ends, len[r] the bases
// of record r.  Copy g of the block (0-based, in input order) is ">%llu\nBASES\n" with the number ordinal_base + g + 1.  The output can be
// many times the input, so a call writes a window of whole copies [copy_begin, copy_end) and the caller walks the block window by window;
// the scans are made by the call with copy_begin == 0 and stay in the context's workspace for the calls after it.  Launches, none of which
// waits on another workgroup:
//   counts     per record its read count (fxg_reads_count of its id line);
//   scan       the project's exclusive u64 scan: C[r], the copies before record r, C[n] their total;
//   sizes      per record its bytes, count * (len + 3) + the digits of its count numbers in closed form (fxg_dec_width_sum), and its pieces
//              beyond the first -- a piece is up to FXG_UC_PIECE consecutive copies of one record;
//   scan x 2   B[r], the bytes before record r, and P[r], the further pieces before it;
//   window     one thread: copy_end and out_bytes for this call's copy_begin and out_cap by binary search over the monotone
//              off(g) = B[r] + k * (len + 3) + D(base + 1 + C[r], k)  (g = C[r] + k), and the records and further pieces the window touches --
//              the host reads them before the copy is launched;
//   copy       heads: a group of 16 lanes per record of the window writes its first piece, no search (most records have count 1);
//              tails: a group per further piece of the window finds its record by binary search over P.  Either clips its piece to the window.
// Sizes: byte offsets, copies and pieces are u64.  A block holds at most FXG_UC_TEXT_MAX = 2^28 bytes of text: a record takes at least four
// of them (">\nA\n"), so there are at most 2^26 records and the sum of (len + 23) over them stays below 2^31; a count is below 2^31 (an int),
// so the block's bytes stay below 2^62, its copies below 2^57, and no scan can wrap -- the bound is stated, overflow is not detected.
// The per-item bodies are __host__ __device__ so that the CPU emulator runs the same code.
#pragma once
#include "fxg_barcode.h"      // fxg_bc_copy
#include "fxg_kernels.h"      // (fxg_text.h names its result bits)
#include "fxg_text.h"         // fxg_reads_count, fxg_dec_width_sum, fxg_dec_width

#define FXG_UC_PIECE 16u                  // copies of one record that one group of 16 lanes writes
#define FXG_UC_TEXT_MAX (1ull << 28)      // bytes of text in a block at most (see above)
// How a group's 16 lanes share a piece.  0 (the product's build): the piece's copies one after the other, 16 lanes to a copy through fxg_bc_copy.
// 1 (-DFXG_UC_SIDE_BY_SIDE=1: scripts/bench_uncollapse.py builds that library beside the product's, the CPU tier runs both through the emulator):
// lane l builds copy l of the piece alone.  Both give the same bytes; DESIGN.md 3.8 has what was measured.
#ifndef FXG_UC_SIDE_BY_SIDE
#define FXG_UC_SIDE_BY_SIDE 0
#endif

struct FxgUcArgs {
    const uint8_t *text;
    const u32 *ls, *le;               // line starts and chomped ends: record r's id line is 2r, its bases line 2r + 1
    const uint16_t *len;              // bases of record r
    u64 n;                            // records; the arrays hold n + 1 entries (the last one a scan's total)
    u64 base;                         // ordinal_base: copy g is named base + g + 1
    u64 *cnt, *size, *pieces;         // counts, bytes, further pieces; then their exclusive scans C, B, P
    u64 *res;                         // FXG_UC_RES_* words, written by the window kernel
    uint8_t *out;
};
enum { FXG_UC_RES_COPIES = 0, FXG_UC_RES_COPY_END, FXG_UC_RES_OUT_BYTES, FXG_UC_RES_OFF_BEGIN, FXG_UC_RES_R_LO, FXG_UC_RES_R_HI, FXG_UC_RES_P_LO, FXG_UC_RES_P_HI,
       FXG_UC_RES_NEED, FXG_UC_RES_WORDS = 16 };
// a call's window as the copy kernels get it: copies [g0, g1), the byte offset of copy g0 in the block's output, records [r_lo, r_hi] and
// further pieces [p_lo, p_hi) that hold copies of the window
struct FxgUcWindow { u64 g0, g1, off0, r_lo, r_hi, p_lo, p_hi; };

// ---- counts ----
FXG_HD u64 fxg_uc_count(const FxgUcArgs &a, u64 r) { return r < a.n ? (u64)fxg_reads_count(a.text, a.ls[2 * r] + 1u, a.le[2 * r]) : 0ull; }

// ---- sizes: the bytes of the first k copies of record r (k <= its count), the closed form behind off(g) ----
FXG_HD u64 fxg_uc_bytes(const FxgUcArgs &a, u64 r, u64 k)
{
    if (!k) return 0ull;                                                 // (r == n has no length: asked only with k == 0)
    return k * ((u64)a.len[r] + 3ull) + fxg_dec_width_sum(a.base + 1ull + a.cnt[r], k);
}
FXG_HD void fxg_uc_size(const FxgUcArgs &a, u64 r, u64 *size, u64 *pieces)
{
    if (r >= a.n) { *size = 0ull; *pieces = 0ull; return; }
    const u64 count = a.cnt[r + 1] - a.cnt[r];                           // >= 1
    *size = fxg_uc_bytes(a, r, count);
    *pieces = (count - 1ull) / FXG_UC_PIECE;
}

// the last i in [0, entries) with scan[i] <= v (scan: an exclusive scan, scan[0] = 0 <= v)
FXG_HD u64 fxg_uc_find(const u64 *scan, u64 entries, u64 v)
{
    u64 lo = 0, hi = entries;                                            // scan[lo] <= v < scan[hi] (hi == entries: past the end)
    while (hi - lo > 1ull) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (scan[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- window: one thread, after the scans ----
FXG_HD void fxg_uc_window(const FxgUcArgs &a, u64 g0, u64 out_cap)
{
    const u64 n = a.n, copies = a.cnt[n];
    for (u32 i = 0; i < FXG_UC_RES_WORDS; ++i) a.res[i] = 0ull;
    a.res[FXG_UC_RES_COPIES] = copies;
    a.res[FXG_UC_RES_COPY_END] = g0;
    if (g0 > copies || a.base > ~0ull - copies) return;                 // refused by the host; nothing below is used
    // counts are >= 1, so C is strictly increasing: the record of copy g0 (n for g0 == copies, whose offset is the total)
    const u64 r0 = fxg_uc_find(a.cnt, n + 1, g0);
    const u64 off0 = a.size[r0] + fxg_uc_bytes(a, r0, g0 - a.cnt[r0]);
    const u64 limit = out_cap > ~0ull - off0 ? ~0ull : off0 + out_cap;   // the last byte offset a whole copy may end at
    const u64 r1 = fxg_uc_find(a.size, n + 1, limit);                     // B is strictly increasing over the records: the last record that starts at or below the limit
    u64 g1 = copies;
    if (r1 < n) {                                                        // the largest k with off(C[r1] + k) <= limit; k == 0 holds
        u64 lo = 0, hi = a.cnt[r1 + 1] - a.cnt[r1];                      // holds for lo, not for hi (the next record starts past the limit)
        while (hi - lo > 1ull) {
            const u64 mid = lo + ((hi - lo) >> 1);
            if (a.size[r1] + fxg_uc_bytes(a, r1, mid) <= limit) lo = mid; else hi = mid;
        }
        g1 = a.cnt[r1] + lo;
    }
    if (g1 < g0) g1 = g0;                                                // (cannot happen: off(g0) == off0 <= limit)
    a.res[FXG_UC_RES_COPY_END] = g1;
    a.res[FXG_UC_RES_OFF_BEGIN] = off0;
    if (g0 < copies) a.res[FXG_UC_RES_NEED] = (u64)a.len[r0] + 3ull + fxg_dec_width(a.base + 1ull + g0);
    if (g1 == g0) return;
    const u64 rh = fxg_uc_find(a.cnt, n + 1, g1 - 1ull);                 // < n
    const u64 j0 = (g0 - a.cnt[r0]) / FXG_UC_PIECE, j1 = (g1 - 1ull - a.cnt[rh]) / FXG_UC_PIECE;
    a.res[FXG_UC_RES_OUT_BYTES] = a.size[rh] + fxg_uc_bytes(a, rh, g1 - a.cnt[rh]) - off0;
    a.res[FXG_UC_RES_R_LO] = r0; a.res[FXG_UC_RES_R_HI] = rh;
    a.res[FXG_UC_RES_P_LO] = a.pieces[r0] + (j0 ? j0 - 1ull : 0ull);     // further piece j of record r is piece P[r] + j - 1 of the block
    a.res[FXG_UC_RES_P_HI] = a.pieces[rh] + j1;
}

// ---- copy ----
// one copy at d: '>', the digits of id (w of them), '\n', the bases, '\n', by the `lanes` lanes that share it (lane l)
FXG_HD void fxg_uc_put(uint8_t *d, const uint8_t *src, u32 len, u64 id, u32 w, u32 l, u32 lanes)
{
    if (l == 0u) { d[0] = '>'; d[1u + w] = '\n'; d[2u + w + len] = '\n'; }
    if (l == lanes - 1u) { u64 v = id; for (u32 k = w; k-- > 0u; v /= 10ull) d[1u + k] = (uint8_t)('0' + v % 10ull); }
    fxg_bc_copy(d + 2u + w, src, len, l, lanes);
}

// piece j of record r by lane l of its group of 16: copies [16 j, 16 j + 16) of the record, clipped to its count and to the window
FXG_HD void fxg_uc_copy_piece(const FxgUcArgs &a, const FxgUcWindow &w, u64 r, u64 j, u32 l)
{
    const u64 c0 = a.cnt[r], count = a.cnt[r + 1] - c0;
    u64 klo = j * FXG_UC_PIECE, khi = klo + FXG_UC_PIECE;
    if (khi > count) khi = count;
    if (w.g0 > c0 && w.g0 - c0 > klo) klo = w.g0 - c0;
    if (w.g1 <= c0) return;
    if (w.g1 - c0 < khi) khi = w.g1 - c0;
    if (klo >= khi) return;
    const u32 len = a.len[r];
    const uint8_t *src = a.text + a.ls[2 * r + 1];
    if (FXG_UC_SIDE_BY_SIDE) {
        // every lane builds a copy of its own: lane l the copy klo + l, its place in closed form
        const u64 k = klo + l;
        if (k >= khi) return;
        const u64 id = a.base + 1ull + c0 + k;
        fxg_uc_put(a.out + (a.size[r] + fxg_uc_bytes(a, r, k) - w.off0), src, len, id, fxg_dec_width(id), 0u, 1u);
        return;
    }
    // the group writes the piece's copies one after the other, 16 lanes to a copy
    uint8_t *d = a.out + (a.size[r] + fxg_uc_bytes(a, r, klo) - w.off0);
    for (u64 k = klo; k < khi; ++k) {
        const u64 id = a.base + 1ull + c0 + k;
        const u32 dw = fxg_dec_width(id);
        fxg_uc_put(d, src, len, id, dw, l, 16u);
        d += (u64)len + 3ull + dw;
    }
}

// head h of the window: the first piece of record r_lo + h
FXG_HD void fxg_uc_copy_head(const FxgUcArgs &a, const FxgUcWindow &w, u64 h, u32 l) { fxg_uc_copy_piece(a, w, w.r_lo + h, 0ull, l); }
// further piece p of the block (p_lo <= p < p_hi): piece p - P[r] + 1 of its record
FXG_HD void fxg_uc_copy_tail(const FxgUcArgs &a, const FxgUcWindow &w, u64 p, u32 l)
{
    const u64 r = fxg_uc_find(a.pieces, a.n + 1, p);                     // the last record with P[r] <= p: records without further pieces share their successor's P and lose
    fxg_uc_copy_piece(a, w, r, p - a.pieces[r] + 1ull, l);
}

// ---- host side of fxg_fasta_uncollapse, one copy for the engine and tests/emu ----
static inline int fxg_uc_check(const uint8_t *text, u64 text_len, const u32 *line, u64 cap_lines, u64 n, const uint16_t *len, const fxg_uncollapse_opts *o, fxg_uncollapse_info *info,
                               char *err, size_t cap)
{
    if (!o || !info) return FXG_E_INVALID;
    memset(info, 0, sizeof *info);
    if (n && (!text || !line || !len)) return FXG_E_INVALID;
    if (text_len > FXG_UC_TEXT_MAX) FXG_PLAN_FAIL("fxg_fasta_uncollapse: a block of %llu bytes; at most %llu, so that no byte offset can pass 2^63", (unsigned long long)text_len, (unsigned long long)FXG_UC_TEXT_MAX);
    if (2 * n + 1 > cap_lines && n) FXG_PLAN_FAIL("fxg_fasta_uncollapse: %llu records need more than %llu lines", (unsigned long long)n, (unsigned long long)cap_lines);
    if (4 * n > text_len) FXG_PLAN_FAIL("fxg_fasta_uncollapse: %llu records do not fit %llu bytes of text", (unsigned long long)n, (unsigned long long)text_len);
    return FXG_OK;
}
// u64 words of the workspace for n records: three arrays of n + 1 entries, the levels of a scan, the result words
static inline u64 fxg_uc_level_words(u64 entries) { return entries / 512 + 64; }
static inline u64 fxg_uc_ws_words(u64 n) { return 3 * (n + 1) + fxg_uc_level_words(n + 1) + FXG_UC_RES_WORDS; }
static inline FxgUcArgs fxg_uc_args(const uint8_t *text, const u32 *line, u64 cap_lines, u64 n, const uint16_t *len, u64 base, u64 *ws, uint8_t *out)
{
    FxgUcArgs a;
    const u64 M = n + 1;
    a.text = text; a.ls = line; a.le = line + cap_lines; a.len = len; a.n = n; a.base = base;
    a.cnt = ws; a.size = ws + M; a.pieces = ws + 2 * M;
    a.res = ws + 3 * M + fxg_uc_level_words(M);
    a.out = out;
    return a;
}
static inline u64 *fxg_uc_levels(const FxgUcArgs &a) { return a.pieces + (a.n + 1); }
// the window's results, once they are on the host: refused (nothing has been written), or the caller's info and the copy kernels' window
static inline int fxg_uc_results(const u64 *res, const fxg_uncollapse_opts *o, bool has_out, fxg_uncollapse_info *info, FxgUcWindow *w, char *err, size_t cap)
{
    const u64 copies = res[FXG_UC_RES_COPIES];
    if (o->ordinal_base > ~0ull - copies) FXG_PLAN_FAIL("fxg_fasta_uncollapse: %llu copies numbered from %llu on pass 2^64 - 1", (unsigned long long)copies, (unsigned long long)o->ordinal_base + 1ull);
    if (o->copy_begin > copies) FXG_PLAN_FAIL("fxg_fasta_uncollapse: copy_begin %llu, the block has %llu copies", (unsigned long long)o->copy_begin, (unsigned long long)copies);
    if (o->copy_begin < copies && res[FXG_UC_RES_COPY_END] == o->copy_begin)
        FXG_PLAN_FAIL("fxg_fasta_uncollapse: copy %llu needs %llu bytes, d_out takes %llu", (unsigned long long)o->copy_begin, (unsigned long long)res[FXG_UC_RES_NEED], (unsigned long long)o->out_cap);
    if (res[FXG_UC_RES_OUT_BYTES] && !has_out) return FXG_E_INVALID;
    info->copies = copies; info->copy_end = res[FXG_UC_RES_COPY_END]; info->out_bytes = res[FXG_UC_RES_OUT_BYTES];
    w->g0 = o->copy_begin; w->g1 = res[FXG_UC_RES_COPY_END]; w->off0 = res[FXG_UC_RES_OFF_BEGIN];
    w->r_lo = res[FXG_UC_RES_R_LO]; w->r_hi = res[FXG_UC_RES_R_HI]; w->p_lo = res[FXG_UC_RES_P_LO]; w->p_hi = res[FXG_UC_RES_P_HI];
    return FXG_OK;
}

#ifndef FXG_HOST_EMULATION
__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_uc_counts(const FxgUcArgs a)
{
    const u64 r = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x;
    if (r <= a.n) a.cnt[r] = fxg_uc_count(a, r);
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_uc_sizes(const FxgUcArgs a)
{
    const u64 r = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x;
    if (r <= a.n) {
        u64 sz, pc;
        fxg_uc_size(a, r, &sz, &pc);
        a.size[r] = sz; a.pieces[r] = pc;
    }
}

__global__ void fxg_kernel_uc_window(const FxgUcArgs a, u64 g0, u64 out_cap) { fxg_uc_window(a, g0, out_cap); }

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_uc_copy_heads(const FxgUcArgs a, const FxgUcWindow w)
{
    const u64 h = ((u64)blockIdx.x * FXG_BLOCK + threadIdx.x) >> 4;
    if (h <= w.r_hi - w.r_lo) fxg_uc_copy_head(a, w, h, threadIdx.x & 15u);
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_uc_copy_tails(const FxgUcArgs a, const FxgUcWindow w)
{
    const u64 p = w.p_lo + (((u64)blockIdx.x * FXG_BLOCK + threadIdx.x) >> 4);
    if (p < w.p_hi) fxg_uc_copy_tail(a, w, p, threadIdx.x & 15u);
}
#endif  // FXG_HOST_EMULATION
