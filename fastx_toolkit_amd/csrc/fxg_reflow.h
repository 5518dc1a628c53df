// fxg_reflow.h -- fasta_formatter on the device: multi-line FASTA text reflowed to one line per record, to lines of a fixed width, or to
// the tabular form (reference src/fasta_formatter/fasta_formatter.cpp:136-201, sequence_writers.h:31-109).
//
// A block of text is a list of lines (the newline kernels of fxg_text.h give their starts; a line's raw end is the next start minus 1,
// nothing is chomped).  A line is empty, a header (first byte '>') or a sequence line.  The block's items are its L lines plus one end
// item behind them, which stands for the end of input when the block is the last one.  Launches, none of which waits on another workgroup:
//   classify   per item its element (header flag, sequence bytes, 1);
//   segscan    a segmented exclusive scan of the elements, restarting at each header: every item learns whether a header precedes it in
//              the block, the bases of the open record before it (c) and how many items back that record's header lies (k);
//   sizes      per item the output bytes it owns and the pieces (<= FXG_RF_PIECE bytes of a line) its copy takes beyond the first;
//   scan x 2   the project's exclusive u64 scan over the sizes and over those further pieces;
//   finish     one thread: consumed, the carry for the next block, the totals -- the host checks them against out_cap before the copy;
//   copy       work is dealt by pieces of lines, not by lines (an unwrapped chromosome is one line of hundreds of MB).  A group of 16 lanes
//              per item writes what the item owns up to its line's first piece -- all of it for a line of a wrapped file, which needs no
//              search; a group per further piece finds its item by binary search over the scanned pieces (long lines only).
// Who owns what.  A record's header bytes ("H\n", or "H[1:]\t") go out with its first non-empty sequence line (c == 0).  What closes a
// record is written by the next header line or the end item: the '\n' that ends its last line of bases if one is due, or, for a record
// without bases when empty records are kept, its whole id line.  So nothing needs a look ahead, and the carry between blocks is one number:
// the bases already written for the open record, 0 if none is open.  Not at the end of input, the block's last header line is not consumed
// while no non-empty sequence line follows it: it closes the record before it here and is read again, as an opener, with the next block.
// The per-item bodies are __host__ __device__ so that the CPU emulator runs the same code.
#pragma once
#include "fxg_barcode.h"      // fxg_bc_copy

#define FXG_RF_PIECE 4096u            // bytes of one line that one group of 16 lanes copies
#define FXG_RF_SCAN_BLOCK 1024u       // items per workgroup of the segmented scan: fxg_text.h's FXG_SCAN_PER_BLOCK
#define FXG_RF_EMPTY 0u
#define FXG_RF_HEADER 1u
#define FXG_RF_SEQ 2u

struct FxgRfArgs {
    const uint8_t *text;
    const u32 *ls;                    // line starts ls[0 .. L]
    u64 L;                            // complete lines; items: L + 1, arrays: L + 2 entries (the last one holds a scan's total)
    u64 open_in;
    u32 width, tabular, keep_empty, at_eof;
    u64 *seg_s, *seg_kf;              // elements, then their segmented exclusive scan: bases | (items since the header << 1 | header seen)
    u64 *size, *pieces;               // per item its output bytes and its pieces beyond the first, then their exclusive scans
    u64 *res;                         // FXG_RF_RES_* words; [FXG_RF_RES_BAD] and [FXG_RF_RES_HEADERS] are zeroed before classify
    uint8_t *out;
};
enum { FXG_RF_RES_BAD = 0, FXG_RF_RES_HEADERS, FXG_RF_RES_CONSUMED, FXG_RF_RES_OUT_BYTES, FXG_RF_RES_OPEN, FXG_RF_RES_PIECES, FXG_RF_RES_WORDS = 8 };

// ---- the segmented operator: (f, s, k) o (f', s', k') = (f | f', f' ? s' : s + s', f' ? k' : k + k'), kf = k << 1 | f ----
struct FxgRfSeg { u64 s, kf; };
FXG_HD FxgRfSeg fxg_rf_combine(FxgRfSeg a, FxgRfSeg b)
{
    FxgRfSeg r;
    const bool reset = (b.kf & 1ull) != 0;
    r.s = reset ? b.s : a.s + b.s;
    r.kf = reset ? b.kf : a.kf + b.kf;      // (b's flag is 0 here: the sum keeps a's flag and adds the counts)
    return r;
}

// line i of the block: its kind and raw length
FXG_HD u32 fxg_rf_kind(const FxgRfArgs &a, u64 i, u32 *n)
{
    if (i >= a.L) { *n = 0u; return FXG_RF_EMPTY; }
    const u32 s = a.ls[i], len = a.ls[i + 1] - 1u - s;
    *n = len;
    if (len == 0u) return FXG_RF_EMPTY;
    return a.text[s] == '>' ? FXG_RF_HEADER : FXG_RF_SEQ;
}

// item i's element of the segmented scan; returns 1 for a header line
FXG_HD u32 fxg_rf_classify(const FxgRfArgs &a, u64 i)
{
    u32 n;
    const u32 kind = fxg_rf_kind(a, i, &n);
    a.seg_s[i] = kind == FXG_RF_SEQ ? (u64)n : 0ull;
    a.seg_kf[i] = 2ull | (kind == FXG_RF_HEADER ? 1ull : 0ull);
    return kind == FXG_RF_HEADER ? 1u : 0u;
}

// what the scan says about item i: a record is open before it, its bases so far, the line of its header (valid when seen in this block)
struct FxgRfBefore { bool open, seen; u64 c, hdr; };
FXG_HD FxgRfBefore fxg_rf_before(const FxgRfArgs &a, u64 i)
{
    FxgRfBefore b;
    const u64 kf = a.seg_kf[i];
    b.seen = (kf & 1ull) != 0;
    b.c = a.seg_s[i] + (b.seen ? 0ull : a.open_in);
    b.open = b.seen || a.open_in > 0ull;
    b.hdr = i - (kf >> 1);
    return b;
}
// the bytes a record's id line takes in front of its bases ("H\n" / "H[1:]\t") or alone ("H\n" / "H[1:]\n"): the same count either way
FXG_HD u64 fxg_rf_id_bytes(const FxgRfArgs &a, u64 hdr) { return (u64)(a.ls[hdr + 1] - a.ls[hdr]) - (a.tabular ? 1ull : 0ull); }
FXG_HD bool fxg_rf_wraps(const FxgRfArgs &a) { return a.width != 0u && !a.tabular; }

// output bytes of item i and the pieces of its line beyond the first; *bad: a sequence line with no record open (the caller's precondition)
FXG_HD void fxg_rf_size(const FxgRfArgs &a, u64 i, u64 *size, u64 *pieces, u32 *bad)
{
    u32 n;
    const u32 kind = fxg_rf_kind(a, i, &n);
    const FxgRfBefore b = fxg_rf_before(a, i);
    u64 sz = 0, pc = 0;
    *bad = 0u;
    if (kind == FXG_RF_SEQ) {
        if (!b.open) *bad = 1u;
        else {
            sz = n;
            if (fxg_rf_wraps(a)) sz += (b.c + n) / a.width - b.c / a.width;
            if (b.c == 0ull) sz += fxg_rf_id_bytes(a, b.hdr);
            pc = ((u64)n - 1ull) / FXG_RF_PIECE;
        }
    } else if (kind == FXG_RF_HEADER || (i == a.L && a.at_eof)) {      // closes the record before it
        if (b.open) {
            if (b.c > 0ull) sz = (!fxg_rf_wraps(a) || b.c % a.width != 0ull) ? 1ull : 0ull;
            else if (a.keep_empty) sz = fxg_rf_id_bytes(a, b.hdr);
        }
    }
    *size = sz; *pieces = pc;
}

// after the scans: consumed, the carry, the totals
FXG_HD void fxg_rf_finish(const FxgRfArgs &a)
{
    const FxgRfBefore e = fxg_rf_before(a, a.L);
    u64 consumed = a.L ? a.ls[a.L] : 0ull, open = e.open ? e.c : 0ull;
    if (a.at_eof) open = 0ull;
    else if (e.seen && e.c == 0ull) { consumed = a.ls[e.hdr]; open = 0ull; }      // the last header has no bases behind it yet: read again
    a.res[FXG_RF_RES_CONSUMED] = consumed;
    a.res[FXG_RF_RES_OPEN] = open;
    a.res[FXG_RF_RES_OUT_BYTES] = a.size[a.L + 1];
    a.res[FXG_RF_RES_PIECES] = a.pieces[a.L + 1];
}

// the item of further piece p: the last i with pieces[i] <= p (pieces[]: the exclusive scan over L + 2 entries, pieces[L + 1] = the total > p)
FXG_HD u64 fxg_rf_find(const u64 *pieces, u64 entries, u64 p)
{
    u64 lo = 0, hi = entries;                                            // pieces[lo] <= p < pieces[hi] (hi == entries: past the end)
    while (hi - lo > 1ull) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (pieces[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// an id line in front of dst: tabular drops the '>', `last` ends it
FXG_HD void fxg_rf_put_id(const FxgRfArgs &a, uint8_t *dst, u64 hdr, uint8_t last, u32 l)
{
    const u64 s = (u64)a.ls[hdr] + (a.tabular ? 1ull : 0ull), n = (u64)a.ls[hdr + 1] - 1ull - s;
    fxg_bc_copy(dst, a.text + s, n, l, 16u);
    if (l == 0u) dst[n] = last;
}

// Bases x0 .. x0 + n of a record (record indices) from src to where they land when every width-th base is followed by '\n': dst is the
// place of base x0.  Runs between two newlines are copied with aligned 16-byte stores and byte-wise head and tail; below 16 columns byte by byte.
FXG_HD void fxg_rf_copy_wrapped(uint8_t *dst, const uint8_t *src, u64 x0, u32 n, u32 width, u32 l)
{
    const u32 r0 = (u32)(x0 % width);                                   // column of base x0
    if (width < 16u) {
        for (u32 t = l; t < n; t += 16u) {
            const u32 col = r0 + t, nls = col / width;
            dst[t + nls] = src[t];
            if ((col + 1u) % width == 0u) dst[t + nls + 1u] = '\n';
        }
        return;
    }
    u32 t = 0, room = width - r0, nls = 0;                              // room: bases that still fit on the current line
    while (t < n) {
        const u32 take = n - t < room ? n - t : room;
        fxg_bc_copy(dst + t + nls, src + t, take, l, 16u);
        t += take;
        if (take == room) { if (l == 0u) dst[t + nls] = '\n'; ++nls; }
        room = width;
    }
}

// piece j of item i by lane l of its group of 16; piece 0 brings along whatever else the item owns
FXG_HD void fxg_rf_copy_piece(const FxgRfArgs &a, u64 i, u64 j, u32 l)
{
    u32 n;
    const u32 kind = fxg_rf_kind(a, i, &n);
    const FxgRfBefore b = fxg_rf_before(a, i);
    uint8_t *dst = a.out + a.size[i];
    if (kind != FXG_RF_SEQ) {                                           // a closer: one '\n', or the id line of a record without bases
        if (b.c > 0ull) { if (l == 0u) dst[0] = '\n'; }
        else fxg_rf_put_id(a, dst, b.hdr, '\n', l);
        return;
    }
    if (b.c == 0ull) {
        if (j == 0ull) fxg_rf_put_id(a, dst, b.hdr, a.tabular ? '\t' : '\n', l);
        dst += fxg_rf_id_bytes(a, b.hdr);
    }
    const u64 o = j * FXG_RF_PIECE;                                     // the piece: bytes [o, o + m) of the line
    const u32 m = (u64)n - o < FXG_RF_PIECE ? (u32)((u64)n - o) : FXG_RF_PIECE;
    const uint8_t *src = a.text + (u64)a.ls[i] + o;
    if (!fxg_rf_wraps(a)) { fxg_bc_copy(dst + o, src, m, l, 16u); return; }
    const u64 x0 = b.c + o;
    fxg_rf_copy_wrapped(dst + o + (x0 / a.width - b.c / a.width), src, x0, m, a.width, l);
}

// item i's first piece, if the item owns anything
FXG_HD void fxg_rf_copy_head(const FxgRfArgs &a, u64 i, u32 l)
{
    if (a.size[i + 1] != a.size[i]) fxg_rf_copy_piece(a, i, 0ull, l);
}
// further piece p of the block: piece p - pieces[i] + 1 of its item
FXG_HD void fxg_rf_copy_tail(const FxgRfArgs &a, u64 p, u32 l)
{
    const u64 i = fxg_rf_find(a.pieces, a.L + 2, p);
    fxg_rf_copy_piece(a, i, p - a.pieces[i] + 1ull, l);
}

// ---- host side of fxg_fasta_reflow, one copy for the engine and tests/emu ----
static inline int fxg_rf_check(const uint8_t *text, u64 text_len, const fxg_reflow_opts *o, const u32 *line, u64 cap_lines, fxg_reflow_info *info, char *err, size_t cap)
{
    if (!o || !info || (text_len && (!text || !line))) return FXG_E_INVALID;
    memset(info, 0, sizeof *info);
    if (fxg_text_check_len(text_len, err, cap) != FXG_OK) return FXG_E_INVALID;
    if (text_len && cap_lines < 1) FXG_PLAN_FAIL("fxg_fasta_reflow: no room in the line array");
    return FXG_OK;
}
static inline int fxg_rf_lines_fit(u64 lines, u64 cap_lines, char *err, size_t cap)
{
    if (lines + 1 > cap_lines) FXG_PLAN_FAIL("fxg_fasta_reflow: %llu lines need a line array of %llu entries, it has %llu", (unsigned long long)lines, (unsigned long long)lines + 1ull, (unsigned long long)cap_lines);
    return FXG_OK;
}
// u64 words of the workspace for L lines: four arrays of L + 2 entries and the levels of three scans (two arrays for the segmented one)
static inline u64 fxg_rf_level_words(u64 entries) { return entries / 256 + 128; }
static inline u64 fxg_rf_ws_words(u64 L) { return 4 * (L + 2) + 2 * fxg_rf_level_words(L + 2) + FXG_RF_RES_WORDS; }
static inline FxgRfArgs fxg_rf_args(const uint8_t *text, const u32 *line, u64 L, int at_eof, u64 open_in, const fxg_reflow_opts *o, u64 *ws, uint8_t *out)
{
    FxgRfArgs a;
    const u64 M = L + 2;
    a.text = text; a.ls = line; a.L = L; a.open_in = open_in;
    a.width = o->width; a.tabular = o->tabular ? 1u : 0u; a.keep_empty = o->keep_empty ? 1u : 0u; a.at_eof = at_eof ? 1u : 0u;
    a.seg_s = ws; a.seg_kf = ws + M; a.size = ws + 2 * M; a.pieces = ws + 3 * M;
    a.res = ws + 4 * M + 2 * fxg_rf_level_words(M);
    a.out = out;
    return a;
}
static inline u64 *fxg_rf_levels(const FxgRfArgs &a) { return a.pieces + (a.L + 2); }
// the results of a block, once they are on the host: refused (nothing may have been written yet), or the caller's info
static inline int fxg_rf_results(const u64 *res, u64 L, u64 out_cap, bool has_out, fxg_reflow_info *info, char *err, size_t cap)
{
    if (res[FXG_RF_RES_BAD]) FXG_PLAN_FAIL("fxg_fasta_reflow: a sequence line with no record open (no header before it in the block and open_bases_in == 0)");
    if (res[FXG_RF_RES_OUT_BYTES] > out_cap) FXG_PLAN_FAIL("the reflowed block needs %llu bytes, d_out takes %llu", (unsigned long long)res[FXG_RF_RES_OUT_BYTES], (unsigned long long)out_cap);
    if (res[FXG_RF_RES_OUT_BYTES] && !has_out) return FXG_E_INVALID;
    info->lines = L; info->headers = res[FXG_RF_RES_HEADERS]; info->consumed = res[FXG_RF_RES_CONSUMED];
    info->out_bytes = res[FXG_RF_RES_OUT_BYTES]; info->open_bases = res[FXG_RF_RES_OPEN];
    return FXG_OK;
}

#ifndef FXG_HOST_EMULATION
static_assert(FXG_RF_SCAN_BLOCK == FXG_SCAN_PER_BLOCK && FXG_RF_SCAN_BLOCK == 4u * FXG_BLOCK, "the segmented scan has the plain scan's geometry: 256 threads x 4 items");
__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_rf_classify(const FxgRfArgs a)
{
    const u64 i = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x;
    u32 h = 0;
    if (i < a.L + 2) h = fxg_rf_classify(a, i);
    const u64 b = __ballot(h != 0u);
    if (fxg_lane() == 0u && b) atomicAdd((unsigned long long *)&a.res[FXG_RF_RES_HEADERS], (unsigned long long)__builtin_popcountll(b));
}

__device__ __forceinline__ FxgRfSeg fxg_rf_shfl_up(FxgRfSeg v, int d)
{
    FxgRfSeg r;
    r.s = ((u64)__shfl_up((u32)(v.s >> 32), d, 64) << 32) | __shfl_up((u32)v.s, d, 64);
    r.kf = ((u64)__shfl_up((u32)(v.kf >> 32), d, 64) << 32) | __shfl_up((u32)v.kf, d, 64);
    return r;
}

// The segmented form of fxg_kernel_scan_blocks / fxg_kernel_scan_add (fxg_text.h): in place, each 1024-item block's exclusive scan under
// fxg_rf_combine and the block's aggregate to sums; after the aggregates are scanned the same way, every item whose block prefix holds no
// header yet takes its block's carry in.
__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_rf_segscan_blocks(u64 *ds, u64 *dkf, u64 n, u64 *sums_s, u64 *sums_kf)
{
    __shared__ FxgRfSeg wagg[FXG_WAVES];
    const u64 base = (u64)blockIdx.x * FXG_RF_SCAN_BLOCK + (u64)threadIdx.x * 4;
    const FxgRfSeg zero = {0ull, 0ull};
    FxgRfSeg v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = zero; if (base + i < n) { v[i].s = ds[base + i]; v[i].kf = dkf[base + i]; } }
    const FxgRfSeg mine = fxg_rf_combine(fxg_rf_combine(fxg_rf_combine(v[0], v[1]), v[2]), v[3]);
    const u32 lane = fxg_lane(), wave = threadIdx.x >> 6;
    FxgRfSeg incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const FxgRfSeg t = fxg_rf_shfl_up(incl, d);
        if ((int)lane >= d) incl = fxg_rf_combine(t, incl);
    }
    if (lane == 63u) wagg[wave] = incl;
    FxgRfSeg excl = fxg_rf_shfl_up(incl, 1);                           // the lanes before this one, within the wave
    if (lane == 0u) excl = zero;
    __syncthreads();
    FxgRfSeg off = zero, tot = zero;
#pragma unroll
    for (int w = 0; w < FXG_WAVES; ++w) { if (w < (int)wave) off = fxg_rf_combine(off, wagg[w]); tot = fxg_rf_combine(tot, wagg[w]); }
    FxgRfSeg run = fxg_rf_combine(off, excl);
#pragma unroll
    for (int i = 0; i < 4; ++i) { if (base + i < n) { ds[base + i] = run.s; dkf[base + i] = run.kf; } run = fxg_rf_combine(run, v[i]); }
    if (threadIdx.x == 0) { sums_s[blockIdx.x] = tot.s; sums_kf[blockIdx.x] = tot.kf; }
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_rf_segscan_add(u64 *ds, u64 *dkf, u64 n, const u64 *off_s, const u64 *off_kf)
{
    const u64 base = (u64)blockIdx.x * FXG_RF_SCAN_BLOCK + (u64)threadIdx.x * 4;
    const FxgRfSeg carry = {off_s[blockIdx.x], off_kf[blockIdx.x]};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (base + i < n) {
            const FxgRfSeg mine = {ds[base + i], dkf[base + i]};
            const FxgRfSeg r = fxg_rf_combine(carry, mine);
            ds[base + i] = r.s; dkf[base + i] = r.kf;
        }
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_rf_sizes(const FxgRfArgs a)
{
    const u64 i = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x;
    u32 bad = 0;
    if (i < a.L + 2) {
        u64 sz = 0, pc = 0;
        if (i <= a.L) fxg_rf_size(a, i, &sz, &pc, &bad);
        a.size[i] = sz; a.pieces[i] = pc;
    }
    if (__ballot(bad != 0u) != 0ull && fxg_lane() == 0u) atomicOr((unsigned long long *)&a.res[FXG_RF_RES_BAD], 1ull);
}

__global__ void fxg_kernel_rf_finish(const FxgRfArgs a) { fxg_rf_finish(a); }

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_rf_copy_heads(const FxgRfArgs a)
{
    const u64 i = ((u64)blockIdx.x * FXG_BLOCK + threadIdx.x) >> 4;
    if (i <= a.L) fxg_rf_copy_head(a, i, threadIdx.x & 15u);
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_rf_copy_tails(const FxgRfArgs a, u64 npieces)
{
    const u64 p = ((u64)blockIdx.x * FXG_BLOCK + threadIdx.x) >> 4;
    if (p < npieces) fxg_rf_copy_tail(a, p, threadIdx.x & 15u);
}
#endif  // FXG_HOST_EMULATION
