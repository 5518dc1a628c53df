// collapse_emu.cpp -- TEST-ONLY serial CPU emulation of fxg_collapse_begin / _add / _order / _write (csrc/fxg_collapse.h): the engine's own host half
// (fxg_cl_begin / _add / _order / _write, the replay of the reference's container included) over a backend that keeps "device" memory in
// malloc'ed blocks of exactly the bytes asked for and runs the kernels' per-item bodies record by record, lane by lane and slot by slot.  The
// slot atomics are plain accesses here and the scans are serial; the insert's staging is done as the kernel does it, into a buffer of exactly
// FXG_CL_STAGE_BYTES.  tests/test_collapse_cpu.py calls it through ctypes (with the caller's arrays against guard pages), collapse_stub.cpp puts
// it behind the C-ABI for the tool, and collapse_san_main.cpp runs it under the sanitizers.  Not part of the product library.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fastx_toolkit_amd/csrc/fxg_collapse.h"

struct EmuClBackend {
    char *err; size_t cap;
    int alloc(void **p, u64 bytes, const char *what)
    {
        *p = malloc(bytes ? bytes : 1);
        if (*p) return FXG_OK;
        snprintf(err, cap, "fxg_collapse: the set wanted %llu bytes for %s, and the device did not have them", (unsigned long long)bytes, what);
        return FXG_E_NOMEM;
    }
    void release(void *p) { free(p); }
    int zero(void *p, u64 bytes) { memset(p, 0, bytes); return FXG_OK; }
    int copy(void *dst, const void *src, u64 bytes) { memcpy(dst, src, bytes); return FXG_OK; }
    int up(void *dst, const void *src, u64 bytes) { memcpy(dst, src, bytes); return FXG_OK; }
    int down(void *dst, const void *src, u64 bytes) { memcpy(dst, src, bytes); return FXG_OK; }
    int sync() { return FXG_OK; }
    int scan(u64 *d, u64 n, u64 *) { u64 run = 0; for (u64 i = 0; i < n; ++i) { const u64 v = d[i]; d[i] = run; run += v; } return FXG_OK; }
    int lens(const uint16_t *dlen, u64 n, u64 *tmp) { for (u64 r = 0; r <= n; ++r) tmp[r] = r < n ? (u64)dlen[r] : 0ull; return FXG_OK; }      // fxg_kernel_cl_lens
    int copy_check(const FxgClAddArgs &a)                        // fxg_kernel_cl_copy
    {
        for (u64 r = 0; r < a.n; ++r) {
            u64 c = 0;
            bool bad = false;
            for (u32 l = 0; l < FXG_CL_LANES; ++l) bad |= fxg_cl_copy_record(a, r, l, &c);
            a.s.res[FXG_CL_RES_READS] += c;
            if (bad) { fxg_cl_a_min(a.s.res + FXG_CL_RES_FIRST_BAD, r); a.s.res[FXG_CL_RES_IRREGULAR] |= 1ull; }
        }
        return FXG_OK;
    }
    int init(u64 *slots, u64 nslots) { for (u64 i = 0; i < nslots; ++i) { slots[3 * i] = 0ull; slots[3 * i + 1] = 0ull; slots[3 * i + 2] = FXG_CL_NONE; } return FXG_OK; }
    int rebuild(const u64 *old, u64 nold, const FxgClSet &s, u32 hash_bits)
    {
        for (u64 i = 0; i < nold; ++i) if (fxg_cl_move(old, i, s, hash_bits)) s.res[FXG_CL_RES_ERR] |= 1ull;
        return FXG_OK;
    }
    int insert(const FxgClSet &s, u64 rec0, u64 n, u32 hash_bits)      // fxg_kernel_cl_insert, workgroup by workgroup
    {
        uint8_t *stage = (uint8_t *)aligned_alloc(16, FXG_CL_STAGE_BYTES);
        for (u64 r0 = 0; r0 < n; r0 += FXG_BLOCK) {
            const u32 have = (u32)(n - r0 < (u64)FXG_BLOCK ? n - r0 : (u64)FXG_BLOCK);
            const u64 gl = rec0 + r0 + have - 1u;
            const u64 b0 = s.off[rec0 + r0] & ~15ull, b1 = (s.off[gl] + s.len[gl] + 15ull) & ~15ull;
            const bool staged = b1 - b0 <= (u64)FXG_CL_STAGE_BYTES;
            if (staged) memcpy(stage, s.arena + b0, b1 - b0);
            for (u32 t = 0; t < have; ++t) {
                const u64 g = rec0 + r0 + t;
                const u64 h = staged ? fxg_cl_hash(stage + (s.off[g] - b0), s.len[g]) : fxg_cl_hash(s.arena + s.off[g], s.len[g]);
                const u32 what = fxg_cl_insert(s, g, h, hash_bits);
                if (what == 1u) s.res[FXG_CL_RES_NEW] += 1ull;
                if (what == 2u) s.res[FXG_CL_RES_ERR] |= 1ull;
            }
        }
        free(stage);
        return FXG_OK;
    }
    int mark(const FxgClSet &s, u64 *flags) { for (u64 i = 0; i < s.nslots; ++i) fxg_cl_mark(s, i, flags); return FXG_OK; }
    int scatter(const FxgClOrd &o) { for (u64 i = 0; i < o.s.nslots; ++i) fxg_cl_scatter(o, i); return FXG_OK; }
    int sizes(const FxgClOrd &o) { for (u64 r = 0; r <= o.uniques; ++r) o.size[r] = fxg_cl_size(o, r); return FXG_OK; }
    int window(const FxgClOrd &o, u64 rank_begin, u64 out_cap) { fxg_cl_window(o, rank_begin, out_cap); return FXG_OK; }
    int write(const FxgClOrd &o, u64 rank_begin, u64 rank_end)
    {
        for (u64 rank = rank_begin; rank < rank_end; ++rank)
            for (u32 l = 0; l < FXG_CL_LANES; ++l) fxg_cl_write_record(o, rank_begin, rank, l);
        return FXG_OK;
    }
    void interval_begin() {}
    void interval_end() {}
};

static EmuClBackend backend(char *err, size_t cap, char (&own)[256])
{
    EmuClBackend b;
    b.err = err ? err : own; b.cap = err ? cap : sizeof own;
    return b;
}

extern "C" void *fxg_emu_collapse_new(void) { return calloc(1, sizeof(FxgClState)); }
extern "C" void fxg_emu_collapse_free(void *h)
{
    FxgClState *st = (FxgClState *)h;
    if (!st) return;
    free(st->arena); free(st->off); free(st->cnt); free(st->len); free(st->slots); free(st->tmp); free(st->ord); free(st->res);
    free(st);
}
extern "C" int fxg_emu_collapse_begin(void *h, const fxg_collapse_opts *opts, char *err, size_t cap)
{
    char own[256];
    EmuClBackend b = backend(err, cap, own);
    return fxg_cl_begin(b, *(FxgClState *)h, opts);
}
extern "C" int fxg_emu_collapse_add(void *h, const uint8_t *text, uint64_t text_len, int lpr, const uint32_t *line, uint64_t cap_lines, uint64_t records, const uint16_t *len,
                                    fxg_collapse_info *info, char *err, size_t cap)
{
    char own[256];
    EmuClBackend b = backend(err, cap, own);
    return fxg_cl_add(b, *(FxgClState *)h, text, text_len, lpr, line, cap_lines, records, len, info);
}
extern "C" int fxg_emu_collapse_order(void *h, fxg_collapse_info *info, char *err, size_t cap)
{
    char own[256];
    EmuClBackend b = backend(err, cap, own);
    return fxg_cl_order(b, *(FxgClState *)h, info);
}
extern "C" int fxg_emu_collapse_write(void *h, uint64_t rank_begin, uint64_t out_cap, uint8_t *out, fxg_collapse_window *window, char *err, size_t cap)
{
    char own[256];
    EmuClBackend b = backend(err, cap, own);
    return fxg_cl_write(b, *(FxgClState *)h, rank_begin, out_cap, out, window);
}
// the hash and the replay alone, for the tests that pin them
extern "C" uint64_t fxg_emu_collapse_hash(const uint8_t *p, uint32_t len)
{
    std::vector<u64> pad(len / 8 + 3);                           // (the function reads whole aligned words: from a copy, at the caller's alignment)
    uint8_t *q = (uint8_t *)pad.data() + ((uintptr_t)p & 7u);
    if (len) memcpy(q, p, len);
    return fxg_cl_hash(q, len);
}
extern "C" void fxg_emu_collapse_replay(const uint64_t *hash, const uint64_t *count, uint64_t uniques, uint64_t *perm, uint64_t *out_reads)
{
    u64 total = 0;
    fxg_cl_replay((const u64 *)hash, (const u64 *)count, uniques, (u64 *)perm, &total);
    *out_reads = total;
}
