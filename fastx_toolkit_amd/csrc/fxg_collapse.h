// fxg_collapse.h -- fastx_collapser on the device: identical reads merged into one record each, ">rank-count\nBASES\n", most frequent first
// (reference src/fastx_collapser/fastx_collapser.cpp:112-122).
//
// The set of sequences lives in a context across blocks (fxg_collapse_begin .. _add .. _order .. _write):
//   arena      append-only: the bases of every record added so far, one after the other, and per record (global index g, in input order) its
//              byte offset off[g], its length len[g] and its read count cnt[g];
//   table      open addressing, linear probing, a power-of-two number of slots of three u64 words:
//                key     {fingerprint:24 | representative's global record index + 1 : 40}, 0 = empty
//                count   the reads of the slot's members, summed modulo 2^64 as the reference's size_t does
//                first   the smallest global record index among the members
// Launches per added block (the block has been through fxg_fastq_index: ls / le its line starts and chomped ends, dlen its indexed lengths):
//   lens+scan  the indexed lengths copied to u64 and scanned (the project's exclusive scan): the block's byte offsets in the arena;
//   copy+check a group of 16 lanes per record, at most FXG_CL_GRID_MAX workgroups with further trips: every 16-byte piece of the bases line is
//              checked against upper-case A C G T N, the line is copied into the arena (fxg_bc_copy), lane 0 writes off / len / cnt.  A byte
//              outside the alphabet, an empty line or a length that is not the line's raises the block's irregular word: the host then leaves
//              the set as it was (what the launch wrote lies behind the arena's end and the record count, and the next add overwrites it);
//   rebuild    only when the host finds the table too small for 2 x (uniques + the block's records): every non-empty slot moves into a table
//              of at least twice the size -- all keys differ, so a hash of the representative and a swap, no byte compare;
//   insert     a launch of its own, after the copy: a workgroup takes 256 records, stages their span of the arena in LDS with 16-byte loads
//              (when it fits FXG_CL_STAGE_BYTES; else the hash reads the arena), a lane hashes its record from there and probes.
// A block of packed rows (fxg_collapse_add_rows: what fxg_run_pipeline compacts, record k = rlen[k] bytes at bases + roff[k]) takes the same road
// with launches of its own in place of lens and copy+check: row lens, a lane to a row, the bytes the row gives (all of them, or the window
// [first_base, last_base] of fastx_trimmer -f / -l; a row that ends before first_base gives none and gets no record number) and a flag, both
// scanned: the rows' arena offsets and record numbers; copy rows, 16 lanes to a record as above, no alphabet check (the pack made it), a length
// of zero raises the irregular word; counts, a lane to a record, the read count of the id line of source record kept[k] or 1.  They write only
// arena bytes and off / len / cnt entries behind the set's end and reduce into the result words as copy+check does; the insert launch follows
// as it is.
// Coherence, the property to keep: the only words two workgroups share inside a launch are slot words, and those are touched by agent-scope
// atomics only -- relaxed atomic loads for the probes, one compare-and-swap of `key` to claim an empty slot (a failed swap examines the value it
// got back: the same slot again), atomic add on `count`, atomic min on `first`.  Every arena byte and every off / len / cnt entry a lane reads
// was written by an earlier launch.  So no lane waits for another, nothing needs a fence, and nothing depends on where a workgroup runs.  The
// probe loop is bounded by the slot count and raises an error word if it runs out; the host keeps the load below a half, so it never does.
// One hash serves the table and the order: libstdc++'s std::hash<std::string> (64-bit Murmur, _Hash_bytes, seed 0xc70f6907), fxg_cl_hash.
// After the last add (fxg_collapse_order): the slots mark `first` in a per-record flag array, its scan numbers the uniques in first-occurrence
// order without a sort, a scatter writes hash[u], count[u] and the arena reference ref[u]; the host downloads hash and count, replays the
// reference's container for real (fxg_cl_replay: a std::unordered_map keyed by u whose hasher returns hash[u], filled in u order, iterated,
// stable-sorted by count, read backwards) and uploads perm[rank]; a launch sizes every rank's record, 4 + width(rank + 1) + width((int)count)
// + len bytes, and a scan places them.  fxg_collapse_write then copies windows of whole records, 16 lanes to a record.
// The per-item bodies are __host__ __device__ so that the CPU emulator runs the same code; the host half (FxgClState, fxg_cl_begin / _add /
// _order / _write over a backend that allocates, copies and launches) is one copy for the engine and tests/emu.
#pragma once
#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "fxg_barcode.h"      // fxg_bc_copy
#include "fxg_kernels.h"      // (fxg_text.h names its result bits)
#include "fxg_text.h"         // fxg_reads_count, fxg_dec_width

#define FXG_CL_LANES 16u                          // lanes that share a record in the copy and write launches
#define FXG_CL_GRID_MAX 2048u                     // workgroups of the copy launch at most: 32 768 records a trip
#define FXG_CL_SLOT_GRID_MAX 65536u               // workgroups of a launch over the slots at most (further trips)
#define FXG_CL_STAGE_BYTES 49152u                 // LDS a workgroup of the insert launch stages its records' bytes in (256 records of 150 bases: 38 400)
#define FXG_CL_REC_BITS 40
#define FXG_CL_REC_MASK ((1ull << FXG_CL_REC_BITS) - 1ull)
#define FXG_CL_MAX_RECORDS ((1ull << FXG_CL_REC_BITS) - 2ull)
#define FXG_CL_SLOTS_DEFAULT (1ull << 16)
#define FXG_CL_SLOTS_MAX (1ull << 38)
#define FXG_CL_NONE (~0ull)
enum { FXG_CL_RES_IRREGULAR = 0, FXG_CL_RES_FIRST_BAD, FXG_CL_RES_READS, FXG_CL_RES_NEW, FXG_CL_RES_ERR, FXG_CL_RES_RANK_END, FXG_CL_RES_OUT_BYTES, FXG_CL_RES_NEED,
       FXG_CL_RES_WORDS = 16 };

struct FxgClSet {
    uint8_t *arena; u64 arena_cap;    // bytes the arena can take (the allocation has 64 more: the hash reads whole aligned words)
    u64 *off; uint16_t *len; u64 *cnt;
    u64 *slots; u64 nslots;
    u64 *res;                         // FXG_CL_RES_* words
};
struct FxgClAddArgs {
    const uint8_t *text;
    const u32 *ls, *le;
    const uint16_t *dlen;             // the block's indexed lengths
    u64 n; u32 lpr;
    const u64 *scan;                  // exclusive scan of dlen: the block's byte offsets
    u64 rec0, off0;                   // records and arena bytes before the block
    FxgClSet s;
};
struct FxgClRowsArgs {
    const uint8_t *bases;             // the caller's packed rows: record k is len(k) bytes at bases + roff[k], any alignment
    const u64 *roff;
    const uint16_t *rlen;
    u32 first, last;                  // the window of a row that goes in: bases first .. last counted from 1; last == 0: to the row's end
    const u32 *kept;                  // null: every record counts 1; else the source record of record k in the indexed FASTA text below
    const uint8_t *text;
    const u32 *ls, *le;
    u64 n;
    const u64 *scan;                  // exclusive scan of the bytes the rows give, n + 1 entries
    const u64 *num;                   // exclusive scan of the rows' flags, n + 1 entries: row k is record rec0 + num[k] if num[k + 1] > num[k]
    u64 rec0, off0;
    FxgClSet s;
};
struct FxgClOrd {
    FxgClSet s;
    u64 uniques;
    const u64 *flags;                 // scanned: the unique number of the record that is a slot's `first`
    u64 *hash, *count, *ref, *perm, *size;
    uint8_t *out;
};

// ---- the slot words: agent-scope atomics on the device, plain accesses in the serial emulation ----
FXG_HD u64 fxg_cl_a_load(u64 *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}
// the value the word held: `expected` if the swap took place
FXG_HD u64 fxg_cl_a_cas(u64 *p, u64 expected, u64 desired)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expected;
#else
    const u64 old = *p;
    if (old == expected) *p = desired;
    return old;
#endif
}
FXG_HD void fxg_cl_a_add(u64 *p, u64 v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p += v;
#endif
}
FXG_HD void fxg_cl_a_min(u64 *p, u64 v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    if (v < *p) *p = v;
#endif
}
FXG_HD void fxg_cl_a_or(u64 *p, u64 v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *p |= v;
#endif
}

// ---- the hash: std::hash<std::string> of libstdc++ (_Hash_bytes, 64-bit: Murmur with seed 0xc70f6907, eight bytes at a time and a tail of
// len & 7 bytes).  It reads the aligned 8-byte words that hold [p, p + len) and no others, so it serves LDS (aligned ds reads) and global
// memory alike; a caller's buffer must be readable to the end of its last such word. ----
FXG_HD u64 fxg_cl_word(const uint8_t *q) { u64 v; __builtin_memcpy(&v, __builtin_assume_aligned(q, 8), 8); return v; }
FXG_HD u64 fxg_cl_shift_mix(u64 v) { return v ^ (v >> 47); }
FXG_HD u64 fxg_cl_hash(const uint8_t *p, u32 len)
{
    const u64 mul = (0xc6a4a793ull << 32) + 0x5bd1e995ull;
    u64 h = 0xc70f6907ull ^ ((u64)len * mul);
    const u32 sh = 8u * (u32)((uintptr_t)p & 7u);
    const uint8_t *w = p - (sh >> 3);                            // the aligned word that holds p[0]
    u64 lo = len ? fxg_cl_word(w) : 0ull;
    u32 i = 0;
    for (; i + 8u <= len; i += 8u) {
        u64 d;
        w += 8;
        if (sh) { const u64 hi = fxg_cl_word(w); d = (lo >> sh) | (hi << (64u - sh)); lo = hi; }
        else { d = lo; lo = i + 8u < len ? fxg_cl_word(w) : 0ull; }
        d = fxg_cl_shift_mix(d * mul) * mul;
        h ^= d; h *= mul;
    }
    const u32 t = len & 7u;
    if (t) {                                                     // lo: the word that holds p[i]
        u64 d = lo >> sh;
        if (sh && (sh >> 3) + t > 8u) d |= fxg_cl_word(w + 8) << (64u - sh);
        d &= (1ull << (8u * t)) - 1ull;
        h ^= d; h *= mul;
    }
    h = fxg_cl_shift_mix(h) * mul;
    return fxg_cl_shift_mix(h);
}

// a[0, len) == b[0, len), touching no other byte
FXG_HD bool fxg_cl_equal(const uint8_t *a, const uint8_t *b, u32 len)
{
    u32 i = 0;
    for (; i + 8u <= len; i += 8u) {
        u64 x, y;
        __builtin_memcpy(&x, a + i, 8); __builtin_memcpy(&y, b + i, 8);
        if (x != y) return false;
    }
    for (; i < len; ++i) if (a[i] != b[i]) return false;
    return true;
}

// ---- copy + check ----
// nonzero if any byte of w selected by m (0x00 / 0xFF per byte) is not one of upper-case A C G T N
FXG_HD u32 fxg_cl_invalid4(u32 w, u32 m)
{
    const u32 x = w ^ 0x40404040u;                          // A=01 C=03 G=07 N=0E T=14; lower case keeps bit 5, bytes of 0x80 and above bit 7
    const u32 LUT = (1u << 0x01) | (1u << 0x03) | (1u << 0x07) | (1u << 0x0E) | (1u << 0x14);
    const u32 nb = (~(LUT >> (x & 31u)) & m) | (~(LUT >> ((x >> 8) & 31u)) & (m >> 8)) |
                   (~(LUT >> ((x >> 16) & 31u)) & (m >> 16)) | (~(LUT >> ((x >> 24) & 31u)) & (m >> 24));
    return (x & 0xE0E0E0E0u & m) | (nb & 1u);
}

// record r of the block by lane l of its group: the lane's pieces checked, its share of the copy; lane 0 writes the record's entries and
// returns its read count in *count.  Returns true if the record is irregular (every lane of the group agrees on all but the alphabet).
FXG_HD bool fxg_cl_copy_record(const FxgClAddArgs &a, u64 r, u32 l, u64 *count)
{
    const u64 li = (u64)a.lpr * r + 1ull;
    const u32 s = a.ls[li], e = a.le[li], len = a.dlen[r];
    const u64 dst = a.off0 + a.scan[r];
    if (len == 0u || e < s || e - s != len || dst + len > a.s.arena_cap) return true;      // (the last: lengths that are not this text's)
    const uint8_t *src = a.text + s;
    u32 bad = 0;
    for (u32 k = l; (k << 4) < len; k += FXG_CL_LANES) {         // loads end at most 15 bytes past e <= text_len: the text path's slack
        const u32x4 v = fxg_ld16(src + (k << 4));
        const u32 rem = len - (k << 4);
        const u32x4 m = fxg_lowmask16((int)(rem < 16u ? rem : 16u));
        bad |= fxg_cl_invalid4(v.x, m.x) | fxg_cl_invalid4(v.y, m.y) | fxg_cl_invalid4(v.z, m.z) | fxg_cl_invalid4(v.w, m.w);
    }
    fxg_bc_copy(a.s.arena + dst, src, len, l, FXG_CL_LANES);
    if (l == 0u) {
        const u64 g = a.rec0 + r;
        const u64 c = a.lpr == 2u ? (u64)fxg_reads_count(a.text, a.ls[2 * r] + 1u, a.le[2 * r]) : 1ull;      // get_reads_count: a FASTQ record counts 1
        a.s.off[g] = dst; a.s.len[g] = (uint16_t)len; a.s.cnt[g] = c;
        *count = c;
    }
    return bad != 0u;
}

// ---- row lens, copy rows, counts (fxg_collapse_add_rows) ----
// the bytes of a row of `len` that go in, from *start on: the trimmer's rule (fastx_trimmer.c:122-134), 0 if the row ends before `first`
FXG_HD u32 fxg_cl_row_take(u32 len, u32 first, u32 last, u32 *start)
{
    *start = 0u;
    if (last != 0u && last < len) len = last;
    if (first > 1u) {
        if (len < first) return 0u;
        *start = first - 1u; len -= *start;
    }
    return len;
}
// entry r of the two arrays to scan (entry n closes them)
FXG_HD void fxg_cl_row_len(const uint16_t *rlen, u64 n, u32 first, u32 last, u64 r, u64 *bytes, u64 *num)
{
    u32 start;
    const u32 take = r < n ? fxg_cl_row_take(rlen[r], first, last, &start) : 0u;
    bytes[r] = take; num[r] = take != 0u ? 1ull : 0ull;
}
// row r of the block by lane l of its group: its share of the copy, lane 0 writes the record's offset and length.  The byte count is the
// scanned one, so the rows of a block fill exactly the bytes the host made room for.  Returns true if the row is empty (every lane of the
// group agrees).
FXG_HD bool fxg_cl_copy_row(const FxgClRowsArgs &a, u64 r, u32 l)
{
    const u32 len = a.rlen[r];
    if (len == 0u) return true;
    const u64 at = a.scan[r], take = a.scan[r + 1ull] - at, dst = a.off0 + at;
    if (take == 0ull) return false;                              // ends before the window: not a record
    u32 start;
    (void)fxg_cl_row_take(len, a.first, a.last, &start);
    fxg_bc_copy(a.s.arena + dst, a.bases + a.roff[r] + start, take, l, FXG_CL_LANES);
    if (l == 0u) { const u64 g = a.rec0 + a.num[r]; a.s.off[g] = dst; a.s.len[g] = (uint16_t)take; }
    return false;
}
// the read count of row r: that of the id line of its source record (get_reads_count, fastx.c:475-495), 1 without a count source; 0 if the
// row is not a record
FXG_HD u64 fxg_cl_row_count(const FxgClRowsArgs &a, u64 r)
{
    if (a.num[r + 1ull] == a.num[r]) return 0ull;
    u64 c = 1ull;
    if (a.kept) { const u64 src = a.kept[r]; c = (u64)fxg_reads_count(a.text, a.ls[2ull * src] + 1u, a.le[2ull * src]); }
    a.s.cnt[a.rec0 + a.num[r]] = c;
    return c;
}

// ---- the table ----
// the part of a hash that reaches the slot index and the fingerprint (hash_bits: a test and measurement aid, fxg_collapse_opts)
FXG_HD u64 fxg_cl_hash_used(u64 h, u32 hash_bits) { return hash_bits && hash_bits < 64u ? h & ((1ull << hash_bits) - 1ull) : h; }
FXG_HD u64 fxg_cl_fingerprint(u64 hm) { return hm >> FXG_CL_REC_BITS; }

// Record g (its bytes at `mine`: the arena, or the staged copy of them) into the table.  Returns 1 if it claimed a slot (a new unique), 0 if it
// joined one, 2 if the probes ran out (cannot happen below a load of one half).
FXG_HD u32 fxg_cl_insert(const FxgClSet &s, u64 g, u64 h, u32 hash_bits)
{
    const u64 hm = fxg_cl_hash_used(h, hash_bits), fp = fxg_cl_fingerprint(hm), mask = s.nslots - 1ull;
    const u64 mykey = (fp << FXG_CL_REC_BITS) | (g + 1ull);
    const u32 len = s.len[g];
    const u64 cnt = s.cnt[g];
    u64 slot = hm & mask;
    for (u64 probes = 0; probes < s.nslots; ++probes, slot = (slot + 1ull) & mask) {
        u64 *w = s.slots + 3ull * slot;
        u64 key = fxg_cl_a_load(w);
        if (key == 0ull) {
            key = fxg_cl_a_cas(w, 0ull, mykey);
            if (key == 0ull) { fxg_cl_a_add(w + 1, cnt); fxg_cl_a_min(w + 2, g); return 1u; }
        }                                                        // a failed swap: the slot as it is now
        if ((key >> FXG_CL_REC_BITS) != fp) continue;
        const u64 rep = (key & FXG_CL_REC_MASK) - 1ull;          // a record of an earlier launch's copy: its entries and bytes are there
        if (s.len[rep] != len || !fxg_cl_equal(s.arena + s.off[rep], s.arena + s.off[g], len)) continue;
        fxg_cl_a_add(w + 1, cnt); fxg_cl_a_min(w + 2, g);
        return 0u;
    }
    return 2u;
}

// slot i of the old table into the new one (s): keys are distinct, so the first empty slot of the probe sequence is its place
FXG_HD u32 fxg_cl_move(const u64 *old, u64 i, const FxgClSet &s, u32 hash_bits)
{
    const u64 key = old[3ull * i];
    if (key == 0ull) return 0u;
    const u64 rep = (key & FXG_CL_REC_MASK) - 1ull, mask = s.nslots - 1ull;
    u64 slot = fxg_cl_hash_used(fxg_cl_hash(s.arena + s.off[rep], s.len[rep]), hash_bits) & mask;
    for (u64 probes = 0; probes < s.nslots; ++probes, slot = (slot + 1ull) & mask) {
        u64 *w = s.slots + 3ull * slot;
        if (fxg_cl_a_load(w) != 0ull || fxg_cl_a_cas(w, 0ull, key) != 0ull) continue;
        fxg_cl_a_add(w + 1, old[3ull * i + 1]); fxg_cl_a_min(w + 2, old[3ull * i + 2]);      // (onto 0 and ~0: the slot is this key's alone)
        return 0u;
    }
    return 2u;
}

// ---- order ----
FXG_HD void fxg_cl_mark(const FxgClSet &s, u64 i, u64 *flags) { if (s.slots[3ull * i]) flags[s.slots[3ull * i + 2]] = 1ull; }
FXG_HD void fxg_cl_scatter(const FxgClOrd &o, u64 i)
{
    const u64 key = o.s.slots[3ull * i];
    if (key == 0ull) return;
    const u64 rep = (key & FXG_CL_REC_MASK) - 1ull, u = o.flags[o.s.slots[3ull * i + 2]];
    o.hash[u] = fxg_cl_hash(o.s.arena + o.s.off[rep], o.s.len[rep]);      // all 64 bits, whatever hash_bits says: the order is the reference's
    o.count[u] = o.s.slots[3ull * i + 1];
    o.ref[u] = rep;
}
// a count as the reference prints it, truncated to int: its sign and magnitude
FXG_HD u64 fxg_cl_printed(u64 count, bool *neg)
{
    const long long v = (long long)(int)(u32)count;
    *neg = v < 0;
    return (u64)(v < 0 ? -v : v);
}
// bytes of rank's record: '>' rank + 1 '-' (int)count '\n' bases '\n'
FXG_HD u64 fxg_cl_size(const FxgClOrd &o, u64 rank)
{
    if (rank >= o.uniques) return 0ull;
    const u64 u = o.perm[rank];
    bool neg;
    const u64 mag = fxg_cl_printed(o.count[u], &neg);
    return 4ull + fxg_dec_width(rank + 1ull) + (neg ? 1ull : 0ull) + fxg_dec_width(mag) + (u64)o.s.len[o.ref[u]];
}

// ---- write ----
// the last i in [0, entries) with scan[i] <= v (scan: an exclusive scan, scan[0] = 0 <= v)
FXG_HD u64 fxg_cl_find(const u64 *scan, u64 entries, u64 v)
{
    u64 lo = 0, hi = entries;
    while (hi - lo > 1ull) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (scan[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}
// one thread: the window of whole records from rank_begin (<= uniques) that fits out_cap
FXG_HD void fxg_cl_window(const FxgClOrd &o, u64 rank_begin, u64 out_cap)
{
    const u64 off0 = o.size[rank_begin], limit = out_cap > ~0ull - off0 ? ~0ull : off0 + out_cap;
    const u64 re = fxg_cl_find(o.size + rank_begin, o.uniques + 1ull - rank_begin, limit) + rank_begin;      // sizes are > 0: the scan is strictly increasing
    o.s.res[FXG_CL_RES_RANK_END] = re;
    o.s.res[FXG_CL_RES_OUT_BYTES] = o.size[re] - off0;
    o.s.res[FXG_CL_RES_NEED] = rank_begin < o.uniques ? o.size[rank_begin + 1ull] - off0 : 0ull;
}
// rank's record by lane l of its group of 16, at its place in the window that begins at rank_begin
FXG_HD void fxg_cl_write_record(const FxgClOrd &o, u64 rank_begin, u64 rank, u32 l)
{
    const u64 u = o.perm[rank], rep = o.ref[u];
    const u32 len = o.s.len[rep];
    uint8_t *d = o.out + (o.size[rank] - o.size[rank_begin]);
    bool neg;
    const u64 mag = fxg_cl_printed(o.count[u], &neg);
    const u32 w1 = fxg_dec_width(rank + 1ull), w2 = fxg_dec_width(mag), head = 3u + w1 + (neg ? 1u : 0u) + w2;
    if (l == 0u) {
        d[0] = '>';
        u64 v = rank + 1ull;
        for (u32 k = w1; k-- > 0u; v /= 10ull) d[1u + k] = (uint8_t)('0' + v % 10ull);
        d[1u + w1] = '-';
        d[head + len] = '\n';
    }
    if (l == FXG_CL_LANES - 1u) {
        uint8_t *q = d + 2u + w1;
        if (neg) *q++ = '-';
        u64 v = mag;
        for (u32 k = w2; k-- > 0u; v /= 10ull) q[k] = (uint8_t)('0' + v % 10ull);
        q[w2] = '\n';
    }
    fxg_bc_copy(d + head, o.s.arena + o.s.off[rep], len, l, FXG_CL_LANES);
}

// ---- the reference's container, for real: the order of equal counts is what libstdc++'s unordered_map gives for these hash codes inserted in
// this order, and nothing of its bucket policy is restated here.  hash / count: per unique, in first-occurrence order.  perm[rank] = u;
// *out_reads: the counts as printed (truncated to int) added into a size_t, the second line of the -v report. ----
struct FxgClHashOf {
    const u64 *hash;
    size_t operator()(u64 u) const { return (size_t)hash[u]; }
};
static inline void fxg_cl_replay(const u64 *hash, const u64 *count, u64 uniques, u64 *perm, u64 *out_reads)
{
    std::unordered_map<uint64_t, uint64_t, FxgClHashOf> seen(0, FxgClHashOf{hash});
    for (u64 u = 0; u < uniques; ++u) seen[u] = count[u];
    std::vector<std::pair<uint64_t, uint64_t>> order(seen.begin(), seen.end());
    std::stable_sort(order.begin(), order.end(), [](const std::pair<uint64_t, uint64_t> &a, const std::pair<uint64_t, uint64_t> &b) { return a.second < b.second; });
    u64 total = 0;
    for (u64 rank = 0; rank < uniques; ++rank) {
        perm[rank] = order[uniques - 1ull - rank].first;
        total += (u64)(long long)(int)(u32)count[perm[rank]];
    }
    *out_reads = total;
}

// ---- host side of fxg_collapse_*, one copy for the engine and tests/emu ----
// what a context knows of its set.  Device memory only grows; fxg_collapse_begin empties the set and keeps the memory.
struct FxgClState {
    int stage;                            // 0: no set; 1: begun, takes blocks; 2: ordered, gives windows
    u32 hash_bits;
    u64 records, reads, uniques, rebuilds, arena_used, nslots, out_reads, out_bytes;
    uint8_t *arena; u64 arena_cap;
    u64 *off, *cnt; uint16_t *len; u64 rec_cap;
    u64 *slots; u64 slots_cap;            // in slots
    u64 *tmp; u64 tmp_cap;                // in words: a block's lengths and their scan's levels
    u64 *ord; u64 ord_cap;                // in words: the flags, the order's arrays, the scans' levels
    u64 *res;
    u64 *o_hash, *o_count, *o_ref, *o_perm, *o_size;
};
static inline u64 fxg_cl_level_words(u64 entries) { return entries / 512 + 64; }      // fxg_scan_u64's block sums
static inline FxgClSet fxg_cl_set(const FxgClState &st)
{
    FxgClSet s;
    s.arena = st.arena; s.arena_cap = st.arena_cap; s.off = st.off; s.len = st.len; s.cnt = st.cnt; s.slots = st.slots; s.nslots = st.nslots; s.res = st.res;
    return s;
}
static inline FxgClOrd fxg_cl_ord(const FxgClState &st, const u64 *flags, uint8_t *out)
{
    FxgClOrd o;
    o.s = fxg_cl_set(st); o.uniques = st.uniques; o.flags = flags;
    o.hash = st.o_hash; o.count = st.o_count; o.ref = st.o_ref; o.perm = st.o_perm; o.size = st.o_size; o.out = out;
    return o;
}
static inline void fxg_cl_info(const FxgClState &st, fxg_collapse_info *info)
{
    info->records = st.records; info->reads = st.reads; info->uniques = st.uniques; info->slots = st.nslots; info->rebuilds = st.rebuilds;
    info->out_reads = st.out_reads; info->out_bytes = st.out_bytes;
}
static inline u64 fxg_cl_grid(u64 items, u64 most) { const u64 g = (items + FXG_BLOCK - 1) / FXG_BLOCK; return g < most ? (g ? g : 1) : most; }

// A backend B allocates, copies and launches: the engine on its context's stream, tests/emu serially over host memory.
//   int alloc(void **p, u64 bytes, const char *what)     FXG_OK, or the failure with a message that says how many bytes the set wanted
//   void release(void *p)                                after the work queued so far
//   int zero(void *p, u64 bytes); int copy(void *dst, const void *src, u64 bytes)        device to device, queued
//   int up(void *dst, const void *src, u64 bytes); int down(void *dst, const void *src, u64 bytes)      both complete when they return
//   int scan(u64 *data, u64 n, u64 *levels)
//   int lens(const uint16_t *dlen, u64 n, u64 *tmp); int copy_check(const FxgClAddArgs &); int init(u64 *slots, u64 nslots);
//   int row_lens(const uint16_t *rlen, u64 n, u32 first, u32 last, u64 *bytes, u64 *num); int copy_rows(const FxgClRowsArgs &);
//   int row_counts(const FxgClRowsArgs &)                (these three only in a backend that offers fxg_cl_add_rows)
//   int rebuild(const u64 *old, u64 nold, const FxgClSet &, u32 hash_bits); int insert(const FxgClSet &, u64 rec0, u64 n, u32 hash_bits);
//   int mark(const FxgClSet &, u64 *flags); int scatter(const FxgClOrd &); int sizes(const FxgClOrd &);
//   int window(const FxgClOrd &, u64 rank_begin, u64 out_cap); int write(const FxgClOrd &, u64 rank_begin, u64 rank_end); int sync();
//   void interval_begin(); void interval_end()           what lies between them is one entry of the profiling ring
//   char *err; size_t cap                                the message buffer
#define FXG_CL_TRY(call) do { const int rc__ = (call); if (rc__ != FXG_OK) return rc__; } while (0)
#define FXG_CL_FAIL(b, ...) do { snprintf((b).err, (b).cap, __VA_ARGS__); return FXG_E_INVALID; } while (0)

// *p holds `want` units of `unit` bytes afterwards (`slack` more bytes behind them); the first `keep` units survive a move
template <class B, class T>
static int fxg_cl_grow(B &b, T **p, u64 *cap, u64 want, u64 keep, u64 unit, u64 slack, const char *what)
{
    if (*cap >= want) return FXG_OK;
    u64 ncap = *cap * 2;
    if (ncap < want) ncap = want + want / 8 + 1024;
    void *np = nullptr;
    FXG_CL_TRY(b.alloc(&np, ncap * unit + slack, what));
    if (keep) { const int rc = b.copy(np, *p, keep * unit); if (rc != FXG_OK) { b.release(np); return rc; } }
    if (*p) b.release(*p);
    *p = (T *)np; *cap = ncap;
    return FXG_OK;
}

template <class B>
static int fxg_cl_begin(B &b, FxgClState &st, const fxg_collapse_opts *opts)
{
    st.stage = 0;
    const u64 asked = opts ? opts->initial_slots : 0;
    const u32 bits = opts ? opts->hash_bits : 0u;
    if (bits > 64u) FXG_CL_FAIL(b, "fxg_collapse_begin: hash_bits %u; 0 (all 64) or 1 .. 64", bits);
    if (asked > FXG_CL_SLOTS_MAX) FXG_CL_FAIL(b, "fxg_collapse_begin: initial_slots %llu; at most %llu", (unsigned long long)asked, (unsigned long long)FXG_CL_SLOTS_MAX);
    u64 ns = asked ? 4 : FXG_CL_SLOTS_DEFAULT;
    while (ns < asked) ns *= 2;                                  // a power of two, four at the least
    if (!st.res) FXG_CL_TRY(b.alloc((void **)&st.res, FXG_CL_RES_WORDS * sizeof(u64), "its result words"));
    if (st.slots_cap < ns) {
        if (st.slots) b.release(st.slots);
        st.slots = nullptr; st.slots_cap = 0;
        FXG_CL_TRY(b.alloc((void **)&st.slots, ns * 24ull, "its table"));
        st.slots_cap = ns;
    }
    st.nslots = ns; st.hash_bits = bits;
    FXG_CL_TRY(b.init(st.slots, ns));
    st.records = st.reads = st.uniques = st.rebuilds = st.arena_used = st.out_reads = st.out_bytes = 0;
    st.stage = 1;
    return FXG_OK;
}

// room for n more records' entries
template <class B>
static int fxg_cl_grow_records(B &b, FxgClState &st, u64 n)
{
    const u64 R = st.records;
    u64 c1 = st.rec_cap, c2 = st.rec_cap, c3 = st.rec_cap;       // three arrays of one capacity
    FXG_CL_TRY(fxg_cl_grow(b, &st.off, &c1, R + n, R, sizeof(u64), 0, "its records' offsets"));
    FXG_CL_TRY(fxg_cl_grow(b, &st.cnt, &c2, c1, R, sizeof(u64), 0, "its records' counts"));
    FXG_CL_TRY(fxg_cl_grow(b, &st.len, &c3, c1, R, sizeof(uint16_t), 0, "its records' lengths"));
    st.rec_cap = c1 < c2 ? (c1 < c3 ? c1 : c3) : (c2 < c3 ? c2 : c3);
    return FXG_OK;
}

template <class B>
static int fxg_cl_add_copied(B &b, FxgClState &st, u64 n, u64 bytes, u64 (&res)[FXG_CL_RES_WORDS], fxg_collapse_info *info, const char *who);

template <class B>
static int fxg_cl_add(B &b, FxgClState &st, const uint8_t *text, u64 text_len, int lpr, const u32 *line, u64 cap_lines, u64 n, const uint16_t *dlen, fxg_collapse_info *info)
{
    if (!info) FXG_CL_FAIL(b, "fxg_collapse_add: info is null");
    memset(info, 0, sizeof *info);
    info->first_bad = FXG_CL_NONE;
    if (st.stage == 0) FXG_CL_FAIL(b, "fxg_collapse_add: no set; fxg_collapse_begin makes one");
    if (st.stage == 2) FXG_CL_FAIL(b, "fxg_collapse_add: the set is ordered and takes no more blocks; fxg_collapse_begin makes another");
    fxg_cl_info(st, info);
    if (!fxg_text_lpr_ok(lpr)) FXG_CL_FAIL(b, "fxg_collapse_add: lines_per_record %d; 2 (FASTA) or 4 (FASTQ)", lpr);
    if (n && (!text || !line || !dlen)) FXG_CL_FAIL(b, "fxg_collapse_add: a null pointer with %llu records", (unsigned long long)n);
    if (fxg_text_check_len(text_len, b.err, b.cap) != FXG_OK) return FXG_E_INVALID;
    if (n && (u64)lpr * n + 1 > cap_lines) FXG_CL_FAIL(b, "fxg_collapse_add: %llu records need more than %llu lines", (unsigned long long)n, (unsigned long long)cap_lines);
    if (n > text_len / (2ull * (u64)lpr)) FXG_CL_FAIL(b, "fxg_collapse_add: %llu records do not fit %llu bytes of text", (unsigned long long)n, (unsigned long long)text_len);      // a line takes two bytes at least
    if (n > FXG_CL_MAX_RECORDS - st.records) FXG_CL_FAIL(b, "fxg_collapse_add: %llu records after %llu; a set holds at most 2^40 - 2", (unsigned long long)n, (unsigned long long)st.records);
    if (n == 0) return FXG_OK;
    // room: the records' entries, the arena (a block's bases are fewer than its bytes), the lengths and their scan
    const u64 R = st.records, M = n + 1;
    FXG_CL_TRY(fxg_cl_grow_records(b, st, n));
    FXG_CL_TRY(fxg_cl_grow(b, &st.arena, &st.arena_cap, st.arena_used + text_len, st.arena_used, 1, 64, "its arena"));
    FXG_CL_TRY(fxg_cl_grow(b, &st.tmp, &st.tmp_cap, M + fxg_cl_level_words(M), 0, sizeof(u64), 0, "a block's offsets"));
    u64 res[FXG_CL_RES_WORDS];
    memset(res, 0, sizeof res);
    res[FXG_CL_RES_FIRST_BAD] = FXG_CL_NONE;
    FXG_CL_TRY(b.up(st.res, res, sizeof res));
    FxgClAddArgs a;
    a.text = text; a.ls = line; a.le = line + cap_lines; a.dlen = dlen; a.n = n; a.lpr = (u32)lpr; a.scan = st.tmp; a.rec0 = R; a.off0 = st.arena_used; a.s = fxg_cl_set(st);
    b.interval_begin();
    FXG_CL_TRY(b.lens(dlen, n, st.tmp));
    FXG_CL_TRY(b.scan(st.tmp, M, st.tmp + M));
    FXG_CL_TRY(b.copy_check(a));
    b.interval_end();
    u64 bytes = 0;
    FXG_CL_TRY(b.down(&bytes, st.tmp + n, sizeof bytes));
    FXG_CL_TRY(b.down(res, st.res, sizeof res));
    return fxg_cl_add_copied(b, st, n, bytes, res, info, "fxg_collapse_add");
}

// the second half of an add, the same for a block of text and a block of rows: the block's n records lie copied behind the set's end (`bytes`
// arena bytes, their off / len / cnt entries) and res holds the copy's result words
template <class B>
static int fxg_cl_add_copied(B &b, FxgClState &st, u64 n, u64 bytes, u64 (&res)[FXG_CL_RES_WORDS], fxg_collapse_info *info, const char *who)
{
    const u64 R = st.records;
    if (res[FXG_CL_RES_IRREGULAR]) {                             // nothing of the block stays: the set ends where it ended before
        info->irregular = FXG_TEXT_IRR_BASE; info->first_bad = res[FXG_CL_RES_FIRST_BAD];
        return FXG_OK;
    }
    // the table holds 2 x (uniques so far + the block's records) slots before the insert, so an insert never meets a full one
    const u64 want = 2ull * (st.uniques + n);
    if (st.nslots < want) {
        u64 ns = st.nslots;
        while (ns < want) ns *= 2;
        if (ns > FXG_CL_SLOTS_MAX) FXG_CL_FAIL(b, "%s: the table would need %llu slots; at most %llu", who, (unsigned long long)ns, (unsigned long long)FXG_CL_SLOTS_MAX);
        u64 *fresh = nullptr;
        FXG_CL_TRY(b.alloc((void **)&fresh, ns * 24ull, "a larger table"));
        const u64 *old = st.slots; const u64 nold = st.nslots;
        FxgClSet s = fxg_cl_set(st);
        s.slots = fresh; s.nslots = ns;
        b.interval_begin();
        int rc = b.init(fresh, ns);
        if (rc == FXG_OK) rc = b.rebuild(old, nold, s, st.hash_bits);
        b.interval_end();
        if (rc != FXG_OK) { b.release(fresh); return rc; }
        b.release(st.slots);
        st.slots = fresh; st.slots_cap = st.nslots = ns; st.rebuilds++;
    }
    b.interval_begin();
    FXG_CL_TRY(b.insert(fxg_cl_set(st), R, n, st.hash_bits));
    b.interval_end();
    FXG_CL_TRY(b.down(res, st.res, sizeof res));
    if (res[FXG_CL_RES_ERR]) { st.stage = 0; snprintf(b.err, b.cap, "%s: a probe ran through all %llu slots (the set is lost)", who, (unsigned long long)st.nslots); return FXG_E_DEVICE; }
    st.records += n; st.reads += res[FXG_CL_RES_READS]; st.uniques += res[FXG_CL_RES_NEW]; st.arena_used += bytes;
    fxg_cl_info(st, info);
    return FXG_OK;
}

// fxg_collapse_add_rows: a block of packed rows -- what fxg_run_pipeline leaves in out_bases / out_off / out_len -- into the same set.  first,
// last: the window of every row that goes in (0 / 1, 0: the whole row).  kept, text, line, cap_lines, lpr: the count source (all or none); it
// counts for lpr == 2 only.
template <class B>
static int fxg_cl_add_rows(B &b, FxgClState &st, const uint8_t *bases, const u64 *roff, const uint16_t *rlen, u64 n, u32 first, u32 last, const u32 *kept,
                           const uint8_t *text, const u32 *line, u64 cap_lines, int lpr, fxg_collapse_info *info)
{
    if (!info) FXG_CL_FAIL(b, "fxg_collapse_add_rows: info is null");
    memset(info, 0, sizeof *info);
    info->first_bad = FXG_CL_NONE;
    if (st.stage == 0) FXG_CL_FAIL(b, "fxg_collapse_add_rows: no set; fxg_collapse_begin makes one");
    if (st.stage == 2) FXG_CL_FAIL(b, "fxg_collapse_add_rows: the set is ordered and takes no more blocks; fxg_collapse_begin makes another");
    fxg_cl_info(st, info);
    const bool source = kept || text || line || cap_lines || lpr;
    if (source && (!kept || !text || !line || cap_lines < 2))
        FXG_CL_FAIL(b, "fxg_collapse_add_rows: a count source is d_kept_index, d_text, d_line and cap_lines together, or none of them with lines_per_record 0");
    if (source && !fxg_text_lpr_ok(lpr)) FXG_CL_FAIL(b, "fxg_collapse_add_rows: lines_per_record %d; 2 (FASTA) or 4 (FASTQ)", lpr);
    if (last != 0u && last < first) FXG_CL_FAIL(b, "fxg_collapse_add_rows: last_base %u is before first_base %u", last, first);
    if (n && (!bases || !roff || !rlen)) FXG_CL_FAIL(b, "fxg_collapse_add_rows: a null pointer with %llu records", (unsigned long long)n);
    if (n > FXG_CL_MAX_RECORDS - st.records) FXG_CL_FAIL(b, "fxg_collapse_add_rows: %llu records after %llu; a set holds at most 2^40 - 2", (unsigned long long)n, (unsigned long long)st.records);
    if (n == 0) return FXG_OK;
    const u64 R = st.records, M = n + 1, LV = fxg_cl_level_words(M);
    FXG_CL_TRY(fxg_cl_grow_records(b, st, n));
    FXG_CL_TRY(fxg_cl_grow(b, &st.tmp, &st.tmp_cap, 2 * (M + LV), 0, sizeof(u64), 0, "a block's offsets"));
    u64 *scan = st.tmp, *num = st.tmp + M + LV;
    u64 res[FXG_CL_RES_WORDS];
    memset(res, 0, sizeof res);
    res[FXG_CL_RES_FIRST_BAD] = FXG_CL_NONE;
    FXG_CL_TRY(b.up(st.res, res, sizeof res));
    b.interval_begin();
    FXG_CL_TRY(b.row_lens(rlen, n, first, last, scan, num));
    FXG_CL_TRY(b.scan(scan, M, scan + M));
    FXG_CL_TRY(b.scan(num, M, num + M));
    u64 bytes = 0, m = 0;                                        // the rows' bytes are known only now: the arena's room follows the scan
    int rc = b.down(&bytes, scan + n, sizeof bytes);
    if (rc == FXG_OK) rc = b.down(&m, num + n, sizeof m);
    if (rc == FXG_OK) rc = fxg_cl_grow(b, &st.arena, &st.arena_cap, st.arena_used + bytes, st.arena_used, 1, 64, "its arena");
    FxgClRowsArgs a;
    a.bases = bases; a.roff = roff; a.rlen = rlen; a.first = first; a.last = last; a.kept = source && lpr == 2 ? kept : nullptr; a.text = text; a.ls = line;
    a.le = line + cap_lines; a.n = n; a.scan = scan; a.num = num; a.rec0 = R; a.off0 = st.arena_used; a.s = fxg_cl_set(st);
    if (rc == FXG_OK) rc = b.copy_rows(a);
    if (rc == FXG_OK) rc = b.row_counts(a);
    b.interval_end();
    FXG_CL_TRY(rc);
    FXG_CL_TRY(b.down(res, st.res, sizeof res));
    if (m == 0 && !res[FXG_CL_RES_IRREGULAR]) return FXG_OK;     // every row ends before the window: nothing to insert
    return fxg_cl_add_copied(b, st, m, bytes, res, info, "fxg_collapse_add_rows");
}

template <class B>
static int fxg_cl_order(B &b, FxgClState &st, fxg_collapse_info *info)
{
    if (!info) FXG_CL_FAIL(b, "fxg_collapse_order: info is null");
    memset(info, 0, sizeof *info);
    info->first_bad = FXG_CL_NONE;
    if (st.stage == 0) FXG_CL_FAIL(b, "fxg_collapse_order: no set; fxg_collapse_begin makes one");
    if (st.stage == 2) FXG_CL_FAIL(b, "fxg_collapse_order: the set is ordered already");
    const u64 R = st.records, U = st.uniques, MR = R + 1, MU = U + 1;
    const u64 words = MR + fxg_cl_level_words(MR) + 4 * U + MU + fxg_cl_level_words(MU);
    FXG_CL_TRY(fxg_cl_grow(b, &st.ord, &st.ord_cap, words, 0, sizeof(u64), 0, "its order"));
    u64 *flags = st.ord, *lev = flags + MR;
    st.o_hash = lev + fxg_cl_level_words(MR); st.o_count = st.o_hash + U; st.o_ref = st.o_count + U; st.o_perm = st.o_ref + U; st.o_size = st.o_perm + U;
    u64 *lev2 = st.o_size + MU;
    const FxgClOrd o = fxg_cl_ord(st, flags, nullptr);
    FXG_CL_TRY(b.zero(flags, MR * sizeof(u64)));
    b.interval_begin();
    FXG_CL_TRY(b.mark(o.s, flags));
    FXG_CL_TRY(b.scan(flags, MR, lev));
    u64 marked = 0;
    FXG_CL_TRY(b.down(&marked, flags + R, sizeof marked));      // the scatter's arrays hold U entries: nothing is scattered unless the numbers agree
    if (marked != U) { st.stage = 0; snprintf(b.err, b.cap, "fxg_collapse_order: %llu slots are marked, the inserts counted %llu uniques (the set is lost)", (unsigned long long)marked, (unsigned long long)U); return FXG_E_DEVICE; }
    FXG_CL_TRY(b.scatter(o));
    b.interval_end();
    {
        std::vector<u64> hc(2 * U + 1), perm(U + 1);
        if (U) {
            FXG_CL_TRY(b.down(hc.data(), st.o_hash, 2 * U * sizeof(u64)));      // hash[], then count[]: 16 bytes per unique
            fxg_cl_replay(hc.data(), hc.data() + U, U, perm.data(), &st.out_reads);
            FXG_CL_TRY(b.up(st.o_perm, perm.data(), U * sizeof(u64)));
        } else st.out_reads = 0;
    }
    b.interval_begin();
    FXG_CL_TRY(b.sizes(o));
    FXG_CL_TRY(b.scan(st.o_size, MU, lev2));
    b.interval_end();
    FXG_CL_TRY(b.down(&st.out_bytes, st.o_size + U, sizeof(u64)));
    st.stage = 2;
    fxg_cl_info(st, info);
    return FXG_OK;
}

template <class B>
static int fxg_cl_write(B &b, FxgClState &st, u64 rank_begin, u64 out_cap, uint8_t *out, fxg_collapse_window *win)
{
    if (!win) FXG_CL_FAIL(b, "fxg_collapse_write: the window is null");
    memset(win, 0, sizeof *win);
    win->rank_end = rank_begin;
    if (st.stage == 0) FXG_CL_FAIL(b, "fxg_collapse_write: no set; fxg_collapse_begin makes one");
    if (st.stage == 1) FXG_CL_FAIL(b, "fxg_collapse_write: the set is not ordered; fxg_collapse_order comes first");
    const u64 U = st.uniques;
    if (rank_begin > U) FXG_CL_FAIL(b, "fxg_collapse_write: rank_begin %llu, the set has %llu sequences", (unsigned long long)rank_begin, (unsigned long long)U);
    if (rank_begin == U) return FXG_OK;
    const FxgClOrd o = fxg_cl_ord(st, nullptr, out);
    u64 res[FXG_CL_RES_WORDS];
    FXG_CL_TRY(b.window(o, rank_begin, out_cap));
    FXG_CL_TRY(b.down(res, st.res, sizeof res));                 // nothing may be written before the window is known to fit
    const u64 re = res[FXG_CL_RES_RANK_END];
    if (re == rank_begin) FXG_CL_FAIL(b, "fxg_collapse_write: rank %llu needs %llu bytes, d_out takes %llu", (unsigned long long)rank_begin, (unsigned long long)res[FXG_CL_RES_NEED], (unsigned long long)out_cap);
    if (!out) FXG_CL_FAIL(b, "fxg_collapse_write: d_out is null");
    if ((re - rank_begin) > (0x7FFFFFFFull * FXG_BLOCK) / FXG_CL_LANES) FXG_CL_FAIL(b, "fxg_collapse_write: the window holds too many records for one launch (2^27 groups); give it a smaller out_cap");
    b.interval_begin();
    FXG_CL_TRY(b.write(o, rank_begin, re));
    b.interval_end();
    FXG_CL_TRY(b.sync());
    win->rank_end = re; win->out_bytes = res[FXG_CL_RES_OUT_BYTES];
    return FXG_OK;
}

#ifndef FXG_HOST_EMULATION
__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_lens(const uint16_t *dlen, u64 n, u64 *tmp)
{
    const u64 r = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x;
    if (r <= n) tmp[r] = r < n ? (u64)dlen[r] : 0ull;
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_copy(const FxgClAddArgs a)
{
    const u64 g0 = ((u64)blockIdx.x * FXG_BLOCK + threadIdx.x) / FXG_CL_LANES, groups = (u64)gridDim.x * (FXG_BLOCK / FXG_CL_LANES);
    const u32 l = threadIdx.x & (FXG_CL_LANES - 1u);
    u64 reads = 0, first = FXG_CL_NONE;
    for (u64 r = g0; r < a.n; r += groups) {
        u64 c = 0;
        if (fxg_cl_copy_record(a, r, l, &c) && first == FXG_CL_NONE) first = r;      // (r only grows)
        reads += c;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 lo = __shfl_down((u32)reads, d, 64), hi = __shfl_down((u32)(reads >> 32), d, 64);
        reads += ((u64)hi << 32) | lo;
    }
    if (fxg_lane() == 0 && reads) fxg_cl_a_add(a.s.res + FXG_CL_RES_READS, reads);
    if (__ballot(first != FXG_CL_NONE) != 0ull) {                // (wave-uniform, and rare: the host drops the block)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const u64 o = ((u64)__shfl_xor((u32)(first >> 32), d, 64) << 32) | __shfl_xor((u32)first, d, 64);
            first = o < first ? o : first;
        }
        if (fxg_lane() == 0) { fxg_cl_a_min(a.s.res + FXG_CL_RES_FIRST_BAD, first); fxg_cl_a_or(a.s.res + FXG_CL_RES_IRREGULAR, 1ull); }
    }
}

// the irregular word and the smallest irregular record of a wave, as fxg_kernel_cl_copy raises them
__device__ __forceinline__ void fxg_cl_raise_first(u64 *res, u64 first)
{
    if (__ballot(first != FXG_CL_NONE) == 0ull) return;          // (wave-uniform, and rare: the host drops the block)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 o = ((u64)__shfl_xor((u32)(first >> 32), d, 64) << 32) | __shfl_xor((u32)first, d, 64);
        first = o < first ? o : first;
    }
    if (fxg_lane() == 0) { fxg_cl_a_min(res + FXG_CL_RES_FIRST_BAD, first); fxg_cl_a_or(res + FXG_CL_RES_IRREGULAR, 1ull); }
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_row_lens(const uint16_t *rlen, u64 n, u32 first, u32 last, u64 *bytes, u64 *num)
{
    const u64 r = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x;
    if (r <= n) fxg_cl_row_len(rlen, n, first, last, r, bytes, num);
}

// 16 lanes to a row, at most FXG_CL_GRID_MAX workgroups with further trips, as fxg_kernel_cl_copy
__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_copy_rows(const FxgClRowsArgs a)
{
    const u64 g0 = ((u64)blockIdx.x * FXG_BLOCK + threadIdx.x) / FXG_CL_LANES, groups = (u64)gridDim.x * (FXG_BLOCK / FXG_CL_LANES);
    const u32 l = threadIdx.x & (FXG_CL_LANES - 1u);
    u64 first = FXG_CL_NONE;
    for (u64 r = g0; r < a.n; r += groups)
        if (fxg_cl_copy_row(a, r, l) && first == FXG_CL_NONE) first = r;      // (r only grows)
    fxg_cl_raise_first(a.s.res, first);
}

// a lane to a row, further trips as above
__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_row_counts(const FxgClRowsArgs a)
{
    u64 reads = 0;
    for (u64 r = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x; r < a.n; r += (u64)gridDim.x * FXG_BLOCK) reads += fxg_cl_row_count(a, r);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 lo = __shfl_down((u32)reads, d, 64), hi = __shfl_down((u32)(reads >> 32), d, 64);
        reads += ((u64)hi << 32) | lo;
    }
    if (fxg_lane() == 0 && reads) fxg_cl_a_add(a.s.res + FXG_CL_RES_READS, reads);
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_init(u64 *slots, u64 nslots)
{
    for (u64 i = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x; i < nslots; i += (u64)gridDim.x * FXG_BLOCK) { slots[3 * i] = 0ull; slots[3 * i + 1] = 0ull; slots[3 * i + 2] = FXG_CL_NONE; }
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_rebuild(const u64 *old, u64 nold, const FxgClSet s, u32 hash_bits)
{
    u32 err = 0;
    for (u64 i = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x; i < nold; i += (u64)gridDim.x * FXG_BLOCK) err |= fxg_cl_move(old, i, s, hash_bits);
    if (err) fxg_cl_a_or(s.res + FXG_CL_RES_ERR, 1ull);
}

// a workgroup takes the records [rec0 + 256 b, rec0 + 256 b + 256) of the block just copied: consecutive in the arena
__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_insert(const FxgClSet s, u64 rec0, u64 n, u32 hash_bits)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[FXG_CL_STAGE_BYTES];
    const u64 r0 = (u64)blockIdx.x * FXG_BLOCK;
    const u32 have = (u32)(n - r0 < (u64)FXG_BLOCK ? n - r0 : (u64)FXG_BLOCK);
    const u64 gl = rec0 + r0 + have - 1u;
    const u64 b0 = s.off[rec0 + r0] & ~15ull, b1 = (s.off[gl] + s.len[gl] + 15ull) & ~15ull;      // whole 16-byte pieces: inside the arena's allocation
    const bool staged = b1 - b0 <= (u64)FXG_CL_STAGE_BYTES;      // (uniform)
    if (staged) {
        for (u64 i = (u64)threadIdx.x << 4; i < b1 - b0; i += (u64)FXG_BLOCK << 4) *reinterpret_cast<u32x4 *>(stage + i) = *reinterpret_cast<const u32x4 *>(s.arena + b0 + i);
        __syncthreads();
    }
    u32 what = 0;
    if (threadIdx.x < have) {
        const u64 g = rec0 + r0 + threadIdx.x;
        const u32 len = s.len[g];
        const u64 h = staged ? fxg_cl_hash(stage + (s.off[g] - b0), len) : fxg_cl_hash(s.arena + s.off[g], len);
        what = fxg_cl_insert(s, g, h, hash_bits);
    }
    const u64 fresh = (u64)__builtin_popcountll(__ballot(what == 1u));
    if (fxg_lane() == 0 && fresh) fxg_cl_a_add(s.res + FXG_CL_RES_NEW, fresh);
    if (__ballot(what == 2u) != 0ull && fxg_lane() == 0) fxg_cl_a_or(s.res + FXG_CL_RES_ERR, 1ull);
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_mark(const FxgClSet s, u64 *flags)
{
    for (u64 i = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x; i < s.nslots; i += (u64)gridDim.x * FXG_BLOCK) fxg_cl_mark(s, i, flags);
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_scatter(const FxgClOrd o)
{
    for (u64 i = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x; i < o.s.nslots; i += (u64)gridDim.x * FXG_BLOCK) fxg_cl_scatter(o, i);
}

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_sizes(const FxgClOrd o)
{
    for (u64 r = (u64)blockIdx.x * FXG_BLOCK + threadIdx.x; r <= o.uniques; r += (u64)gridDim.x * FXG_BLOCK) o.size[r] = fxg_cl_size(o, r);
}

__global__ void fxg_kernel_cl_window(const FxgClOrd o, u64 rank_begin, u64 out_cap) { fxg_cl_window(o, rank_begin, out_cap); }

__global__ __launch_bounds__(FXG_BLOCK) void fxg_kernel_cl_write(const FxgClOrd o, u64 rank_begin, u64 rank_end)
{
    const u64 rank = rank_begin + (((u64)blockIdx.x * FXG_BLOCK + threadIdx.x) >> 4);
    if (rank < rank_end) fxg_cl_write_record(o, rank_begin, rank, threadIdx.x & (FXG_CL_LANES - 1u));
}
#endif  // FXG_HOST_EMULATION
