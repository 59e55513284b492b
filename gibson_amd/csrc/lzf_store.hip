/*
 * lzf_store.hip -- the device SET path: gbSingleSet's store decision and the
 * dense copy into the store (src/query.c:384-417), for a whole batch, with the
 * values staying in HBM (lzf_gpu_set_store, include/lzf_gpu.h).
 *
 * The reference compresses a value above the `compression` threshold into
 * lzf_buffer with out_len = vlen - 4 (src/query.c:389-391), stores the stream
 * when there is one and the plain bytes when there is none (zmemdup,
 * src/query.c:409) and records item->size and item->encoding.  Here, on one
 * stream, with no host wait:
 *
 *   1. plan: per value whether it is a candidate (in_len > compression, within
 *      max_in_len) and its cap (gb_needcompr, gb_policy.h); the exclusive scan
 *      of the caps gives every candidate a scratch slot of exactly cap bytes
 *      (at most in_len + 8).  The slots must fit in in_bytes + 8 * count
 *      (LZF_STORE_EWORK otherwise).  A work copy of the lengths has 0 for
 *      every value that is not a candidate.
 *   2. compress: the routed compress launch over all `count` values with the
 *      work lengths (a 0-length value: out_len 0, src/lzf_c.c:131), handed in
 *      as a function pointer.
 *   3. size: val_size (the stream length, or in_len where there is no stream)
 *      and enc; the 64-bit exclusive scan of the sizes from base = *store_used
 *      gives val_off; base + total must fit in store_cap (LZF_STORE_FULL).
 *   4. pack: the stored bytes of every value to store + val_off[i].
 *
 * Scans (steps 1 and 3) are reduce-then-scan over tiles of 1024 values: tile
 * sums (wave prefix sums by __shfl_up, the 4 wave totals through LDS), one
 * workgroup's running scan over the tile sums (any tile count), and a second
 * pass that writes the absolute offsets.  No workgroup waits for another.
 *
 * Pack layout.  Work is balanced by DESTINATION bytes: the packed range
 * [store + base, store + base + total) is cut into tiles of ST_PACK_TILE bytes
 * whose starts are 16-byte aligned absolute addresses, so no two workgroups
 * ever touch one 16-byte granule; workgroups take tiles grid-stride (the grid
 * is fixed at launch, the tile count is computed on the device).  A workgroup
 * finds the value that holds its tile's first byte by a search in val_off for
 * the LAST index with val_off[i] <= p, which steps over runs of zero-size
 * values, whose offsets tie (all its threads probe at once: 256 entries per
 * round).  It copies the offsets and sources of the tile's values (up to 512)
 * into LDS, and every lane finds the value of a granule there the same way; a
 * tile of more values (runs of tiny ones) looks them up in HBM.  A granule
 * that lies wholly inside one value moves as one 16-byte load and one aligned
 * 16-byte store, whatever the source's alignment (an unaligned global load;
 * LZF_GPU_STORE_PACK=realign: two aligned loads realigned in registers).
 * Value heads, tails and values shorter than a granule are gathered byte by
 * byte into one aligned 16-byte store, one lane per granule, after the tile's
 * whole granules.
 *
 * The store's lifecycle (lzf_gpu_store_delete / _expire / _usage / _compact)
 * is further down: items are marked dead in enc, and the live ones are packed
 * into a second arena by the same scans and the same pack kernel, which is a
 * template over where its offset table and its sources come from.
 *
 * The kernels are helpers of this translation unit, not part of the library's
 * routed kernel set: they have internal linkage (anonymous namespace).
 */
#include <stdlib.h>
#include <string.h>

#include "lzf_store_dev.h"
#include "gb_policy.h"
#include "../../include/lzf_gpu.h"

/* The scans and sweeps run on the toolkit's geometry (lzf_store_dev.h).  The
 * pack kernel's own: it is balanced by destination bytes, not by entries.
 * Destination bytes per pack tile (a multiple of 16 * SD_BLOCK = 4096, so
 * every lane of a workgroup has the same number of granules).  256 K x 4 KiB
 * json, 500 MB packed: the pack kernel takes 467 us at 16 KiB and 300 us at
 * 64 KiB (a plain copy of the same bytes: 184 us); 4 KiB is slower again and
 * 256 KiB no faster (profiles/r08/store/): per tile the workgroup pays the
 * search and the table fill before it copies, and past 64 KiB a small batch
 * would sit on few workgroups */
#define ST_PACK_TILE 65536u
#define ST_PACK_GRID 2048u                /* 256 CUs x 8 workgroups */

namespace {

/* state words of the work area */
enum { ST_EWORK = 0, ST_BASE = 1, ST_TOTAL = 2, ST_STATUS = 3 };

/* what the scan of step 1 (SIZE false: the cap of a candidate, 0 otherwise)
 * and of step 3 (SIZE true: the stored size) adds up */
template <bool SIZE>
__device__ inline uint64_t st_item(const LzfStoreArgs &a, uint64_t i, bool ework)
{
    const uint32_t len = a.in_len[i];
    if (SIZE) {
        const uint32_t got = a.w_out[i];
        return ework ? 0ull : got ? got : len;
    }
    /* src/query.c:389, strict; past max_in_len: not compressed, stored plain */
    return (len > a.compression && len <= a.max_in_len) ? gb_needcompr(len) : 0u;
}

template <bool SIZE>
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_reduce_kernel(LzfStoreArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    const bool ework = SIZE && a.w_state[ST_EWORK] != 0ull;
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t s = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++)
        if (first + k < a.count) s += st_item<SIZE>(a, first + k, ework);
    uint64_t tot;
    (void)dv_block_excl<SD_WAVES>(s, sw, &tot);
    if (threadIdx.x == 0u) a.w_tile[blockIdx.x] = tot;
}

/* one workgroup: the exclusive scan of the tile sums in place, and the
 * batch-wide decision */
template <bool SIZE>
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_carry_kernel(LzfStoreArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t run = dv_carry_scan<SD_WAVES>(a.w_tile, ntile, sw);
    if (threadIdx.x != 0u) return;
    if (!SIZE) {
        a.w_state[ST_EWORK] = run > sd_slot_room(a.in_bytes, a.count) ? 1ull : 0ull;
        return;
    }
    const uint64_t base = *a.store_used, end = base + run;
    uint32_t st = LZF_STORE_OK;
    if (a.w_state[ST_EWORK]) st = LZF_STORE_EWORK;
    else if (end < base || end > a.store_cap) st = LZF_STORE_FULL;
    a.w_state[ST_BASE] = base;
    a.w_state[ST_TOTAL] = st == LZF_STORE_OK ? run : 0ull;
    a.w_state[ST_STATUS] = st;
    *a.status = st;
    if (st == LZF_STORE_OK) *a.store_used = end;
}

template <bool SIZE>
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_write_kernel(LzfStoreArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    const bool ework = a.w_state[ST_EWORK] != 0ull;
    const bool refused = SIZE && a.w_state[ST_STATUS] != 0ull;
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t v[SD_PER], s = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        v[k] = first + k < a.count ? st_item<SIZE>(a, first + k, ework) : 0ull;
        s += v[k];
    }
    uint64_t tot;
    uint64_t o = dv_block_excl<SD_WAVES>(s, sw, &tot) + a.w_tile[blockIdx.x];
    if (SIZE) o += a.w_state[ST_BASE];
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t i = first + k;
        if (i >= a.count) break;
        if (SIZE) {
            /* a refused batch: nothing stored, every item skipped by kv_frame */
            a.val_off[i] = refused ? a.w_state[ST_BASE] : o;
            a.val_size[i] = refused ? 0u : (uint32_t)v[k];
            a.enc[i] = refused ? (uint8_t)LZF_ENC_NULL : a.w_out[i] ? (uint8_t)LZF_ENC_LZF : (uint8_t)LZF_ENC_PLAIN;
        } else {
            /* on EWORK no slot is used: every value goes in with length 0 */
            const uint32_t cap = ework ? 0u : (uint32_t)v[k];
            a.w_slot_off[i] = ework ? 0ull : o;
            a.w_cap[i] = cap;
            a.w_len[i] = cap ? a.in_len[i] : 0u;
        }
        o += v[k];
    }
}

/* the last index i in [lo, hi) with off[i] <= p; needs off[lo] <= p.  Among
 * equal offsets (zero-size values) it is the last one: the value that holds
 * byte p, when any does */
__device__ inline uint32_t st_find(const uint64_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t p)
{
    while (hi - lo > 1u) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (off[m] <= p) lo = m;
        else hi = m;
    }
    return lo;
}

/* how many threads of the workgroup say yes; sc: SD_WAVES words of LDS */
__device__ inline uint32_t st_block_count(uint32_t wave_yes, uint32_t *sc)
{
    if ((threadIdx.x & 63u) == 0u) sc[threadIdx.x >> 6] = wave_yes;
    __syncthreads();
    uint32_t n = 0u;
    for (uint32_t w = 0; w < SD_WAVES; w++) n += sc[w];
    __syncthreads();
    return n;
}

/* st_find by the whole workgroup: every round the threads probe SD_BLOCK
 * evenly spaced entries of [lo, hi) at once and the range shrinks to one
 * stride, so 2^32 entries take four dependent loads, not 32.  The same
 * result in every thread */
__device__ inline uint32_t st_find_block(const uint64_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t p,
                                         uint32_t *sc)
{
    while (hi - lo > 1u) {
        const uint32_t step = (uint32_t)(((uint64_t)(hi - lo) + SD_BLOCK - 1u) / SD_BLOCK);
        const uint64_t i = lo + (uint64_t)threadIdx.x * step;
        const bool yes = i < hi && off[i] <= p;       /* true for the threads up to the one that holds p */
        const uint32_t c = st_block_count((uint32_t)__popcll(__ballot(yes)), sc);
        lo += (c ? c - 1u : 0u) * step;
        hi = (uint64_t)lo + step < hi ? lo + step : hi;
    }
    return lo;
}

/* 16 bytes at s (any alignment) from the two aligned 16-byte pieces around it;
 * the second piece is read only when s is not aligned, and then holds byte
 * s + 15, so neither load leaves the pages the 16 bytes lie in */
__device__ inline uint4 st_ld16_realign(const uint8_t *s)
{
    const uint32_t k = (uint32_t)((uintptr_t)s & 15u);
    const uint4 *q = (const uint4 *)(s - k);
    const uint4 a = q[0];
    if (!k) return a;
    const uint4 b = q[1];
    const uint32_t ws = k >> 2, sh = k & 3u;
    const uint32_t x0 = ws == 0u ? a.x : ws == 1u ? a.y : ws == 2u ? a.z : a.w;
    const uint32_t x1 = ws == 0u ? a.y : ws == 1u ? a.z : ws == 2u ? a.w : b.x;
    const uint32_t x2 = ws == 0u ? a.z : ws == 1u ? a.w : ws == 2u ? b.x : b.y;
    const uint32_t x3 = ws == 0u ? a.w : ws == 1u ? b.x : ws == 2u ? b.y : b.z;
    const uint32_t x4 = ws == 0u ? b.x : ws == 1u ? b.y : ws == 2u ? b.z : b.w;
    return make_uint4(__builtin_amdgcn_alignbyte(x1, x0, sh), __builtin_amdgcn_alignbyte(x2, x1, sh),
                      __builtin_amdgcn_alignbyte(x3, x2, sh), __builtin_amdgcn_alignbyte(x4, x3, sh));
}

/* where value i's stored bytes come from, as one word: the offset in the
 * scratch slots (top bit set) or in the input arena */
#define ST_FROM_SLOT (1ull << 63)
__device__ inline uint64_t st_source(const LzfStoreArgs &a, uint32_t i)
{
    return a.w_out[i] ? a.w_slot_off[i] | ST_FROM_SLOT : a.in_off[i];
}

__device__ inline const uint8_t *st_source_ptr(const LzfStoreArgs &a, uint64_t from)
{
    return (from & ST_FROM_SLOT ? a.w_slots : a.in) + (from & ~ST_FROM_SLOT);
}

/* What the pack kernel packs, the one thing its two callers differ in: a
 * table of `entries()` destination offsets (monotone, ties at entries without
 * bytes; entries() may be known on the device only), the source of entry i as
 * one word and the address that word names, the destination arena, and the
 * packed range [base(), base() + total()).  set_store: one entry per value of
 * the batch, the sources in the input arena or the compress slots */
struct StPackSet {
    LzfStoreArgs a;
    __device__ inline const uint64_t *off() const { return a.val_off; }
    __device__ inline uint32_t entries() const { return a.count; }
    __device__ inline uint64_t source(uint32_t i) const { return st_source(a, i); }
    __device__ inline const uint8_t *source_ptr(uint64_t from) const { return st_source_ptr(a, from); }
    __device__ inline uint8_t *store() const { return a.store; }
    __device__ inline uint64_t base() const { return a.w_state[ST_BASE]; }
    __device__ inline uint64_t total() const { return a.w_state[ST_TOTAL]; }
};

/* The entry that holds byte p of the store (an offset from the store's start),
 * for the entries [i0, i1) of one tile: its first byte vo, its end ve -- the
 * next entry's offset, the packing is dense -- and its source.  From the
 * arrays in HBM: */
template <typename P>
struct StMapGlobal {
    const P &p;
    const uint64_t *off;
    uint32_t i0, i1, n;
    uint64_t end;                      /* base + total */
    __device__ inline void at(uint64_t b, uint64_t &vo, uint64_t &ve, const uint8_t *&src) const
    {
        const uint32_t i = st_find(off, i0, i1, b);
        vo = off[i];
        ve = i + 1u < n ? off[i + 1u] : end;
        src = p.source_ptr(p.source(i));
    }
};

/* ... and from the tile's copy of them in LDS (off: n + 1 entries), which
 * takes the dependent loads from HBM out of every granule's way */
template <typename P>
struct StMapLds {
    const P &p;
    const uint64_t *off, *from;
    uint32_t n;
    __device__ inline void at(uint64_t b, uint64_t &vo, uint64_t &ve, const uint8_t *&src) const
    {
        const uint32_t k = st_find(off, 0u, n, b);
        vo = off[k];
        ve = off[k + 1u];
        src = p.source_ptr(from[k]);
    }
};

/* one granule that is not wholly inside one value -- a value's head and its
 * neighbour's tail, values shorter than a granule, the packed range's first
 * and last granule: its bytes [q0, q1) gathered byte by byte, every load in
 * flight at once, then one aligned 16-byte store (byte stores for a partial
 * granule).  Absolute addresses; sa: the store's address */
template <typename Map>
__device__ inline void st_pack_edge(uint8_t *store, const Map &m, uint64_t sa, uint64_t g, uint64_t lo, uint64_t hi)
{
    const uint64_t q0 = g > lo ? g : lo, q1 = g + 16u < hi ? g + 16u : hi;
    uint64_t vo = 0ull, ve = 0ull;
    const uint8_t *src = nullptr;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++) {
        if (g + j < q0 || g + j >= q1) continue;
        const uint64_t p = g + j - sa;
        if (p >= ve) m.at(p, vo, ve, src);                /* the next value that has bytes */
        w[j >> 2] |= (uint32_t)src[p - vo] << (8u * (j & 3u));
    }
    if (q1 - q0 == 16u) {
        *(uint4 *)(store + (g - sa)) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++)
        if (g + j >= q0 && g + j < q1) store[g + j - sa] = (uint8_t)(w[j >> 2] >> (8u * (j & 3u)));
}

/* one tile: bytes [lo, hi), absolute addresses like the tile's 16-byte
 * aligned start ta.  Four granules per lane and pass, the loads of a pass
 * before its stores; a granule inside one value is one 16-byte load and one
 * aligned 16-byte store.  The other granules: in place (EDGES), or left to
 * the caller */
template <bool REALIGN, bool EDGES, typename Map>
__device__ inline void st_pack_tile(uint8_t *store, const Map &m, uint64_t sa, uint64_t ta, uint64_t lo, uint64_t hi)
{
    for (uint64_t gb = ta + 16ull * threadIdx.x; gb < hi; gb += 64ull * SD_BLOCK) {
        uint4 v[4];
        uint32_t how[4];               /* 0: nothing, 1: v is the granule, 2: not inside one value */
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const uint64_t g = gb + 16ull * SD_BLOCK * u;
            how[u] = 0u;
            if (g < lo || g + 16u > hi) {                 /* a partial granule, or past the tile */
                if (g + 16u > lo && g < hi) how[u] = 2u;
                continue;
            }
            uint64_t vo, ve;
            const uint8_t *src;
            m.at(g - sa, vo, ve, src);
            if (ve < g + 16u - sa) {
                how[u] = 2u;
                continue;
            }
            const uint8_t *s = src + (g - sa - vo);
            v[u] = REALIGN ? st_ld16_realign(s) : dv_ld16(s);
            how[u] = 1u;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++)
            if (how[u] == 1u) *(uint4 *)(store + (gb + 16ull * SD_BLOCK * u - sa)) = v[u];
        if (EDGES) {
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++)
                if (how[u] == 2u) st_pack_edge(store, m, sa, gb + 16ull * SD_BLOCK * u, lo, hi);
        }
    }
}

/* values of a tile kept in LDS; a tile of more (runs of tiny values) looks
 * them up in HBM */
#define ST_LDS_VALS 512u

template <bool REALIGN, typename P>
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_pack_kernel(P p, uint32_t tile)
{
    __shared__ uint64_t s_off[ST_LDS_VALS + 1u], s_from[ST_LDS_VALS];
    __shared__ uint32_t sc[SD_WAVES];
    const uint64_t total = p.total();
    if (!total) return;                                   /* refused, or nothing to store */
    /* absolute addresses: the packed range [d0, d1), tiles from a0 (which may
     * lie up to 15 bytes before d0: nothing is accessed there) */
    uint8_t *const store = p.store();
    const uint64_t sa = (uint64_t)(uintptr_t)store, d0 = sa + p.base(), d1 = d0 + total;
    const uint64_t a0 = d0 & ~15ull;
    const uint64_t ntile = (d1 - a0 + tile - 1u) / tile;
    const uint64_t *__restrict__ voff = p.off();
    const uint32_t count = p.entries();
    for (uint64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
        const uint64_t ta = a0 + t * tile;
        const uint64_t lo = ta > d0 ? ta : d0, hi = ta + tile < d1 ? ta + tile : d1;
        /* i0: the value that holds byte lo */
        const uint32_t i0 = st_find_block(voff, 0u, count, lo - sa, sc);
        __syncthreads();                                  /* the tile before is done with the table */
        /* the ST_LDS_VALS + 1 entries from i0 into LDS, and n: how many of
         * them start at or before the tile's last byte -- the tile's values
         * [i0, i0 + n), entry n being the end of the last one */
        uint32_t yes = 0u;
        for (uint32_t k = threadIdx.x; k < ST_LDS_VALS + SD_BLOCK; k += SD_BLOCK) {
            const uint64_t i = (uint64_t)i0 + k;
            const bool in = k <= ST_LDS_VALS && i < count;
            const uint64_t o = in ? voff[i] : d1 - sa;
            if (k <= ST_LDS_VALS) s_off[k] = o;
            if (in && k < ST_LDS_VALS) s_from[k] = p.source((uint32_t)i);
            yes += (uint32_t)__popcll(__ballot(in && o <= hi - 1u - sa));
        }
        const uint32_t n = st_block_count(yes, sc);       /* its barrier: the table is written */
        if (n > ST_LDS_VALS) {                            /* a run of tiny values: look them up in HBM */
            const uint32_t i1 = st_find_block(voff, i0, count, hi - 1u - sa, sc) + 1u;
            st_pack_tile<REALIGN, true>(store, StMapGlobal<P>{p, voff, i0, i1, count, d1 - sa}, sa, ta, lo, hi);
            continue;
        }
        const StMapLds<P> m{p, s_off, s_from, n};
        st_pack_tile<REALIGN, false>(store, m, sa, ta, lo, hi);
        /* the granules not inside one value are those that hold a cut -- a
         * value's start, or the range's end -- at an address that is no
         * multiple of 16: one lane per cut, so a wave works on 64 of them at
         * once.  Cuts in one granule are neighbours in the table: the first
         * takes the granule */
        for (uint32_t k = threadIdx.x; k <= n; k += SD_BLOCK) {
            const uint64_t c = sa + s_off[k];
            if (!(c & 15ull) || c < lo || c > hi) continue;
            const uint64_t g = c & ~15ull;
            if (k) {
                const uint64_t pc = sa + s_off[k - 1u];
                if ((pc & 15ull) && (pc & ~15ull) == g && pc >= lo) continue;
            }
            st_pack_edge(store, m, sa, g, lo, hi);
        }
    }
}

/* ---- the store's lifecycle: delete, expire, usage, compact ------------------
 *
 * An item is dead once enc[i] == LZF_ENC_NULL.  Compaction is a semispace
 * copy: the same reduce / carry / write scan as above, over two sums per item
 * (live items and live bytes), decides the whole call in the carry kernel,
 * and the write pass -- only when the call was accepted -- emits the dense
 * list of the live items (destination offset, source offset, one entry per
 * live rank) that the pack kernel then runs over: a tile's table holds live
 * items only, however many dead ones lie between them. */

enum { ST_NLIVE = 4 };

/* both sums of one item in one word, for the scan inside a tile: a tile's
 * live bytes stay below 2^42 (1024 items of less than 2^32 bytes), its live
 * count (at most 1024) rides from bit 48 up */
#define ST_LIVE_ONE   (1ull << 48)
#define ST_LIVE_BYTES (ST_LIVE_ONE - 1ull)
/* w_tile_n, between reduce and carry: a live item of the tile is out of range */
#define ST_TILE_BAD   (1ull << 63)

/* RANGE: also fold whether a live item's [val_off, val_off + val_size) leaves
 * [0, src_cap) (usage has no offsets to check) */
template <bool RANGE>
__global__ __launch_bounds__(SD_BLOCK) void lzf_compact_reduce_kernel(LzfCompactArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t s = 0ull, dead = 0ull;
    int bad = 0;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t i = first + k;
        if (i >= a.count) break;
        const uint64_t size = a.val_size[i];
        if (a.enc[i] == (uint8_t)LZF_ENC_NULL) {
            dead += size;
            continue;
        }
        s += ST_LIVE_ONE + size;
        if (RANGE) {
            const uint64_t off = a.val_off[i];
            bad |= off > a.src_cap || size > a.src_cap - off;
        }
    }
    uint64_t tot, dtot;
    (void)dv_block_excl<SD_WAVES>(s, sw, &tot);
    (void)dv_block_excl<SD_WAVES>(dead, sw, &dtot);
    if (RANGE) bad = __syncthreads_or(bad);
    if (threadIdx.x != 0u) return;
    a.w_tile_n[blockIdx.x] = (tot >> 48) | (bad ? ST_TILE_BAD : 0ull);
    a.w_tile_b[blockIdx.x] = tot & ST_LIVE_BYTES;
    a.w_tile_d[blockIdx.x] = dtot;
}

/* one workgroup: the totals for the report and, COMPACT, the exclusive scans
 * of the tiles' live counts and live bytes in place and the whole-call
 * decision */
template <bool COMPACT>
__global__ __launch_bounds__(SD_BLOCK) void lzf_compact_carry_kernel(LzfCompactArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    uint64_t rn = 0ull, rb = 0ull, rd = 0ull;
    int bad = 0;
    for (uint32_t c = 0; c < ntile; c += SD_BLOCK) {
        const uint32_t i = c + threadIdx.x;
        uint64_t xn = i < ntile ? a.w_tile_n[i] : 0ull;
        const uint64_t xb = i < ntile ? a.w_tile_b[i] : 0ull, xd = i < ntile ? a.w_tile_d[i] : 0ull;
        bad |= (int)(xn >> 63);
        xn &= ~ST_TILE_BAD;
        uint64_t tn, tb, td;
        const uint64_t on = dv_block_excl<SD_WAVES>(xn, sw, &tn), ob = dv_block_excl<SD_WAVES>(xb, sw, &tb);
        (void)dv_block_excl<SD_WAVES>(xd, sw, &td);
        if (COMPACT && i < ntile) {
            a.w_tile_n[i] = rn + on;
            a.w_tile_b[i] = rb + ob;
        }
        rn += tn;
        rb += tb;
        rd += td;
    }
    if (COMPACT) bad = __syncthreads_or(bad);
    if (threadIdx.x != 0u) return;
    a.report[0] = rn;
    a.report[1] = rb;
    a.report[2] = (uint64_t)a.count - rn;
    a.report[3] = rd;
    if (!COMPACT) return;
    const uint64_t base = *a.dst_used, end = base + rb;
    uint32_t st = LZF_STORE_OK;
    if (bad) st = LZF_STORE_ERANGE;
    else if (end < base || end > a.dst_cap) st = LZF_STORE_FULL;
    a.w_state[ST_BASE] = base;
    a.w_state[ST_TOTAL] = st == LZF_STORE_OK ? rb : 0ull;
    a.w_state[ST_STATUS] = st;
    a.w_state[ST_NLIVE] = st == LZF_STORE_OK ? rn : 0ull;
    *a.status = st;
    if (st == LZF_STORE_OK) *a.dst_used = end;
}

/* an accepted call only: the live list, then every item's new offset and a
 * dead item's size 0.  An item's old offset is read by the thread that
 * replaces it, and the pack kernel reads the list, not val_off */
__global__ __launch_bounds__(SD_BLOCK) void lzf_compact_write_kernel(LzfCompactArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    if (a.w_state[ST_STATUS] != 0ull) return;             /* refused: the arrays stay as they are */
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t v[SD_PER], s = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t i = first + k;
        v[k] = i < a.count && a.enc[i] != (uint8_t)LZF_ENC_NULL ? ST_LIVE_ONE + a.val_size[i] : 0ull;
        s += v[k];
    }
    uint64_t tot;
    const uint64_t o = dv_block_excl<SD_WAVES>(s, sw, &tot);
    uint64_t rank = a.w_tile_n[blockIdx.x] + (o >> 48);
    uint64_t off = a.w_state[ST_BASE] + a.w_tile_b[blockIdx.x] + (o & ST_LIVE_BYTES);
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t i = first + k;
        if (i >= a.count) break;
        if (v[k]) {
            a.w_live_dst[rank] = off;
            a.w_live_src[rank] = a.val_off[i];
            rank++;
        } else {
            a.val_size[i] = 0u;
        }
        a.val_off[i] = off;
        off += v[k] & ST_LIVE_BYTES;
    }
}

/* compaction's plan for the pack kernel: one entry per live item, the source
 * an offset into the old arena.  A realigning load reads the aligned 16 bytes
 * around a value's last byte, which lie in that byte's page */
struct StPackLive {
    LzfCompactArgs a;
    __device__ inline const uint64_t *off() const { return a.w_live_dst; }
    __device__ inline uint32_t entries() const { return (uint32_t)a.w_state[ST_NLIVE]; }
    __device__ inline uint64_t source(uint32_t i) const { return a.w_live_src[i]; }
    __device__ inline const uint8_t *source_ptr(uint64_t from) const { return a.src + from; }
    __device__ inline uint8_t *store() const { return a.dst; }
    __device__ inline uint64_t base() const { return a.w_state[ST_BASE]; }
    __device__ inline uint64_t total() const { return a.w_state[ST_TOTAL]; }
};

/* DEL / overwrite by index.  Byte stores: indices that share a 4-byte word of
 * enc, or repeat, all store the same byte and none reads */
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_delete_kernel(const uint32_t *__restrict__ idx, uint32_t n,
                                                                    uint8_t *enc, uint32_t count)
{
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    for (uint64_t k = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; k < n; k += step) {
        const uint32_t i = idx[k];
        if (i < count) enc[i] = (uint8_t)LZF_ENC_NULL;
    }
}

/* the TTL rule (mg_ttl_reached) over every item that is not NULL yet; the
 * count by wave ballot, one atomic add per wave.  Every lane of a workgroup
 * makes the same number of rounds */
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_expire_kernel(LzfItems it, uint32_t *expired)
{
    const int64_t *__restrict__ item_time = it.item_time;
    const int32_t *__restrict__ ttl = it.item_ttl;
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t hits = 0u;
    for (uint64_t b = (uint64_t)blockIdx.x * SD_BLOCK; b < it.count; b += step) {
        const uint64_t i = b + threadIdx.x;
        bool hit = false;
        if (i < it.count && it.enc[i] != (uint8_t)LZF_ENC_NULL) {
            hit = mg_ttl_reached(ttl[i], it.now, item_time, i);
            if (hit) it.enc[i] = (uint8_t)LZF_ENC_NULL;
        }
        hits += sd_count(hit);
    }
    sd_leader_add(expired, hits);
}

/* LZF_GPU_STORE_TILE_KB (diagnostics, read per launch): the pack tile in KiB,
 * a multiple of 4 up to 1024 */
uint32_t st_pack_tile()
{
    const char *e = getenv("LZF_GPU_STORE_TILE_KB");
    if (e) {
        const unsigned long kb = strtoul(e, nullptr, 10);
        if (kb >= 4u && kb <= 1024u && kb % 4u == 0u) return (uint32_t)kb << 10;
    }
    return ST_PACK_TILE;
}

/* LZF_GPU_STORE_PACK=realign (diagnostics): aligned loads realigned in
 * registers instead of unaligned global loads */
bool st_pack_realign()
{
    const char *e = getenv("LZF_GPU_STORE_PACK");
    return e && !strcmp(e, "realign");
}

/* the pack launch: the grid from the host's bound on the packed bytes; the
 * kernel strides over the tiles there really are */
template <typename P>
hipError_t st_launch_pack(const P &p, uint64_t most_bytes, hipStream_t s)
{
    const uint32_t tile = st_pack_tile();
    const uint64_t most = most_bytes / tile + 2u;
    const uint32_t grid = (uint32_t)(most < ST_PACK_GRID ? most : ST_PACK_GRID);
    if (st_pack_realign())
        hipLaunchKernelGGL((lzf_store_pack_kernel<true, P>), dim3(grid), dim3(SD_BLOCK), 0, s, p, tile);
    else
        hipLaunchKernelGGL((lzf_store_pack_kernel<false, P>), dim3(grid), dim3(SD_BLOCK), 0, s, p, tile);
    return hipGetLastError();
}

}  // namespace

hipError_t lzf_launch_store(LzfStoreArgs &a, hipStream_t s, hipError_t (*compress)(const LzfBatch &, hipStream_t))
{
    const uint32_t nt = sd_tiles(a.count);
    hipLaunchKernelGGL(lzf_store_reduce_kernel<false>, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_store_carry_kernel<false>, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_store_write_kernel<false>, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    /* a batch with no candidate at all (max_in_len 0) is not compressed */
    if ((e = hipMemsetAsync(a.w_out, 0, (size_t)a.count * sizeof(uint32_t), s)) != hipSuccess) return e;
    if (a.max_in_len) {
        LzfBatch b{a.in, a.in_off, a.w_len, a.w_slots, a.w_slot_off, a.w_cap, a.w_out, nullptr, a.count, a.max_in_len};
        if ((e = compress(b, s)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lzf_store_reduce_kernel<true>, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_store_carry_kernel<true>, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_store_write_kernel<true>, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return st_launch_pack(StPackSet{a}, sd_slot_room(a.in_bytes, a.count), s);
}

hipError_t lzf_launch_store_delete(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count, hipStream_t s)
{
    hipLaunchKernelGGL(lzf_store_delete_kernel, dim3(sd_sweep_grid(n)), dim3(SD_BLOCK), 0, s, idx, n, enc, count);
    return hipGetLastError();
}

hipError_t lzf_launch_store_expire(const LzfItems &it, uint32_t *expired, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(expired, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_store_expire_kernel, dim3(sd_sweep_grid(it.count)), dim3(SD_BLOCK), 0, s, it, expired);
    return hipGetLastError();
}

hipError_t lzf_launch_store_usage(LzfCompactArgs &a, hipStream_t s)
{
    const uint32_t nt = sd_tiles(a.count);
    hipLaunchKernelGGL(lzf_compact_reduce_kernel<false>, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_compact_carry_kernel<false>, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    return hipGetLastError();
}

hipError_t lzf_launch_store_compact(LzfCompactArgs &a, hipStream_t s)
{
    const uint32_t nt = sd_tiles(a.count);
    hipLaunchKernelGGL(lzf_compact_reduce_kernel<true>, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_compact_carry_kernel<true>, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_compact_write_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    /* the live bytes fit in both arenas, or the call is refused */
    return st_launch_pack(StPackLive{a}, a.dst_cap < a.src_cap ? a.dst_cap : a.src_cap, s);
}
