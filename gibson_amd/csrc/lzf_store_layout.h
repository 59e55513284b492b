/*
 * lzf_store_layout.h -- the work areas of the device store's operators, host
 * side and free of kernels: the geometry a work area's size depends on, a bump
 * carver, and per work area ONE layout function that names every array with
 * its length.  lzf_X_work_bytes is the layout run in measuring mode plus the
 * slack the caller's pointer may need; lzf_X_carve is the same function run
 * over that pointer (lzf_layout.cpp).  A size and a carve therefore cannot
 * disagree, and csrc/carve_check.cpp writes every byte of every array of every
 * layout at every base misalignment, under the host sanitizers.
 */
#ifndef GIBSON_AMD_LZF_STORE_LAYOUT_H
#define GIBSON_AMD_LZF_STORE_LAYOUT_H

#include "lzf_internal.h"
#include "gb_policy.h"
#include "../../include/lzf_gpu.h"

/* The one geometry of the store's kernels (lzf_store_dev.h has the device
 * side): workgroups of 256 threads, 4 waves; a scan tile is 4 neighbouring
 * entries per thread; a grid-stride sweep runs on 256 CUs x 8 workgroups; a
 * wave-per-entry kernel on at most 16384 workgroups, past which its waves
 * stride over the list */
#define SD_BLOCK     256u
#define SD_PER       4u
#define SD_TILE      (SD_BLOCK * SD_PER)
#define SD_WAVES     (SD_BLOCK / 64u)
#define SD_GRID      2048u
#define SD_WAVE_GRID 16384u
#define SD_WORDS     (SD_TILE / 64u)      /* ballot words per select tile */

static inline uint32_t sd_tiles(uint64_t n)
{
    return (uint32_t)((n + SD_TILE - 1u) / SD_TILE);
}

/* the grid of a sweep with one thread per entry */
static inline uint32_t sd_sweep_grid(uint64_t n)
{
    const uint64_t g = (n + SD_BLOCK - 1u) / SD_BLOCK;
    return (uint32_t)(g < SD_GRID ? g : SD_GRID);
}

/* the grid of a kernel with one wave per entry */
static inline uint32_t sd_wave_grid(uint64_t n)
{
    const uint64_t g = (n + SD_WAVES - 1u) / SD_WAVES;
    return (uint32_t)(g < SD_WAVE_GRID ? g : SD_WAVE_GRID);
}

/* set_store's scratch slots' room: in_bytes + 8 * count, saturating */
static __host__ __device__ inline uint64_t sd_slot_room(uint64_t in_bytes, uint32_t count)
{
    const uint64_t r = in_bytes + 8ull * count;
    return r < in_bytes ? ~0ull : r;
}

/* MSET's compress slot: gb_needcompr(vlen) bytes at most, rounded up */
static inline uint64_t sd_mset_slot_bytes(uint32_t vlen)
{
    return ((uint64_t)vlen + vlen / 16u + 8u + 15u) & ~15ull;
}

/* A bump carver.  Over a work pointer it hands out that memory; without one
 * (measuring mode) it only counts, from a start taken to be aligned.  The
 * count saturates at ~0, so a size past 2^64 reads as ~0 and not as a small
 * number.  take() does not align: a layout aligns its start and orders its
 * arrays by falling element size */
struct LzfCarver {
    uint8_t *base;
    uint64_t at;

    explicit LzfCarver(void *work = nullptr) : base((uint8_t *)work), at(0ull) {}
    void pad(uint64_t bytes) { at = at + bytes < at ? ~0ull : at + bytes; }
    void align(uint64_t k) { pad((k - ((uint64_t)(uintptr_t)base + at) % k) % k); }
    template <typename T>
    T *take(uint64_t count)
    {
        T *p = base ? (T *)(base + at) : nullptr;
        pad(count * sizeof(T));
        return p;
    }
    uint64_t bytes() const { return at; }
};

/* the state words of every work area but the frame's: 8 x u64 */
#define SD_STATE_WORDS 8u

/* kv_frame's tiles, in 32 bits as its launch has always counted them: the sum
 * wraps for a count within 1023 of 2^32, far past any frame that fits a reply */
static inline uint32_t sd_frame_tiles(uint32_t count)
{
    return (count + SD_TILE - 1u) / SD_TILE;
}

/* kv_frame (lzf_frame.hip) */
static inline void lzf_frame_layout(LzfFrameArgs &a, LzfCarver &c)
{
    const uint64_t n = a.count;
    c.align(8);
    a.w_off = c.take<uint64_t>(n);
    a.w_voff = c.take<uint64_t>(n);
    a.w_bsum = c.take<uint64_t>(sd_frame_tiles(a.count));
    a.w_state = c.take<uint64_t>(2);
    a.w_len = c.take<uint32_t>(n);
    a.w_err = c.take<int32_t>(n);
    a.w_skip = c.take<uint8_t>(n);
}

/* set_store (lzf_store.hip); past the slots, 16 bytes the realigning loads of
 * the pack kernel may read */
static inline void lzf_store_layout(LzfStoreArgs &a, LzfCarver &c)
{
    const uint64_t n = a.count;
    c.align(16);
    a.w_state = c.take<uint64_t>(SD_STATE_WORDS);
    a.w_slot_off = c.take<uint64_t>(n);
    a.w_tile = c.take<uint64_t>(sd_tiles(n));
    a.w_len = c.take<uint32_t>(n);
    a.w_cap = c.take<uint32_t>(n);
    a.w_out = c.take<uint32_t>(n);
    a.w_slots = c.take<uint8_t>(sd_slot_room(a.in_bytes, a.count));
    c.pad(16);
}

/* usage and compact (lzf_store.hip) */
static inline void lzf_compact_layout(LzfCompactArgs &a, LzfCarver &c)
{
    const uint64_t n = a.count, nt = sd_tiles(n);
    c.align(16);
    a.w_state = c.take<uint64_t>(SD_STATE_WORDS);
    a.w_tile_n = c.take<uint64_t>(nt);
    a.w_tile_b = c.take<uint64_t>(nt);
    a.w_tile_d = c.take<uint64_t>(nt);
    a.w_live_dst = c.take<uint64_t>(n);
    a.w_live_src = c.take<uint64_t>(n);
}

/* renumber (lzf_renumber.hip): per-tile sums only -- the write and the key
 * pack rescan their own tile, so nothing is kept per item */
static inline void lzf_renumber_layout(LzfRenumberArgs &a, LzfCarver &c)
{
    const uint64_t nt = sd_tiles(a.count);
    c.align(8);
    a.w_state = c.take<uint64_t>(SD_STATE_WORDS);
    a.w_tile_n = c.take<uint64_t>(nt);
    a.w_tile_b = c.take<uint64_t>(nt);
    a.w_tile_d = c.take<uint64_t>(nt);
}

/* append_keys (lzf_request.hip): per-tile sums only, as the renumbering */
static inline void lzf_append_layout(LzfAppendArgs &a, LzfCarver &c)
{
    const uint64_t nt = sd_tiles(a.n);
    c.align(8);
    a.w_state = c.take<uint64_t>(SD_STATE_WORDS);
    a.w_tile_n = c.take<uint64_t>(nt);
    a.w_tile_b = c.take<uint64_t>(nt);
}

/* request_bucket (lzf_dispatch.hip): one count per class and scan tile, u64 as
 * dv_carry_scan scans them in place */
static inline void lzf_bucket_layout(LzfBucketArgs &a, LzfCarver &c)
{
    c.align(8);
    a.w_table = c.take<uint64_t>((uint64_t)LZF_RQ_NCLASS * sd_tiles(a.n));
}

/* select (lzf_mget.hip) */
static inline void lzf_select_layout(LzfSelectArgs &a, LzfCarver &c)
{
    const uint64_t nt = sd_tiles(a.count);
    c.align(8);
    a.w_mask = c.take<uint64_t>(nt * SD_WORDS);
    a.w_tile = c.take<uint64_t>(nt);
}

/* the node table of the ordered select: a power of two of at least twice the
 * node words, at least 2; 0 where 2^63 does not hold it */
static __host__ __device__ inline uint64_t sd_order_slots(uint64_t node_words)
{
    if (node_words > (1ull << 62)) return 0ull;
    uint64_t s = 2ull;
    while (s < 2ull * node_words) s <<= 1;
    return s;
}

/* select_ordered (lzf_order.hip); a table past 2^63 words saturates the size */
static inline void lzf_order_layout(LzfOrderArgs &a, LzfCarver &c)
{
    const uint64_t nt = sd_tiles(a.count), cn = a.cand_cap, ct = sd_tiles(cn);
    a.slots = sd_order_slots(a.node_cap);
    c.align(8);
    a.w_state = c.take<uint64_t>(SD_STATE_WORDS);
    a.w_mask = c.take<uint64_t>(nt * SD_WORDS);
    a.w_tile_n = c.take<uint64_t>(nt);
    a.w_tile_b = c.take<uint64_t>(nt);
    a.w_tile_m = c.take<uint64_t>(nt);
    if (!a.slots || a.slots > (~0ull >> 3)) c.pad(~0ull);
    a.w_table = c.take<uint64_t>(a.slots);
    a.w_ctile_n = c.take<uint64_t>(ct);
    a.w_ctile_b = c.take<uint64_t>(ct);
    a.w_row_off = c.take<uint64_t>(cn);
    if (a.node_cap > (~0ull >> 2)) c.pad(~0ull);
    a.w_rows = c.take<uint32_t>(a.node_cap);
    a.w_cand = c.take<uint32_t>(cn);
    a.w_live = c.take<uint32_t>(cn);
    a.w_row_len = c.take<uint32_t>(cn);
    a.w_sort[0] = c.take<uint32_t>(cn);
    a.w_sort[1] = c.take<uint32_t>(cn);
}

/* mget (lzf_mget.hip) */
static inline void lzf_mget_layout(LzfMgetArgs &a, LzfCarver &c)
{
    const uint64_t n = a.n, nt = sd_tiles(n);
    c.align(8);
    a.w_state = c.take<uint64_t>(SD_STATE_WORDS);
    a.g_key_off = c.take<uint64_t>(n);
    a.g_val_off = c.take<uint64_t>(n);
    a.w_off = c.take<uint64_t>(n);
    a.w_voff = c.take<uint64_t>(n);
    a.w_tile = c.take<uint64_t>(nt);
    a.w_tcnt = c.take<uint64_t>(nt);
    a.g_key_len = c.take<uint32_t>(n);
    a.g_val_size = c.take<uint32_t>(n);
    a.g_val_len = c.take<uint32_t>(n);
    a.g_null = c.take<uint32_t>(n);
    a.w_len = c.take<uint32_t>(n);
    a.w_err = c.take<int32_t>(n);
    a.g_enc = c.take<uint8_t>(n);
    a.w_skip = c.take<uint8_t>(n);
}

/* replies (lzf_reply.hip); w_skip: LZF_DECODE_NCLASS lists of n */
static inline void lzf_reply_layout(LzfReplyArgs &a, LzfCarver &c)
{
    const uint64_t n = a.n, nt = sd_tiles(n);
    c.align(8);
    a.w_state = c.take<uint64_t>(SD_STATE_WORDS);
    a.g_val_off = c.take<uint64_t>(n);
    a.w_off = c.take<uint64_t>(n);
    a.w_voff = c.take<uint64_t>(n);
    a.w_tile = c.take<uint64_t>(nt);
    a.w_tcnt = c.take<uint64_t>(nt);
    a.g_val_size = c.take<uint32_t>(n);
    a.g_val_len = c.take<uint32_t>(n);
    a.g_null = c.take<uint32_t>(n);
    a.w_len = c.take<uint32_t>(n);
    a.w_err = c.take<int32_t>(n);
    a.g_enc = c.take<uint8_t>(n);
    a.g_code = c.take<uint8_t>(n);
    a.g_cls = c.take<uint8_t>(n);
    a.w_skip = c.take<uint8_t>(n * LZF_DECODE_NCLASS);
}

/* minc (lzf_ops.hip) */
static inline void lzf_minc_layout(LzfMincArgs &a, LzfCarver &c)
{
    const uint64_t n = a.n;
    c.align(8);
    a.w_state = c.take<uint64_t>(SD_STATE_WORDS);
    a.w_val = c.take<int64_t>(n);
    a.w_tile = c.take<uint64_t>(sd_tiles(n));
    a.w_cls = c.take<uint8_t>(n);
}

/* mset (lzf_mset.hip).  The compress batch's descriptors share 64 bytes: c_off
 * (in_off, out_off), then c_len (in_len, out_cap, out_len).  The compress slot
 * is 16-byte aligned and comes before the arrays whose length depends on n, so
 * that it needs no alignment step of its own; the classes are rounded up to 16 */
static inline void lzf_mset_layout(LzfMsetArgs &a, LzfCarver &c)
{
    const uint64_t n = a.n;
    c.align(16);
    a.w_state = c.take<uint64_t>(SD_STATE_WORDS);
    a.c_off = c.take<uint64_t>(2);
    a.c_len = c.take<uint32_t>(3);
    c.pad(64u - 2u * 8u - 3u * 4u);
    a.w_slot = c.take<uint8_t>(sd_mset_slot_bytes(a.vlen));
    a.w_tile = c.take<uint64_t>(sd_tiles(n));
    a.w_cls = c.take<uint8_t>((n + 15u) & ~15ull);
}

/* keys (lzf_meta.hip) */
static inline void lzf_keys_layout(LzfKeysArgs &a, LzfCarver &c)
{
    const uint64_t nt = sd_tiles(a.n);
    c.align(8);
    a.w_state = c.take<uint64_t>(SD_STATE_WORDS);
    a.w_tile_n = c.take<uint64_t>(nt);
    a.w_tile_b = c.take<uint64_t>(nt);
}

#endif
