/*
 * lzf_renumber.hip -- the device store gives item indices and key bytes back:
 * the live items (enc != LZF_ENC_NULL) copied, dense and in index order, into
 * a second set of item arrays, their key bytes packed into a second key arena
 * (lzf_gpu_store_renumber, include/lzf_gpu.h), and an index list from before
 * the call translated through its remap (lzf_gpu_store_remap).
 *
 * A semispace copy like the compaction (lzf_store.hip): nothing is done in
 * place and no workgroup waits for another.  Five launches:
 *   1. reduce: per scan tile (SD_TILE items, 4 neighbours per thread) the live
 *      count, the live key bytes, the dead items' key bytes, and whether a
 *      live key leaves the source arena.
 *   2. carry (one workgroup): the exclusive scans of both live sums over the
 *      tiles, the report, and the whole-call decision -- status, and on OK
 *      *dst_keys_used.  The three launches behind it do nothing on a refusal.
 *   3. write: a tile rescans its own items; a live item's ten members go to
 *      its rank, with the new key_off, and remap is filled.
 *   4. key pack: the same rescan gives every live key its place.  Pack and
 *      item order agree, so a tile owns ONE contiguous range of the
 *      destination arena and stages it through LDS in windows of RN_WIN
 *      bytes: a short key is copied into the window by its own lane, a long
 *      one (RN_LONG bytes and more) by its lane's whole wave, and after one
 *      barrier the workgroup writes the window out in aligned 16-byte stores.
 *      Windows are cut on 16-byte boundaries of the destination address, so
 *      only the tile's first and last granule can be partial; those go out
 *      byte by byte, the neighbouring tile owning the granule's other bytes.
 *      No byte is stored twice.
 *   5. pad: entries [live, dst_cap) of dst become dead items.
 *
 * The kernels are helpers of this translation unit, not part of the library's
 * routed kernel set: they have internal linkage (anonymous namespace).
 */
#include "lzf_store_dev.h"
#include "../../include/lzf_gpu.h"

/* both sums of one item in one word, as ST_LIVE_ONE of lzf_store.hip: a tile's
 * live key bytes stay below 2^42 (1024 keys of less than 2^32 bytes), its live
 * count (at most 1024) rides from bit 48 up */
#define RN_ONE   (1ull << 48)
#define RN_BYTES (RN_ONE - 1ull)
/* w_tile_n, between reduce and carry: a live key of the tile is out of range */
#define RN_BAD   (1ull << 63)
#define RN_DEAD  0xFFFFFFFFu              /* remap of a dead item */
/* the staging window: 32 KiB of the CU's 160 KiB of LDS, so four workgroups
 * stay resident, and a tile of 1024 keys of 16-40 bytes (28 KiB on average)
 * mostly needs one window */
#define RN_WIN   32768u
#define RN_LONG  256u                     /* from here on a key is staged by the whole wave */

namespace {

/* w_state.  VEND: the highest end of a live item's stored bytes, the val_off
 * of the dead tail */
enum { RN_BASE = 0, RN_TOTAL = 1, RN_STATUS = 2, RN_NLIVE = 3, RN_VEND = 4 };

__global__ __launch_bounds__(SD_BLOCK) void lzf_renumber_reduce_kernel(LzfRenumberArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t s = 0ull, dead = 0ull;
    int bad = 0;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t i = first + k;
        if (i >= a.count) break;
        const uint64_t len = a.src.key_len[i];
        if (a.src.enc[i] == (uint8_t)LZF_ENC_NULL) {
            dead += len;                  /* a dead item's key_off is never read */
            continue;
        }
        s += RN_ONE + len;
        const uint64_t off = a.src.key_off[i];
        bad |= off > a.src_keys_cap || len > a.src_keys_cap - off;
    }
    uint64_t tot, dtot;
    (void)dv_block_excl<SD_WAVES>(s, sw, &tot);
    (void)dv_block_excl<SD_WAVES>(dead, sw, &dtot);
    bad = __syncthreads_or(bad);
    if (threadIdx.x != 0u) return;
    a.w_tile_n[blockIdx.x] = (tot >> 48) | (bad ? RN_BAD : 0ull);
    a.w_tile_b[blockIdx.x] = tot & RN_BYTES;
    a.w_tile_d[blockIdx.x] = dtot;
}

/* one workgroup, any number of tiles in pieces of SD_BLOCK: the exclusive
 * scans of the tiles' live counts and live key bytes in place, the report and
 * the whole-call decision */
__global__ __launch_bounds__(SD_BLOCK) void lzf_renumber_carry_kernel(LzfRenumberArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    uint64_t rn = 0ull, rb = 0ull, rd = 0ull;
    int bad = 0;
    for (uint32_t c = 0; c < ntile; c += SD_BLOCK) {
        const uint32_t i = c + threadIdx.x;
        uint64_t xn = i < ntile ? a.w_tile_n[i] : 0ull;
        const uint64_t xb = i < ntile ? a.w_tile_b[i] : 0ull, xd = i < ntile ? a.w_tile_d[i] : 0ull;
        bad |= (int)(xn >> 63);
        xn &= ~RN_BAD;
        uint64_t tn, tb, td;
        const uint64_t on = dv_block_excl<SD_WAVES>(xn, sw, &tn), ob = dv_block_excl<SD_WAVES>(xb, sw, &tb);
        (void)dv_block_excl<SD_WAVES>(xd, sw, &td);
        if (i < ntile) {
            a.w_tile_n[i] = rn + on;
            a.w_tile_b[i] = rb + ob;
        }
        rn += tn;
        rb += tb;
        rd += td;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x != 0u) return;
    a.report[0] = rn;
    a.report[1] = rb;
    a.report[2] = (uint64_t)a.count - rn;
    a.report[3] = rd;
    const uint64_t base = *a.dst_keys_used, end = base + rb;
    uint32_t st = LZF_STORE_OK;
    if (bad) st = LZF_STORE_ERANGE;
    else if (rn > a.dst_cap || end < base || end > a.dst_keys_cap) st = LZF_STORE_FULL;
    a.w_state[RN_BASE] = base;
    a.w_state[RN_TOTAL] = st == LZF_STORE_OK ? rb : 0ull;
    a.w_state[RN_STATUS] = st;
    a.w_state[RN_NLIVE] = st == LZF_STORE_OK ? rn : 0ull;
    a.w_state[RN_VEND] = 0ull;
    *a.status = st;
    if (st == LZF_STORE_OK) *a.dst_keys_used = end;
}

/* an accepted call only: a live item's members to its rank, every item's
 * remap, and the workgroup's highest value end for the dead tail */
__global__ __launch_bounds__(SD_BLOCK) void lzf_renumber_write_kernel(LzfRenumberArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    if (a.w_state[RN_STATUS] != 0ull) return;             /* refused: no byte of dst or remap is written */
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t v[SD_PER], s = 0ull;
    uint8_t e[SD_PER];
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t i = first + k;
        e[k] = i < a.count ? a.src.enc[i] : (uint8_t)LZF_ENC_NULL;
        v[k] = e[k] != (uint8_t)LZF_ENC_NULL ? RN_ONE + a.src.key_len[i] : 0ull;
        s += v[k];
    }
    uint64_t tot;
    const uint64_t o = dv_block_excl<SD_WAVES>(s, sw, &tot);
    uint64_t rank = a.w_tile_n[blockIdx.x] + (o >> 48);
    uint64_t off = a.w_state[RN_BASE] + a.w_tile_b[blockIdx.x] + (o & RN_BYTES);
    uint64_t vend = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t i = first + k;
        if (i >= a.count) break;
        if (!v[k]) {
            if (a.remap) a.remap[i] = RN_DEAD;
            continue;
        }
        const uint64_t vo = a.src.val_off[i], vs = a.src.val_size[i];
        a.dst.val_off[rank] = vo;
        a.dst.val_size[rank] = (uint32_t)vs;
        a.dst.enc[rank] = e[k];
        a.dst.val_len[rank] = a.src.val_len[i];
        a.dst.key_off[rank] = off;
        a.dst.key_len[rank] = (uint32_t)(v[k] & RN_BYTES);
        if (a.src.item_time) {
            a.dst.item_time[rank] = a.src.item_time[i];
            a.dst.item_ttl[rank] = a.src.item_ttl[i];
        }
        if (a.src.item_lock) a.dst.item_lock[rank] = a.src.item_lock[i];
        if (a.src.last_access) a.dst.last_access[rank] = a.src.last_access[i];
        if (a.remap) a.remap[i] = (uint32_t)rank;
        const uint64_t ve = vo + vs < vo ? ~0ull : vo + vs;
        vend = ve > vend ? ve : vend;
        rank++;
        off += v[k] & RN_BYTES;
    }
    vend = sd_wave_max(vend);
    if ((threadIdx.x & 63u) == 0u && vend) atomicMax((unsigned long long *)&a.w_state[RN_VEND], (unsigned long long)vend);
}

/* window bytes [x0, x1) from src, the source byte of x0, by lane `lane` of
 * `lanes`: whole dwords of the window as one unaligned load and one aligned
 * LDS store each, the bytes before the first and after the last on their own.
 * No window byte outside [x0, x1) is touched: it is another key's */
__device__ inline void rn_stage(uint8_t *win, uint32_t x0, uint32_t x1, const uint8_t *src, uint32_t lane,
                                uint32_t lanes)
{
    const uint32_t a4 = (x0 + 3u) & ~3u, b4 = x1 & ~3u;
    const uint32_t head = a4 < x1 ? a4 : x1, tail = b4 > a4 ? b4 : a4;
    for (uint32_t j = x0 + lane; j < head; j += lanes) win[j] = src[j - x0];
    for (uint32_t j = a4 + 4u * lane; j < b4; j += 4u * lanes) {
        const uint32_t x = dv_ld4(src + (j - x0));
        __builtin_memcpy(__builtin_assume_aligned(win + j, 4), &x, 4);
    }
    for (uint32_t j = tail + lane; j < x1; j += lanes) win[j] = src[j - x0];
}

/* the part of the key [ks, ks + len) that lies in the window [ws, ws + RN_WIN) */
__device__ inline void rn_stage_key(uint8_t *win, uint64_t ws, uint64_t ks, uint32_t len, const uint8_t *key,
                                    uint32_t lane, uint32_t lanes)
{
    const uint64_t we = ws + RN_WIN, ke = ks + len;
    const uint64_t x0 = ks > ws ? ks : ws, x1 = ke < we ? ke : we;
    if (x0 < x1) rn_stage(win, (uint32_t)(x0 - ws), (uint32_t)(x1 - ws), key + (x0 - ks), lane, lanes);
}

/* an accepted call only: the tile's keys into its range of the destination
 * arena.  Positions are counted from the 16-byte boundary at or below the
 * range's first byte, so a window's granules are the destination's */
__global__ __launch_bounds__(SD_BLOCK) void lzf_renumber_pack_kernel(LzfRenumberArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    __shared__ uint4 win4[RN_WIN / 16u];
    if (a.w_state[RN_STATUS] != 0ull) return;
    uint8_t *win = (uint8_t *)win4;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint32_t len[SD_PER];
    uint64_t from[SD_PER], s = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t i = first + k;
        len[k] = i < a.count && a.src.enc[i] != (uint8_t)LZF_ENC_NULL ? a.src.key_len[i] : 0u;
        from[k] = len[k] ? a.src.key_off[i] : 0ull;
        s += len[k];
    }
    uint64_t tot;
    const uint64_t o = dv_block_excl<SD_WAVES>(s, sw, &tot);
    if (!tot) return;                                     /* the whole workgroup */
    uint8_t *out = a.dst_keys + a.w_state[RN_BASE] + a.w_tile_b[blockIdx.x];
    const uint64_t lo_all = (uint64_t)(uintptr_t)out & 15u, hi_all = lo_all + tot;
    out -= lo_all;                                        /* 16-byte aligned: position 0 */
    uint64_t at[SD_PER], run = lo_all + o;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        at[k] = run;
        run += len[k];
    }
    for (uint64_t ws = 0ull; ws < hi_all; ws += RN_WIN) {
#pragma unroll
        for (uint32_t k = 0; k < SD_PER; k++)
            if (len[k] && len[k] < RN_LONG) rn_stage_key(win, ws, at[k], len[k], a.src_keys + from[k], 0u, 1u);
#pragma unroll
        for (uint32_t k = 0; k < SD_PER; k++) {
            uint64_t m = __ballot(len[k] >= RN_LONG && at[k] < ws + RN_WIN && at[k] + len[k] > ws);
            while (m) {                                   /* the same in every lane of the wave */
                const int l = __ffsll((unsigned long long)m) - 1;
                m &= m - 1ull;
                const uint64_t ks = sd_lane_u64(at[k], l), fr = sd_lane_u64(from[k], l);
                const uint32_t ln = (uint32_t)__shfl((int)len[k], l, 64);
                rn_stage_key(win, ws, ks, ln, a.src_keys + fr, lane, 64u);
            }
        }
        __syncthreads();
        const uint64_t lo = ws > lo_all ? ws : lo_all, hi = ws + RN_WIN < hi_all ? ws + RN_WIN : hi_all;
        for (uint64_t g = ws + threadIdx.x * 16u; g < hi; g += SD_BLOCK * 16u) {
            if (g >= lo && g + 16u <= hi) {
                const uint4 x = win4[(g - ws) >> 4];
                __builtin_memcpy(__builtin_assume_aligned(out + g, 16), &x, 16);
            } else {                                      /* the tile's first or last granule */
                const uint64_t j0 = g > lo ? g : lo, j1 = g + 16u < hi ? g + 16u : hi;
                for (uint64_t j = j0; j < j1; j++) out[j] = win[j - ws];
            }
        }
        __syncthreads();
    }
}

/* an accepted call only: entries [live, dst_cap) of dst as dead items whose
 * offsets are the end offsets, as compaction leaves ties */
__global__ __launch_bounds__(SD_BLOCK) void lzf_renumber_pad_kernel(LzfRenumberArgs a)
{
    if (a.w_state[RN_STATUS] != 0ull) return;
    const uint64_t kend = a.w_state[RN_BASE] + a.w_state[RN_TOTAL], vend = a.w_state[RN_VEND];
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    for (uint64_t r = a.w_state[RN_NLIVE] + (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; r < a.dst_cap; r += step) {
        a.dst.val_off[r] = vend;
        a.dst.val_size[r] = 0u;
        a.dst.enc[r] = (uint8_t)LZF_ENC_NULL;
        a.dst.val_len[r] = 0u;
        a.dst.key_off[r] = kend;
        a.dst.key_len[r] = 0u;
        if (a.dst.item_time) {
            a.dst.item_time[r] = 0;
            a.dst.item_ttl[r] = 0;
        }
        if (a.dst.item_lock) a.dst.item_lock[r] = 0;
        if (a.dst.last_access) a.dst.last_access[r] = 0;
    }
}

/* duplicates, padding and indices past the old store are all fine: an entry is
 * read and written by one thread */
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_remap_kernel(uint32_t *idx, uint32_t n,
                                                                   const uint32_t *__restrict__ remap, uint32_t count)
{
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    for (uint64_t k = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; k < n; k += step) {
        const uint32_t i = idx[k];
        idx[k] = i < count ? remap[i] : RN_DEAD;
    }
}

}  // namespace

hipError_t lzf_launch_store_renumber(LzfRenumberArgs &a, hipStream_t s)
{
    const uint32_t nt = sd_tiles(a.count);
    hipLaunchKernelGGL(lzf_renumber_reduce_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_renumber_carry_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_renumber_write_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_renumber_pack_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_renumber_pad_kernel, dim3(sd_sweep_grid(a.dst_cap)), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t lzf_launch_store_remap(uint32_t *idx, uint32_t n, const uint32_t *remap, uint32_t count, hipStream_t s)
{
    hipLaunchKernelGGL(lzf_store_remap_kernel, dim3(sd_sweep_grid(n)), dim3(SD_BLOCK), 0, s, idx, n, remap, count);
    return hipGetLastError();
}
