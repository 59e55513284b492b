/*
 * lzf_request.hip -- request ingest: raw request buffers become the
 * descriptors of the device store's calls without the host reading a request.
 *
 * lzf_gpu_request_parse: one lane per request runs lzf_request_entry
 * (lzf_request.h, the one copy of the grammar), which finds the first space a
 * 64-bit word at a time.  A key-only request is 2 + 16-40 bytes and a SET's
 * scan touches at most max_key bytes whatever its value's size, so the cost is
 * the scattered cache lines of the requests, not bytes: a lane's loads are
 * unaligned 8-byte loads inside its own request, and the seven outputs are
 * coalesced stores.
 *
 * lzf_gpu_store_append_keys: reduce / carry / write over scan tiles of SD_TILE
 * requests, as the compaction and the renumbering, with no workgroup waiting
 * for another.  Three launches:
 *   1. reduce: per tile the accepted requests and their key bytes.
 *   2. carry (one workgroup): the exclusive scan of the key bytes over the
 *      tiles, the result, and the whole-call decision -- FULL, or OK and the
 *      new *keys_used -- before any byte is written.
 *   3. write: a tile rescans its own requests, fills its items' members,
 *      set_len and void_idx, and packs its keys into its ONE contiguous range
 *      of the key arena, staged through 32 KiB LDS windows cut on 16-byte
 *      boundaries of the destination as lzf_renumber_pack_kernel stages its
 *      own; the sources are key spans inside request buffers, a whole request
 *      apart.  On FULL it fills the refusal and writes no key byte.
 *
 * The window staging (ap_stage, ap_stage_key, ap_pack_tile) is a second copy
 * of lzf_renumber_pack_kernel's, not a function shared with it: with the
 * staging moved into one __device__ function of lzf_store_dev.h the
 * renumbering's kernel compiled to a different instruction stream (the
 * long-key ballot lost its branches, 12 lines of 4305), so lzf_renumber.hip
 * stays as it was.
 *
 * The kernels are helpers of this translation unit, not part of the library's
 * routed kernel set: they have internal linkage (anonymous namespace).
 */
#include "lzf_store_dev.h"
#include "../../include/lzf_gpu.h"

/* both sums of one request in one word, as RN_ONE of lzf_renumber.hip: a tile's
 * key bytes stay below 2^42, its accepted count rides from bit 48 up */
#define AP_ONE   (1ull << 48)
#define AP_BYTES (AP_ONE - 1ull)
#define AP_VOID  0xFFFFFFFFu              /* void_idx of an accepted request: padding for the delete */
/* the staging window: 32 KiB of the CU's 160 KiB of LDS, so four workgroups
 * stay resident, and a tile of 1024 keys of 16-40 bytes (28 KiB on average)
 * mostly needs one window; the values of RN_WIN and RN_LONG (lzf_renumber.hip) */
#define AP_WIN   32768u
#define AP_LONG  256u                     /* from here on a key is staged by the whole wave */

namespace {

enum { AP_BASE = 0, AP_STATUS = 1 };      /* w_state */

__global__ __launch_bounds__(SD_BLOCK) void lzf_request_parse_kernel(LzfRequestArgs a)
{
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t cnt[LZF_REQ_NSTATUS];
#pragma unroll
    for (uint32_t c = 0; c < LZF_REQ_NSTATUS; c++) cnt[c] = 0u;
    for (uint64_t b = (uint64_t)blockIdx.x * SD_BLOCK; b < a.n; b += step) {
        const uint64_t k = b + threadIdx.x;
        const uint32_t st = k < a.n ? lzf_request_entry(a, k) : SD_NONE;
#pragma unroll
        for (uint32_t c = 0; c < LZF_REQ_NSTATUS; c++) cnt[c] += sd_count(st == c);
    }
#pragma unroll
    for (uint32_t c = 0; c < LZF_REQ_NSTATUS; c++) sd_leader_add(a.result + c, (uint64_t)cnt[c]);
}

/* window bytes [x0, x1) from src, the source byte of x0, by lane `lane` of
 * `lanes`: whole dwords of the window as one unaligned load and one aligned
 * LDS store each, the bytes before the first and after the last on their own.
 * No window byte outside [x0, x1) is touched: it is another key's.  No source
 * byte outside the key is read */
__device__ inline void ap_stage(uint8_t *win, uint32_t x0, uint32_t x1, const uint8_t *src, uint32_t lane,
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

/* the part of the key [ks, ks + len) that lies in the window [ws, ws + AP_WIN) */
__device__ inline void ap_stage_key(uint8_t *win, uint64_t ws, uint64_t ks, uint32_t len, const uint8_t *key,
                                    uint32_t lane, uint32_t lanes)
{
    const uint64_t we = ws + AP_WIN, ke = ks + len;
    const uint64_t x0 = ks > ws ? ks : ws, x1 = ke < we ? ke : we;
    if (x0 < x1) ap_stage(win, (uint32_t)(x0 - ws), (uint32_t)(x1 - ws), key + (x0 - ks), lane, lanes);
}

/* The whole workgroup: the tile's keys -- this thread's are len[k] bytes at
 * src + from[k], len 0 for none -- to out, the tile's range of `tot` bytes of
 * the key arena; o is the exclusive scan of the thread's key bytes over the
 * tile.  Positions are counted from the 16-byte boundary at or below the
 * range's first byte, so a window's granules are the destination's: a short
 * key is copied into the window by its own lane, a long one (AP_LONG bytes and
 * more) by its lane's whole wave, and after one barrier the workgroup writes
 * the window out in aligned 16-byte stores.  Only the tile's first and last
 * granule can be partial; those go out byte by byte, the neighbouring tile
 * owning the granule's other bytes.  No byte is stored twice.  win4: AP_WIN
 * bytes of LDS */
__device__ inline void ap_pack_tile(uint4 *win4, uint8_t *out, uint64_t tot, uint64_t o, const uint32_t (&len)[SD_PER],
                                    const uint64_t (&from)[SD_PER], const uint8_t *src)
{
    uint8_t *win = (uint8_t *)win4;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lo_all = (uint64_t)(uintptr_t)out & 15u, hi_all = lo_all + tot;
    out -= lo_all;                                        /* 16-byte aligned: position 0 */
    uint64_t at[SD_PER], run = lo_all + o;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        at[k] = run;
        run += len[k];
    }
    for (uint64_t ws = 0ull; ws < hi_all; ws += AP_WIN) {
#pragma unroll
        for (uint32_t k = 0; k < SD_PER; k++)
            if (len[k] && len[k] < AP_LONG) ap_stage_key(win, ws, at[k], len[k], src + from[k], 0u, 1u);
#pragma unroll
        for (uint32_t k = 0; k < SD_PER; k++) {
            uint64_t m = __ballot(len[k] >= AP_LONG && at[k] < ws + AP_WIN && at[k] + len[k] > ws);
            while (m) {                                   /* the same in every lane of the wave */
                const int l = __ffsll((unsigned long long)m) - 1;
                m &= m - 1ull;
                const uint64_t ks = sd_lane_u64(at[k], l), fr = sd_lane_u64(from[k], l);
                const uint32_t ln = (uint32_t)__shfl((int)len[k], l, 64);
                ap_stage_key(win, ws, ks, ln, src + fr, lane, 64u);
            }
        }
        __syncthreads();
        const uint64_t lo = ws > lo_all ? ws : lo_all, hi = ws + AP_WIN < hi_all ? ws + AP_WIN : hi_all;
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

/* request k's key bytes if it is accepted -- a SET that parsed, its key span
 * inside the request arena -- else 0 with *ok false */
__device__ inline uint32_t ap_accepted_len(const LzfAppendArgs &a, uint64_t k, bool *ok)
{
    *ok = false;
    if (k >= a.n || a.op[k] != (uint8_t)LZF_OP_SET || a.status[k] != (uint8_t)LZF_REQ_OK) return 0u;
    const uint64_t off = a.rq_key_off[k];
    const uint32_t len = a.rq_key_len[k];
    if (off > a.req_bytes || len > a.req_bytes - off) return 0u;
    *ok = true;
    return len;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_append_reduce_kernel(LzfAppendArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t s = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        bool ok;
        const uint32_t len = ap_accepted_len(a, first + j, &ok);
        if (ok) s += AP_ONE + len;
    }
    uint64_t tot;
    (void)dv_block_excl<SD_WAVES>(s, sw, &tot);
    if (threadIdx.x != 0u) return;
    a.w_tile_n[blockIdx.x] = tot >> 48;
    a.w_tile_b[blockIdx.x] = tot & AP_BYTES;
}

/* one workgroup, any number of tiles in pieces of SD_BLOCK: the exclusive scan
 * of the tiles' key bytes in place, the result and the whole-call decision */
__global__ __launch_bounds__(SD_BLOCK) void lzf_append_carry_kernel(LzfAppendArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    uint64_t rn = 0ull, rb = 0ull;
    for (uint32_t c = 0; c < ntile; c += SD_BLOCK) {
        const uint32_t i = c + threadIdx.x;
        const uint64_t xn = i < ntile ? a.w_tile_n[i] : 0ull, xb = i < ntile ? a.w_tile_b[i] : 0ull;
        uint64_t tn, tb;
        (void)dv_block_excl<SD_WAVES>(xn, sw, &tn);
        const uint64_t ob = dv_block_excl<SD_WAVES>(xb, sw, &tb);
        if (i < ntile) a.w_tile_b[i] = rb + ob;
        rn += tn;
        rb += tb;
    }
    if (threadIdx.x != 0u) return;
    const uint64_t base = *a.keys_used, end = base + rb;
    const bool full = end < base || end > a.keys_cap;
    a.w_state[AP_BASE] = base;
    a.w_state[AP_STATUS] = full ? LZF_STORE_FULL : LZF_STORE_OK;
    a.result[0] = full ? 0ull : rn;
    a.result[1] = (uint64_t)a.n - (full ? 0ull : rn);
    a.result[2] = full ? 0ull : rb;
    a.result[3] = full ? LZF_STORE_FULL : LZF_STORE_OK;
    if (!full) *a.keys_used = end;
}

/* the tile's items, set_len and void_idx, then its keys into its range of the
 * key arena.  On FULL every request is refused and no key byte is written */
__global__ __launch_bounds__(SD_BLOCK) void lzf_append_write_kernel(LzfAppendArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    __shared__ uint4 win4[AP_WIN / 16u];
    const bool full = a.w_state[AP_STATUS] != 0ull;
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint32_t len[SD_PER];
    uint64_t from[SD_PER], s = 0ull;
    bool ok[SD_PER];
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        len[j] = ap_accepted_len(a, first + j, &ok[j]);
        if (full) {
            ok[j] = false;
            len[j] = 0u;
        }
        from[j] = len[j] ? a.rq_key_off[first + j] : 0ull;
        s += len[j];
    }
    uint64_t tot;
    const uint64_t o = dv_block_excl<SD_WAVES>(s, sw, &tot);
    const uint64_t tile = a.w_state[AP_BASE] + (full ? 0ull : a.w_tile_b[blockIdx.x]);
    uint64_t off = tile + o;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        const uint64_t k = first + j;
        if (k >= a.n) break;
        const uint64_t i = (uint64_t)a.first + k;
        a.key_off[i] = off;
        a.key_len[i] = len[j];
        if (a.item_time) {
            const int64_t ttl = ok[j] ? a.num[k] : 0;
            a.item_time[i] = a.now;
            a.item_ttl[i] = ttl > 0 ? (int32_t)(ttl < (int64_t)a.max_item_ttl ? ttl : (int64_t)a.max_item_ttl) : -1;
        }
        if (a.item_lock) a.item_lock[i] = 0;
        if (a.last_access) a.last_access[i] = a.now;
        a.set_len[k] = ok[j] ? a.rq_val_len[k] : 0u;
        a.void_idx[k] = ok[j] ? AP_VOID : (uint32_t)i;
        off += len[j];
    }
    if (!tot) return;                                     /* the whole workgroup */
    ap_pack_tile(win4, a.keys + tile, tot, o, len, from, a.req);
}

}  // namespace

hipError_t lzf_launch_request_parse(const LzfRequestArgs &a, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(a.result, 0, LZF_REQ_NSTATUS * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_request_parse_kernel, dim3(sd_sweep_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t lzf_launch_store_append_keys(LzfAppendArgs &a, hipStream_t s)
{
    const uint32_t nt = sd_tiles(a.n);
    hipLaunchKernelGGL(lzf_append_reduce_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_append_carry_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_append_write_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}
