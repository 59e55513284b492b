/*
 * lzf_mset.hip -- MSET by prefix over the device store (lzf_gpu_store_mset,
 * include/lzf_gpu.h): gbQueryMultiSetHandler / gbMultiSetCallback
 * (src/query.c:479-537) applied to an index list.  One new value replaces the
 * value of every entry that is valid and not locked; the item keeps its index
 * and its key, so the key index is not touched.
 *
 * The reference runs gbSingleSet (:375-425) once per matched key and so
 * compresses the same bytes once per key.  Here the stored form is decided
 * once, by the rule of the device SET path (lzf_store.hip): the value is a
 * candidate iff vlen > compression, its cap is gb_needcompr(vlen), and the
 * routed compress -- handed in as a function pointer, as lzf_launch_store
 * takes it -- runs over that one value into a slot of the work area.  With a
 * stream the stored form is the stream (LZF), without one the input bytes
 * (PLAIN).  S, its length, is known on the device only, and the call is
 * refused as a whole when done * S bytes do not fit, so nothing is written
 * before that is known (the shape of minc, lzf_ops.hip).  On one stream:
 *   1. classify (read-only on the store): per entry its LZF_ENT_* class into
 *      the work area, per tile of the list its DONE entries; its first thread
 *      writes the one-value compress batch's descriptors;
 *   2. the routed compress over that batch (vlen > compression only);
 *   3. scan: one workgroup's running scan of the tile counts; S and the stored
 *      encoding from the compress's out_len; base = *store_used, the status,
 *      and on LZF_STORE_OK the new *store_used and result[3], [4];
 *   4. apply (nothing on LZF_STORE_FULL): one lane per entry, its rank among
 *      the DONE ones from the classes alone, then the item's descriptors --
 *      val_off = base + S * rank and the rest of what gbCreateItem sets
 *      (:113-146) -- enc nulled for an expired entry, entry_status, the counts;
 *   5. replicate (nothing on FULL): the done * S stored bytes.
 *
 * The replicate kernel.  The copies abut, so their destination is the one
 * range [base, base + S * done) of the arena in which byte b is src[b mod S],
 * src being the stored form (the compress slot, or the caller's value).  It is
 * written by destination: the range is cut into 16-byte granules at 16-aligned
 * absolute addresses, a lane assembles a granule from src at (b mod S) -- one
 * unaligned 16-byte load, or two joined in registers where the granule
 * straddles the wrap at S; byte by byte for S < 16, where it wraps more than
 * once -- and stores it with one aligned 16-byte store.  The first and the
 * last granule of the range may be partial and are stored byte-exactly
 * (dv_st_exact).  The grid is sized by bytes, from the host's bound vlen * n,
 * one granule per lane up to SD_GRID workgroups and grid-stride past that,
 * four granules in flight per lane; workgroups past the real range (S < vlen,
 * done < n) leave at once.  b mod S is one 64-bit division per lane, then an
 * add and a compare per granule.  src is at most 64 MiB read by every
 * workgroup in the same order, so it is served by the caches, not by HBM.
 *
 * The kernels are helpers of this translation unit, not part of the library's
 * routed kernel set: they have internal linkage (anonymous namespace).
 */
#include "lzf_store_dev.h"
#include "gb_policy.h"
#include "../../include/lzf_gpu.h"

/* the replicate kernel's own: granules in flight per lane.  The rest of the
 * geometry is the toolkit's (lzf_store_dev.h) */
#define MS_UNROLL 4u

namespace {

/* state words of the work area */
enum { MS_BASE = 0, MS_FULL = 1, MS_SIZE = 2, MS_ENC = 3, MS_DONE = 4 };

__global__ __launch_bounds__(SD_BLOCK) void lzf_mset_classify_kernel(LzfMsetArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        /* the batch of one value: a candidate iff vlen > compression
         * (src/query.c:389, strict), else length 0, which yields out_len 0 */
        a.c_off[0] = 0ull;                                /* in_off */
        a.c_off[1] = 0ull;                                /* out_off */
        a.c_len[0] = a.vlen > a.compression ? a.vlen : 0u;
        a.c_len[1] = gb_needcompr(a.vlen);                /* out_cap */
        a.c_len[2] = 0u;                                  /* out_len */
    }
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t done = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        const uint64_t k = first + j;
        if (k >= a.n) continue;
        /* gbMultiSetCallback (src/query.c:490-502): dead, then the lock -- on an
         * expired item too (:493 comes before :496) -- then the validity */
        const uint32_t cls = sd_entry_class(a.idx[k], a.it, false);
        a.w_cls[k] = (uint8_t)cls;
        done += cls == LZF_ENT_DONE;
    }
    uint64_t tot;
    (void)dv_block_excl<SD_WAVES>(done, sw, &tot);
    if (threadIdx.x == 0u) a.w_tile[blockIdx.x] = tot;
}

/* one workgroup: the exclusive scan of the tile counts in place, the stored
 * form, and the call's decision */
__global__ __launch_bounds__(SD_BLOCK) void lzf_mset_scan_kernel(LzfMsetArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t run = dv_carry_scan<SD_WAVES>(a.w_tile, ntile, sw);
    if (threadIdx.x != 0u) return;
    /* a stream or the plain bytes, as the store decision of lzf_store.hip */
    const uint32_t got = a.c_len[2];
    const uint64_t size = got ? got : a.vlen;
    const uint64_t enc = got ? LZF_ENC_LZF : LZF_ENC_PLAIN;
    /* run <= n < 2^32 and size < 2^27: the product cannot wrap, the sum can */
    const uint64_t base = *a.store_used, end = base + size * run;
    const bool full = end < base || end > a.store_cap;
    a.w_state[MS_BASE] = base;
    a.w_state[MS_FULL] = full ? 1ull : 0ull;
    a.w_state[MS_SIZE] = size;
    a.w_state[MS_ENC] = enc;
    a.w_state[MS_DONE] = full ? 0ull : run;
    *a.status = full ? LZF_STORE_FULL : LZF_STORE_OK;
    if (full) return;
    *a.store_used = end;
    a.result[3] = size;
    a.result[4] = enc;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_mset_apply_kernel(LzfMsetArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    if (a.w_state[MS_FULL]) return;                       /* refused: the same for every lane */
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint32_t cls[SD_PER];
    uint64_t mine = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        cls[j] = first + j < a.n ? a.w_cls[first + j] : SD_NONE;
        mine += cls[j] == LZF_ENT_DONE;
    }
    uint64_t tot;
    uint64_t rank = a.w_tile[blockIdx.x] + dv_block_excl<SD_WAVES>(mine, sw, &tot);
    const uint64_t base = a.w_state[MS_BASE], size = a.w_state[MS_SIZE];
    const uint8_t enc = (uint8_t)a.w_state[MS_ENC];
    uint32_t done = 0u, expired = 0u, locked = 0u;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        const uint64_t k = first + j;
        const uint32_t c = cls[j];
        if (c != SD_NONE) {
            const uint32_t i = a.idx[k];
            if (c == LZF_ENT_EXPIRED) {
                a.it.enc[i] = (uint8_t)LZF_ENC_NULL;
            } else if (c == LZF_ENT_DONE) {
                /* gbCreateItem (src/query.c:113-146) with ttl -1 (:417) */
                a.val_off[i] = base + size * rank++;      /* its end <= store_cap: the scan's decision */
                a.val_size[i] = (uint32_t)size;
                a.it.enc[i] = enc;
                a.val_len[i] = a.vlen;
                a.it.item_time[i] = a.it.now;
                a.it.item_ttl[i] = -1;
                if (a.it.item_lock) a.it.item_lock[i] = 0;
                if (a.it.last_access) a.it.last_access[i] = a.it.now;
            }
            if (a.entry_status) a.entry_status[k] = (uint8_t)c;
        }
        done += sd_count(c == LZF_ENT_DONE);
        expired += sd_count(c == LZF_ENT_EXPIRED);
        locked += sd_count(c == LZF_ENT_LOCKED);
    }
    sd_leader_add(a.result, done);
    sd_leader_add(a.result + 1, expired);
    sd_leader_add(a.result + 2, locked);
}

/* v shifted up by sh (0 .. 15) bytes, zeros in */
__device__ inline uint4 ms_shl16(uint4 v, uint32_t sh)
{
    uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
    const bool big = sh >= 8u;
    hi = big ? lo : hi;
    lo = big ? 0ull : lo;
    const uint32_t b = 8u * (sh & 7u);
    hi = b ? (hi << b) | (lo >> (64u - b)) : hi;
    lo <<= b;
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

/* the 16 bytes src[(m + k) mod S], k = 0 .. 15, for m < S.  No load leaves
 * [src, src + S).  pat: for S < 16 the S bytes of src, zero beyond */
__device__ inline uint4 ms_cyclic16(const uint8_t *__restrict__ src, uint32_t S, uint32_t m, uint4 pat)
{
    if (S >= 16u) {
        if (m + 16u <= S) return dv_ld16(src + m);
        /* straddles the wrap once: src[m, S) below, src[0, 16 - (S - m)) above */
        const uint32_t low = S - m;                       /* 1 .. 15 */
        const uint4 a = dv_shr16(dv_ld16(src + S - 16u), 16u - low);
        const uint4 b = ms_shl16(dv_ld16(src), low);
        return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w);
    }
    /* wraps more than once: correct, not fast */
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    uint32_t p = m;
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) {
        const uint32_t byte = (dv_sel4(pat, p >> 2) >> (8u * (p & 3u))) & 0xFFu;
        w[k >> 2] |= byte << (8u * (k & 3u));
        p = p + 1u == S ? 0u : p + 1u;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_mset_replicate_kernel(LzfMsetArgs a)
{
    if (a.w_state[MS_FULL]) return;
    const uint32_t S = (uint32_t)a.w_state[MS_SIZE];
    const uint64_t total = (uint64_t)S * a.w_state[MS_DONE];
    if (!total) return;
    const uint8_t *__restrict__ src = a.w_state[MS_ENC] == (uint64_t)LZF_ENC_LZF ? a.w_slot : a.value;
    /* absolute addresses: the range [d0, d1), granules from a0 (which may lie
     * up to 15 bytes before d0: nothing is accessed there) */
    const uint64_t sa = (uint64_t)(uintptr_t)a.store, d0 = sa + a.w_state[MS_BASE], d1 = d0 + total;
    const uint64_t a0 = d0 & ~15ull;
    const uint32_t head = (uint32_t)(d0 - a0);
    const uint64_t ngran = (d1 - a0 + 15u) / 16u;
    const uint64_t stride = (uint64_t)gridDim.x * SD_BLOCK;
    uint64_t j = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x;
    if (j >= ngran) return;
    const uint4 pat = S < 16u ? dv_ld16_tail(src, S) : make_uint4(0u, 0u, 0u, 0u);
    uint8_t *__restrict__ const store = a.store;
    if (j == 0u && head) {
        /* the range's first granule, partial: bytes [d0, min(a0 + 16, d1)) = src from 0 */
        const uint64_t q1 = a0 + 16u < d1 ? a0 + 16u : d1;
        dv_st_exact(store + (d0 - sa), ms_cyclic16(src, S, 0u, pat), (uint32_t)(q1 - d0));
        j += stride;
        if (j >= ngran) return;
    }
    /* granule j holds range bytes from 16 j - head on */
    uint32_t m = (uint32_t)((16ull * j - head) % S);
    const uint32_t step = (uint32_t)((16ull * stride) % S);
    while (j < ngran) {
        uint4 v[MS_UNROLL];
        uint32_t len[MS_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < MS_UNROLL; u++) {
            const uint64_t g = a0 + 16ull * (j + u * stride);
            len[u] = 0u;
            if (j + u * stride >= ngran) continue;
            len[u] = g + 16u <= d1 ? 16u : (uint32_t)(d1 - g);     /* the last granule may be partial */
            v[u] = ms_cyclic16(src, S, m, pat);
            m += step;                                    /* both below S <= 2^27: no wrap */
            m = m >= S ? m - S : m;
        }
#pragma unroll
        for (uint32_t u = 0; u < MS_UNROLL; u++) {
            uint8_t *p = store + (a0 + 16ull * (j + u * stride) - sa);
            if (len[u] == 16u) *(uint4 *)p = v[u];
            else if (len[u]) dv_st_exact(p, v[u], len[u]);
        }
        j += (uint64_t)MS_UNROLL * stride;
    }
}

}  // namespace

hipError_t lzf_launch_store_mset(LzfMsetArgs &a, hipStream_t s, hipError_t (*compress)(const LzfBatch &, hipStream_t))
{
    hipError_t e = hipMemsetAsync(a.result, 0, 5 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const uint32_t nt = sd_tiles(a.n);
    hipLaunchKernelGGL(lzf_mset_classify_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.vlen > a.compression) {
        LzfBatch b{a.value, a.c_off, a.c_len, a.w_slot, a.c_off + 1, a.c_len + 1, a.c_len + 2, nullptr, 1u, a.vlen};
        if ((e = compress(b, s)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lzf_mset_scan_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_mset_apply_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    /* the host's bound on the range: n copies of vlen bytes, and a partial granule at either end */
    const uint64_t gran = ((uint64_t)a.vlen * a.n + 15u) / 16u + 1u;
    const uint64_t wg = (gran + SD_BLOCK - 1u) / SD_BLOCK;
    hipLaunchKernelGGL(lzf_mset_replicate_kernel, dim3((uint32_t)(wg < SD_GRID ? wg : SD_GRID)), dim3(SD_BLOCK), 0, s,
                       a);
    return hipGetLastError();
}
