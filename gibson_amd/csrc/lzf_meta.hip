/*
 * lzf_meta.hip -- the last three item operators of the reference's table over
 * the device store (include/lzf_gpu.h): the memory sweep, META and the KEYS
 * reply frame.
 *
 * gc: gbMemoryFreeHandler (src/server.c:311-327) over every item, one
 * grid-stride pass; the cron's gate memused > maxmem (:403) is read from
 * device memory by every workgroup, so a closed gate costs one launch and no
 * host read.
 *
 * meta: gbQueryMetaHandler (src/query.c:1302-1339) over an index list, one
 * grid-stride pass, one lane per entry, as mlock / mttl are; the field name is
 * resolved on the host (lzf_meta_field: gbGetItemMeta's strncmp chain,
 * :1263-1297).
 *
 * keys: gbQueryKeysHandler (:1341-1391) after tr_search.  The j-th
 * participating entry of the list becomes the pair ["j" in decimal -> the
 * item's key as a PLAIN item] of a KVAL frame, byte for byte what
 * lzf_gpu_kv_frame writes for those pairs.  A pair takes 9 + digits(j) +
 * key_len bytes, and the digits of all the ranks below r add up to a closed
 * form D(r), so a pair's place follows from two sums over the entries before
 * it: how many take part, and their key bytes.  Three launches, no workgroup
 * waiting for another:
 *   1. reduce: per tile of the list its participating entries and their key
 *      bytes;
 *   2. scan: one workgroup's running scan of both; found, the payload size,
 *      the status, result[], frame_len, and on LZF_MGET_OK the reply header
 *      and the element count;
 *   3. write (nothing unless LZF_MGET_OK): one lane per entry, its rank and
 *      offset from the tile's sums and a scan over the workgroup, then the
 *      pair.
 * Thread t of a tile takes entries t * SD_PER .. + SD_PER, so the scan over
 * the threads is the scan over the list and the ranks are in list order.
 *
 * Counts by wave ballot, one atomic add per wave and counter.  The kernels are
 * helpers of this translation unit, not part of the library's routed kernel
 * set: they have internal linkage (anonymous namespace).
 */
#include <string.h>

#include "lzf_store_dev.h"
#include "../../include/lzf_gpu.h"

namespace {

/* state words of the keys work area */
enum { MT_FOUND = 0, MT_PAYLOAD = 1, MT_STATUS = 2 };

/* ---- gc ------------------------------------------------------------------------ */

/* src/server.c:318-326: eta = now - last_access (mg_age); freed iff eta &&
 * eta >= gc_ratio.
 * Locks and TTLs are not consulted, as there.  result[0]: items freed, [1]:
 * their stored bytes, [2]: 1, the sweep ran */
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_gc_kernel(LzfItems it, int64_t gc_ratio,
                                                                const uint32_t *__restrict__ val_size,
                                                                const uint64_t *gate, uint64_t max_bytes,
                                                                uint64_t *result)
{
    const int64_t *__restrict__ last_access = it.last_access;
    if (gate && *gate <= max_bytes) return;               /* src/server.c:403; the same for every lane */
    if (blockIdx.x == 0u && threadIdx.x == 0u) result[2] = 1ull;
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t freed = 0u;
    uint64_t bytes = 0ull;
    for (uint64_t b = (uint64_t)blockIdx.x * SD_BLOCK; b < it.count; b += step) {
        const uint64_t i = b + threadIdx.x;
        bool hit = false;
        if (i < it.count && it.enc[i] != (uint8_t)LZF_ENC_NULL) {
            const int64_t eta = mg_age(it.now, last_access[i]);
            hit = eta != 0 && eta >= gc_ratio;
            if (hit) {
                it.enc[i] = (uint8_t)LZF_ENC_NULL;        /* GB_DEL_ITEM */
                bytes += val_size[i];
            }
        }
        freed += sd_count(hit);
    }
    sd_leader_add(result, freed);
    sd_leader_add(result + 1, sd_wave_sum(bytes));
}

/* ---- meta ---------------------------------------------------------------------- */

/* gbQueryMetaHandler (src/query.c:1317-1335) over the list: the validity with
 * remove = 1, no lock test; the value, then last_access = now (:1330), so
 * ACCESS reports the time before this call.  result[0]: found, [1]: expired */
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_meta_kernel(LzfMetaArgs a)
{
    const LzfItems &it = a.it;
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t found = 0u, expired = 0u;
    for (uint64_t b = (uint64_t)blockIdx.x * SD_BLOCK; b < a.n; b += step) {
        const uint64_t k = b + threadIdx.x;
        uint32_t st = SD_NONE;
        if (k < a.n) {
            const uint32_t i = a.idx[k];
            const int v = mg_validity(i, it);
            int64_t val = 0;
            if (v == MG_DEAD) {
                st = LZF_ENT_DEAD;
            } else if (v == MG_EXPIRED) {
                st = LZF_ENT_EXPIRED;
                it.enc[i] = (uint8_t)LZF_ENC_NULL;
            } else {
                st = LZF_ENT_DONE;
                const int32_t ttl = it.item_ttl[i];
                switch (a.field) {                        /* gbGetItemMeta, :1263-1297 */
                case LZF_META_SIZE: val = (int64_t)a.val_size[i]; break;
                case LZF_META_ENCODING: val = (int64_t)it.enc[i]; break;
                case LZF_META_ACCESS: val = it.last_access[i]; break;
                case LZF_META_CREATED: val = it.item_time[i]; break;
                case LZF_META_TTL: val = (int64_t)ttl; break;
                case LZF_META_LEFT:                       /* :1290, the time arithmetic modulo 2^64 */
                    val = ttl <= 0 ? -1 : (int64_t)((uint64_t)(int64_t)ttl - (uint64_t)mg_age(it.now, it.item_time[i]));
                    break;
                default: val = it.item_lock ? it.item_lock[i] : 0; break;
                }
                if (it.last_access) it.last_access[i] = it.now;
            }
            a.entry_value[k] = val;
            if (a.entry_status) a.entry_status[k] = (uint8_t)st;
        }
        found += sd_count(st == LZF_ENT_DONE);
        expired += sd_count(st == LZF_ENT_EXPIRED);
    }
    sd_leader_add(a.result, found);
    sd_leader_add(a.result + 1, expired);
}

/* ---- keys ---------------------------------------------------------------------- */

/* whether entry i takes part: in range, not nulled, a key of at least one
 * byte.  The reference makes no validity test here (src/query.c:1353-1368) */
__device__ inline bool mt_takes_part(const LzfKeysArgs &a, uint32_t i)
{
    return i < a.count && a.enc[i] != (uint8_t)LZF_ENC_NULL && a.key_len[i] != 0u;
}

__device__ inline uint32_t mt_digits(uint64_t j)          /* of "%lu" */
{
    uint32_t d = 1u;
    for (uint64_t p = 10ull; j >= p && d < 20u; p *= 10ull) d++;
    return d;
}

/* D(r): the digits of all the ranks 0 .. r - 1 together, r <= 2^32 */
__device__ inline uint64_t mt_digits_below(uint64_t r)
{
    uint64_t sum = 0ull, lo = 0ull, hi = 10ull;
    for (uint32_t d = 1u; d <= 10u && lo < r; d++) {
        sum += ((r < hi ? r : hi) - lo) * d;
        lo = hi;
        hi *= 10ull;
    }
    return sum;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_keys_reduce_kernel(LzfKeysArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t cnt = 0ull, bytes = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        if (first + j >= a.n) continue;
        const uint32_t i = a.idx[first + j];
        if (!mt_takes_part(a, i)) continue;
        cnt++;
        bytes += a.key_len[i];
    }
    uint64_t tn, tb;
    (void)dv_block_excl<SD_WAVES>(cnt, sw, &tn);
    (void)dv_block_excl<SD_WAVES>(bytes, sw, &tb);
    if (threadIdx.x == 0u) {
        a.w_tile_n[blockIdx.x] = tn;
        a.w_tile_b[blockIdx.x] = tb;
    }
}

/* one workgroup: the exclusive scans of the tile sums in place, and the call's
 * decision */
__global__ __launch_bounds__(SD_BLOCK) void lzf_keys_scan_kernel(LzfKeysArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t run_n = dv_carry_scan<SD_WAVES>(a.w_tile_n, ntile, sw);
    const uint64_t run_b = dv_carry_scan<SD_WAVES>(a.w_tile_b, ntile, sw);
    if (threadIdx.x != 0u) return;
    /* u32 element count, then per pair [u32][digits][u8][u32][key]: below 2^65
     * only in theory -- found < 2^32 and the key bytes < 2^64 / 2 in any store */
    const uint64_t payload = 4ull + 9ull * run_n + mt_digits_below(run_n) + run_b;
    uint64_t st = LZF_MGET_OK;
    if (!run_n) st = LZF_MGET_NOT_FOUND;                  /* src/query.c:1387 */
    else if (payload > a.max_response) st = LZF_MGET_TOO_BIG;   /* CHECK_SPACE, src/net.c:1272-1277 */
    a.w_state[MT_FOUND] = run_n;
    a.w_state[MT_PAYLOAD] = payload;
    a.w_state[MT_STATUS] = st;
    a.result[0] = run_n;
    a.result[1] = st;
    const uint64_t hdr = a.reply_header ? SD_HDR : 0u;
    *a.frame_len = st == (uint64_t)LZF_MGET_OK ? payload + hdr : 0ull;
    if (st != (uint64_t)LZF_MGET_OK) return;
    uint8_t *f = a.frame;
    if (a.reply_header) sd_put_header(f, LZF_REPL_KVAL, (uint8_t)LZF_ENC_PLAIN, (uint32_t)payload);   /* src/net.c:1339 */
    sd_put32(f + hdr, (uint32_t)run_n);                                       /* src/net.c:1282 */
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_keys_write_kernel(LzfKeysArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    if (a.w_state[MT_STATUS] != (uint64_t)LZF_MGET_OK) return;   /* the same for every lane */
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint32_t item[SD_PER], kl[SD_PER];
    uint64_t cnt = 0ull, bytes = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        kl[j] = 0u;                                       /* 0: the entry does not take part */
        item[j] = 0u;
        if (first + j >= a.n) continue;
        const uint32_t i = a.idx[first + j];
        if (!mt_takes_part(a, i)) continue;
        item[j] = i;
        kl[j] = a.key_len[i];
        cnt++;
        bytes += kl[j];
    }
    uint64_t tn, tb;
    uint64_t rank = a.w_tile_n[blockIdx.x] + dv_block_excl<SD_WAVES>(cnt, sw, &tn);
    uint64_t kb = a.w_tile_b[blockIdx.x] + dv_block_excl<SD_WAVES>(bytes, sw, &tb);
    if (!cnt) return;
    /* every byte written lies below hdr + payload <= hdr + max_response */
    uint8_t *f = a.frame + (a.reply_header ? SD_HDR : 0u) + 4u + 9ull * rank + mt_digits_below(rank) + kb;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        if (!kl[j]) continue;
        const uint32_t nd = mt_digits(rank);
        sd_put32(f, nd);                                  /* the KVAL key: sprintf "%lu" of the rank (:1364) */
        uint64_t r = rank;
        for (uint32_t d = nd; d-- > 0u; r /= 10ull) f[4u + d] = (uint8_t)('0' + (uint32_t)(r % 10ull));
        f += 4u + nd;
        f[0] = (uint8_t)LZF_ENC_PLAIN;                    /* gbCreateVolatileItem(..., GB_ENC_PLAIN), :1367 */
        sd_put32(f + 1, kl[j]);
        const uint8_t *key = a.keys + a.key_off[item[j]];
        for (uint32_t c = 0; c < kl[j]; c++) f[5u + c] = key[c];
        f += 5ull + kl[j];
        rank++;
    }
}

}  // namespace

/* gbGetItemMeta's chain (src/query.c:1263-1297): strncmp over min(mlen,
 * strlen(name)) bytes, in the reference's order.  strncmp ends early only at
 * a NUL in both strings; a name has none within the compared bytes, so a NUL
 * in m there is a difference and memcmp over the same bytes decides alike */
int lzf_meta_field(const uint8_t *m, uint32_t mlen)
{
    static const char *const names[7] = {"size", "encoding", "access", "created", "ttl", "left", "lock"};
    if (!m || !mlen) return -1;
    for (int f = 0; f < 7; f++) {
        const size_t len = strlen(names[f]);
        if (memcmp(m, names[f], mlen < len ? mlen : len) == 0) return f;
    }
    return -1;
}

hipError_t lzf_launch_store_gc(const LzfItems &it, int64_t gc_ratio, const uint32_t *val_size, const uint64_t *gate,
                               uint64_t max_bytes, uint64_t *result, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(result, 0, 3 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_store_gc_kernel, dim3(sd_sweep_grid(it.count)), dim3(SD_BLOCK), 0, s, it, gc_ratio, val_size,
                       gate, max_bytes, result);
    return hipGetLastError();
}

hipError_t lzf_launch_store_meta(const LzfMetaArgs &a, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(a.result, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_store_meta_kernel, dim3(sd_sweep_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t lzf_launch_store_keys(LzfKeysArgs &a, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(a.result, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const uint32_t nt = sd_tiles(a.n);
    hipLaunchKernelGGL(lzf_keys_reduce_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_keys_scan_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_keys_write_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}
