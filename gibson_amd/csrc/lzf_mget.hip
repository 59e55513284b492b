/*
 * lzf_mget.hip -- the operator layer over the device store: a prefix select
 * that yields an index list in HBM, and the index-list operators that need no
 * value arithmetic: MGET, COUNT and MTTL (include/lzf_gpu.h).  INC / DEC and
 * the lock operators are in lzf_ops.hip.
 *
 * Every multi-key operator of the reference is tr_search over a prefix plus a
 * callback per item found (src/query.c:526, 620, 687, 1171).  The callbacks of
 * MGET, COUNT and MTTL apply the TTL rule lazily: an expired item is removed
 * on the spot (gbIsItemStillValid(..., remove = 1), src/query.c:204-224) and a
 * valid one gets last_access_time = now.  Here an operator takes an index
 * list idx[n] (entries >= count are ignored, so 0xFFFFFFFF pads a list made
 * on the device) and applies mg_validity, the one rule all of them share.
 *
 * select: one streaming pass over the descriptors and the key bytes, and a
 * stable compaction in three launches, no workgroup waiting for another:
 *   1. match: per item whether it is live and its key starts with the prefix
 *      (dword compares; the key's address may have any alignment); the wave's
 *      ballot is kept as one 64-bit word per 64 items, and the tile's count;
 *   2. carry: one workgroup's running scan of the tile counts, and result[];
 *   3. write: from the ballot words alone -- the keys are not read again --
 *      every match's rank, sel[rank] = index for rank < cap, and the padding
 *      of sel[min(matches, cap) .. cap).
 *
 * mget: what gbQueryMultiGetHandler does after tr_search (src/query.c:688-
 * 706), then the payload of gbClientEnqueueKeyValueSet as lzf_frame.hip
 * builds it, over the valid entries in list order:
 *   1. gather (fused): the validity rule, last_access, the entry's six
 *      descriptors copied into the work area (a dropped entry: encoding NULL),
 *      its frame bytes and the tile-local exclusive scan of them;
 *   2. scan: one workgroup over the tile sums; found / expired / skipped, the
 *      payload size and the status (NOT_FOUND, CHECK_SPACE);
 *   3. write: one wave per entry: an expired entry is nulled in enc (here and
 *      not in step 1, so that every copy of a duplicated entry is judged on
 *      what enc held before the call), headers, key, a PLAIN / NUMBER value;
 *      an LZF entry is described to the decoder.  The element count in the
 *      frame is `found`, read on the device;
 *   4. the routed decoder over the gathered arrays, in place in the frame;
 *   5. check, by the whole grid: every LZF entry decoded to its val_len;
 *      finish: frame_len and the status.
 *
 * count / mttl: one grid-stride pass over the list; the counts by wave
 * ballot, one atomic add per wave.
 *
 * The kernels are helpers of this translation unit, not part of the library's
 * routed kernel set: they have internal linkage (anonymous namespace).
 */
#include "lzf_store_dev.h"
#include "../../include/lzf_gpu.h"

namespace {

/* state words of the mget work area */
enum { MG_PAYLOAD = 0, MG_STATUS = 1, MG_FOUND = 2, MG_BAD = 3 };

/* the geometry, the scans, the byte helpers and mg_validity, the validity rule
 * of every index-list operator: lzf_store_dev.h */

/* ---- select ----------------------------------------------------------------- */

/* mg_prefix_match, the prefix test of both selects: lzf_store_dev.h */

/* item i of a tile sits in round k = (i % SD_TILE) / SD_BLOCK at thread
 * i % SD_BLOCK, so a wave reads 64 neighbouring descriptors and its ballot
 * word is number (i % SD_TILE) / 64 of the tile's SD_WORDS, in index order */
__global__ __launch_bounds__(SD_BLOCK) void lzf_select_match_kernel(LzfSelectArgs a)
{
    __shared__ uint32_t sc[SD_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE;
    uint32_t hits = 0u;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t i = first + k * SD_BLOCK + threadIdx.x;
        bool m = false;
        if (i < a.count && a.enc[i] != (uint8_t)LZF_ENC_NULL && a.key_len[i] >= a.prefix_len)
            m = mg_prefix_match(a.keys + a.key_off[i], a.prefix, a.prefix_len);
        const uint64_t word = __ballot(m);
        if (lane == 0u) a.w_mask[(uint64_t)blockIdx.x * SD_WORDS + k * SD_WAVES + wave] = word;
        hits += (uint32_t)__popcll(word);
    }
    if (lane == 0u) sc[wave] = hits;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t n = 0u;
        for (uint32_t w = 0; w < SD_WAVES; w++) n += sc[w];
        a.w_tile[blockIdx.x] = n;
    }
}

/* one workgroup: the exclusive scan of the tile counts in place (dv_carry_scan,
 * 8 tiles per thread), and result[] */
__global__ __launch_bounds__(SD_BLOCK) void lzf_select_carry_kernel(LzfSelectArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t run = dv_carry_scan<SD_WAVES>(a.w_tile, ntile, sw);
    if (threadIdx.x != 0u) return;
    a.result[0] = (uint32_t)(run < a.cap ? run : a.cap);
    a.result[1] = (uint32_t)run;                          /* at most count */
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_select_write_kernel(LzfSelectArgs a)
{
    __shared__ uint32_t pre[SD_WORDS + 1u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t *mask = a.w_mask + (uint64_t)blockIdx.x * SD_WORDS;
    if (threadIdx.x == 0u) {
        uint32_t s = 0u;
        for (uint32_t w = 0; w < SD_WORDS; w++) {
            pre[w] = s;
            s += (uint32_t)__popcll(mask[w]);
        }
    }
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE, base = a.w_tile[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint32_t w = k * SD_WAVES + wave;
        const uint64_t word = mask[w];
        if (!((word >> lane) & 1ull)) continue;
        const uint64_t r = base + pre[w] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
        if (r < a.cap) a.sel[r] = (uint32_t)(first + k * SD_BLOCK + threadIdx.x);
    }
    /* the padding, by all the workgroups together */
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    for (uint64_t r = (uint64_t)a.result[0] + (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; r < a.cap; r += step)
        a.sel[r] = SD_PAD;
}

/* ---- mget ------------------------------------------------------------------- */

/* a tile's three counts in one word for the scan inside the tile: each is at
 * most SD_TILE = 2^10 */
#define MG_ONE_FOUND   1ull
#define MG_ONE_EXPIRED (1ull << 21)
#define MG_ONE_SKIPPED (1ull << 42)
#define MG_CNT_MASK    ((1ull << 21) - 1ull)

/* thread t of a tile takes entries t * SD_PER .. + SD_PER, so the scan over the
 * threads is the scan over the list */
__global__ __launch_bounds__(SD_BLOCK) void lzf_mget_gather_kernel(LzfMgetArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t sz[SD_PER], s = 0ull, cnt = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        const uint64_t k = first + j;
        sz[j] = 0ull;
        if (k >= a.n) continue;
        const uint32_t i = a.idx[k];
        const int v = mg_validity(i, a.it);
        uint8_t e = (uint8_t)LZF_ENC_NULL;
        uint64_t ko = 0ull, vo = 0ull;
        uint32_t kl = 0u, vs = 0u, vl = 0u;
        if (v == MG_VALID) {
            e = a.it.enc[i];
            ko = a.key_off[i];
            kl = a.key_len[i];
            vo = a.val_off[i];
            vs = a.val_size[i];
            vl = e == (uint8_t)LZF_ENC_LZF ? a.val_len[i] : vs;
            sz[j] = 4ull + kl + 1ull + 4ull + vl;         /* src/net.c:1294-1333 */
            if (a.it.last_access) a.it.last_access[i] = a.it.now;   /* src/query.c:693 */
            cnt += MG_ONE_FOUND;
        } else {
            cnt += v == MG_EXPIRED ? MG_ONE_EXPIRED : MG_ONE_SKIPPED;
        }
        a.g_key_off[k] = ko;
        a.g_key_len[k] = kl;
        a.g_val_off[k] = vo;
        a.g_val_size[k] = vs;
        a.g_val_len[k] = vl;
        a.g_enc[k] = e;
        a.g_null[k] = v == MG_EXPIRED ? i : SD_PAD;
        s += sz[j];
    }
    uint64_t tot, ctot;
    uint64_t o = dv_block_excl<SD_WAVES>(s, sw, &tot);
    (void)dv_block_excl<SD_WAVES>(cnt, sw, &ctot);
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        if (first + j < a.n) a.w_off[first + j] = o;
        o += sz[j];
    }
    if (threadIdx.x == 0u) {
        a.w_tile[blockIdx.x] = tot;
        a.w_tcnt[blockIdx.x] = ctot;
    }
}

/* one workgroup: the exclusive scan of the tiles' frame bytes in place, the
 * three counts, and the call's decision */
__global__ __launch_bounds__(SD_BLOCK) void lzf_mget_scan_kernel(LzfMgetArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    uint64_t run = 0ull, found = 0ull, expired = 0ull, skipped = 0ull;
    for (uint32_t c = 0; c < ntile; c += SD_BLOCK) {
        const uint32_t i = c + threadIdx.x;
        const uint64_t x = i < ntile ? a.w_tile[i] : 0ull, cn = i < ntile ? a.w_tcnt[i] : 0ull;
        uint64_t tot, tf, te, ts;
        const uint64_t o = dv_block_excl<SD_WAVES>(x, sw, &tot);
        (void)dv_block_excl<SD_WAVES>(cn & MG_CNT_MASK, sw, &tf);
        (void)dv_block_excl<SD_WAVES>((cn >> 21) & MG_CNT_MASK, sw, &te);
        (void)dv_block_excl<SD_WAVES>((cn >> 42) & MG_CNT_MASK, sw, &ts);
        if (i < ntile) a.w_tile[i] = run + o;
        run += tot;
        found += tf;
        expired += te;
        skipped += ts;
    }
    if (threadIdx.x != 0u) return;
    const uint64_t payload = 4ull + run;                  /* u32 element count + items */
    uint64_t st = LZF_MGET_OK;
    if (!found) st = LZF_MGET_NOT_FOUND;                  /* src/query.c:731-735 */
    else if (payload > a.max_response) st = LZF_MGET_TOO_BIG;   /* CHECK_SPACE, src/net.c:1272-1277 */
    a.w_state[MG_PAYLOAD] = payload;
    a.w_state[MG_STATUS] = st;
    a.w_state[MG_FOUND] = found;
    a.w_state[MG_BAD] = 0ull;
    a.result[0] = found;
    a.result[1] = expired;
    a.result[2] = skipped;
    a.result[3] = st;
}

/* one wave per entry, the waves striding over the list */
__global__ __launch_bounds__(SD_BLOCK) void lzf_mget_write_kernel(LzfMgetArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const bool go = a.w_state[MG_STATUS] == (uint64_t)LZF_MGET_OK;
    const uint64_t hdr = a.reply_header ? SD_HDR : 0u;
    const uint64_t w0 = (uint64_t)blockIdx.x * SD_WAVES + (threadIdx.x >> 6), step = (uint64_t)gridDim.x * SD_WAVES;
    if (w0 == 0ull && lane == 0u && go) {
        uint8_t *f = a.frame;
        if (a.reply_header)                                                       /* src/net.c:1339 */
            sd_put_header(f, LZF_REPL_KVAL, (uint8_t)LZF_ENC_PLAIN, (uint32_t)a.w_state[MG_PAYLOAD]);
        sd_put32(f + hdr, (uint32_t)a.w_state[MG_FOUND]);                         /* src/net.c:1282 */
    }
    for (uint64_t k = w0; k < a.n; k += step) {
        /* whatever the status: the reference's validity pass runs before the reply is built */
        const uint32_t dead = a.g_null[k];
        if (dead != SD_PAD && lane == 0u) a.it.enc[dead] = (uint8_t)LZF_ENC_NULL;
        const uint8_t e = a.g_enc[k];
        bool dec = false;
        uint64_t voff = 0ull;
        if (go && e != (uint8_t)LZF_ENC_NULL) {
            const uint32_t kl = a.g_key_len[k], vl = a.g_val_len[k];
            uint8_t *f = a.frame + hdr + 4u + a.w_off[k] + a.w_tile[k / SD_TILE];
            const uint8_t *key = a.keys + a.g_key_off[k];
            if (lane == 0u) {
                sd_put32(f, kl);                                                  /* :1294 */
                f[4u + kl] = e == (uint8_t)LZF_ENC_LZF ? (uint8_t)LZF_ENC_PLAIN : e;   /* :1313, :1331 */
                sd_put32(f + 5u + kl, vl);                                        /* :1332 */
            }
            for (uint32_t j = lane; j < kl; j += 64u) f[4u + j] = key[j];        /* :1295 */
            uint8_t *v = f + 9u + kl;
            if (e == (uint8_t)LZF_ENC_LZF) {
                dec = true;
                voff = (uint64_t)(v - a.frame);
            } else {
                sd_wave_copy(v, a.store + a.g_val_off[k], vl, lane);              /* :1333 */
            }
        }
        if (lane == 0u) {
            a.w_voff[k] = voff;
            a.w_skip[k] = dec ? 0u : 1u;
        }
    }
}

/* every LZF entry must have decoded to its recorded length.  By the whole
 * grid: one workgroup walking 100 000 entries took 373 us, a third of the
 * call (profiles/r10/mget/).  A workgroup that finds a bad entry says so in
 * the state word the scan kernel cleared; the finish kernel reads it */
__global__ __launch_bounds__(SD_BLOCK) void lzf_mget_check_kernel(LzfMgetArgs a)
{
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    int bad = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; k < a.n; k += step)
        if (!a.w_skip[k] && (a.w_err[k] != 0 || a.w_len[k] != a.g_val_len[k])) bad = 1;
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0u && bad) atomicOr((unsigned long long *)&a.w_state[MG_BAD], 1ull);
}

__global__ void lzf_mget_finish_kernel(LzfMgetArgs a)
{
    uint64_t st = a.w_state[MG_STATUS];
    if (st == (uint64_t)LZF_MGET_OK && a.w_state[MG_BAD]) st = LZF_MGET_EDECODE;
    a.result[3] = st;
    *a.frame_len = st == (uint64_t)LZF_MGET_OK ? a.w_state[MG_PAYLOAD] + (a.reply_header ? SD_HDR : 0u) : 0ull;
}

/* ---- count, mttl ------------------------------------------------------------ */

/* gbCountCallback (src/query.c:1139-1157) and, MTTL, gbMultiTtlCallback
 * (src/query.c:580-600) over the list.  Every lane of a workgroup makes the
 * same number of rounds.  out[0]: valid entries, out[1]: expired ones */
template <bool MTTL>
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_index_kernel(const uint32_t *__restrict__ idx, uint32_t n,
                                                                   int32_t ttl, LzfItems it, uint64_t *out)
{
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t valid = 0u, expired = 0u;
    for (uint64_t b = (uint64_t)blockIdx.x * SD_BLOCK; b < n; b += step) {
        const uint64_t k = b + threadIdx.x;
        int v = MG_DEAD;
        if (k < n) {
            const uint32_t i = idx[k];
            v = mg_validity(i, it);
            if (v == MG_EXPIRED) it.enc[i] = (uint8_t)LZF_ENC_NULL;
            if (v == MG_VALID) {
                if (MTTL) {
                    it.item_time[i] = it.now;             /* src/query.c:590-592 */
                    it.item_ttl[i] = ttl;
                }
                if (it.last_access) it.last_access[i] = it.now;
            }
        }
        valid += sd_count(v == MG_VALID);
        expired += sd_count(v == MG_EXPIRED);
    }
    sd_leader_add(out, valid);
    sd_leader_add(out + 1, expired);
}

}  // namespace

hipError_t lzf_launch_store_select(LzfSelectArgs &a, hipStream_t s)
{
    const uint32_t nt = sd_tiles(a.count);
    hipLaunchKernelGGL(lzf_select_match_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_select_carry_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_select_write_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t lzf_launch_store_mget(LzfMgetArgs &a, hipStream_t s, hipError_t (*decode)(const LzfBatch &, hipStream_t))
{
    const uint32_t nt = sd_tiles(a.n);
    hipLaunchKernelGGL(lzf_mget_gather_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_mget_scan_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_mget_write_kernel, dim3(sd_wave_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const LzfBatch b = sd_decode_batch(a.store, a.g_val_off, a.g_val_size, a.frame, a.w_voff, a.g_val_len, a.w_len,
                                       a.w_err, a.n, a.max_val_len, a.w_skip);
    if ((e = decode(b, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_mget_check_kernel, dim3(sd_sweep_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_mget_finish_kernel, dim3(1), dim3(1), 0, s, a);
    return hipGetLastError();
}

hipError_t lzf_launch_store_count(const uint32_t *idx, uint32_t n, const LzfItems &it, uint64_t *result, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(result, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_store_index_kernel<false>, dim3(sd_sweep_grid(n)), dim3(SD_BLOCK), 0, s, idx, n, 0, it, result);
    return hipGetLastError();
}

hipError_t lzf_launch_store_mttl(const uint32_t *idx, uint32_t n, int32_t ttl, const LzfItems &it, uint64_t *result,
                                 hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(result, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_store_index_kernel<true>, dim3(sd_sweep_grid(n)), dim3(SD_BLOCK), 0, s, idx, n, ttl, it, result);
    return hipGetLastError();
}
