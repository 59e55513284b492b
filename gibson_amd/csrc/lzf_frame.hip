/*
 * lzf_frame.hip -- the MGET / KEYS reply payload assembled in HBM, with the
 * LZF items decompressed straight into it.
 *
 * The reference builds the payload item by item on the host
 * (gbClientEnqueueKeyValueSet, src/net.c:1256-1342): a u32 element count,
 * then per non-null item [u32 key size][key][u8 encoding][u32 value size]
 * [value], where an LZF item is first decompressed into the shared
 * lzf_buffer (src/net.c:1301-1311) and then copied (src/net.c:1333-1335),
 * and framed again by gbClientEnqueueData (src/net.c:1162-1205) behind
 * [i16 code][u8 encoding][u32 size].  Here:
 *
 *   1. frame_size: per item its frame bytes; a block-local exclusive scan;
 *   2. frame_scan: exclusive scan of the block sums (one workgroup), the
 *      payload size and the max-response check (CHECK_SPACE, src/net.c:
 *      1272-1277: the per-write checks fail iff the final size exceeds);
 *   3. frame_write: one wave per item writes its headers and key, copies a
 *      PLAIN / NUMBER value, and describes an LZF item to the decoder: its
 *      output offset inside the frame and its recorded original length;
 *   4. the tokpar64 decoder over the same items (the others skipped)
 *      decodes every LZF value in place -- no lzf_buffer, no second copy;
 *   5. frame_check: every LZF item must decode to its recorded length.
 *
 * The decoded length of an LZF item must be known up front (the side table
 * of original lengths, §8(f) rank 3): the caller passes it in val_len.
 *
 * The scans, the header and the geometry are the store toolkit's
 * (lzf_store_dev.h); the work area is lzf_frame_layout (lzf_store_layout.h).
 */
#include "lzf_store_dev.h"
#include "../../include/lzf_gpu.h"

__device__ __forceinline__ uint64_t fr_item_bytes(const LzfFrameArgs &a, uint32_t i)
{
    const uint8_t e = a.enc[i];
    if (e == LZF_ENC_NULL) return 0;                      /* src/net.c:1287 */
    const uint32_t v = e == LZF_ENC_LZF ? a.val_len[i] : a.val_size[i];
    return 4ull + a.key_len[i] + 1ull + 4ull + v;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_frame_size_kernel(LzfFrameArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint32_t base = blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t sz[SD_PER], s = 0;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        sz[k] = base + k < a.count ? fr_item_bytes(a, base + k) : 0ull;
        s += sz[k];
    }
    uint64_t tot;
    uint64_t o = dv_block_excl<SD_WAVES>(s, sw, &tot);
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        if (base + k < a.count) a.w_off[base + k] = o;
        o += sz[k];
    }
    if (threadIdx.x == 0) a.w_bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_frame_scan_kernel(LzfFrameArgs a, uint32_t nblocks)
{
    __shared__ uint64_t sw[SD_WAVES];
    uint64_t run = 0;
    for (uint32_t c = 0; c < nblocks; c += SD_BLOCK) {
        const uint32_t i = c + threadIdx.x;
        const uint64_t x = i < nblocks ? a.w_bsum[i] : 0ull;
        uint64_t tot;
        const uint64_t o = dv_block_excl<SD_WAVES>(x, sw, &tot);
        if (i < nblocks) a.w_bsum[i] = run + o;
        run += tot;
    }
    if (threadIdx.x == 0) {
        const uint64_t payload = 4ull + run;              /* u32 element count + items */
        a.w_state[0] = payload;
        a.w_state[1] = payload > a.max_response ? 1ull : 0ull;   /* CHECK_SPACE */
    }
}

/* one wave per item, and one workgroup of 64 threads per item: not the
 * toolkit's 256-thread geometry, and the value copied byte by byte -- the
 * kernel is kept as it was measured (lzf_mget_write_kernel is the strided,
 * 16-bytes-per-lane form) */
__global__ __launch_bounds__(64) void lzf_frame_write_kernel(LzfFrameArgs a)
{
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    const bool over = a.w_state[1] != 0ull;
    const uint64_t hdr = a.reply_header ? SD_HDR : 0u;
    if (i == 0 && lane == 0 && !over) {
        uint8_t *f = a.frame;
        if (a.reply_header) sd_put_header(f, LZF_REPL_KVAL, LZF_ENC_PLAIN, (uint32_t)a.w_state[0]);   /* src/net.c:1339 */
        sd_put32(f + hdr, a.elements);                                            /* src/net.c:1282 */
    }
    const uint8_t e = a.enc[i];
    bool dec = false;
    if (!over && e != LZF_ENC_NULL) {
        const uint32_t kl = a.key_len[i];
        const uint32_t vl = e == LZF_ENC_LZF ? a.val_len[i] : a.val_size[i];
        uint8_t *f = a.frame + hdr + 4u + a.w_off[i] + a.w_bsum[i / SD_TILE];
        const uint8_t *key = a.keys + a.key_off[i];
        if (lane == 0) {
            sd_put32(f, kl);                                                      /* :1294 */
            f[4 + kl] = e == LZF_ENC_LZF ? LZF_ENC_PLAIN : e;                     /* :1313, :1331 */
            sd_put32(f + 5 + kl, vl);                                             /* :1332 */
        }
        for (uint32_t k = lane; k < kl; k += 64u) f[4 + k] = key[k];             /* :1295 */
        uint8_t *v = f + 9u + kl;
        if (e == LZF_ENC_LZF) {
            dec = true;
            if (lane == 0) a.w_voff[i] = (uint64_t)(v - a.frame);
        } else {
            const uint8_t *s = a.vals + a.val_off[i];
            for (uint32_t k = lane; k < vl; k += 64u) v[k] = s[k];               /* :1333 */
        }
    }
    if (lane == 0) a.w_skip[i] = dec ? 0u : 1u;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_frame_check_kernel(LzfFrameArgs a)
{
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.count; i += SD_BLOCK)
        if (!a.w_skip[i] && (a.w_err[i] != 0 || a.w_len[i] != a.val_len[i])) bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool ok = !bad && a.w_state[1] == 0ull;
        *a.frame_len = ok ? a.w_state[0] + (a.reply_header ? SD_HDR : 0u) : 0ull;
    }
}

hipError_t lzf_launch_frame(LzfFrameArgs &a, hipStream_t s,
                            hipError_t (*decode)(const LzfBatch &, hipStream_t))
{
    const uint32_t nb = sd_frame_tiles(a.count);
    hipLaunchKernelGGL(lzf_frame_size_kernel, dim3(nb), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_frame_scan_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nb);
    hipLaunchKernelGGL(lzf_frame_write_kernel, dim3(a.count), dim3(64), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = decode(sd_decode_batch(a.vals, a.val_off, a.val_size, a.frame, a.w_voff, a.val_len, a.w_len, a.w_err, a.count,
                               a.max_val_len, a.w_skip),
               s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_frame_check_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}
