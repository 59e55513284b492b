/*
 * lzf_reply.hip -- per-request reply frames over an index list
 * (lzf_gpu_store_replies, include/lzf_gpu.h): the reply of GET
 * (gbQueryGetHandler, src/query.c:634-663) and of the single-key INC / DEC
 * (src/query.c:867, 882) for the requests of many clients in one list.  Where
 * MGET builds one REPL_KVAL frame over the valid entries, this writes one
 * self-contained frame per entry -- gbClientEnqueueData's buffer
 * (src/net.c:1170-1202) -- into a reply arena, densely in list order, so every
 * client's reply is a slice of one device-to-host copy.
 *
 * The shape is MGET's (lzf_mget.hip), with per-entry outcomes:
 *   1. classify (fused): the mode's rule -- the validity rule and last_access
 *      (GET), or the reply code of the operator's status (VALUE) -- the
 *      entry's descriptors copied into the work area, its slot size, its
 *      decode class, entry_status, and the tile-local exclusive scan of the
 *      slots;
 *   2. scan: one workgroup over the tile sums; the counts, the bytes needed,
 *      the TOO_BIG decision, *rep_used;
 *   3. write: one wave per entry: rep_off, rep_len, an expired entry nulled in
 *      enc (here and not in step 1, so that every copy of a duplicated entry is
 *      judged on what enc held before the call), the 7 header bytes, a code
 *      reply's byte, a PLAIN / NUMBER value; an LZF entry is described to the
 *      decoder and entered in its class's skip list;
 *   4. the routed decoder over the gathered arrays, in place in the arena:
 *      one launch bounded by max_val_len (the default), or, one_route off, one
 *      launch per decode size class with that class's bound and skip list, so
 *      tokpar64, the far form and the pipe each take only their own entries
 *      (measured slower on a mixed list, DESIGN.md 7.5: the launches queue
 *      behind one another);
 *   5. check, by the whole grid: an LZF entry that did not decode to its
 *      val_len gets the REPL_ERR code reply at the start of its slot.
 *
 * Nothing crosses between the threads of one launch but inside a workgroup's
 * scan; everything else crosses at a kernel boundary.  The kernels are helpers
 * of this translation unit, not part of the library's routed kernel set: they
 * have internal linkage (anonymous namespace).
 */
#include "lzf_store_dev.h"
#include "../../include/lzf_gpu.h"

/* the geometry, the scans and the byte helpers: lzf_store_dev.h */
#define RP_CODE  (SD_HDR + 1u)            /* a code reply: the header and one 0x00 byte */
/* g_cls of an entry the decoder has nothing to do for */
#define RP_NO_CLASS 0xFFu

namespace {

enum { RP_STATUS = 0 };                   /* state words of the work area */

/* a tile's four counts in one word: each is at most SD_TILE = 2^10 */
#define RP_ONE_VALUE   1ull
#define RP_ONE_EXPIRED (1ull << 16)
#define RP_ONE_SKIPPED (1ull << 32)
#define RP_ONE_REFUSED (1ull << 48)
#define RP_CNT_MASK    0xFFFFull

/* thread t of a tile takes entries t * SD_PER .. + SD_PER, so the scan over the
 * threads is the scan over the list */
__global__ __launch_bounds__(SD_BLOCK) void lzf_reply_classify_kernel(LzfReplyArgs a)
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
        int code, st;
        uint32_t dead = SD_PAD;
        if (a.mode == LZF_REPLY_GET) {
            const int v = mg_validity(i, a.it);
            if (v == MG_VALID) {
                code = LZF_REPL_VAL;
                st = LZF_ENT_DONE;
                if (a.it.last_access) a.it.last_access[i] = a.it.now;   /* src/query.c:650 */
            } else {
                code = LZF_REPL_ERR_NOT_FOUND;                 /* src/query.c:659 */
                st = v == MG_EXPIRED ? LZF_ENT_EXPIRED : LZF_ENT_DEAD;
                if (v == MG_EXPIRED) dead = i;
                cnt += v == MG_EXPIRED ? RP_ONE_EXPIRED : RP_ONE_SKIPPED;
            }
        } else {
            st = a.op_status[k];
            code = lzf_reply_code_of(st);
            if (code == LZF_REPL_VAL && (i >= a.it.count || a.it.enc[i] == (uint8_t)LZF_ENC_NULL)) code = LZF_REPL_ERR;
            if (code != LZF_REPL_VAL) cnt += RP_ONE_SKIPPED;
        }
        uint8_t e = (uint8_t)LZF_ENC_NULL, cls = (uint8_t)RP_NO_CLASS;
        uint64_t vo = 0ull;
        uint32_t vs = 0u, vl = 0u;
        sz[j] = RP_CODE;
        if (code == LZF_REPL_VAL) {
            e = a.it.enc[i];
            vo = a.val_off[i];
            vs = a.val_size[i];
            vl = e == (uint8_t)LZF_ENC_LZF ? a.val_len[i] : vs;
            if (e == (uint8_t)LZF_ENC_LZF) cls = (uint8_t)lzf_size_class_of(vl, a.max_val_len, LZF_GPU_KIND_DECOMPRESS);
            if (cls == (uint8_t)LZF_GPU_NCLASS) {
                /* val_len past the call's bound: a decode failure known here */
                code = LZF_REPL_ERR;
                st = LZF_ENT_EDECODE;
                e = (uint8_t)LZF_ENC_NULL;
                cls = (uint8_t)RP_NO_CLASS;
                vl = 0u;
                cnt += RP_ONE_REFUSED;
            } else {
                const uint64_t whole = (uint64_t)SD_HDR + vl;
                sz[j] = whole < RP_CODE ? (uint64_t)RP_CODE : whole;
                cnt += RP_ONE_VALUE;
            }
        }
        a.g_val_off[k] = vo;
        a.g_val_size[k] = vs;
        a.g_val_len[k] = vl;
        a.g_enc[k] = e;
        a.g_code[k] = (uint8_t)code;
        a.g_cls[k] = cls;
        a.g_null[k] = dead;
        a.entry_status[k] = (uint8_t)st;
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

/* one workgroup: the exclusive scan of the tiles' slot bytes in place (8 tile
 * sums per thread, as the select's carry), the four counts, and the call's
 * decision */
__global__ __launch_bounds__(SD_BLOCK) void lzf_reply_scan_kernel(LzfReplyArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    uint64_t c[4] = {0ull, 0ull, 0ull, 0ull};
    for (uint32_t t = threadIdx.x; t < ntile; t += SD_BLOCK) {
        const uint64_t cn = a.w_tcnt[t];
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) c[q] += (cn >> (16u * q)) & RP_CNT_MASK;
    }
    uint64_t tot[4];
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) (void)dv_block_excl<SD_WAVES>(c[q], sw, &tot[q]);
    const uint64_t need = dv_carry_scan<SD_WAVES>(a.w_tile, ntile, sw);
    if (threadIdx.x != 0u) return;
    const uint64_t st = need > a.rep_cap ? LZF_REPLY_TOO_BIG : LZF_REPLY_OK;
    a.w_state[RP_STATUS] = st;
    a.result[0] = tot[0];
    a.result[1] = tot[1];
    a.result[2] = tot[2];
    a.result[3] = st;
    a.result[4] = need;
    a.result[5] = tot[3];
    *a.rep_used = st == (uint64_t)LZF_REPLY_OK ? need : 0ull;
}

/* gbClientEnqueueCode's reply (src/net.c:1204-1214): size 1, one 0x00 byte */
__device__ inline void rp_put_code(uint8_t *f, int code)
{
    sd_put_header(f, code, (uint8_t)LZF_ENC_PLAIN, 1u);
    f[SD_HDR] = 0u;
}

/* one wave per entry, the waves striding over the list.  nskip: the number of
 * skip lists (one per decode class, or one for all of them) */
__global__ __launch_bounds__(SD_BLOCK) void lzf_reply_write_kernel(LzfReplyArgs a, uint32_t nskip)
{
    const uint32_t lane = threadIdx.x & 63u;
    const bool go = a.w_state[RP_STATUS] == (uint64_t)LZF_REPLY_OK;
    const uint64_t w0 = (uint64_t)blockIdx.x * SD_WAVES + (threadIdx.x >> 6), step = (uint64_t)gridDim.x * SD_WAVES;
    for (uint64_t k = w0; k < a.n; k += step) {
        /* whatever the status: the reference's validity pass runs before the reply is built */
        const uint32_t dead = a.g_null[k];
        if (dead != SD_PAD && lane == 0u) a.it.enc[dead] = (uint8_t)LZF_ENC_NULL;
        const uint8_t e = a.g_enc[k];
        const int code = a.g_code[k];
        const uint32_t vl = a.g_val_len[k];
        const uint64_t off = a.w_off[k] + a.w_tile[k / SD_TILE];
        const bool dec = go && a.g_cls[k] != (uint8_t)RP_NO_CLASS;
        if (go) {
            uint8_t *f = a.replies + off;
            if (code != LZF_REPL_VAL) {
                if (lane == 0u) rp_put_code(f, code);
            } else {
                if (lane == 0u)                                                   /* src/net.c:1233, :1250 */
                    sd_put_header(f, LZF_REPL_VAL, e == (uint8_t)LZF_ENC_LZF ? (uint8_t)LZF_ENC_PLAIN : e, vl);
                if (e != (uint8_t)LZF_ENC_LZF) sd_wave_copy(f + SD_HDR, a.store + a.g_val_off[k], vl, lane);
            }
        }
        if (lane == 0u) {
            a.rep_off[k] = off;
            a.rep_len[k] = code == LZF_REPL_VAL ? SD_HDR + vl : RP_CODE;
            a.w_voff[k] = off + SD_HDR;
            const uint32_t cls = nskip == 1u ? 0u : a.g_cls[k];
            for (uint32_t c = 0; c < nskip; c++) a.w_skip[(uint64_t)c * a.n + k] = dec && cls == c ? 0u : 1u;
        }
    }
}

/* every LZF entry must have decoded to its recorded length; one that did not
 * gets the REPL_ERR code reply at the start of its slot.  By the whole grid,
 * the failures summed per workgroup and added with one atomic per workgroup */
__global__ __launch_bounds__(SD_BLOCK) void lzf_reply_check_kernel(LzfReplyArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    if (a.w_state[RP_STATUS] != (uint64_t)LZF_REPLY_OK) return;   /* nothing was decoded; the same for every thread */
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint64_t bad = 0ull;
    for (uint64_t k = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; k < a.n; k += step) {
        if (a.g_cls[k] == (uint8_t)RP_NO_CLASS) continue;
        if (a.w_err[k] == 0 && a.w_len[k] == a.g_val_len[k]) continue;
        rp_put_code(a.replies + a.rep_off[k], LZF_REPL_ERR);
        a.rep_len[k] = RP_CODE;
        a.entry_status[k] = (uint8_t)LZF_ENT_EDECODE;
        bad++;
    }
    uint64_t tot;
    (void)dv_block_excl<SD_WAVES>(bad, sw, &tot);
    if (threadIdx.x == 0u && tot) {
        atomicAdd((unsigned long long *)&a.result[5], (unsigned long long)tot);
        atomicAdd((unsigned long long *)&a.result[0], 0ull - (unsigned long long)tot);
    }
}

}  // namespace

hipError_t lzf_launch_store_replies(LzfReplyArgs &a, hipStream_t s,
                                    hipError_t (*decode)(const LzfBatch &, hipStream_t), bool one_route)
{
    const uint32_t nt = sd_tiles(a.n);
    /* the classes that can hold an entry: those whose sizes begin at or below
     * the call's bound */
    uint32_t nclass = 1u;
    while (!one_route && nclass < LZF_DECODE_NCLASS && a.max_val_len > lzf_decode_class_edge(nclass - 1u)) nclass++;
    hipLaunchKernelGGL(lzf_reply_classify_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_reply_scan_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_reply_write_kernel, dim3(sd_wave_grid(a.n)), dim3(SD_BLOCK), 0, s, a, nclass);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (uint32_t c = 0; c < nclass; c++) {
        const uint32_t edge = one_route ? 0xFFFFFFFFu : lzf_decode_class_edge(c);
        const LzfBatch b = sd_decode_batch(a.store, a.g_val_off, a.g_val_size, a.replies, a.w_voff, a.g_val_len, a.w_len,
                                           a.w_err, a.n, edge < a.max_val_len ? edge : a.max_val_len,
                                           a.w_skip + (size_t)c * a.n);
        if ((e = decode(b, s)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lzf_reply_check_kernel, dim3(sd_sweep_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}

int lzf_reply_code(int ent_status) { return lzf_reply_code_of(ent_status); }
