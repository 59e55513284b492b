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
#include "lzf_dev.h"
#include "../../include/lzf_gpu.h"

#define MG_BLOCK 256u
#define MG_PER   4u
#define MG_TILE  (MG_BLOCK * MG_PER)      /* items / entries per tile */
#define MG_WAVES (MG_BLOCK / 64u)
#define MG_WORDS (MG_TILE / 64u)          /* ballot words per select tile */
#define MG_GRID  2048u                    /* grid-stride kernels: 256 CUs x 8 workgroups */
#define MG_PAD   0xFFFFFFFFu
/* the write kernel works a wave per entry, MG_WAVES entries per workgroup:
 * the cap of its grid, past which the waves stride over the list */
#define MG_WRITE_GRID 16384u

static inline uint32_t mg_tiles(uint32_t n)
{
    return (uint32_t)(((uint64_t)n + MG_TILE - 1u) / MG_TILE);
}

namespace {

/* state words of the mget work area */
enum { MG_PAYLOAD = 0, MG_STATUS = 1, MG_FOUND = 2, MG_BAD = 3 };

/* mg_validity, the validity rule of every index-list operator: lzf_dev.h */

/* ---- select ----------------------------------------------------------------- */

/* whether the plen bytes at key equal the prefix: whole dwords, the last one
 * overlapping the one before it when plen is no multiple of 4, so only a
 * prefix of 1-3 bytes is compared byte by byte.  Most keys leave at the first
 * dword */
__device__ inline bool mg_prefix_match(const uint8_t *key, const uint8_t *__restrict__ prefix, uint32_t plen)
{
    if (plen < 4u) {
        bool same = true;
        for (uint32_t j = 0; j < plen; j++) same &= key[j] == prefix[j];
        return same;
    }
    for (uint32_t j = 0; j + 4u <= plen; j += 4u)
        if (dv_ld4(key + j) != dv_ld4(prefix + j)) return false;
    return !(plen & 3u) || dv_ld4(key + plen - 4u) == dv_ld4(prefix + plen - 4u);
}

/* item i of a tile sits in round k = (i % MG_TILE) / MG_BLOCK at thread
 * i % MG_BLOCK, so a wave reads 64 neighbouring descriptors and its ballot
 * word is number (i % MG_TILE) / 64 of the tile's MG_WORDS, in index order */
__global__ __launch_bounds__(MG_BLOCK) void lzf_select_match_kernel(LzfSelectArgs a)
{
    __shared__ uint32_t sc[MG_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * MG_TILE;
    uint32_t hits = 0u;
#pragma unroll
    for (uint32_t k = 0; k < MG_PER; k++) {
        const uint64_t i = first + k * MG_BLOCK + threadIdx.x;
        bool m = false;
        if (i < a.count && a.enc[i] != (uint8_t)LZF_ENC_NULL && a.key_len[i] >= a.prefix_len)
            m = mg_prefix_match(a.keys + a.key_off[i], a.prefix, a.prefix_len);
        const uint64_t word = __ballot(m);
        if (lane == 0u) a.w_mask[(uint64_t)blockIdx.x * MG_WORDS + k * MG_WAVES + wave] = word;
        hits += (uint32_t)__popcll(word);
    }
    if (lane == 0u) sc[wave] = hits;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t n = 0u;
        for (uint32_t w = 0; w < MG_WAVES; w++) n += sc[w];
        a.w_tile[blockIdx.x] = n;
    }
}

/* one workgroup: the exclusive scan of the tile counts in place, and result[].
 * In pieces of MG_BLOCK * MG_CARRY_PER with a running carry, a thread taking
 * MG_CARRY_PER neighbouring tiles: 16 M items are 16 384 tiles, and at one
 * tile per thread the 64 dependent rounds took 50 us of the select's 240
 * (profiles/r10/mget/) */
#define MG_CARRY_PER 8u
__global__ __launch_bounds__(MG_BLOCK) void lzf_select_carry_kernel(LzfSelectArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[MG_WAVES];
    uint64_t run = 0ull;
    for (uint64_t c = 0; c < ntile; c += MG_BLOCK * MG_CARRY_PER) {
        const uint64_t first = c + threadIdx.x * MG_CARRY_PER;
        uint64_t v[MG_CARRY_PER], s = 0ull;
#pragma unroll
        for (uint32_t j = 0; j < MG_CARRY_PER; j++) {
            v[j] = first + j < ntile ? a.w_tile[first + j] : 0ull;
            s += v[j];
        }
        uint64_t tot;
        uint64_t o = run + dv_block_excl<MG_WAVES>(s, sw, &tot);
#pragma unroll
        for (uint32_t j = 0; j < MG_CARRY_PER; j++) {
            if (first + j < ntile) a.w_tile[first + j] = o;
            o += v[j];
        }
        run += tot;
    }
    if (threadIdx.x != 0u) return;
    a.result[0] = (uint32_t)(run < a.cap ? run : a.cap);
    a.result[1] = (uint32_t)run;                          /* at most count */
}

__global__ __launch_bounds__(MG_BLOCK) void lzf_select_write_kernel(LzfSelectArgs a)
{
    __shared__ uint32_t pre[MG_WORDS + 1u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t *mask = a.w_mask + (uint64_t)blockIdx.x * MG_WORDS;
    if (threadIdx.x == 0u) {
        uint32_t s = 0u;
        for (uint32_t w = 0; w < MG_WORDS; w++) {
            pre[w] = s;
            s += (uint32_t)__popcll(mask[w]);
        }
    }
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * MG_TILE, base = a.w_tile[blockIdx.x];
#pragma unroll
    for (uint32_t k = 0; k < MG_PER; k++) {
        const uint32_t w = k * MG_WAVES + wave;
        const uint64_t word = mask[w];
        if (!((word >> lane) & 1ull)) continue;
        const uint64_t r = base + pre[w] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
        if (r < a.cap) a.sel[r] = (uint32_t)(first + k * MG_BLOCK + threadIdx.x);
    }
    /* the padding, by all the workgroups together */
    const uint64_t step = (uint64_t)gridDim.x * MG_BLOCK;
    for (uint64_t r = (uint64_t)a.result[0] + (uint64_t)blockIdx.x * MG_BLOCK + threadIdx.x; r < a.cap; r += step)
        a.sel[r] = MG_PAD;
}

/* ---- mget ------------------------------------------------------------------- */

/* a tile's three counts in one word for the scan inside the tile: each is at
 * most MG_TILE = 2^10 */
#define MG_ONE_FOUND   1ull
#define MG_ONE_EXPIRED (1ull << 21)
#define MG_ONE_SKIPPED (1ull << 42)
#define MG_CNT_MASK    ((1ull << 21) - 1ull)

/* thread t of a tile takes entries t * MG_PER .. + MG_PER, so the scan over the
 * threads is the scan over the list */
__global__ __launch_bounds__(MG_BLOCK) void lzf_mget_gather_kernel(LzfMgetArgs a)
{
    __shared__ uint64_t sw[MG_WAVES];
    const uint64_t first = (uint64_t)blockIdx.x * MG_TILE + threadIdx.x * MG_PER;
    uint64_t sz[MG_PER], s = 0ull, cnt = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < MG_PER; j++) {
        const uint64_t k = first + j;
        sz[j] = 0ull;
        if (k >= a.n) continue;
        const uint32_t i = a.idx[k];
        const int v = mg_validity(i, a.count, a.enc, a.item_time, a.item_ttl, a.now);
        uint8_t e = (uint8_t)LZF_ENC_NULL;
        uint64_t ko = 0ull, vo = 0ull;
        uint32_t kl = 0u, vs = 0u, vl = 0u;
        if (v == MG_VALID) {
            e = a.enc[i];
            ko = a.key_off[i];
            kl = a.key_len[i];
            vo = a.val_off[i];
            vs = a.val_size[i];
            vl = e == (uint8_t)LZF_ENC_LZF ? a.val_len[i] : vs;
            sz[j] = 4ull + kl + 1ull + 4ull + vl;         /* src/net.c:1294-1333 */
            if (a.last_access) a.last_access[i] = a.now;  /* src/query.c:693 */
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
        a.g_null[k] = v == MG_EXPIRED ? i : MG_PAD;
        s += sz[j];
    }
    uint64_t tot, ctot;
    uint64_t o = dv_block_excl<MG_WAVES>(s, sw, &tot);
    (void)dv_block_excl<MG_WAVES>(cnt, sw, &ctot);
#pragma unroll
    for (uint32_t j = 0; j < MG_PER; j++) {
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
__global__ __launch_bounds__(MG_BLOCK) void lzf_mget_scan_kernel(LzfMgetArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[MG_WAVES];
    uint64_t run = 0ull, found = 0ull, expired = 0ull, skipped = 0ull;
    for (uint32_t c = 0; c < ntile; c += MG_BLOCK) {
        const uint32_t i = c + threadIdx.x;
        const uint64_t x = i < ntile ? a.w_tile[i] : 0ull, cn = i < ntile ? a.w_tcnt[i] : 0ull;
        uint64_t tot, tf, te, ts;
        const uint64_t o = dv_block_excl<MG_WAVES>(x, sw, &tot);
        (void)dv_block_excl<MG_WAVES>(cn & MG_CNT_MASK, sw, &tf);
        (void)dv_block_excl<MG_WAVES>((cn >> 21) & MG_CNT_MASK, sw, &te);
        (void)dv_block_excl<MG_WAVES>((cn >> 42) & MG_CNT_MASK, sw, &ts);
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

__device__ inline void mg_put32(uint8_t *p, uint32_t x)
{
    p[0] = (uint8_t)x; p[1] = (uint8_t)(x >> 8); p[2] = (uint8_t)(x >> 16); p[3] = (uint8_t)(x >> 24);
}

/* one wave per entry, the waves striding over the list */
__global__ __launch_bounds__(MG_BLOCK) void lzf_mget_write_kernel(LzfMgetArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const bool go = a.w_state[MG_STATUS] == (uint64_t)LZF_MGET_OK;
    const uint64_t hdr = a.reply_header ? 7u : 0u;       /* [i16 code][u8 enc][u32 size] */
    const uint64_t w0 = (uint64_t)blockIdx.x * MG_WAVES + (threadIdx.x >> 6), step = (uint64_t)gridDim.x * MG_WAVES;
    if (w0 == 0ull && lane == 0u && go) {
        uint8_t *f = a.frame;
        if (a.reply_header) {
            f[0] = (uint8_t)LZF_REPL_KVAL; f[1] = (uint8_t)(LZF_REPL_KVAL >> 8);   /* src/net.c:1185 */
            f[2] = LZF_ENC_PLAIN;                                                 /* src/net.c:1339 */
            mg_put32(f + 3, (uint32_t)a.w_state[MG_PAYLOAD]);
        }
        mg_put32(f + hdr, (uint32_t)a.w_state[MG_FOUND]);                         /* src/net.c:1282 */
    }
    for (uint64_t k = w0; k < a.n; k += step) {
        /* whatever the status: the reference's validity pass runs before the reply is built */
        const uint32_t dead = a.g_null[k];
        if (dead != MG_PAD && lane == 0u) a.enc[dead] = (uint8_t)LZF_ENC_NULL;
        const uint8_t e = a.g_enc[k];
        bool dec = false;
        uint64_t voff = 0ull;
        if (go && e != (uint8_t)LZF_ENC_NULL) {
            const uint32_t kl = a.g_key_len[k], vl = a.g_val_len[k];
            uint8_t *f = a.frame + hdr + 4u + a.w_off[k] + a.w_tile[k / MG_TILE];
            const uint8_t *key = a.keys + a.g_key_off[k];
            if (lane == 0u) {
                mg_put32(f, kl);                                                  /* :1294 */
                f[4u + kl] = e == (uint8_t)LZF_ENC_LZF ? (uint8_t)LZF_ENC_PLAIN : e;   /* :1313, :1331 */
                mg_put32(f + 5u + kl, vl);                                        /* :1332 */
            }
            for (uint32_t j = lane; j < kl; j += 64u) f[4u + j] = key[j];        /* :1295 */
            uint8_t *v = f + 9u + kl;
            if (e == (uint8_t)LZF_ENC_LZF) {
                dec = true;
                voff = (uint64_t)(v - a.frame);
            } else {
                /* :1333; 16 bytes per lane (unaligned loads and stores), then the tail */
                const uint8_t *s = a.store + a.g_val_off[k];
                const uint32_t whole = vl & ~15u;
                for (uint32_t j = lane * 16u; j < whole; j += 64u * 16u) {
                    const uint4 x = dv_ld16(s + j);
                    __builtin_memcpy(v + j, &x, 16);
                }
                for (uint32_t j = whole + lane; j < vl; j += 64u) v[j] = s[j];
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
__global__ __launch_bounds__(MG_BLOCK) void lzf_mget_check_kernel(LzfMgetArgs a)
{
    const uint64_t step = (uint64_t)gridDim.x * MG_BLOCK;
    int bad = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * MG_BLOCK + threadIdx.x; k < a.n; k += step)
        if (!a.w_skip[k] && (a.w_err[k] != 0 || a.w_len[k] != a.g_val_len[k])) bad = 1;
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0u && bad) atomicOr((unsigned long long *)&a.w_state[MG_BAD], 1ull);
}

__global__ void lzf_mget_finish_kernel(LzfMgetArgs a)
{
    uint64_t st = a.w_state[MG_STATUS];
    if (st == (uint64_t)LZF_MGET_OK && a.w_state[MG_BAD]) st = LZF_MGET_EDECODE;
    a.result[3] = st;
    *a.frame_len = st == (uint64_t)LZF_MGET_OK ? a.w_state[MG_PAYLOAD] + (a.reply_header ? 7u : 0u) : 0ull;
}

/* ---- count, mttl ------------------------------------------------------------ */

/* gbCountCallback (src/query.c:1139-1157) and, MTTL, gbMultiTtlCallback
 * (src/query.c:580-600) over the list.  Every lane of a workgroup makes the
 * same number of rounds.  out[0]: valid entries, out[1]: expired ones */
template <bool MTTL>
__global__ __launch_bounds__(MG_BLOCK) void lzf_store_index_kernel(const uint32_t *__restrict__ idx, uint32_t n,
                                                                   int32_t ttl, uint8_t *enc, uint32_t count,
                                                                   int64_t *item_time, int32_t *item_ttl, int64_t now,
                                                                   int64_t *last_access, uint64_t *out)
{
    const uint64_t step = (uint64_t)gridDim.x * MG_BLOCK;
    uint32_t valid = 0u, expired = 0u;
    for (uint64_t b = (uint64_t)blockIdx.x * MG_BLOCK; b < n; b += step) {
        const uint64_t k = b + threadIdx.x;
        int v = MG_DEAD;
        if (k < n) {
            const uint32_t i = idx[k];
            v = mg_validity(i, count, enc, item_time, item_ttl, now);
            if (v == MG_EXPIRED) enc[i] = (uint8_t)LZF_ENC_NULL;
            if (v == MG_VALID) {
                if (MTTL) {
                    item_time[i] = now;                   /* src/query.c:590-592 */
                    item_ttl[i] = ttl;
                }
                if (last_access) last_access[i] = now;
            }
        }
        valid += (uint32_t)__popcll(__ballot(v == MG_VALID));
        expired += (uint32_t)__popcll(__ballot(v == MG_EXPIRED));
    }
    if ((threadIdx.x & 63u) != 0u) return;
    if (valid) atomicAdd((unsigned long long *)out, (unsigned long long)valid);
    if (expired) atomicAdd((unsigned long long *)out + 1, (unsigned long long)expired);
}

static inline uint32_t mg_sweep_grid(uint64_t n, uint32_t per_block)
{
    const uint64_t g = (n + per_block - 1u) / per_block;
    return (uint32_t)(g < MG_GRID ? g : MG_GRID);
}

}  // namespace

uint64_t lzf_select_work_bytes(uint32_t count)
{
    /* the ballot words (u64, MG_WORDS per tile) | the tile counts (u64 per
     * tile); room to align the caller's pointer.  Below 2^30 */
    return (uint64_t)mg_tiles(count) * (MG_WORDS + 1u) * 8u + 16u;
}

void lzf_select_carve(LzfSelectArgs &a, void *work)
{
    uint8_t *w = (uint8_t *)(((uintptr_t)work + 7u) & ~(uintptr_t)7u);
    a.w_mask = (uint64_t *)w;             w += (size_t)mg_tiles(a.count) * MG_WORDS * 8;
    a.w_tile = (uint64_t *)w;
}

hipError_t lzf_launch_store_select(LzfSelectArgs &a, hipStream_t s)
{
    const uint32_t nt = mg_tiles(a.count);
    hipLaunchKernelGGL(lzf_select_match_kernel, dim3(nt), dim3(MG_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_select_carry_kernel, dim3(1), dim3(MG_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_select_write_kernel, dim3(nt), dim3(MG_BLOCK), 0, s, a);
    return hipGetLastError();
}

uint64_t lzf_mget_work_bytes(uint32_t n)
{
    /* state (8 x u64) | key_off, val_off, off, voff (u64) | tile bytes, tile
     * counts (u64 per tile) | key_len, val_size, val_len, null, len, err (u32)
     * | enc, skip (u8); room to align the caller's pointer.  Below 2^38 */
    return 64u + (uint64_t)n * (4u * 8u + 6u * 4u + 2u) + (uint64_t)mg_tiles(n) * 16u + 16u;
}

void lzf_mget_carve(LzfMgetArgs &a, void *work)
{
    uint8_t *w = (uint8_t *)(((uintptr_t)work + 7u) & ~(uintptr_t)7u);
    const size_t n = a.n, nt = mg_tiles(a.n);
    a.w_state = (uint64_t *)w;            w += 64;
    a.g_key_off = (uint64_t *)w;          w += n * 8;
    a.g_val_off = (uint64_t *)w;          w += n * 8;
    a.w_off = (uint64_t *)w;              w += n * 8;
    a.w_voff = (uint64_t *)w;             w += n * 8;
    a.w_tile = (uint64_t *)w;             w += nt * 8;
    a.w_tcnt = (uint64_t *)w;             w += nt * 8;
    a.g_key_len = (uint32_t *)w;          w += n * 4;
    a.g_val_size = (uint32_t *)w;         w += n * 4;
    a.g_val_len = (uint32_t *)w;          w += n * 4;
    a.g_null = (uint32_t *)w;             w += n * 4;
    a.w_len = (uint32_t *)w;              w += n * 4;
    a.w_err = (int32_t *)w;               w += n * 4;
    a.g_enc = w;                          w += n;
    a.w_skip = w;
}

hipError_t lzf_launch_store_mget(LzfMgetArgs &a, hipStream_t s, hipError_t (*decode)(const LzfBatch &, hipStream_t))
{
    const uint32_t nt = mg_tiles(a.n);
    hipLaunchKernelGGL(lzf_mget_gather_kernel, dim3(nt), dim3(MG_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_mget_scan_kernel, dim3(1), dim3(MG_BLOCK), 0, s, a, nt);
    const uint64_t nw = ((uint64_t)a.n + MG_WAVES - 1u) / MG_WAVES;
    hipLaunchKernelGGL(lzf_mget_write_kernel, dim3((uint32_t)(nw < MG_WRITE_GRID ? nw : MG_WRITE_GRID)), dim3(MG_BLOCK),
                       0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    LzfBatch b{};
    b.in = a.store;
    b.in_off = a.g_val_off;
    b.in_len = a.g_val_size;
    b.out = a.frame;
    b.out_off = a.w_voff;
    b.out_cap = a.g_val_len;
    b.out_len = a.w_len;
    b.err = a.w_err;
    b.count = a.n;
    b.max_len = a.max_val_len;
    b.skip = a.w_skip;
    if ((e = decode(b, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_mget_check_kernel, dim3(mg_sweep_grid(a.n, MG_BLOCK)), dim3(MG_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_mget_finish_kernel, dim3(1), dim3(1), 0, s, a);
    return hipGetLastError();
}

hipError_t lzf_launch_store_count(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count,
                                  const int64_t *item_time, const int32_t *item_ttl, int64_t now, int64_t *last_access,
                                  uint64_t *result, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(result, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    /* COUNT reads the time arrays only */
    hipLaunchKernelGGL(lzf_store_index_kernel<false>, dim3(mg_sweep_grid(n, MG_BLOCK)), dim3(MG_BLOCK), 0, s, idx, n, 0,
                       enc, count, const_cast<int64_t *>(item_time), const_cast<int32_t *>(item_ttl), now, last_access,
                       result);
    return hipGetLastError();
}

hipError_t lzf_launch_store_mttl(const uint32_t *idx, uint32_t n, int32_t ttl, uint8_t *enc, uint32_t count,
                                 int64_t *item_time, int32_t *item_ttl, int64_t now, int64_t *last_access,
                                 uint64_t *result, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(result, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_store_index_kernel<true>, dim3(mg_sweep_grid(n, MG_BLOCK)), dim3(MG_BLOCK), 0, s, idx, n, ttl,
                       enc, count, item_time, item_ttl, now, last_access, result);
    return hipGetLastError();
}
