/*
 * lzf_dispatch.hip -- request dispatch: a parsed batch of mixed operators is
 * bucketed by operator class on the device, and the per-class replies are
 * stitched back into one reply table in request order.
 *
 * lzf_gpu_request_bucket: the stable multi-class partition of lzf_mixed.hip in
 * the store's reduce / carry / write shape, over scan tiles of SD_TILE
 * requests, with no workgroup waiting for another.  The class rule is
 * lzf_request_class_of (lzf_request.h, the only place it is written).  Round r
 * of a tile gives thread t request tile * SD_TILE + r * SD_BLOCK + t, so a
 * wave holds 64 neighbouring requests and a tile is SD_PER * SD_WAVES = 16
 * segments of one wave each, in request order.  Three launches:
 *   1. hist: per tile the count per class, to row c of the class-major
 *      classes x tiles table.
 *   2. scan (one workgroup): dv_carry_scan over the table, row after row --
 *      any number of tiles, in pieces with a carry.  Entry (c, t) becomes the
 *      position in perm of tile t's first request of class c; the first entry
 *      of every row, and n, are class_first.
 *   3. write: a tile recomputes its classes; a request's rank inside its class
 *      and segment is the popcount of the class's ballot over the lanes below,
 *      the segments' class counts meet in LDS, and one thread per class turns
 *      them into positions.  Then perm, slot and the seven gathers.
 * A wave does not take one ballot per class (23 rounds): it peels the classes
 * it holds -- the first remaining lane's class, its ballot, those lanes off --
 * which is as many rounds as the wave has distinct classes.
 *
 * The gather is done by the write kernel, not by a second kernel through perm:
 * the write kernel has the request index and the position in registers, its
 * loads are coalesced, and its stores fall into at most 23 streams that each
 * advance densely through the tile -- the lanes of one class in a wave write
 * neighbouring entries.  A second kernel would read perm back and turn the
 * seven coalesced loads into scattered ones for the sake of coalesced stores,
 * at the price of a fourth launch.
 *
 * lzf_gpu_request_stitch: one lane per request, grid-stride, runs
 * lzf_stitch_entry (lzf_request.h, the one copy of the seven rules); the first
 * workgroup writes the 64 bytes of the code area.
 *
 * The kernels are helpers of this translation unit, not part of the library's
 * routed kernel set: they have internal linkage (anonymous namespace).
 */
#include "lzf_store_dev.h"
#include "../../include/lzf_gpu.h"

#define DP_NC   ((uint32_t)LZF_RQ_NCLASS)
#define DP_SEGS (SD_PER * SD_WAVES)       /* the tile's wave-sized segments, in request order */
#define DP_STITCH_GRID 512u               /* the stitch's workgroups at most (lzf_launch_request_stitch) */

namespace {

/* the class of request i, SD_NONE past the batch's end */
__device__ inline uint32_t dp_class(const LzfBucketArgs &a, uint64_t i)
{
    return i < a.n ? lzf_request_class_of(a.op[i], a.status[i]) : SD_NONE;
}

/* The wave's classes peeled one at a time; the same trip count in every lane.
 * each(c, m): class c -- wave-uniform -- is held by the lanes of ballot m */
template <typename F>
__device__ inline void dp_peel(uint32_t cls, F each)
{
    uint64_t left = __ballot(cls != SD_NONE);
    while (left) {
        const int l = __ffsll((unsigned long long)left) - 1;
        const uint32_t c = (uint32_t)__shfl((int)cls, l, 64);
        const uint64_t m = __ballot(cls == c);
        each(c, m);
        left &= ~m;
    }
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_bucket_hist_kernel(LzfBucketArgs a, uint32_t ntile)
{
    __shared__ uint32_t s_cnt[DP_NC];
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x < DP_NC) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * SD_TILE;
#pragma unroll
    for (uint32_t r = 0; r < SD_PER; r++) {
        const uint32_t cls = dp_class(a, base + r * SD_BLOCK + threadIdx.x);
        dp_peel(cls, [&](uint32_t c, uint64_t m) {
            if (lane == 0u) atomicAdd(&s_cnt[c], (uint32_t)__popcll(m));
        });
    }
    __syncthreads();
    if (threadIdx.x < DP_NC) a.w_table[(uint64_t)threadIdx.x * ntile + blockIdx.x] = s_cnt[threadIdx.x];
}

/* one workgroup: the exclusive scan of the class-major table in place, and
 * class_first from the rows' first entries */
__global__ __launch_bounds__(SD_BLOCK) void lzf_bucket_scan_kernel(LzfBucketArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t total = dv_carry_scan<SD_WAVES>(a.w_table, DP_NC * ntile, sw);
    __syncthreads();                                          /* the rows' first entries, written by other threads */
    if (threadIdx.x < DP_NC) a.class_first[threadIdx.x] = (uint32_t)a.w_table[(uint64_t)threadIdx.x * ntile];
    if (threadIdx.x == DP_NC) a.class_first[DP_NC] = (uint32_t)total;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_bucket_write_kernel(LzfBucketArgs a, uint32_t ntile)
{
    __shared__ uint32_t s_seg[DP_SEGS][DP_NC];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t j = threadIdx.x; j < DP_SEGS * DP_NC; j += SD_BLOCK) (&s_seg[0][0])[j] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * SD_TILE;
    uint32_t cls[SD_PER], rank[SD_PER];
#pragma unroll
    for (uint32_t r = 0; r < SD_PER; r++) {
        cls[r] = dp_class(a, base + r * SD_BLOCK + threadIdx.x);
        const uint32_t mine = cls[r], seg = r * SD_WAVES + wave;
        uint32_t rk = 0u;
        dp_peel(mine, [&](uint32_t c, uint64_t m) {
            if (mine == c) rk = (uint32_t)__popcll(m & below);
            if (lane == 0u) s_seg[seg][c] = (uint32_t)__popcll(m);
        });
        rank[r] = rk;
    }
    __syncthreads();
    if (threadIdx.x < DP_NC) {                                /* counts -> positions in perm, segment after segment */
        uint32_t x = (uint32_t)a.w_table[(uint64_t)threadIdx.x * ntile + blockIdx.x];
        for (uint32_t g = 0; g < DP_SEGS; g++) {
            const uint32_t cnt = s_seg[g][threadIdx.x];
            s_seg[g][threadIdx.x] = x;
            x += cnt;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < SD_PER; r++) {
        if (cls[r] == SD_NONE) continue;
        const uint64_t i = base + r * SD_BLOCK + threadIdx.x;
        const uint32_t j = s_seg[r * SD_WAVES + wave][cls[r]] + rank[r];
        if (j >= a.n) continue;                               /* op / status changed under the call: nothing past the arrays */
        a.perm[j] = (uint32_t)i;
        a.slot[i] = j;
        a.b_op[j] = a.op[i];
        a.b_status[j] = a.status[i];
        a.b_key_off[j] = a.key_off[i];
        a.b_key_len[j] = a.key_len[i];
        a.b_val_off[j] = a.val_off[i];
        a.b_val_len[j] = a.val_len[i];
        a.b_num[j] = a.num[i];
    }
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_request_stitch_kernel(LzfStitchArgs a)
{
    if (blockIdx.x == 0u && threadIdx.x < LZF_STITCH_CODES)
        a.replies[a.code_base + threadIdx.x] = lzf_stitch_code_byte(threadIdx.x);
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t cnt[LZF_ST_NTALLY];
#pragma unroll
    for (uint32_t c = 0; c < LZF_ST_NTALLY; c++) cnt[c] = 0u;
    for (uint64_t b = (uint64_t)blockIdx.x * SD_BLOCK; b < a.n; b += step) {
        const uint64_t k = b + threadIdx.x;
        const uint32_t t = k < a.n ? lzf_stitch_entry(a, k) : SD_NONE;
        cnt[LZF_ST_ARENA] += sd_count(t == LZF_ST_ARENA);
        cnt[LZF_ST_CODE] += sd_count(t == LZF_ST_CODE || t == LZF_ST_BAD);
        cnt[LZF_ST_CLOSE] += sd_count(t == LZF_ST_CLOSE);
        cnt[LZF_ST_HOST] += sd_count(t == LZF_ST_HOST);
        cnt[LZF_ST_BAD] += sd_count(t == LZF_ST_BAD);
    }
#pragma unroll
    for (uint32_t c = 0; c < LZF_ST_NTALLY; c++) sd_leader_add(a.result + c, (uint64_t)cnt[c]);
}

}  // namespace

hipError_t lzf_launch_request_bucket(const LzfBucketArgs &a, hipStream_t s)
{
    const uint32_t nt = sd_tiles(a.n);
    hipLaunchKernelGGL(lzf_bucket_hist_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_bucket_scan_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_bucket_write_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a, nt);
    return hipGetLastError();
}

/* At most DP_STITCH_GRID workgroups, a quarter of a sweep's SD_GRID: every wave
 * ends with up to five atomic adds to the same five result words, and on 1 M
 * requests the kernel took 373 us with 2048 workgroups and 118 us with 512
 * (profiles/r19/dispatch/), the time following the number of waves */
hipError_t lzf_launch_request_stitch(const LzfStitchArgs &a, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(a.result, 0, LZF_ST_NTALLY * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const uint32_t grid = sd_sweep_grid(a.n);
    hipLaunchKernelGGL(lzf_request_stitch_kernel, dim3(grid < DP_STITCH_GRID ? grid : DP_STITCH_GRID), dim3(SD_BLOCK), 0, s,
                       a);
    return hipGetLastError();
}
