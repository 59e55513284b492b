/*
 * lzf_mixed.hip -- size classes for mixed-size batches: the class rule, a
 * stable multi-class partition of a batch's lengths on the device (and its
 * host twin), and the descriptor gather / result scatter through the
 * partition's permutation.
 *
 * The batch calls pick one kernel plan per batch from one bound, so a single
 * large value moves a whole batch to the plan its size needs (DESIGN.md
 * §4.0).  The mixed calls (lzf_gpu_compress_mixed / lzf_gpu_decompress_mixed,
 * lzf_api.cpp) partition the batch by the size edges that routing already
 * uses and run every class as a batch of its own.  The rule is
 * lzf_size_class_of (lzf_dev.h, the only place the edges are written); this
 * file holds the kernels that apply it; the codec kernels are untouched.
 *
 * Partition, three launches on one stream (no workgroup waits for another):
 *   1. lzf_mixed_hist_kernel: a workgroup of 4 waves takes a tile of 2048
 *      lengths and writes its per-class count and maximum to row c of the
 *      classes x tiles tables.
 *   2. lzf_mixed_scan_kernel: one workgroup reduces each table row to the
 *      class totals and maxima, then runs an exclusive scan over the count
 *      table laid out class-major (row after row), in pieces of 1024 entries
 *      with a running carry -- any number of tiles.  Entry (c, t) becomes the
 *      position in perm of tile t's first value of class c.
 *   3. lzf_mixed_perm_kernel: each tile ranks its values inside their class
 *      (ballot + popcount of the lanes below within a wave; the 8 rounds x
 *      4 waves of a tile get their offsets from a 32-step scan in LDS) and
 *      writes perm.  The order inside a class is the original order.
 * The kernels are helpers of this translation unit, not part of the library's
 * kernel set: they have internal linkage (anonymous namespace).
 */
#include <errno.h>

#include "lzf_dev.h"
#include "../../include/lzf_gpu.h"

#define MX_NC      (LZF_GPU_NCLASS + 1)   /* the classes and "refused" */
#define MX_THREADS 256u
#define MX_ROUNDS  8u
#define MX_TILE    (MX_THREADS * MX_ROUNDS)
#define MX_WAVES   (MX_THREADS / 64u)
#define MX_SEGS    (MX_ROUNDS * MX_WAVES)

/* lzf_size_class_of, the class rule and the only place the edges are written:
 * lzf_dev.h */

static inline uint32_t mx_tiles(uint32_t count)
{
    return (uint32_t)(((uint64_t)count + MX_TILE - 1u) / MX_TILE);
}

namespace {

__device__ inline uint32_t mx_wave_max(uint32_t v)
{
    for (int d = 32; d; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ inline uint32_t mx_wave_sum(uint32_t v)
{
    for (int d = 32; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

/* tile_cnt / tile_max: [MX_NC][ntiles] */
__global__ __launch_bounds__(MX_THREADS) void lzf_mixed_hist_kernel(const uint32_t *__restrict__ len, uint32_t count,
                                                                    uint32_t bound, int kind, uint32_t ntiles,
                                                                    uint32_t *__restrict__ tile_cnt,
                                                                    uint32_t *__restrict__ tile_max)
{
    __shared__ uint32_t s_cnt[MX_WAVES][MX_NC], s_max[MX_WAVES][MX_NC];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * MX_TILE;
    uint32_t cnt[MX_NC], mx[MX_NC];
#pragma unroll
    for (uint32_t c = 0; c < MX_NC; c++) cnt[c] = mx[c] = 0u;
#pragma unroll
    for (uint32_t r = 0; r < MX_ROUNDS; r++) {
        const uint64_t i = base + r * MX_THREADS + tid;
        const bool live = i < count;
        const uint32_t n = live ? len[i] : 0u;
        const uint32_t cls = live ? lzf_size_class_of(n, bound, kind) : (uint32_t)MX_NC;
#pragma unroll
        for (uint32_t c = 0; c < MX_NC; c++) {
            const bool m = cls == c;
            cnt[c] += (uint32_t)__popcll(__ballot(m));
            mx[c] = (m && n > mx[c]) ? n : mx[c];
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < MX_NC; c++) {
        const uint32_t m = mx_wave_max(mx[c]);
        if (lane == 0u) {
            s_cnt[wave][c] = cnt[c];
            s_max[wave][c] = m;
        }
    }
    __syncthreads();
    if (tid < MX_NC) {
        uint32_t n = 0u, m = 0u;
        for (uint32_t w = 0; w < MX_WAVES; w++) {
            n += s_cnt[w][tid];
            m = s_max[w][tid] > m ? s_max[w][tid] : m;
        }
        tile_cnt[(uint64_t)tid * ntiles + blockIdx.x] = n;
        tile_max[(uint64_t)tid * ntiles + blockIdx.x] = m;
    }
}

/* one workgroup: class totals and maxima, then the exclusive scan of the
 * class-major count table in place */
__global__ __launch_bounds__(MX_THREADS) void lzf_mixed_scan_kernel(uint32_t ntiles, uint32_t *__restrict__ tile_cnt,
                                                                    const uint32_t *__restrict__ tile_max,
                                                                    uint32_t *__restrict__ class_count,
                                                                    uint32_t *__restrict__ class_max)
{
    __shared__ uint32_t s_a[MX_WAVES], s_b[MX_WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t c = 0; c < MX_NC; c++) {
        uint32_t n = 0u, m = 0u;
        for (uint32_t t = tid; t < ntiles; t += MX_THREADS) {
            n += tile_cnt[(uint64_t)c * ntiles + t];
            const uint32_t v = tile_max[(uint64_t)c * ntiles + t];
            m = v > m ? v : m;
        }
        n = mx_wave_sum(n);
        m = mx_wave_max(m);
        if (lane == 0u) {
            s_a[wave] = n;
            s_b[wave] = m;
        }
        __syncthreads();
        if (tid == 0u) {
            uint32_t tn = 0u, tm = 0u;
            for (uint32_t w = 0; w < MX_WAVES; w++) {
                tn += s_a[w];
                tm = s_b[w] > tm ? s_b[w] : tm;
            }
            class_count[c] = tn;
            class_max[c] = tm;
        }
        __syncthreads();
    }
    /* every thread takes 4 consecutive entries of a 1024-entry piece; all
     * sums stay below count, so 32 bits hold them */
    const uint64_t total = (uint64_t)MX_NC * ntiles;
    uint32_t carry = 0u;
    for (uint64_t p = 0; p < total; p += 4u * MX_THREADS) {
        const uint64_t j = p + 4u * tid;
        uint32_t v[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) v[q] = j + q < total ? tile_cnt[j + q] : 0u;
        const uint32_t mine = v[0] + v[1] + v[2] + v[3];
        uint32_t inc = mine;                        /* inclusive scan in the wave */
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
            if (lane >= (uint32_t)d) inc += o;
        }
        if (lane == 63u) s_a[wave] = inc;
        __syncthreads();
        uint32_t before = carry, all = 0u;
        for (uint32_t w = 0; w < MX_WAVES; w++) {
            if (w < wave) before += s_a[w];
            all += s_a[w];
        }
        uint32_t x = before + inc - mine;
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) {
            if (j + q < total) tile_cnt[j + q] = x;
            x += v[q];
        }
        carry += all;
        __syncthreads();
    }
}

/* tile_base: the scanned count table */
__global__ __launch_bounds__(MX_THREADS) void lzf_mixed_perm_kernel(const uint32_t *__restrict__ len, uint32_t count,
                                                                    uint32_t bound, int kind, uint32_t ntiles,
                                                                    const uint32_t *__restrict__ tile_base,
                                                                    uint32_t *__restrict__ perm)
{
    __shared__ uint32_t s_seg[MX_SEGS][MX_NC];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * MX_TILE;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t cls[MX_ROUNDS], rank[MX_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < MX_ROUNDS; r++) {
        const uint64_t i = base + r * MX_THREADS + tid;
        const bool live = i < count;
        cls[r] = live ? lzf_size_class_of(len[live ? i : 0u], bound, kind) : (uint32_t)MX_NC;
        uint32_t mine = 0u;
        rank[r] = 0u;
#pragma unroll
        for (uint32_t c = 0; c < MX_NC; c++) {
            const uint64_t b = __ballot(cls[r] == c);
            if (lane == c) mine = (uint32_t)__popcll(b);
            if (cls[r] == c) rank[r] = (uint32_t)__popcll(b & below);
        }
        if (lane < MX_NC) s_seg[r * MX_WAVES + wave][lane] = mine;
    }
    __syncthreads();
    if (tid < MX_NC) {
        uint32_t x = tile_base[(uint64_t)tid * ntiles + blockIdx.x];
        for (uint32_t g = 0; g < MX_SEGS; g++) {
            const uint32_t n = s_seg[g][tid];
            s_seg[g][tid] = x;
            x += n;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < MX_ROUNDS; r++) {
        const uint64_t i = base + r * MX_THREADS + tid;
        if (cls[r] < MX_NC) perm[s_seg[r * MX_WAVES + wave][cls[r]] + rank[r]] = (uint32_t)i;
    }
}

/* the four descriptor arrays into class-contiguous copies: entry k is value
 * perm[k] */
__global__ __launch_bounds__(MX_THREADS) void lzf_mixed_gather_kernel(
    const uint32_t *__restrict__ perm, uint32_t count, const uint64_t *__restrict__ in_off,
    const uint32_t *__restrict__ in_len, const uint64_t *__restrict__ out_off, const uint32_t *__restrict__ out_cap,
    uint64_t *__restrict__ c_in_off, uint32_t *__restrict__ c_in_len, uint64_t *__restrict__ c_out_off,
    uint32_t *__restrict__ c_out_cap)
{
    const uint64_t step = (uint64_t)gridDim.x * MX_THREADS;
    for (uint64_t k = (uint64_t)blockIdx.x * MX_THREADS + threadIdx.x; k < count; k += step) {
        const uint32_t i = perm[k];
        c_in_off[k] = in_off[i];
        c_in_len[k] = in_len[i];
        c_out_off[k] = out_off[i];
        c_out_cap[k] = out_cap[i];
    }
}

/* the results back to the caller's order; the refused values (the last
 * class_count[LZF_GPU_NCLASS] entries of perm) get out_len 0 and err EINVAL */
__global__ __launch_bounds__(MX_THREADS) void lzf_mixed_scatter_kernel(const uint32_t *__restrict__ perm,
                                                                       uint32_t count,
                                                                       const uint32_t *__restrict__ class_count,
                                                                       const uint32_t *__restrict__ c_out_len,
                                                                       const int32_t *__restrict__ c_err,
                                                                       uint32_t *__restrict__ out_len,
                                                                       int32_t *__restrict__ err)
{
    const uint64_t taken = (uint64_t)count - class_count[LZF_GPU_NCLASS];
    const uint64_t step = (uint64_t)gridDim.x * MX_THREADS;
    for (uint64_t k = (uint64_t)blockIdx.x * MX_THREADS + threadIdx.x; k < count; k += step) {
        const uint32_t i = perm[k];
        out_len[i] = k < taken ? c_out_len[k] : 0u;
        if (err) err[i] = k < taken ? c_err[k] : (int32_t)EINVAL;
    }
}

uint32_t mx_flat_grid(uint32_t count)
{
    const uint64_t g = ((uint64_t)count + MX_THREADS - 1u) / MX_THREADS;
    return (uint32_t)(g < 65536u ? g : 65536u);
}

}  // namespace

size_t lzf_partition_work_bytes(uint32_t count)
{
    return 2u * (size_t)MX_NC * mx_tiles(count) * sizeof(uint32_t);
}

hipError_t lzf_launch_size_partition(const uint32_t *len, uint32_t count, uint32_t bound, int kind, uint32_t *perm,
                                     uint32_t *class_count, uint32_t *class_max, void *work, hipStream_t s)
{
    const uint32_t ntiles = mx_tiles(count);
    uint32_t *tile_cnt = (uint32_t *)work, *tile_max = tile_cnt + (size_t)MX_NC * ntiles;
    hipLaunchKernelGGL(lzf_mixed_hist_kernel, dim3(ntiles), dim3(MX_THREADS), 0, s, len, count, bound, kind, ntiles,
                       tile_cnt, tile_max);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_mixed_scan_kernel, dim3(1), dim3(MX_THREADS), 0, s, ntiles, tile_cnt, tile_max,
                       class_count, class_max);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_mixed_perm_kernel, dim3(ntiles), dim3(MX_THREADS), 0, s, len, count, bound, kind, ntiles,
                       tile_cnt, perm);
    return hipGetLastError();
}

hipError_t lzf_launch_mixed_gather(const uint32_t *perm, uint32_t count, const uint64_t *in_off,
                                   const uint32_t *in_len, const uint64_t *out_off, const uint32_t *out_cap,
                                   uint64_t *c_in_off, uint32_t *c_in_len, uint64_t *c_out_off, uint32_t *c_out_cap,
                                   hipStream_t s)
{
    hipLaunchKernelGGL(lzf_mixed_gather_kernel, dim3(mx_flat_grid(count)), dim3(MX_THREADS), 0, s, perm, count,
                       in_off, in_len, out_off, out_cap, c_in_off, c_in_len, c_out_off, c_out_cap);
    return hipGetLastError();
}

hipError_t lzf_launch_mixed_scatter(const uint32_t *perm, uint32_t count, const uint32_t *class_count,
                                    const uint32_t *c_out_len, const int32_t *c_err, uint32_t *out_len, int32_t *err,
                                    hipStream_t s)
{
    hipLaunchKernelGGL(lzf_mixed_scatter_kernel, dim3(mx_flat_grid(count)), dim3(MX_THREADS), 0, s, perm, count,
                       class_count, c_out_len, c_err, out_len, err);
    return hipGetLastError();
}

extern "C" {

int lzf_gpu_size_class(uint32_t len, int kind)
{
    if (kind != LZF_GPU_KIND_COMPRESS && kind != LZF_GPU_KIND_DECOMPRESS) return LZF_GPU_EARG;
    return (int)lzf_size_class_of(len, 0xFFFFFFFFu, kind);
}

uint64_t lzf_gpu_size_partition_work_size(uint32_t count)
{
    return lzf_partition_work_bytes(count) + 16u;
}

int lzf_gpu_size_partition(const uint32_t *len, uint32_t count, uint32_t bound, int kind, uint32_t *perm,
                           uint32_t *class_count, uint32_t *class_max, void *work, void *stream)
{
    if (!count || !len || !perm || !class_count || !class_max || !work) return LZF_GPU_EARG;
    if (kind != LZF_GPU_KIND_COMPRESS && kind != LZF_GPU_KIND_DECOMPRESS) return LZF_GPU_EARG;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || !lzf_device_ok(dev)) return LZF_GPU_ENODEV;
    return lzf_launch_size_partition(len, count, bound, kind, perm, class_count, class_max, work,
                                     (hipStream_t)stream) == hipSuccess
               ? LZF_GPU_OK
               : LZF_GPU_ELAUNCH;
}

/* the same partition in plain C++ (a counting sort): no HIP call */
int lzf_host_size_partition(const uint32_t *len, uint32_t count, uint32_t bound, int kind, uint32_t *perm,
                            uint32_t *class_count, uint32_t *class_max)
{
    if (!count || !len || !perm || !class_count || !class_max) return LZF_GPU_EARG;
    if (kind != LZF_GPU_KIND_COMPRESS && kind != LZF_GPU_KIND_DECOMPRESS) return LZF_GPU_EARG;
    for (uint32_t c = 0; c < MX_NC; c++) class_count[c] = class_max[c] = 0u;
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t c = lzf_size_class_of(len[i], bound, kind);
        class_count[c]++;
        if (len[i] > class_max[c]) class_max[c] = len[i];
    }
    uint32_t at[MX_NC], x = 0u;
    for (uint32_t c = 0; c < MX_NC; c++) {
        at[c] = x;
        x += class_count[c];
    }
    for (uint32_t i = 0; i < count; i++) perm[at[lzf_size_class_of(len[i], bound, kind)]++] = i;
    return LZF_GPU_OK;
}

}  // extern "C"
