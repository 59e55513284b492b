/*
 * lzf_dev.h -- device helpers shared by the compress kernels (lzf_cand.hip):
 * unaligned byte-window loads that never touch memory past a value's end,
 * and the reference's slot function; and the block-wide scan of the store's
 * kernels (lzf_store.hip, lzf_mget.hip) with the carry scan over tile sums
 * (lzf_mset.hip, lzf_meta.hip); and the per-item rules the index-list
 * operators share (lzf_mget.hip, lzf_ops.hip, lzf_mset.hip, lzf_meta.hip):
 * validity, lock, number parse; and the size-class rule (lzf_mixed.hip,
 * lzf_reply.hip) and the reply code of an entry status (lzf_reply.hip).
 */
#ifndef GIBSON_AMD_LZF_DEV_H
#define GIBSON_AMD_LZF_DEV_H

#include "lzf_internal.h"
#include "../../include/lzf_gpu.h"

__device__ __forceinline__ uint4 dv_ld16(const uint8_t *p)          /* unaligned */
{
    uint4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

__device__ __forceinline__ uint2 dv_ld8(const uint8_t *p)
{
    uint2 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

__device__ __forceinline__ uint32_t dv_ld4(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

/* bytes [p, p + avail), avail < 16, zero beyond: never touches p + avail */
__device__ __forceinline__ uint4 dv_ld16_tail(const uint8_t *p, uint32_t avail)
{
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++)
        if (k < avail) w[k >> 2] |= (uint32_t)p[k] << (8u * (k & 3u));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint4 dv_ld16_safe(const uint8_t *p, uint32_t avail)
{
    return avail >= 16u ? dv_ld16(p) : dv_ld16_tail(p, avail);
}

/* 8 bytes at p, zero past avail (never touches p + avail) */
__device__ __forceinline__ uint2 dv_ld8_safe(const uint8_t *p, uint32_t avail)
{
    if (avail >= 8u) return dv_ld8(p);
    const uint4 t = dv_ld16_tail(p, avail);
    return make_uint2(t.x, t.y);
}

/* 8 bytes at src + pp, zero past n, with one unconditional 8-byte load
 * (needs n >= 8): near the end the load is moved back to n - 8 and the
 * bytes shifted into place; pp past n gives zeros.  Branch-free, so the
 * compiler can count such loads in flight instead of draining them. */
__device__ __forceinline__ uint2 dv_ld8_clamped(const uint8_t *src, uint32_t n, uint32_t pp)
{
    const uint32_t at = pp + 8u <= n ? pp : n - 8u;
    const uint2 v = dv_ld8(src + at);
    const uint32_t sh = pp - at;
    const uint64_t x = ((uint64_t)v.y << 32) | v.x;
    const uint64_t y = sh < 8u ? x >> (8u * sh) : 0ull;
    return make_uint2((uint32_t)y, (uint32_t)(y >> 32));
}

/* the 16-byte load address for bytes from pp in a value of n >= 16 bytes:
 * moved back to n - 16 near the end, so the load stays inside the value */
__device__ __forceinline__ uint32_t dv_at16(uint32_t n, uint32_t pp) { return pp + 16u <= n ? pp : n - 16u; }

/* v shifted down by sh (0 .. 15) bytes, zeros in */
__device__ __forceinline__ uint4 dv_shr16(uint4 v, uint32_t sh)
{
    uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
    const bool big = sh >= 8u;
    lo = big ? hi : lo;
    hi = big ? 0ull : hi;
    const uint32_t b = 8u * (sh & 7u);
    lo = b ? (lo >> b) | (hi << (64u - b)) : lo;
    hi >>= b;
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

/* slot(p) of src/lzf_c.c:47-57 (VERY_FAST, HLOG 16) from b[p..p+2] = tri */
__device__ __forceinline__ uint32_t dv_slot(uint32_t tri)
{
    const uint32_t b0 = tri & 0xFFu, b1 = (tri >> 8) & 0xFFu, b2 = (tri >> 16) & 0xFFu;
    return (((b0 << 8) | b1) - 5u * ((b1 << 8) | b2)) & 0xFFFFu;
}

/* index of the first differing byte of two 16-byte pieces, 16 if equal */
__device__ __forceinline__ uint32_t dv_first_diff(uint4 a, uint4 b)
{
    uint32_t x;
    if ((x = a.x ^ b.x)) return (uint32_t)__builtin_ctz(x) >> 3;
    if ((x = a.y ^ b.y)) return 4u + ((uint32_t)__builtin_ctz(x) >> 3);
    if ((x = a.z ^ b.z)) return 8u + ((uint32_t)__builtin_ctz(x) >> 3);
    if ((x = a.w ^ b.w)) return 12u + ((uint32_t)__builtin_ctz(x) >> 3);
    return 16u;
}

__device__ __forceinline__ uint32_t dv_sel4(uint4 v, uint32_t i)
{
    return i == 0u ? v.x : i == 1u ? v.y : i == 2u ? v.z : v.w;
}

/* store exactly len (<= 16) bytes of v at p (unaligned) */
__device__ __forceinline__ void dv_st_exact(uint8_t *p, uint4 v, uint32_t len)
{
    if (len >= 16u) {
        __builtin_memcpy(p, &v, 16);
        return;
    }
    uint32_t a = v.x, b = v.y, c = v.z, d = v.w;
    if (len & 8u) {
        uint2 t = make_uint2(a, b);
        __builtin_memcpy(p, &t, 8);
        p += 8;
        a = c;
        b = d;
    }
    if (len & 4u) {
        __builtin_memcpy(p, &a, 4);
        p += 4;
        a = b;
    }
    if (len & 2u) {
        const uint16_t t = (uint16_t)a;
        __builtin_memcpy(p, &t, 2);
        p += 2;
        a >>= 16;
    }
    if (len & 1u) *p = (uint8_t)a;
}

__device__ inline uint64_t dv_shfl_up64(uint64_t x, int d)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, d, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

/* block-wide exclusive scan of one u64 per thread (the scans of lzf_store.hip
 * and lzf_mget.hip), for a workgroup of WAVES waves: an inclusive wave scan,
 * then the totals of the waves before this one; sw: WAVES words of LDS */
template <uint32_t WAVES>
__device__ inline uint64_t dv_block_excl(uint64_t x, uint64_t *sw, uint64_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = x;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = dv_shfl_up64(inc, d);
        if (lane >= (uint32_t)d) inc += o;
    }
    if (lane == 63u) sw[wave] = inc;
    __syncthreads();
    uint64_t before = 0ull, all = 0ull;
    for (uint32_t w = 0; w < WAVES; w++) {
        if (w < wave) before += sw[w];
        all += sw[w];
    }
    __syncthreads();
    *total = all;
    return before + inc - x;
}

/* one workgroup of WAVES waves: the exclusive scan of the n sums at v in place,
 * in pieces of 64 * WAVES * DV_CARRY_PER with a running carry, a thread taking
 * DV_CARRY_PER neighbouring sums (the carry step between a per-tile reduce and
 * a per-tile write, lzf_mset.hip, lzf_meta.hip); the total, in every thread */
#define DV_CARRY_PER 8u
template <uint32_t WAVES>
__device__ inline uint64_t dv_carry_scan(uint64_t *v, uint32_t n, uint64_t *sw)
{
    uint64_t run = 0ull;
    for (uint64_t c = 0; c < n; c += 64u * WAVES * DV_CARRY_PER) {
        const uint64_t first = c + threadIdx.x * DV_CARRY_PER;
        uint64_t x[DV_CARRY_PER], s = 0ull;
#pragma unroll
        for (uint32_t j = 0; j < DV_CARRY_PER; j++) {
            x[j] = first + j < n ? v[first + j] : 0ull;
            s += x[j];
        }
        uint64_t tot;
        uint64_t o = run + dv_block_excl<WAVES>(s, sw, &tot);
#pragma unroll
        for (uint32_t j = 0; j < DV_CARRY_PER; j++) {
            if (first + j < n) v[first + j] = o;
            o += x[j];
        }
        run += tot;
    }
    return run;
}

enum { MG_DEAD = 0, MG_EXPIRED = 1, MG_VALID = 2 };

/* The validity rule of every index-list operator (gbIsItemStillValid,
 * src/query.c:204-224, over the rule of src/query.c:186-189): entry i is dead
 * when it is out of range or already NULL, expired when its ttl is positive
 * and reached -- the caller then nulls enc[i], the device form of tr_remove --
 * and valid otherwise.  No time arrays: nothing expires */
__device__ inline int mg_validity(uint32_t i, uint32_t count, const uint8_t *enc, const int64_t *item_time,
                                  const int32_t *item_ttl, int64_t now)
{
    if (i >= count || enc[i] == (uint8_t)LZF_ENC_NULL) return MG_DEAD;
    if (item_ttl) {
        const int32_t t = item_ttl[i];
        /* now - time in two's complement, as the reference's time_t arithmetic wraps */
        const int64_t age = (int64_t)((uint64_t)now - (uint64_t)item_time[i]);
        if (t > 0 && age >= (int64_t)t) return MG_EXPIRED;
    }
    return MG_VALID;
}

/* The lock rule (gbItemIsLocked, src/query.c:171-178) for an in-range item i:
 * locked for good at -1, otherwise while now - time is below the lock time.
 * No lock array: nothing is locked */
__device__ inline bool mg_locked(uint32_t i, const int64_t *item_time, const int64_t *item_lock, int64_t now)
{
    if (!item_lock) return false;
    const int64_t lock = item_lock[i];
    const int64_t age = (int64_t)((uint64_t)now - (uint64_t)item_time[i]);
    return lock == -1 || age < lock;
}

/* gbQueryParseLong (src/query.c:39-76), quirk for quirk: a first byte '0'
 * yields 0 whatever follows; a leading '-' negates and a lone "-" is 0; every
 * other byte must be a digit; no length limit, the accumulation n * 10 + d and
 * the negation modulo 2^64 (what the reference's x86-64 build computes where C
 * leaves the signed overflow undefined).  len == 0: not a number (the
 * reference asserts vlen > 0) */
__host__ __device__ inline int lzf_parse_long(const uint8_t *v, uint32_t len, int64_t *out)
{
    if (!len) return 0;
    if (v[0] == (uint8_t)'0') {
        *out = 0;
        return 1;
    }
    const uint32_t neg = v[0] == (uint8_t)'-' ? 1u : 0u;
    uint64_t n = 0ull;
    for (uint32_t i = neg; i < len; i++) {
        const uint32_t d = (uint32_t)v[i] - (uint32_t)'0';
        if (d > 9u) return 0;
        n = n * 10ull + d;
    }
    *out = (int64_t)(neg ? 0ull - n : n);
    return 1;
}

/* The size classes.  Compress, by in_len: the edges of the routing's value
 * sizes (lane_min_count and LANE_DEFAULT_MAX of lzf_api.cpp; window64 past
 * 64 KiB).  Decompress, by out_cap: tokpar64 up to 4 KiB, tokpar64-far up to
 * CD_FAR_MAX (16 KiB), the pipe past it (lzf_launch_decompress).  A length
 * past the caller's bound is refused: class LZF_GPU_NCLASS.  The only place
 * the edges are written: lzf_decode_class_edge names the decode ones. */
#define LZF_DECODE_NCLASS 3u
#define LZF_DECODE_EDGE0  4096u
#define LZF_DECODE_EDGE1  16384u
static __host__ __device__ inline uint32_t lzf_size_class_of(uint32_t len, uint32_t bound, int kind)
{
    if (len > bound) return (uint32_t)LZF_GPU_NCLASS;
    if (kind == LZF_GPU_KIND_COMPRESS)
        return len <= 4096u ? 0u : len <= 8192u ? 1u : len <= 16384u ? 2u : len <= 65536u ? 3u : 4u;
    return len <= LZF_DECODE_EDGE0 ? 0u : len <= LZF_DECODE_EDGE1 ? 1u : 2u;
}

/* the largest out_cap of decode class c; the last class has none */
static inline uint32_t lzf_decode_class_edge(uint32_t c)
{
    return c == 0u ? LZF_DECODE_EDGE0 : c == 1u ? LZF_DECODE_EDGE1 : 0xFFFFFFFFu;
}

/* The reply code of an operator's entry status, the single-key replies of
 * gbQueryIncDecHandler and its kin (src/query.c:853-886): REPL_VAL for an
 * entry the operator applied to, the error code of the others.  One rule for
 * the reply kernels and lzf_host_reply_code */
__host__ __device__ inline int lzf_reply_code_of(int ent_status)
{
    switch (ent_status) {
    case LZF_ENT_DONE:
    case LZF_ENT_CONVERTED: return LZF_REPL_VAL;
    case LZF_ENT_DEAD:
    case LZF_ENT_EXPIRED: return LZF_REPL_ERR_NOT_FOUND;
    case LZF_ENT_LOCKED: return LZF_REPL_ERR_LOCKED;
    case LZF_ENT_NAN:
    case LZF_ENT_UNCHANGED: return LZF_REPL_ERR_NAN;
    default: return LZF_REPL_ERR;
    }
}

#endif
