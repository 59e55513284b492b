/*
 * lzf_dev.h -- the codec kernels' one toolkit (lzf_lane.hip, lzf_lane_diag.hip,
 * lzf_cand.hip, lzf_stream.hip, lzf_wparse.hip, lzf_compress.hip,
 * lzf_decompress.hip): unaligned byte-window loads that never touch memory
 * past a value's end, the reference's slot function, the agreement codes of
 * the cand words and records, the wave fence and scan, and the lane-ordered
 * LDS exchange; and the size-class rule of the mixed-size batches
 * (lzf_mixed.hip), which the reply kernels share.  The store's kernels take
 * all of it through their own toolkit, lzf_store_dev.h.  The parses' output
 * cursor is lzf_emit.h.
 *
 * Two helpers exist in two forms, dv_ld16_tail / dv_ld16_tail_w and dv_sel4 /
 * dv_sel4_bits.  Each pair computes the same value; the difference is the
 * code the compiler makes of it, and each product kernel keeps the form its
 * instruction stream was measured with (profiles/r16/toolkit/isa.md).
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

/* dv_ld16_tail with one accumulator per word instead of an indexed array: the
 * same bytes, other code.  lzf_parse_lane_kernel depends on this form (with
 * the array form it grows by 6 % of its instructions), lzf_cand.hip's kernels
 * on the other; lzf_lane_diag.hip's kernels keep this one. */
__device__ __forceinline__ uint4 dv_ld16_tail_w(const uint8_t *p, uint32_t avail)
{
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) {
        const uint32_t b = k < avail ? (uint32_t)p[k] : 0u;
        const uint32_t s = 8u * (k & 3u);
        if (k < 4u) w0 |= b << s;
        else if (k < 8u) w1 |= b << s;
        else if (k < 12u) w2 |= b << s;
        else w3 |= b << s;
    }
    return make_uint4(w0, w1, w2, w3);
}

__device__ __forceinline__ uint4 dv_ld16_safe_w(const uint8_t *p, uint32_t avail)
{
    return avail >= 16u ? dv_ld16(p) : dv_ld16_tail_w(p, avail);
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

/* bytes p, p+1, p+2 (p + 3 <= n) in bits 0-23, with one 4-byte load moved
 * back inside the value near its end */
__device__ __forceinline__ uint32_t dv_tri(const uint8_t *src, uint32_t n, uint32_t p)
{
    if (n >= 4u) {
        const uint32_t at = p + 4u <= n ? p : n - 4u;
        return dv_ld4(src + at) >> (8u * (p - at));
    }
    return (uint32_t)src[p] | ((uint32_t)src[p + 1u] << 8) | ((uint32_t)src[p + 2u] << 16);
}

/* slot(p) of src/lzf_c.c:47-57 (VERY_FAST, HLOG 16) from b[p..p+2] = tri */
__device__ __forceinline__ uint32_t dv_slot(uint32_t tri)
{
    const uint32_t b0 = tri & 0xFFu, b1 = (tri >> 8) & 0xFFu, b2 = (tri >> 16) & 0xFFu;
    return (((b0 << 8) | b1) - 5u * ((b1 << 8) | b2)) & 0xFFFFu;
}

/* bijective 16-bit mix of the slot: bucket = high bits, identity = low bits */
__device__ __forceinline__ uint32_t dv_mix(uint32_t s) { return (s * 40503u) & 0xFFFFu; }

/* The agreement code of a cand word or record, bits 13-15 over the 13-bit
 * offset p - q - 1 (src/lzf_c.c:151-158 and the parses' walks):
 *   0     no earlier position with p's slot inside p's window (or only
 *         position 0, which is never a ref: src/lzf_c.c:155 `ref > in_data`)
 *   1     same slot, the three bytes differ (slot collision)
 *   2..6  the bytes agree for exactly code + 1 bytes (3..7)
 *   7     the bytes agree for >= 8 bytes */
#define DV_CODE_DIFF 1u
#define DV_CODE_LONG 7u
__device__ __forceinline__ uint32_t dv_code(uint32_t k)     /* of k equal bytes */
{
    return k < 3u ? DV_CODE_DIFF : (k >= 8u ? DV_CODE_LONG : k - 1u);
}

/* rel of p to the next link r of a chain, from its rel to q and q's code for
 * r.  rel: the codes 0..7, plus 8 (the first 3 bytes agree, length unknown)
 * and 9 (unknown).  3-byte agreements combine: both agree => p~r agree,
 * exactly one => they differ in the first 3 bytes.  exact (a compile-time
 * choice of each parse): exact agreements combine too -- p~q exactly a bytes
 * and q~r exactly b != a give p~r exactly min(a, b) (the first mismatch of the
 * shorter one is a mismatch of p~r, the bytes before it agree in all three);
 * one exact and one >= 8 give the exact one; both >= 8 give >= 8.  A word's
 * agreement is capped at its own remaining bytes, which are more than p's, so
 * the rule holds at the value's end too. */
__device__ __forceinline__ uint32_t dv_comb(uint32_t rel, uint32_t code, bool exact)
{
    if (rel == 9u) return 9u;
    const bool e1 = rel >= 2u, e2 = code >= 2u;
    if (!(e1 && e2)) return (e1 != e2) ? DV_CODE_DIFF : 9u;
    if (exact && rel <= DV_CODE_LONG) {            /* rel exact (2..6) or >= 8 (7); code is 2..7 */
        if (rel != code) return rel < code ? rel : code;
        if (rel == DV_CODE_LONG) return DV_CODE_LONG;
    }
    return 8u;
}

/* v_ffbl_b32: the lowest set bit's index, 0xFFFFFFFF for 0 (defined here,
 * unlike __builtin_ctz) */
__device__ __forceinline__ uint32_t dv_ffbl(uint32_t x)
{
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
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

/* dv_sel4 by selects on the index bits: three v_cndmask, where the compare
 * chain may become branches around a divergent index.  The same word, other
 * code: lzf_parse_lane_kernel depends on this form, lzf_parse_rec_kernel on
 * the chain. */
__device__ __forceinline__ uint32_t dv_sel4_bits(uint4 v, uint32_t i)
{
    const uint32_t a = (i & 1u) ? v.y : v.x, b = (i & 1u) ? v.w : v.z;
    return (i & 2u) ? b : a;
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

/* Order-preserving LDS hand-off between the lanes of one wave: LDS ops of one
 * wave execute in order, so only the compiler must not move memory operations
 * across this point. */
__device__ __forceinline__ void dv_wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

/* Inclusive prefix sum over the 64 lanes (DPP row shifts + row broadcasts). */
__device__ __forceinline__ uint32_t dv_wave_incl_sum(uint32_t x)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false); /* row_shr:1 */
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false); /* row_shr:2 */
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false); /* row_shr:4 */
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false); /* row_shr:8 */
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false); /* row_bcast:15 */
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false); /* row_bcast:31 */
    return x;
}

/* LDS byte address of a __shared__ object */
__device__ __forceinline__ uint32_t dv_lds_addr(const void *p)
{
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}

/* The lane-ordered 16-bit exchange on an exact table in LDS: ds_mskor_rtn_b32
 * replaces the slot's 16-bit half (mask m, data d, dword address a) and
 * returns the old dword.  The LDS runs one wave's same-address operations in
 * lane order (tools/lds_mskor_order.hip; checked at run time by
 * lzf_selfcheck.hip), so each lane gets the latest earlier same-slot position
 * -- the table's or an earlier lane's -- and the highest lane's stays; and one
 * wave's LDS operations execute in order, so windows exchanged in position
 * order update the table in position order.  DV_MSKOR / DV_MSKOR_IN: operand
 * i of an asm group, taken from element o + i of a, m and d. */
#define DV_MSKOR(i_) "ds_mskor_rtn_b32 %" #i_ ", %[a" #i_ "], %[m" #i_ "], %[d" #i_ "]\n\t"
#define DV_MSKOR_IN(i_, o_) [a##i_] "v"(a[(o_) + i_]), [m##i_] "v"(m[(o_) + i_]), [d##i_] "v"(d[(o_) + i_])
/* a block's 15 windows, issued in window (= position) order with one wait at
 * the end.  Three asm groups of five: the later groups take the earlier
 * results as in-out operands, so nothing reads a result before the single
 * wait.  (lzf_cand.hip's kt_xchg5 waits per group of five: its table wave's
 * register budget.) */
__device__ __forceinline__ void dv_xchg15(uint32_t (&r)[15], const uint32_t (&a)[15], const uint32_t (&m)[15],
                                          const uint32_t (&d)[15])
{
    asm volatile(DV_MSKOR(0) DV_MSKOR(1) DV_MSKOR(2) DV_MSKOR(3) DV_MSKOR(4)
                 : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3]), "=&v"(r[4])
                 : DV_MSKOR_IN(0, 0), DV_MSKOR_IN(1, 0), DV_MSKOR_IN(2, 0), DV_MSKOR_IN(3, 0), DV_MSKOR_IN(4, 0)
                 : "memory");
    asm volatile(DV_MSKOR(0) DV_MSKOR(1) DV_MSKOR(2) DV_MSKOR(3) DV_MSKOR(4)
                 : "=&v"(r[5]), "=&v"(r[6]), "=&v"(r[7]), "=&v"(r[8]), "=&v"(r[9]),
                   "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4])
                 : DV_MSKOR_IN(0, 5), DV_MSKOR_IN(1, 5), DV_MSKOR_IN(2, 5), DV_MSKOR_IN(3, 5), DV_MSKOR_IN(4, 5)
                 : "memory");
    asm volatile(DV_MSKOR(0) DV_MSKOR(1) DV_MSKOR(2) DV_MSKOR(3) DV_MSKOR(4) "s_waitcnt lgkmcnt(0)"
                 : "=&v"(r[10]), "=&v"(r[11]), "=&v"(r[12]), "=&v"(r[13]), "=&v"(r[14]),
                   "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]),
                   "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), "+v"(r[8]), "+v"(r[9])
                 : DV_MSKOR_IN(0, 10), DV_MSKOR_IN(1, 10), DV_MSKOR_IN(2, 10), DV_MSKOR_IN(3, 10), DV_MSKOR_IN(4, 10)
                 : "memory");
}

/* The size classes.  Compress, by in_len: the edges of the routing's value
 * sizes (lane_min_count and LANE_DEFAULT_MAX of lzf_api.cpp; window64 past
 * 64 KiB).  Decompress, by out_cap: tokpar64 up to 4 KiB, tokpar64-far up to
 * CD_FAR_MAX (16 KiB), the pipe past it (lzf_launch_decompress).  A length
 * past the caller's bound is refused: class LZF_GPU_NCLASS.  The only place
 * the edges are used: LZF_DECODE_EDGE* (lzf_internal.h) and
 * lzf_decode_class_edge name the decode ones. */
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

#endif
