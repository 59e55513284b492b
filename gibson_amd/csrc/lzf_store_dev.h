/*
 * lzf_store_dev.h -- the toolkit of the device store's kernels (lzf_frame.hip,
 * lzf_store.hip, lzf_mget.hip, lzf_kidx.hip, lzf_ops.hip, lzf_mset.hip,
 * lzf_meta.hip, lzf_reply.hip, lzf_renumber.hip, lzf_request.hip, lzf_dispatch.hip,
 * lzf_order.hip), over the byte helpers of
 * lzf_dev.h, the geometry of lzf_store_layout.h and the request grammar of
 * lzf_request.h, where the number parse lives.  One copy of each: the pad and the "no
 * entry" class; the ballot count, the 64-bit wave sum and the wave leader's
 * add; the block scan and the carry scan over tile sums; put32, the reply
 * header, the wave copy and the decode batch; and the per-item rules over the
 * item view (LzfItems): age, TTL, validity, lock, the entry class, the number
 * parse and the reply code of an entry status.  What is new here is sd_*; the
 * dv_*, mg_* and lzf_* names are older than this file.  The size-class rule
 * (lzf_size_class_of) stays in lzf_dev.h, where lzf_mixed.hip reads it.
 */
#ifndef GIBSON_AMD_LZF_STORE_DEV_H
#define GIBSON_AMD_LZF_STORE_DEV_H

#include "lzf_dev.h"
#include "lzf_store_layout.h"
#include "lzf_request.h"

#define SD_PAD  0xFFFFFFFFu               /* an index-list entry that names no item */
#define SD_NONE 0xFFu                     /* no entry: the class of a lane past the list's end */

/* ---- counting ------------------------------------------------------------------ */

/* how many lanes of the wave say yes; the same in every lane */
__device__ inline uint32_t sd_count(bool x)
{
    return (uint32_t)__popcll(__ballot(x));
}

/* the wave's sum of one u64 per lane, in every lane */
__device__ inline uint64_t sd_wave_sum(uint64_t x)
{
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d, 64);
        x += ((uint64_t)hi << 32) | lo;
    }
    return x;
}

/* the wave's largest of one u64 per lane, in every lane */
__device__ inline uint64_t sd_wave_max(uint64_t x)
{
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, d, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), d, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        x = o > x ? o : x;
    }
    return x;
}

/* one lane's u64, in every lane */
__device__ inline uint64_t sd_lane_u64(uint64_t x, int lane)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, lane, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), lane, 64);
    return ((uint64_t)hi << 32) | lo;
}

/* the wave's leader adds the wave's count x, if any, to a result word: one
 * atomic add per wave and counter.  x is the same in every lane */
__device__ inline void sd_leader_add(uint64_t *word, uint64_t x)
{
    if ((threadIdx.x & 63u) == 0u && x) atomicAdd((unsigned long long *)word, (unsigned long long)x);
}

__device__ inline void sd_leader_add(uint32_t *word, uint32_t x)
{
    if ((threadIdx.x & 63u) == 0u && x) atomicAdd(word, x);
}

/* ---- scans --------------------------------------------------------------------- */

__device__ inline uint64_t dv_shfl_up64(uint64_t x, int d)
{
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, d, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

/* block-wide exclusive scan of one u64 per thread, for a workgroup of WAVES
 * waves: an inclusive wave scan, then the totals of the waves before this one;
 * sw: WAVES words of LDS */
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
 * a per-tile write); the total, in every thread.  16 M items are 16 384 tiles,
 * and at one tile per thread the 64 dependent rounds took 50 us of the
 * select's 240 (profiles/r10/mget/) */
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

/* ---- bytes --------------------------------------------------------------------- */

__device__ inline void sd_put32(uint8_t *p, uint32_t x)               /* little-endian, any alignment */
{
    p[0] = (uint8_t)x; p[1] = (uint8_t)(x >> 8); p[2] = (uint8_t)(x >> 16); p[3] = (uint8_t)(x >> 24);
}

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

/* gbClientEnqueueData's reply header (src/net.c:1162-1205):
 * [i16 code][u8 encoding][u32 size] */
#define SD_HDR 7u
__device__ inline void sd_put_header(uint8_t *f, int code, uint8_t enc, uint32_t size)
{
    f[0] = (uint8_t)code; f[1] = (uint8_t)((uint32_t)code >> 8);     /* src/net.c:1185 */
    f[2] = enc;
    sd_put32(f + 3, size);
}

/* len bytes from s to d by one wave: 16 bytes per lane (unaligned loads and
 * stores), then the tail byte by byte */
__device__ inline void sd_wave_copy(uint8_t *d, const uint8_t *s, uint32_t len, uint32_t lane)
{
    const uint32_t whole = len & ~15u;
    for (uint32_t j = lane * 16u; j < whole; j += 64u * 16u) {
        const uint4 x = dv_ld16(s + j);
        __builtin_memcpy(d + j, &x, 16);
    }
    for (uint32_t j = whole + lane; j < len; j += 64u) d[j] = s[j];
}

/* the decoder's batch over gathered entries: value k is in_len[k] bytes at
 * in + in_off[k], decoded to out + out_off[k] unless skip[k] */
static inline LzfBatch sd_decode_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint8_t *out,
                                       const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                                       int32_t *err, uint32_t count, uint32_t max_len, const uint8_t *skip)
{
    return LzfBatch{in, in_off, in_len, out, out_off, out_cap, out_len, err, count, max_len, skip};
}

/* ---- the per-item rules ---------------------------------------------------------- */

/* now - t in two's complement, as the reference's time_t arithmetic wraps */
__device__ inline int64_t mg_age(int64_t now, int64_t t)
{
    return (int64_t)((uint64_t)now - (uint64_t)t);
}

/* the TTL rule of src/query.c:186-189: a positive ttl that the item's age has
 * reached.  The item's time is read for a positive ttl only: an item without a
 * TTL costs no read of item_time */
__device__ inline bool mg_ttl_reached(int32_t ttl, int64_t now, const int64_t *item_time, uint64_t i)
{
    return ttl > 0 && mg_age(now, item_time[i]) >= (int64_t)ttl;
}

enum { MG_DEAD = 0, MG_EXPIRED = 1, MG_VALID = 2 };

/* The validity rule of every index-list operator (gbIsItemStillValid,
 * src/query.c:204-224, over the rule of src/query.c:186-189): entry i is dead
 * when it is out of range or already NULL, expired when its ttl is positive
 * and reached -- the caller then nulls enc[i], the device form of tr_remove --
 * and valid otherwise.  No time arrays: nothing expires */
__device__ inline int mg_validity(uint32_t i, const LzfItems &it)
{
    if (i >= it.count || it.enc[i] == (uint8_t)LZF_ENC_NULL) return MG_DEAD;
    if (it.item_ttl && mg_ttl_reached(it.item_ttl[i], it.now, it.item_time, i)) return MG_EXPIRED;
    return MG_VALID;
}

/* The lock rule (gbItemIsLocked, src/query.c:171-178) for an in-range item i:
 * locked for good at -1, otherwise while now - time is below the lock time.
 * No lock array: nothing is locked */
__device__ inline bool mg_locked(uint32_t i, const LzfItems &it)
{
    if (!it.item_lock) return false;
    const int64_t lock = it.item_lock[i];
    const int64_t age = mg_age(it.now, it.item_time[i]);   /* read beside the lock, not after it */
    return lock == -1 || age < lock;
}

/* The class of entry i under an operator that refuses a locked item: DEAD,
 * then the lock and the expiry in the operator's order, DONE for an item it
 * may apply to.  Lock first -- the lock is tested on an expired item too --
 * is gbMultiSetCallback (src/query.c:493 before :496), gbMultiDelCallback
 * (:789-792) and gbMultiIncDecCallback (:910, :913); expiry first is the
 * single-key gbQueryIncDecHandler (:853, :858).  Reads only */
__device__ inline uint32_t sd_entry_class(uint32_t i, const LzfItems &it, bool expiry_first)
{
    const int v = mg_validity(i, it);
    if (v == MG_DEAD) return LZF_ENT_DEAD;
    if (expiry_first && v == MG_EXPIRED) return LZF_ENT_EXPIRED;
    if (mg_locked(i, it)) return LZF_ENT_LOCKED;
    return v == MG_EXPIRED ? LZF_ENT_EXPIRED : LZF_ENT_DONE;
}

/* the number parse, gbQueryParseLong: lzf_parse_long of lzf_request.h, beside
 * the request grammar that needs it on the host too */

/* the reply code of an operator's entry status: lzf_reply_code_of of
 * lzf_request.h, beside the stitch rule that needs it on the host too */

#endif
