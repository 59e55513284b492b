/*
 * lzf_kidx.hip -- the device key index: an exact-key map from key bytes to an
 * item index of the device store, as an open-addressing hash table in HBM
 * (include/lzf_gpu.h).  Insert is tr_insert plus gbDestroyItem(old)
 * (src/query.c:418-422) for a batch of items, lookup is tr_find_node for a
 * batch of query keys.
 *
 * The slot.  One 64-bit word: the upper 32 bits of the key's hash (the tag),
 * then the item index.  All ones is the empty slot -- no item has index
 * 0xFFFFFFFF -- so a memset with 0xFF clears the table.  Key bytes are never
 * copied: a slot whose tag matches is confirmed against the store's keys /
 * key_off / key_len of the item it names.  A probe therefore costs one
 * scattered read when the tag differs (a wrong occupant leaves there), and
 * three dependent ones -- slot, descriptor, key bytes -- when it matches.
 * home = the hash's low bits, then home + 1, ... modulo slots.
 *
 * Two invariants carry everything below.  A slot never returns to empty
 * except by a clear, and the key a slot stands for never changes: an occupant
 * is only ever replaced by an item with the same key bytes.  So a chain never
 * breaks, and a key sits in at most one slot -- two claimers of one key walk
 * the same chain, and the second finds the first's slot before any empty one.
 *
 * insert, three launches, no workgroup waiting for another:
 *   1. decide (one thread): refuse the batch as a whole when *used + n passes
 *      3/4 of the slots, judged on *used before any claim; status and the
 *      zeroed result.  The two launches behind it do nothing on FULL.
 *   2. claim: every live batch item walks its chain.  An empty slot is claimed
 *      by compare-and-swap.  A slot holding the same key is taken over by CAS
 *      unless its occupant is a live batch item with a higher index: a batch
 *      item beats any occupant from outside the batch and any lower batch
 *      item, so the holder only ever rises and the highest batch index ends
 *      up there whatever the order of the attempts.  The one thread whose CAS
 *      removes an outside occupant nulls it (replaced).  A failed CAS returns
 *      the slot's new word, which is judged again.  enc of a batch item is
 *      only read here, never written, so the judgement does not race.
 *   3. settle: with all claims visible, every live batch item looks its own
 *      key up; it is the mapping, or it is superseded and nulls itself.
 *
 * rebuild: the table and *used cleared on the stream, then the insert of
 * [0, count) with a decide of its own: a counting pass leaves the number of
 * items the claim will not skip in result[0], and FULL is judged on that, not
 * on count, so the dead tail a renumbering leaves costs no slot.  Claim and
 * settle are the insert's, unchanged.
 *
 * lookup: one thread per query key, one pass.
 *
 * The kernels are helpers of this translation unit, not part of the library's
 * routed kernel set: they have internal linkage (anonymous namespace).
 */
#include "lzf_store_dev.h"
#include "../../include/lzf_gpu.h"

/* the grid-stride geometry and the wave sum: lzf_store_dev.h */
#define KI_EMPTY 0xFFFFFFFFFFFFFFFFull
#define KI_MISS  0xFFFFFFFFu

/* the hash of a key: 8 bytes a step (little-endian words, read at any
 * alignment), the last 1-7 bytes as one more word, zero above them, the length
 * in the seed so that "a" and "a\0" differ */
__host__ __device__ inline uint64_t ki_seed(uint32_t len)
{
    return 0x9E3779B97F4A7C15ull ^ ((uint64_t)len * 0xC2B2AE3D27D4EB4Full);
}

__host__ __device__ inline uint64_t ki_mix(uint64_t h, uint64_t w)
{
    h = (h ^ w) * 0xFF51AFD7ED558CCDull;
    return h ^ (h >> 32);
}

__host__ __device__ inline uint64_t ki_finish(uint64_t h)
{
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 33);
}

/* the host's form: the definition */
static inline uint64_t ki_hash_host(const uint8_t *key, uint32_t len)
{
    uint64_t h = ki_seed(len);
    uint32_t j = 0;
    for (; j + 8u <= len; j += 8u) {
        uint64_t w;
        __builtin_memcpy(&w, key + j, 8);
        h = ki_mix(h, w);
    }
    if (j < len) {
        uint64_t w = 0ull;
        for (uint32_t t = 0; j + t < len; t++) w |= (uint64_t)key[j + t] << (8u * t);
        h = ki_mix(h, w);
    }
    return ki_finish(h);
}

namespace {

__device__ inline uint64_t ki_u64(uint2 v) { return ((uint64_t)v.y << 32) | v.x; }

/* the device's form, the same value from fewer loads -- every load of a wave
 * is up to 64 scattered requests, and a tail read byte by byte is up to 7
 * loads: 16 bytes a load, and the last 1-7 bytes out of the key's last 8, a
 * load that overlaps the words before it.  No byte outside [key, key + len)
 * is read.  Worth 2 % of a lookup while the result's adds still set its time
 * (profiles/r11/kidx/kidx_bench_wide_loads.json); not measured on its own
 * since */
__device__ inline uint64_t ki_hash(const uint8_t *key, uint32_t len)
{
    uint64_t h = ki_seed(len);
    uint32_t j = 0;
    for (; j + 16u <= len; j += 16u) {
        const uint4 v = dv_ld16(key + j);
        h = ki_mix(h, ki_u64(make_uint2(v.x, v.y)));
        h = ki_mix(h, ki_u64(make_uint2(v.z, v.w)));
    }
    if (j + 8u <= len) {
        h = ki_mix(h, ki_u64(dv_ld8(key + j)));
        j += 8u;
    }
    if (j < len) {
        const uint32_t r = len - j;                    /* 1 .. 7 */
        uint64_t w = 0ull;
        if (len >= 8u) {
            w = ki_u64(dv_ld8(key + len - 8u)) >> (8u * (8u - r));
        } else {                                       /* j == 0 */
            for (uint32_t t = 0; t < r; t++) w |= (uint64_t)key[t] << (8u * t);
        }
        h = ki_mix(h, w);
    }
    return ki_finish(h);
}

/* whether two keys of len bytes are equal; the pieces past the last whole one
 * by a load that ends at the key's end and overlaps the one before */
__device__ inline bool ki_same_key(const uint8_t *a, const uint8_t *b, uint32_t len)
{
    uint32_t j = 0;
    for (; j + 16u <= len; j += 16u)
        if (dv_first_diff(dv_ld16(a + j), dv_ld16(b + j)) != 16u) return false;
    if (j == len) return true;
    if (len >= 16u) return dv_first_diff(dv_ld16(a + len - 16u), dv_ld16(b + len - 16u)) == 16u;
    if (len >= 8u)
        return ki_u64(dv_ld8(a)) == ki_u64(dv_ld8(b)) && ki_u64(dv_ld8(a + len - 8u)) == ki_u64(dv_ld8(b + len - 8u));
    if (len >= 4u) return dv_ld4(a) == dv_ld4(b) && dv_ld4(a + len - 4u) == dv_ld4(b + len - 4u);
    for (; j < len; j++)
        if (a[j] != b[j]) return false;
    return true;
}

/* the workgroup's sums of three per-thread counts, valid on thread 0 (true
 * there): one atomic add per count and workgroup then goes to the result.
 * Per wave they were 16 384 adds per count for 1 M keys, all to one cache
 * line, and the adds, not the probes, set the call's time: a lookup of 1 M
 * present keys took 0.325 ms with them and takes 0.200 ms without
 * (profiles/r11/kidx/) */
__device__ inline bool ki_block_sums(uint64_t (&v)[3])
{
    __shared__ uint64_t sh[3][SD_WAVES];
    for (uint32_t c = 0; c < 3u; c++) {
        const uint64_t x = sd_wave_sum(v[c]);
        if ((threadIdx.x & 63u) == 0u) sh[c][threadIdx.x >> 6] = x;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return false;
    for (uint32_t c = 0; c < 3u; c++) {
        v[c] = 0ull;
        for (uint32_t w = 0; w < SD_WAVES; w++) v[c] += sh[c][w];
    }
    return true;
}

/* whether the occupant j of a slot whose tag matched stands for this key */
__device__ inline bool ki_occupant_is(const LzfKidxArgs &a, uint32_t j, const uint8_t *key, uint32_t len)
{
    return a.key_len[j] == len && ki_same_key(a.keys + a.key_off[j], key, len);
}

__global__ void lzf_kidx_decide_kernel(LzfKidxArgs a)
{
    const uint32_t bound = a.slots - a.slots / 4u;
    *a.status = (uint64_t)*a.used + a.n > bound ? (uint32_t)LZF_KIDX_FULL : (uint32_t)LZF_KIDX_OK;
    a.result[0] = a.result[1] = a.result[2] = a.result[3] = 0ull;
}

/* rebuild: the items of [0, count) the insert will not skip, into result[0],
 * which was zeroed on the stream before the launch; one add per workgroup */
__global__ __launch_bounds__(SD_BLOCK) void lzf_kidx_count_kernel(LzfKidxArgs a)
{
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t takes = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; i < a.n; i += step)
        if (a.enc[i] != (uint8_t)LZF_ENC_NULL && a.key_len[i]) takes++;
    uint64_t v[3] = {takes, 0ull, 0ull};
    if (!ki_block_sums(v)) return;
    if (v[0]) atomicAdd((unsigned long long *)&a.result[0], (unsigned long long)v[0]);
}

/* rebuild's decide: the table and *used were cleared on the stream, so FULL is
 * judged on the counted items alone, not on n -- a dead tail costs no slot */
__global__ void lzf_kidx_decide_counted_kernel(LzfKidxArgs a)
{
    const uint32_t bound = a.slots - a.slots / 4u;
    *a.status = a.result[0] > bound ? (uint32_t)LZF_KIDX_FULL : (uint32_t)LZF_KIDX_OK;
    a.result[0] = a.result[1] = a.result[2] = a.result[3] = 0ull;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_kidx_claim_kernel(LzfKidxArgs a)
{
    if (*a.status != (uint32_t)LZF_KIDX_OK) return;
    unsigned long long *table = (unsigned long long *)a.table;
    const uint32_t mask = a.slots - 1u;
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t claimed = 0u, replaced = 0u;
    for (uint64_t k = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; k < a.n; k += step) {
        const uint32_t i = a.first + (uint32_t)k, len = a.key_len[i];
        if (a.enc[i] == (uint8_t)LZF_ENC_NULL || !len) continue;
        const uint8_t *key = a.keys + a.key_off[i];
        const uint64_t h = ki_hash(key, len);
        const uint32_t tag = (uint32_t)(h >> 32);
        const unsigned long long want = ((unsigned long long)tag << 32) | i;
        uint32_t pos = (uint32_t)h & mask;
        bool done = false;
        /* at most `slots` slots, so the walk ends on any table contents */
        for (uint32_t seen = 0; !done && seen < a.slots; seen++, pos = (pos + 1u) & mask) {
            unsigned long long cur = __hip_atomic_load(&table[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (;;) {                    /* until this slot's word is settled for item i */
                if (cur == KI_EMPTY) {
                    const unsigned long long old = atomicCAS(&table[pos], KI_EMPTY, want);
                    if (old == KI_EMPTY) {
                        claimed++;
                        done = true;
                        break;
                    }
                    cur = old;
                    continue;
                }
                const uint32_t j = (uint32_t)cur;
                if ((uint32_t)(cur >> 32) != tag || j >= a.count) break;      /* a wrong occupant */
                if (j == i) {
                    done = true;          /* already indexed */
                    break;
                }
                if (!ki_occupant_is(a, j, key, len)) break;
                const bool in_batch = j - a.first < a.n;                       /* wraps high for j < first */
                if (in_batch && j > i && a.enc[j] != (uint8_t)LZF_ENC_NULL) {
                    done = true;          /* a higher batch item holds the key: i is superseded in settle */
                    break;
                }
                const unsigned long long old = atomicCAS(&table[pos], cur, want);
                if (old == cur) {
                    if (!in_batch && a.enc[j] != (uint8_t)LZF_ENC_NULL) {
                        a.enc[j] = (uint8_t)LZF_ENC_NULL;                      /* gbDestroyItem(old) */
                        replaced++;
                    }
                    done = true;
                    break;
                }
                cur = old;                /* another item of this key got in first */
            }
        }
    }
    uint64_t v[3] = {claimed, replaced, 0ull};
    if (!ki_block_sums(v)) return;
    if (v[0]) atomicAdd(a.used, (uint32_t)v[0]);
    if (v[1]) atomicAdd((unsigned long long *)&a.result[1], (unsigned long long)v[1]);
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_kidx_settle_kernel(LzfKidxArgs a)
{
    if (*a.status != (uint32_t)LZF_KIDX_OK) return;
    const uint64_t *table = (const uint64_t *)a.table;
    const uint32_t mask = a.slots - 1u;
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t mapped = 0u, superseded = 0u, skipped = 0u;
    for (uint64_t k = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; k < a.n; k += step) {
        const uint32_t i = a.first + (uint32_t)k, len = a.key_len[i];
        if (a.enc[i] == (uint8_t)LZF_ENC_NULL || !len) {
            skipped++;
            continue;
        }
        const uint8_t *key = a.keys + a.key_off[i];
        const uint64_t h = ki_hash(key, len);
        const uint32_t tag = (uint32_t)(h >> 32);
        uint32_t pos = (uint32_t)h & mask;
        for (uint32_t seen = 0; seen < a.slots; seen++, pos = (pos + 1u) & mask) {
            const uint64_t cur = table[pos];
            if (cur == KI_EMPTY) break;   /* not on a table that was cleared: the item stays as it is */
            const uint32_t j = (uint32_t)cur;
            if ((uint32_t)(cur >> 32) != tag || j >= a.count) continue;
            if (j == i) {
                mapped++;
                break;
            }
            if (!ki_occupant_is(a, j, key, len)) continue;
            a.enc[i] = (uint8_t)LZF_ENC_NULL;      /* only ever the item's own thread writes it */
            superseded++;
            break;
        }
    }
    uint64_t v[3] = {mapped, superseded, skipped};
    if (!ki_block_sums(v)) return;
    if (v[0]) atomicAdd((unsigned long long *)&a.result[0], (unsigned long long)v[0]);
    if (v[1]) atomicAdd((unsigned long long *)&a.result[2], (unsigned long long)v[1]);
    if (v[2]) atomicAdd((unsigned long long *)&a.result[3], (unsigned long long)v[2]);
}

/* result[] was zeroed on the stream before the launch */
__global__ __launch_bounds__(SD_BLOCK) void lzf_kidx_lookup_kernel(LzfKidxArgs a, const uint8_t *__restrict__ qkeys,
                                                                   const uint64_t *__restrict__ q_off,
                                                                   const uint32_t *__restrict__ q_len, uint32_t nq,
                                                                   uint32_t *__restrict__ idx)
{
    const uint64_t *table = (const uint64_t *)a.table;
    const uint32_t mask = a.slots - 1u;
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint64_t hits = 0ull, misses = 0ull, examined = 0ull;
    for (uint64_t k = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; k < nq; k += step) {
        const uint32_t len = q_len[k];
        uint32_t found = KI_MISS;
        if (len) {
            const uint8_t *key = qkeys + q_off[k];
            const uint64_t h = ki_hash(key, len);
            const uint32_t tag = (uint32_t)(h >> 32);
            uint32_t pos = (uint32_t)h & mask;
            for (uint32_t seen = 0; seen < a.slots; seen++, pos = (pos + 1u) & mask) {
                const uint64_t cur = table[pos];
                examined++;
                if (cur == KI_EMPTY) break;
                const uint32_t j = (uint32_t)cur;
                /* an index past the store is a wrong occupant and is never dereferenced */
                if ((uint32_t)(cur >> 32) != tag || j >= a.count) continue;
                if (!ki_occupant_is(a, j, key, len)) continue;
                if (a.enc[j] != (uint8_t)LZF_ENC_NULL) found = j;   /* a key sits in one slot: dead is a miss */
                break;
            }
        }
        idx[k] = found;
        if (found != KI_MISS) hits++;
        else misses++;
    }
    uint64_t v[3] = {hits, misses, examined};
    if (!ki_block_sums(v)) return;
    if (v[0]) atomicAdd((unsigned long long *)&a.result[0], (unsigned long long)v[0]);
    if (v[1]) atomicAdd((unsigned long long *)&a.result[1], (unsigned long long)v[1]);
    if (v[2]) atomicAdd((unsigned long long *)&a.result[2], (unsigned long long)v[2]);
}

}  // namespace

bool lzf_kidx_slots_ok(uint32_t slots)
{
    return slots >= 16u && slots <= 0x80000000u && !(slots & (slots - 1u));
}

uint64_t lzf_kidx_table_bytes(uint32_t slots) { return (uint64_t)slots * 8u; }

uint32_t lzf_kidx_home(const uint8_t *key, uint32_t len, uint32_t slots)
{
    return (uint32_t)ki_hash_host(key, len) & (slots - 1u);
}

hipError_t lzf_launch_kidx_insert(LzfKidxArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(lzf_kidx_decide_kernel, dim3(1), dim3(1), 0, s, a);
    hipLaunchKernelGGL(lzf_kidx_claim_kernel, dim3(sd_sweep_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_kidx_settle_kernel, dim3(sd_sweep_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}

/* first == 0 and n == count.  The counting word is result[0]: no work area */
hipError_t lzf_launch_kidx_rebuild(LzfKidxArgs &a, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(a.table, 0xFF, (size_t)lzf_kidx_table_bytes(a.slots), s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.used, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.result, 0, 4 * sizeof(uint64_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_kidx_count_kernel, dim3(sd_sweep_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_kidx_decide_counted_kernel, dim3(1), dim3(1), 0, s, a);
    hipLaunchKernelGGL(lzf_kidx_claim_kernel, dim3(sd_sweep_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_kidx_settle_kernel, dim3(sd_sweep_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t lzf_launch_kidx_lookup(LzfKidxArgs &a, const uint8_t *qkeys, const uint64_t *q_off, const uint32_t *q_len,
                                  uint32_t nq, uint32_t *idx, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(a.result, 0, 3 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_kidx_lookup_kernel, dim3(sd_sweep_grid(nq)), dim3(SD_BLOCK), 0, s, a, qkeys, q_off, q_len, nq, idx);
    return hipGetLastError();
}
