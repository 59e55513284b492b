/*
 * lzf_ops.hip -- the lock-aware index-list operators over the device store
 * (include/lzf_gpu.h): LOCK / MLOCK, UNLOCK / MUNLOCK, the lock-aware DEL /
 * MDEL, INC / DEC / MINC / MDEC, and the guard that refuses a SET on a locked
 * key.  With lzf_mget.hip they are the reference's operator table: each is the
 * callback of a tr_search (src/query.c:778-800, 898-940, 1015-1036, 1097-1114)
 * applied to an index list, one lane per entry, under the validity rule
 * (mg_validity) and the lock rule (mg_locked) of lzf_dev.h.
 *
 * mlock / munlock / mdel: one grid-stride pass over the list, as count and
 * mttl are; the counts by wave ballot, one atomic add per wave and counter.
 *
 * minc: a PLAIN item that parses as a number becomes a NUMBER item, whose 8
 * bytes need a place in the arena, and the call is refused as a whole when
 * they do not fit -- so nothing may be written before that is known.  Three
 * launches, no workgroup waiting for another:
 *   1. classify (read-only on the store): per entry its LZF_ENT_* class and
 *      its new number (a NUMBER's 8 bytes + delta, or the parsed bytes +
 *      delta) into the work area; per tile of the list its converted entries;
 *   2. scan: one workgroup's running scan of the tile counts; base =
 *      *store_used, the status, and on LZF_STORE_OK the new *store_used;
 *   3. apply (nothing on LZF_STORE_FULL): the entry's rank among the
 *      converted ones from the classes alone, then what its class says --
 *      enc nulled, the number stored in place or at base + 8 * rank,
 *      last_access, entry_status, entry_value -- and the six counts.
 * Thread t of a tile takes entries t * OP_PER .. + OP_PER, so the scan over
 * the threads is the scan over the list and the ranks are in list order.
 * Stored numbers sit at any alignment (the arena is dense): they are read and
 * written as 8 unaligned bytes, never by a 64-bit atomic.
 *
 * set_guard: one lane per new item of a SET batch, over the lookup's output.
 *
 * The kernels are helpers of this translation unit, not part of the library's
 * routed kernel set: they have internal linkage (anonymous namespace).
 */
#include "lzf_dev.h"
#include "../../include/lzf_gpu.h"

#define OP_BLOCK 256u
#define OP_PER   4u
#define OP_TILE  (OP_BLOCK * OP_PER)      /* entries per minc tile */
#define OP_WAVES (OP_BLOCK / 64u)
#define OP_GRID  2048u                    /* grid-stride kernels: 256 CUs x 8 workgroups */
#define OP_NONE  0xFFu                    /* no entry: a lane past the list's end */

static inline uint32_t op_tiles(uint32_t n)
{
    return (uint32_t)(((uint64_t)n + OP_TILE - 1u) / OP_TILE);
}

namespace {

enum { OP_MLOCK = 0, OP_MUNLOCK = 1, OP_MDEL = 2 };

/* state words of the minc work area */
enum { OP_BASE = 0, OP_FULL = 1 };

__device__ inline uint32_t op_count(bool x)
{
    return (uint32_t)__popcll(__ballot(x));
}

/* ---- mlock, munlock, mdel ----------------------------------------------------- */

/* gbMultiLockCallback (src/query.c:1015-1036), gbMultiUnlockCallback
 * (:1097-1114) and gbMultiDelCallback (:778-800) over the list.  Every lane of
 * a workgroup makes the same number of rounds.  result[0]: entries the
 * operator applied to, [1]: expired ones, [2] (not MUNLOCK): locked ones */
template <int OP>
__global__ __launch_bounds__(OP_BLOCK) void lzf_store_lock_kernel(LzfLockArgs a)
{
    const uint64_t step = (uint64_t)gridDim.x * OP_BLOCK;
    uint32_t done = 0u, expired = 0u, locked = 0u;
    for (uint64_t b = (uint64_t)blockIdx.x * OP_BLOCK; b < a.n; b += step) {
        const uint64_t k = b + threadIdx.x;
        uint32_t st = OP_NONE;
        if (k < a.n) {
            const uint32_t i = a.idx[k];
            const int v = mg_validity(i, a.count, a.enc, a.item_time, a.item_ttl, a.now);
            if (v == MG_DEAD) {
                st = LZF_ENT_DEAD;
            } else if (OP == OP_MDEL) {
                /* the lock is tested first, on an expired item too (:789-792) */
                if (mg_locked(i, a.item_time, a.item_lock, a.now)) st = LZF_ENT_LOCKED;
                else st = v == MG_EXPIRED ? LZF_ENT_EXPIRED : LZF_ENT_DONE;
                if (st != LZF_ENT_LOCKED) a.enc[i] = (uint8_t)LZF_ENC_NULL;
            } else if (v == MG_EXPIRED) {
                st = LZF_ENT_EXPIRED;
                a.enc[i] = (uint8_t)LZF_ENC_NULL;
            } else if (OP == OP_MUNLOCK) {
                st = LZF_ENT_DONE;
                a.item_lock[i] = 0;                       /* :1107-1108 */
                if (a.last_access) a.last_access[i] = a.now;
            } else if (mg_locked(i, a.item_time, a.item_lock, a.now)) {
                st = LZF_ENT_LOCKED;
            } else {
                st = LZF_ENT_DONE;
                a.item_time[i] = a.now;                   /* :1028-1030: the TTL clock restarts */
                if (a.last_access) a.last_access[i] = a.now;
                a.item_lock[i] = a.lock_time;
            }
            if (a.entry_status) a.entry_status[k] = (uint8_t)st;
        }
        done += op_count(st == LZF_ENT_DONE);
        expired += op_count(st == LZF_ENT_EXPIRED);
        if (OP != OP_MUNLOCK) locked += op_count(st == LZF_ENT_LOCKED);
    }
    if ((threadIdx.x & 63u) != 0u) return;
    if (done) atomicAdd((unsigned long long *)a.result, (unsigned long long)done);
    if (expired) atomicAdd((unsigned long long *)a.result + 1, (unsigned long long)expired);
    if (OP != OP_MUNLOCK && locked) atomicAdd((unsigned long long *)a.result + 2, (unsigned long long)locked);
}

/* ---- minc --------------------------------------------------------------------- */

/* whether [off, off + size) lies in [0, cap) */
__device__ inline bool op_in_arena(uint64_t off, uint64_t size, uint64_t cap)
{
    return off <= cap && size <= cap - off;
}

__device__ inline int64_t op_ld_i64(const uint8_t *p)               /* little-endian, any alignment */
{
    const uint2 v = dv_ld8(p);
    return (int64_t)(((uint64_t)v.y << 32) | v.x);
}

__device__ inline void op_st_i64(uint8_t *p, int64_t x)
{
    const uint2 v = make_uint2((uint32_t)(uint64_t)x, (uint32_t)((uint64_t)x >> 32));
    __builtin_memcpy(p, &v, 8);
}

/* the class of entry i and, for DONE and CONVERTED, its new number: the rule
 * of gbMultiIncDecCallback (src/query.c:898-940) or, single, of
 * gbQueryIncDecHandler (:853-886).  Reads only */
__device__ inline uint32_t op_minc_class(const LzfMincArgs &a, uint32_t i, int64_t *val)
{
    const int v = mg_validity(i, a.count, a.enc, a.item_time, a.item_ttl, a.now);
    if (v == MG_DEAD) return LZF_ENT_DEAD;
    if (a.single) {
        if (v == MG_EXPIRED) return LZF_ENT_EXPIRED;                                  /* :853 */
        if (mg_locked(i, a.item_time, a.item_lock, a.now)) return LZF_ENT_LOCKED;     /* :858 */
    } else {
        if (mg_locked(i, a.item_time, a.item_lock, a.now)) return LZF_ENT_LOCKED;     /* :910 */
        if (v == MG_EXPIRED) return LZF_ENT_EXPIRED;                                  /* :913 */
    }
    const uint8_t e = a.enc[i];
    const uint64_t off = a.val_off[i];
    const uint32_t size = a.val_size[i];
    if (e == (uint8_t)LZF_ENC_NUMBER) {
        /* a malformed item is not dereferenced */
        if (size != 8u || !op_in_arena(off, 8u, a.store_cap)) return LZF_ENT_NAN;
        *val = (int64_t)((uint64_t)op_ld_i64(a.store + off) + (uint64_t)a.delta);    /* :865, :920 */
        return LZF_ENT_DONE;
    }
    if (e == (uint8_t)LZF_ENC_PLAIN) {
        int64_t num;
        if (!size || !op_in_arena(off, size, a.store_cap) || !lzf_parse_long(a.store + off, size, &num))
            return LZF_ENT_NAN;                                                       /* :885, :936 */
        *val = (int64_t)((uint64_t)num + (uint64_t)a.delta);                          /* :871, :924 */
        return LZF_ENT_CONVERTED;
    }
    /* an LZF item: the callback falls through to return 1 (:939), the single
     * handler replies REPL_ERR_NAN (:885) */
    return a.single ? LZF_ENT_NAN : LZF_ENT_UNCHANGED;
}

__global__ __launch_bounds__(OP_BLOCK) void lzf_minc_classify_kernel(LzfMincArgs a)
{
    __shared__ uint64_t sw[OP_WAVES];
    const uint64_t first = (uint64_t)blockIdx.x * OP_TILE + threadIdx.x * OP_PER;
    uint64_t conv = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < OP_PER; j++) {
        const uint64_t k = first + j;
        if (k >= a.n) continue;
        int64_t val = 0;
        const uint32_t cls = op_minc_class(a, a.idx[k], &val);
        a.w_cls[k] = (uint8_t)cls;
        a.w_val[k] = val;
        conv += cls == LZF_ENT_CONVERTED;
    }
    uint64_t tot;
    (void)dv_block_excl<OP_WAVES>(conv, sw, &tot);
    if (threadIdx.x == 0u) a.w_tile[blockIdx.x] = tot;
}

/* one workgroup: the exclusive scan of the tile counts in place, in pieces of
 * OP_BLOCK * OP_CARRY_PER with a running carry (as the select's carry kernel),
 * and the call's decision */
#define OP_CARRY_PER 8u
__global__ __launch_bounds__(OP_BLOCK) void lzf_minc_scan_kernel(LzfMincArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[OP_WAVES];
    uint64_t run = 0ull;
    for (uint64_t c = 0; c < ntile; c += OP_BLOCK * OP_CARRY_PER) {
        const uint64_t first = c + threadIdx.x * OP_CARRY_PER;
        uint64_t v[OP_CARRY_PER], s = 0ull;
#pragma unroll
        for (uint32_t j = 0; j < OP_CARRY_PER; j++) {
            v[j] = first + j < ntile ? a.w_tile[first + j] : 0ull;
            s += v[j];
        }
        uint64_t tot;
        uint64_t o = run + dv_block_excl<OP_WAVES>(s, sw, &tot);
#pragma unroll
        for (uint32_t j = 0; j < OP_CARRY_PER; j++) {
            if (first + j < ntile) a.w_tile[first + j] = o;
            o += v[j];
        }
        run += tot;
    }
    if (threadIdx.x != 0u) return;
    /* run <= n < 2^32: 8 * run cannot wrap, the sum can */
    const uint64_t base = *a.store_used, end = base + 8ull * run;
    const bool full = end < base || end > a.store_cap;
    a.w_state[OP_BASE] = base;
    a.w_state[OP_FULL] = full ? 1ull : 0ull;
    *a.status = full ? LZF_STORE_FULL : LZF_STORE_OK;
    if (!full) *a.store_used = end;
}

__global__ __launch_bounds__(OP_BLOCK) void lzf_minc_apply_kernel(LzfMincArgs a)
{
    __shared__ uint64_t sw[OP_WAVES];
    if (a.w_state[OP_FULL]) return;                       /* refused: the same for every lane */
    const uint64_t first = (uint64_t)blockIdx.x * OP_TILE + threadIdx.x * OP_PER;
    uint32_t cls[OP_PER];
    uint64_t conv = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < OP_PER; j++) {
        cls[j] = first + j < a.n ? a.w_cls[first + j] : OP_NONE;
        conv += cls[j] == LZF_ENT_CONVERTED;
    }
    uint64_t tot;
    uint64_t rank = a.w_tile[blockIdx.x] + dv_block_excl<OP_WAVES>(conv, sw, &tot);
    const uint64_t base = a.w_state[OP_BASE];
    uint32_t done = 0u, expired = 0u, locked = 0u, nan = 0u, converted = 0u, unchanged = 0u;
#pragma unroll
    for (uint32_t j = 0; j < OP_PER; j++) {
        const uint64_t k = first + j;
        const uint32_t c = cls[j];
        if (c != OP_NONE) {
            const uint32_t i = a.idx[k];
            int64_t val = 0;
            if (c == LZF_ENT_EXPIRED) a.enc[i] = (uint8_t)LZF_ENC_NULL;
            /* every valid entry, a NAN one too: :861, :917 come before the value test */
            if (c == LZF_ENT_DONE || c == LZF_ENT_CONVERTED || c == LZF_ENT_NAN || c == LZF_ENT_UNCHANGED)
                if (a.last_access) a.last_access[i] = a.now;
            if (c == LZF_ENT_DONE) {
                val = a.w_val[k];
                op_st_i64(a.store + a.val_off[i], val);   /* its range was checked by the classify pass */
            } else if (c == LZF_ENT_CONVERTED) {
                val = a.w_val[k];
                const uint64_t slot = base + 8ull * rank++;   /* < store_cap: the scan's decision */
                op_st_i64(a.store + slot, val);
                a.val_off[i] = slot;
                a.val_size[i] = 8u;
                a.enc[i] = (uint8_t)LZF_ENC_NUMBER;
            }
            if (a.entry_status) a.entry_status[k] = (uint8_t)c;
            if (a.entry_value) a.entry_value[k] = val;
        }
        done += op_count(c == LZF_ENT_DONE);
        expired += op_count(c == LZF_ENT_EXPIRED);
        locked += op_count(c == LZF_ENT_LOCKED);
        nan += op_count(c == LZF_ENT_NAN);
        converted += op_count(c == LZF_ENT_CONVERTED);
        unchanged += op_count(c == LZF_ENT_UNCHANGED);
    }
    if ((threadIdx.x & 63u) != 0u) return;
    unsigned long long *r = (unsigned long long *)a.result;
    const uint32_t found = done + converted + unchanged;
    if (found) atomicAdd(r, (unsigned long long)found);
    if (expired) atomicAdd(r + 1, (unsigned long long)expired);
    if (locked) atomicAdd(r + 2, (unsigned long long)locked);
    if (nan) atomicAdd(r + 3, (unsigned long long)nan);
    if (converted) atomicAdd(r + 4, (unsigned long long)converted);
    if (unchanged) atomicAdd(r + 5, (unsigned long long)unchanged);
}

/* ---- set_guard ---------------------------------------------------------------- */

/* src/query.c:446-451: a SET on a key whose item is locked is refused.  New
 * item first + k, whose key the lookup found at occ[k]: an occupant outside
 * the batch that is not dead and is locked keeps the key, and the new item
 * dies.  No validity test, as in the reference.  The occupants read lie
 * outside [first, first + n), the items written inside it */
__global__ __launch_bounds__(OP_BLOCK) void lzf_store_set_guard_kernel(const uint32_t *__restrict__ occ, uint32_t first,
                                                                       uint32_t n, uint8_t *enc, uint32_t count,
                                                                       const int64_t *item_time,
                                                                       const int64_t *item_lock, int64_t now,
                                                                       uint8_t *refused, uint64_t *result)
{
    const uint64_t step = (uint64_t)gridDim.x * OP_BLOCK;
    uint32_t hits = 0u;
    for (uint64_t b = (uint64_t)blockIdx.x * OP_BLOCK; b < n; b += step) {
        const uint64_t k = b + threadIdx.x;
        bool refuse = false;
        if (k < n) {
            const uint32_t j = occ[k];
            const bool inside = j >= first && (uint64_t)j < (uint64_t)first + n;
            refuse = j < count && !inside && enc[j] != (uint8_t)LZF_ENC_NULL && mg_locked(j, item_time, item_lock, now);
            if (refuse) enc[first + k] = (uint8_t)LZF_ENC_NULL;
            if (refused) refused[k] = refuse ? 1u : 0u;
        }
        hits += op_count(refuse);
    }
    if ((threadIdx.x & 63u) == 0u && hits) atomicAdd((unsigned long long *)result, (unsigned long long)hits);
}

static inline uint32_t op_sweep_grid(uint64_t n)
{
    const uint64_t g = (n + OP_BLOCK - 1u) / OP_BLOCK;
    return (uint32_t)(g < OP_GRID ? g : OP_GRID);
}

template <int OP>
hipError_t op_launch_lock(const LzfLockArgs &a, uint32_t words, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(a.result, 0, words * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_store_lock_kernel<OP>, dim3(op_sweep_grid(a.n)), dim3(OP_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t lzf_launch_store_mlock(const LzfLockArgs &a, hipStream_t s)
{
    return op_launch_lock<OP_MLOCK>(a, 3u, s);
}

hipError_t lzf_launch_store_munlock(const LzfLockArgs &a, hipStream_t s)
{
    return op_launch_lock<OP_MUNLOCK>(a, 2u, s);
}

hipError_t lzf_launch_store_mdel(const LzfLockArgs &a, hipStream_t s)
{
    return op_launch_lock<OP_MDEL>(a, 3u, s);
}

uint64_t lzf_minc_work_bytes(uint32_t n)
{
    /* state (8 x u64) | the new numbers (i64) | tile counts (u64 per tile) |
     * the classes (u8); room to align the caller's pointer.  Below 2^36 */
    return 64u + (uint64_t)n * 9u + (uint64_t)op_tiles(n) * 8u + 16u;
}

void lzf_minc_carve(LzfMincArgs &a, void *work)
{
    uint8_t *w = (uint8_t *)(((uintptr_t)work + 7u) & ~(uintptr_t)7u);
    a.w_state = (uint64_t *)w;            w += 64;
    a.w_val = (int64_t *)w;               w += (size_t)a.n * 8;
    a.w_tile = (uint64_t *)w;             w += (size_t)op_tiles(a.n) * 8;
    a.w_cls = w;
}

hipError_t lzf_launch_store_minc(LzfMincArgs &a, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(a.result, 0, 6 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const uint32_t nt = op_tiles(a.n);
    hipLaunchKernelGGL(lzf_minc_classify_kernel, dim3(nt), dim3(OP_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_minc_scan_kernel, dim3(1), dim3(OP_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_minc_apply_kernel, dim3(nt), dim3(OP_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t lzf_launch_store_set_guard(const uint32_t *occ, uint32_t first, uint32_t n, uint8_t *enc, uint32_t count,
                                      const int64_t *item_time, const int64_t *item_lock, int64_t now,
                                      uint8_t *refused, uint64_t *result, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(result, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_store_set_guard_kernel, dim3(op_sweep_grid(n)), dim3(OP_BLOCK), 0, s, occ, first, n, enc,
                       count, item_time, item_lock, now, refused, result);
    return hipGetLastError();
}

int lzf_ops_parse_long(const uint8_t *v, uint32_t len, int64_t *out)
{
    return lzf_parse_long(v, len, out);
}
