/*
 * lzf_ops.hip -- the lock-aware index-list operators over the device store
 * (include/lzf_gpu.h): LOCK / MLOCK, UNLOCK / MUNLOCK, the lock-aware DEL /
 * MDEL, INC / DEC / MINC / MDEC, and the guard that refuses a SET on a locked
 * key.  With lzf_mget.hip they are the reference's operator table: each is the
 * callback of a tr_search (src/query.c:778-800, 898-940, 1015-1036, 1097-1114)
 * applied to an index list, one lane per entry, under the validity rule
 * (mg_validity), the lock rule (mg_locked) and their order (sd_entry_class)
 * of lzf_store_dev.h, whose geometry, counts and scans the kernels use.
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
 * Thread t of a tile takes entries t * SD_PER .. + SD_PER, so the scan over
 * the threads is the scan over the list and the ranks are in list order.
 * Stored numbers sit at any alignment (the arena is dense): they are read and
 * written as 8 unaligned bytes, never by a 64-bit atomic.
 *
 * set_guard: one lane per new item of a SET batch, over the lookup's output.
 *
 * The kernels are helpers of this translation unit, not part of the library's
 * routed kernel set: they have internal linkage (anonymous namespace).
 */
#include "lzf_store_dev.h"
#include "../../include/lzf_gpu.h"

namespace {

enum { OP_MLOCK = 0, OP_MUNLOCK = 1, OP_MDEL = 2 };

/* state words of the minc work area */
enum { OP_BASE = 0, OP_FULL = 1 };

/* ---- mlock, munlock, mdel ----------------------------------------------------- */

/* gbMultiLockCallback (src/query.c:1015-1036), gbMultiUnlockCallback
 * (:1097-1114) and gbMultiDelCallback (:778-800) over the list.  Every lane of
 * a workgroup makes the same number of rounds.  result[0]: entries the
 * operator applied to, [1]: expired ones, [2] (not MUNLOCK): locked ones */
template <int OP>
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_lock_kernel(LzfLockArgs a)
{
    const LzfItems &it = a.it;
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t done = 0u, expired = 0u, locked = 0u;
    for (uint64_t b = (uint64_t)blockIdx.x * SD_BLOCK; b < a.n; b += step) {
        const uint64_t k = b + threadIdx.x;
        uint32_t st = SD_NONE;
        if (k < a.n) {
            const uint32_t i = a.idx[k];
            if (OP == OP_MDEL) {
                /* the lock is tested first, on an expired item too (:789-792) */
                st = sd_entry_class(i, it, false);
                if (st == LZF_ENT_DONE || st == LZF_ENT_EXPIRED) it.enc[i] = (uint8_t)LZF_ENC_NULL;
            } else {
                const int v = mg_validity(i, it);
                if (v == MG_DEAD) {
                    st = LZF_ENT_DEAD;
                } else if (v == MG_EXPIRED) {
                    st = LZF_ENT_EXPIRED;
                    it.enc[i] = (uint8_t)LZF_ENC_NULL;
                } else if (OP == OP_MUNLOCK) {
                    st = LZF_ENT_DONE;
                    it.item_lock[i] = 0;                  /* :1107-1108 */
                    if (it.last_access) it.last_access[i] = it.now;
                } else if (mg_locked(i, it)) {
                    st = LZF_ENT_LOCKED;
                } else {
                    st = LZF_ENT_DONE;
                    it.item_time[i] = it.now;             /* :1028-1030: the TTL clock restarts */
                    if (it.last_access) it.last_access[i] = it.now;
                    it.item_lock[i] = a.lock_time;
                }
            }
            if (a.entry_status) a.entry_status[k] = (uint8_t)st;
        }
        done += sd_count(st == LZF_ENT_DONE);
        expired += sd_count(st == LZF_ENT_EXPIRED);
        if (OP != OP_MUNLOCK) locked += sd_count(st == LZF_ENT_LOCKED);
    }
    sd_leader_add(a.result, done);
    sd_leader_add(a.result + 1, expired);
    if (OP != OP_MUNLOCK) sd_leader_add(a.result + 2, locked);
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
    /* the encoding is read once, here, ahead of the class rule, whose own range test and read the compiler
     * then folds into these: read after the rule it is one more scattered load per entry, a tenth of the pass */
    if (i >= a.it.count) return LZF_ENT_DEAD;
    const uint8_t e = a.it.enc[i];
    /* single: the expiry (:853), then the lock (:858); else the lock (:910), then the expiry (:913) */
    const uint32_t c = sd_entry_class(i, a.it, a.single != 0);
    if (c != LZF_ENT_DONE) return c;
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

__global__ __launch_bounds__(SD_BLOCK) void lzf_minc_classify_kernel(LzfMincArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint64_t conv = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        const uint64_t k = first + j;
        if (k >= a.n) continue;
        int64_t val = 0;
        const uint32_t cls = op_minc_class(a, a.idx[k], &val);
        a.w_cls[k] = (uint8_t)cls;
        a.w_val[k] = val;
        conv += cls == LZF_ENT_CONVERTED;
    }
    uint64_t tot;
    (void)dv_block_excl<SD_WAVES>(conv, sw, &tot);
    if (threadIdx.x == 0u) a.w_tile[blockIdx.x] = tot;
}

/* one workgroup: the exclusive scan of the tile counts in place, and the call's
 * decision */
__global__ __launch_bounds__(SD_BLOCK) void lzf_minc_scan_kernel(LzfMincArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t run = dv_carry_scan<SD_WAVES>(a.w_tile, ntile, sw);
    if (threadIdx.x != 0u) return;
    /* run <= n < 2^32: 8 * run cannot wrap, the sum can */
    const uint64_t base = *a.store_used, end = base + 8ull * run;
    const bool full = end < base || end > a.store_cap;
    a.w_state[OP_BASE] = base;
    a.w_state[OP_FULL] = full ? 1ull : 0ull;
    *a.status = full ? LZF_STORE_FULL : LZF_STORE_OK;
    if (!full) *a.store_used = end;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_minc_apply_kernel(LzfMincArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    if (a.w_state[OP_FULL]) return;                       /* refused: the same for every lane */
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER;
    uint32_t cls[SD_PER];
    uint64_t conv = 0ull;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        cls[j] = first + j < a.n ? a.w_cls[first + j] : SD_NONE;
        conv += cls[j] == LZF_ENT_CONVERTED;
    }
    uint64_t tot;
    uint64_t rank = a.w_tile[blockIdx.x] + dv_block_excl<SD_WAVES>(conv, sw, &tot);
    const uint64_t base = a.w_state[OP_BASE];
    uint32_t done = 0u, expired = 0u, locked = 0u, nan = 0u, converted = 0u, unchanged = 0u;
#pragma unroll
    for (uint32_t j = 0; j < SD_PER; j++) {
        const uint64_t k = first + j;
        const uint32_t c = cls[j];
        if (c != SD_NONE) {
            const uint32_t i = a.idx[k];
            int64_t val = 0;
            if (c == LZF_ENT_EXPIRED) a.it.enc[i] = (uint8_t)LZF_ENC_NULL;
            /* every valid entry, a NAN one too: :861, :917 come before the value test */
            if (c == LZF_ENT_DONE || c == LZF_ENT_CONVERTED || c == LZF_ENT_NAN || c == LZF_ENT_UNCHANGED)
                if (a.it.last_access) a.it.last_access[i] = a.it.now;
            if (c == LZF_ENT_DONE) {
                val = a.w_val[k];
                op_st_i64(a.store + a.val_off[i], val);   /* its range was checked by the classify pass */
            } else if (c == LZF_ENT_CONVERTED) {
                val = a.w_val[k];
                const uint64_t slot = base + 8ull * rank++;   /* < store_cap: the scan's decision */
                op_st_i64(a.store + slot, val);
                a.val_off[i] = slot;
                a.val_size[i] = 8u;
                a.it.enc[i] = (uint8_t)LZF_ENC_NUMBER;
            }
            if (a.entry_status) a.entry_status[k] = (uint8_t)c;
            if (a.entry_value) a.entry_value[k] = val;
        }
        done += sd_count(c == LZF_ENT_DONE);
        expired += sd_count(c == LZF_ENT_EXPIRED);
        locked += sd_count(c == LZF_ENT_LOCKED);
        nan += sd_count(c == LZF_ENT_NAN);
        converted += sd_count(c == LZF_ENT_CONVERTED);
        unchanged += sd_count(c == LZF_ENT_UNCHANGED);
    }
    sd_leader_add(a.result, done + converted + unchanged);
    sd_leader_add(a.result + 1, expired);
    sd_leader_add(a.result + 2, locked);
    sd_leader_add(a.result + 3, nan);
    sd_leader_add(a.result + 4, converted);
    sd_leader_add(a.result + 5, unchanged);
}

/* ---- set_guard ---------------------------------------------------------------- */

/* src/query.c:446-451: a SET on a key whose item is locked is refused.  New
 * item first + k, whose key the lookup found at occ[k]: an occupant outside
 * the batch that is not dead and is locked keeps the key, and the new item
 * dies.  No validity test, as in the reference.  The occupants read lie
 * outside [first, first + n), the items written inside it */
__global__ __launch_bounds__(SD_BLOCK) void lzf_store_set_guard_kernel(const uint32_t *__restrict__ occ, uint32_t first,
                                                                       uint32_t n, LzfItems it, uint8_t *refused,
                                                                       uint64_t *result)
{
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    uint32_t hits = 0u;
    for (uint64_t b = (uint64_t)blockIdx.x * SD_BLOCK; b < n; b += step) {
        const uint64_t k = b + threadIdx.x;
        bool refuse = false;
        if (k < n) {
            const uint32_t j = occ[k];
            const bool inside = j >= first && (uint64_t)j < (uint64_t)first + n;
            refuse = j < it.count && !inside && it.enc[j] != (uint8_t)LZF_ENC_NULL && mg_locked(j, it);
            if (refuse) it.enc[first + k] = (uint8_t)LZF_ENC_NULL;
            if (refused) refused[k] = refuse ? 1u : 0u;
        }
        hits += sd_count(refuse);
    }
    sd_leader_add(result, hits);
}

template <int OP>
hipError_t op_launch_lock(const LzfLockArgs &a, uint32_t words, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(a.result, 0, words * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_store_lock_kernel<OP>, dim3(sd_sweep_grid(a.n)), dim3(SD_BLOCK), 0, s, a);
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

hipError_t lzf_launch_store_minc(LzfMincArgs &a, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(a.result, 0, 6 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    const uint32_t nt = sd_tiles(a.n);
    hipLaunchKernelGGL(lzf_minc_classify_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_minc_scan_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_minc_apply_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t lzf_launch_store_set_guard(const uint32_t *occ, uint32_t first, uint32_t n, const LzfItems &it,
                                      uint8_t *refused, uint64_t *result, hipStream_t s)
{
    const hipError_t e = hipMemsetAsync(result, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lzf_store_set_guard_kernel, dim3(sd_sweep_grid(n)), dim3(SD_BLOCK), 0, s, occ, first, n, it,
                       refused, result);
    return hipGetLastError();
}

int lzf_ops_parse_long(const uint8_t *v, uint32_t len, int64_t *out)
{
    return lzf_parse_long(v, len, out);
}
