/*
 * lzf_order.hip -- the ordered prefix select (lzf_gpu_store_select_ordered,
 * include/lzf_gpu.h): the live items whose key starts with a prefix, in the
 * order of the reference's tr_search (src/trie.c:154-176), cut to its limit.
 *
 * The rule (include/lzf_gpu.h states it in full).  birth(P) is the smallest
 * item index whose key starts with P, live or dead; row(K) is birth(K[0..d))
 * for d = plen + 1 .. len(K); the reference's order of the live matches is the
 * ascending lexicographic order of their rows, a shorter row before its
 * extensions.  DESIGN.md §7.10 argues why, and what the table below relies on.
 *
 * The launches, each reading what the ones before it left in the work area; no
 * workgroup waits for another, and inside a launch data crosses between
 * threads only in one 64-bit table word:
 *   1. match: the candidates' ballot per 64 items (the select's match without
 *      the enc test), and per tile [live:32 | candidates:32], the node words
 *      and the longest candidate;
 *      carry: one workgroup scans the tile sums and decides: LZF_ORDER_EWORK,
 *      or the table's size for this call (a power of two of at least twice the
 *      node words needed, so at most the one the caller sized) and how many
 *      tag bits the depth takes; result[1 .. 4];
 *      clear: the table's words to all ones;  cands: the candidate list, in
 *      ascending index, from the ballots.
 *   2. births: one thread per candidate walks the depths plen + 1 .. len with
 *      a running hash.  A table word is [tag:32 | index:32], all ones empty;
 *      the tag is [hash | depth - plen], the depth in as many low bits as the
 *      longest candidate needs, so two words of one tag are of one depth.  An
 *      empty slot is claimed by compare-and-swap; a slot whose tag matches is
 *      confirmed against the key bytes of the item it names and then lowered
 *      by atomicMin, unless the index it holds is below the walker's already;
 *      a failed swap re-judges the word it returned.  A slot, once taken,
 *      stands for one node to the end of the call: only confirmed walkers of
 *      that node ever write it, and they keep its tag.  So a stale read is
 *      still a right answer to "is this my node", a node is never in two
 *      slots (the slots between its home and its slot were taken before it and
 *      stay taken), and after the launch every word holds birth(node).
 *   3. live: per tile of the candidate list its matches and their row words;
 *      carry; lists: per match its item, row offset and row length (packed
 *      rows: a key may be 512 bytes and most are short);  rows: one thread
 *      per match looks its births up in the finished table.
 *   4. sort: each tile of SD_TILE matches by a bitonic network in LDS, then
 *      ceil(log2(tiles of cand_cap)) merge passes between two buffers: an
 *      element's place is its rank in its own run plus a binary search in the
 *      sibling run.  Rows of different keys differ, so the order is strict;
 *      two live items of one key (a store the key index keeps never holds
 *      them) fall back to their index.  Passes past the real length copy.
 *   5. emit: sel, its padding, result[0].
 *
 * The kernels are helpers of this translation unit, not part of the library's
 * routed kernel set: they have internal linkage (anonymous namespace).
 */
#include "lzf_store_dev.h"
#include "../../include/lzf_gpu.h"

namespace {

/* state words of the work area */
enum { OD_CANDS = 0, OD_WORDS = 1, OD_LIVE = 2, OD_STATUS = 3, OD_MASK = 4, OD_BITS = 5, OD_ROWS = 6 };

#define OD_EMPTY (~0ull)

/* ---- candidates ---------------------------------------------------------------- */

/* the select's match (lzf_mget.hip) without the enc test: item i of a tile
 * sits in round (i % SD_TILE) / SD_BLOCK at thread i % SD_BLOCK */
__global__ __launch_bounds__(SD_BLOCK) void lzf_order_match_kernel(LzfOrderArgs a)
{
    __shared__ uint64_t sn[SD_WAVES], sb[SD_WAVES], sm[SD_WAVES];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE;
    uint64_t n = 0ull, words = 0ull, longest = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t i = first + k * SD_BLOCK + threadIdx.x;
        bool c = false;
        uint32_t len = 0u;
        if (i < a.count) {
            len = a.key_len[i];
            if (len >= a.prefix_len) c = mg_prefix_match(a.keys + a.key_off[i], a.prefix, a.prefix_len);
        }
        const uint64_t word = __ballot(c);
        if (lane == 0u) a.w_mask[(uint64_t)blockIdx.x * SD_WORDS + k * SD_WAVES + wave] = word;
        const bool live = c && a.enc[i] != (uint8_t)LZF_ENC_NULL;
        n += (uint64_t)__popcll(word) | ((uint64_t)sd_count(live) << 32);
        const uint64_t rel = c ? (uint64_t)(len - a.prefix_len) : 0ull;
        words += rel;
        longest = rel > longest ? rel : longest;
    }
    words = sd_wave_sum(words);
    longest = sd_wave_max(longest);
    if (lane == 0u) {
        sn[wave] = n;
        sb[wave] = words;
        sm[wave] = longest;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint64_t tn = 0ull, tb = 0ull, tm = 0ull;
        for (uint32_t w = 0; w < SD_WAVES; w++) {
            tn += sn[w];
            tb += sb[w];
            tm = sm[w] > tm ? sm[w] : tm;
        }
        a.w_tile_n[blockIdx.x] = tn;
        a.w_tile_b[blockIdx.x] = tb;
        a.w_tile_m[blockIdx.x] = tm;
    }
}

/* one workgroup: the scans of the tile sums in place -- the two counts ride in
 * one word, the candidates below 2^32 never carrying into the live count --
 * and the one decision of the call */
__global__ __launch_bounds__(SD_BLOCK) void lzf_order_carry_kernel(LzfOrderArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    const uint64_t n = dv_carry_scan<SD_WAVES>(a.w_tile_n, ntile, sw);
    const uint64_t words = dv_carry_scan<SD_WAVES>(a.w_tile_b, ntile, sw);
    uint64_t longest = 0ull;
    for (uint32_t t = threadIdx.x; t < ntile; t += SD_BLOCK) longest = a.w_tile_m[t] > longest ? a.w_tile_m[t] : longest;
    longest = sd_wave_max(longest);
    if ((threadIdx.x & 63u) == 0u) sw[threadIdx.x >> 6] = longest;
    __syncthreads();
    if (threadIdx.x != 0u) return;
    for (uint32_t w = 0; w < SD_WAVES; w++) longest = sw[w] > longest ? sw[w] : longest;
    const uint64_t cands = n & 0xFFFFFFFFull, live = n >> 32;
    const bool ok = cands <= a.cand_cap && words <= a.node_cap;
    a.w_state[OD_CANDS] = cands;
    a.w_state[OD_WORDS] = words;
    a.w_state[OD_LIVE] = live;
    a.w_state[OD_STATUS] = ok ? LZF_ORDER_OK : LZF_ORDER_EWORK;
    a.w_state[OD_MASK] = ok ? sd_order_slots(words) - 1ull : 0ull;      /* words <= node_cap: within a.slots */
    a.w_state[OD_BITS] = 64u - (uint32_t)__clzll((unsigned long long)longest);   /* depth - plen <= longest < 2^32 */
    a.w_state[OD_ROWS] = 0ull;
    a.result[1] = live;
    a.result[2] = cands;
    a.result[3] = words;
    a.result[4] = ok ? LZF_ORDER_OK : LZF_ORDER_EWORK;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_order_clear_kernel(LzfOrderArgs a)
{
    if (a.w_state[OD_STATUS] != (uint64_t)LZF_ORDER_OK) return;
    const uint64_t slots = a.w_state[OD_MASK] + 1ull, step = (uint64_t)gridDim.x * SD_BLOCK;
    for (uint64_t p = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; p < slots; p += step) a.w_table[p] = OD_EMPTY;
}

/* the candidate list from the ballot words alone, as the select's write */
__global__ __launch_bounds__(SD_BLOCK) void lzf_order_cands_kernel(LzfOrderArgs a)
{
    __shared__ uint32_t pre[SD_WORDS + 1u];
    if (a.w_state[OD_STATUS] != (uint64_t)LZF_ORDER_OK) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t *mask = a.w_mask + (uint64_t)blockIdx.x * SD_WORDS;
    if (threadIdx.x == 0u) {
        uint32_t s = 0u;
        for (uint32_t w = 0; w < SD_WORDS; w++) {
            pre[w] = s;
            s += (uint32_t)__popcll(mask[w]);
        }
    }
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * SD_TILE, base = a.w_tile_n[blockIdx.x] & 0xFFFFFFFFull;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint32_t w = k * SD_WAVES + wave;
        const uint64_t word = mask[w];
        if (!((word >> lane) & 1ull)) continue;
        const uint64_t r = base + pre[w] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
        if (r < a.cand_cap) a.w_cand[r] = (uint32_t)(first + k * SD_BLOCK + threadIdx.x);
    }
}

/* ---- the node table -------------------------------------------------------------- */

/* the running hash over the key bytes past the prefix (FNV-1a's step), and its
 * finish: the home from the low bits, the tag's hash from the high ones */
#define OD_SEED 0xCBF29CE484222325ull
__device__ inline uint64_t od_step(uint64_t h, uint8_t b)
{
    return (h ^ b) * 0x100000001B3ull;
}

__device__ inline uint64_t od_finish(uint64_t h)
{
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    return h;
}

/* [hash | depth - plen]: the depth exact in `bits` low bits */
__device__ inline uint32_t od_tag(uint64_t f, uint32_t rel, uint32_t bits)
{
    return bits >= 32u ? rel : (((uint32_t)(f >> 32)) << bits) | rel;
}

/* the item last confirmed to share the walker's key up to the depth before:
 * at first the walker's own */
struct OdPrev {
    uint32_t j, len;
    const uint8_t *key;
};

/* whether item j's key has d bytes and shares them with `key` (every item in
 * the table is a candidate, so the prefix is shared).  The item confirmed at
 * depth d - 1 takes one byte; another one is compared from the end, where
 * keys of one depth differ first */
__device__ inline bool od_confirm(const LzfOrderArgs &a, uint32_t j, const uint8_t *key, uint32_t d, OdPrev &prev)
{
    if (j == prev.j) return prev.len >= d && prev.key[d - 1u] == key[d - 1u];
    if (j >= a.count) return false;
    const uint32_t len = a.key_len[j];
    if (len < d) return false;
    const uint8_t *kj = a.keys + a.key_off[j];
    for (uint32_t t = d; t-- > a.prefix_len;)
        if (kj[t] != key[t]) return false;
    prev.j = j;
    prev.len = len;
    prev.key = kj;
    return true;
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_order_births_kernel(LzfOrderArgs a)
{
    if (a.w_state[OD_STATUS] != (uint64_t)LZF_ORDER_OK) return;
    unsigned long long *table = (unsigned long long *)a.w_table;
    const uint64_t cands = a.w_state[OD_CANDS], mask = a.w_state[OD_MASK], step = (uint64_t)gridDim.x * SD_BLOCK;
    const uint32_t bits = (uint32_t)a.w_state[OD_BITS], plen = a.prefix_len;
    for (uint64_t c = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; c < cands; c += step) {
        const uint32_t i = a.w_cand[c], len = a.key_len[i];
        const uint8_t *key = a.keys + a.key_off[i];
        OdPrev prev{i, len, key};
        uint64_t h = OD_SEED;
        for (uint32_t d = plen + 1u; d <= len; d++) {
            h = od_step(h, key[d - 1u]);
            const uint64_t f = od_finish(h);
            const uint32_t tag = od_tag(f, d - plen, bits);
            const unsigned long long want = ((unsigned long long)tag << 32) | i;
            uint64_t pos = f & mask;
            bool done = false;
            /* at most every slot once, so the walk ends on any table contents */
            for (uint64_t seen = 0; !done && seen <= mask; seen++, pos = (pos + 1ull) & mask) {
                unsigned long long cur = __hip_atomic_load(&table[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                for (;;) {                /* until this slot's word is judged */
                    if (cur == OD_EMPTY) {
                        const unsigned long long old = atomicCAS(&table[pos], OD_EMPTY, want);
                        if (old == OD_EMPTY) {
                            prev = OdPrev{i, len, key};
                            done = true;
                            break;
                        }
                        cur = old;        /* another walker got in first: judge its word */
                        continue;
                    }
                    if ((uint32_t)(cur >> 32) != tag) break;                  /* another node's slot */
                    const uint32_t j = (uint32_t)cur;
                    if (!od_confirm(a, j, key, d, prev)) break;
                    if (j > i) atomicMin(&table[pos], want);                  /* below already: no atomic */
                    done = true;
                    break;
                }
            }
        }
    }
}

/* ---- matches and rows ------------------------------------------------------------- */

/* thread t of a tile takes candidates t * SD_PER .. + SD_PER, so the scan over
 * the threads is the scan over the list; n: its matches, words: their rows' */
__device__ inline void od_thread_matches(const LzfOrderArgs &a, uint64_t first, uint64_t cands, uint32_t item[SD_PER],
                                         uint32_t rel[SD_PER], uint64_t *n, uint64_t *words)
{
    *n = *words = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        item[k] = SD_PAD;
        rel[k] = 0u;
        if (first + k >= cands) continue;
        const uint32_t i = a.w_cand[first + k];
        if (a.enc[i] == (uint8_t)LZF_ENC_NULL) continue;
        item[k] = i;
        rel[k] = a.key_len[i] - a.prefix_len;
        *n += 1ull;
        *words += rel[k];
    }
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_order_live_kernel(LzfOrderArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    const bool ok = a.w_state[OD_STATUS] == (uint64_t)LZF_ORDER_OK;
    const uint64_t cands = ok ? a.w_state[OD_CANDS] : 0ull;
    uint32_t item[SD_PER], rel[SD_PER];
    uint64_t n, words, tn, tb;
    od_thread_matches(a, (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER, cands, item, rel, &n, &words);
    dv_block_excl<SD_WAVES>(n, sw, &tn);
    dv_block_excl<SD_WAVES>(words, sw, &tb);
    if (threadIdx.x == 0u) {
        a.w_ctile_n[blockIdx.x] = tn;
        a.w_ctile_b[blockIdx.x] = tb;
    }
}

__global__ __launch_bounds__(SD_BLOCK) void lzf_order_live_carry_kernel(LzfOrderArgs a, uint32_t ntile)
{
    __shared__ uint64_t sw[SD_WAVES];
    dv_carry_scan<SD_WAVES>(a.w_ctile_n, ntile, sw);
    const uint64_t words = dv_carry_scan<SD_WAVES>(a.w_ctile_b, ntile, sw);
    if (threadIdx.x == 0u) a.w_state[OD_ROWS] = words;
}

/* per match, in the candidates' order: its item, and its row's place and length */
__global__ __launch_bounds__(SD_BLOCK) void lzf_order_lists_kernel(LzfOrderArgs a)
{
    __shared__ uint64_t sw[SD_WAVES];
    if (a.w_state[OD_STATUS] != (uint64_t)LZF_ORDER_OK) return;
    uint32_t item[SD_PER], rel[SD_PER];
    uint64_t n, words, tn, tb;
    od_thread_matches(a, (uint64_t)blockIdx.x * SD_TILE + threadIdx.x * SD_PER, a.w_state[OD_CANDS], item, rel, &n,
                      &words);
    uint64_t p = a.w_ctile_n[blockIdx.x] + dv_block_excl<SD_WAVES>(n, sw, &tn);
    uint64_t off = a.w_ctile_b[blockIdx.x] + dv_block_excl<SD_WAVES>(words, sw, &tb);
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        if (item[k] == SD_PAD) continue;
        a.w_live[p] = item[k];
        a.w_row_off[p] = off;
        a.w_row_len[p] = rel[k];
        p++;
        off += rel[k];
    }
}

/* one thread per match: the births of its key's nodes, from the finished
 * table.  Every node of a candidate is in it; a walk that found none would
 * name the item itself */
__global__ __launch_bounds__(SD_BLOCK) void lzf_order_rows_kernel(LzfOrderArgs a)
{
    if (a.w_state[OD_STATUS] != (uint64_t)LZF_ORDER_OK) return;
    const uint64_t live = a.w_state[OD_LIVE], mask = a.w_state[OD_MASK], step = (uint64_t)gridDim.x * SD_BLOCK;
    const uint32_t bits = (uint32_t)a.w_state[OD_BITS], plen = a.prefix_len;
    for (uint64_t p = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; p < live; p += step) {
        const uint32_t i = a.w_live[p], len = a.key_len[i];
        const uint8_t *key = a.keys + a.key_off[i];
        uint32_t *row = a.w_rows + a.w_row_off[p];
        OdPrev prev{i, len, key};
        uint64_t h = OD_SEED;
        for (uint32_t d = plen + 1u; d <= len; d++) {
            h = od_step(h, key[d - 1u]);
            const uint64_t f = od_finish(h);
            const uint32_t tag = od_tag(f, d - plen, bits);
            uint64_t pos = f & mask;
            uint32_t birth = i;
            for (uint64_t seen = 0; seen <= mask; seen++, pos = (pos + 1ull) & mask) {
                const uint64_t cur = a.w_table[pos];
                if (cur == OD_EMPTY) break;
                if ((uint32_t)(cur >> 32) != tag || !od_confirm(a, (uint32_t)cur, key, d, prev)) continue;
                birth = (uint32_t)cur;
                break;
            }
            row[d - plen - 1u] = birth;
        }
    }
}

/* ---- sort -------------------------------------------------------------------------- */

/* whether match x comes before match y: their rows word by word, the shorter
 * first, and two items of one key by their place in the list.  SD_PAD, the
 * filler of a short tile, comes after every match */
__device__ inline bool od_before(const LzfOrderArgs &a, uint32_t x, uint32_t y)
{
    if (x == SD_PAD) return false;
    if (y == SD_PAD) return true;
    const uint32_t lx = a.w_row_len[x], ly = a.w_row_len[y], n = lx < ly ? lx : ly;
    const uint32_t *rx = a.w_rows + a.w_row_off[x], *ry = a.w_rows + a.w_row_off[y];
    for (uint32_t t = 0; t < n; t++) {
        const uint32_t bx = rx[t], by = ry[t];
        if (bx != by) return bx < by;
    }
    return lx != ly ? lx < ly : x < y;
}

/* a tile of the match list, sorted by a bitonic network in LDS: 512 pairs a
 * step, two per thread */
__global__ __launch_bounds__(SD_BLOCK) void lzf_order_tile_sort_kernel(LzfOrderArgs a)
{
    __shared__ uint32_t s[SD_TILE];
    if (a.w_state[OD_STATUS] != (uint64_t)LZF_ORDER_OK) return;
    const uint64_t live = a.w_state[OD_LIVE], first = (uint64_t)blockIdx.x * SD_TILE;
    if (first >= live) return;
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t p = first + k * SD_BLOCK + threadIdx.x;
        s[k * SD_BLOCK + threadIdx.x] = p < live ? (uint32_t)p : SD_PAD;
    }
    for (uint32_t k = 2u; k <= SD_TILE; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            __syncthreads();
#pragma unroll
            for (uint32_t q = threadIdx.x; q < SD_TILE / 2u; q += SD_BLOCK) {
                const uint32_t lo = ((q & ~(j - 1u)) << 1) | (q & (j - 1u)), hi = lo | j;
                const uint32_t x = s[lo], y = s[hi];
                const bool up = !(lo & k);
                if (up ? od_before(a, y, x) : od_before(a, x, y)) {
                    s[lo] = y;
                    s[hi] = x;
                }
            }
        }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < SD_PER; k++) {
        const uint64_t p = first + k * SD_BLOCK + threadIdx.x;
        if (p < live) a.w_sort[0][p] = s[k * SD_BLOCK + threadIdx.x];
    }
}

/* one merge pass over sorted runs of `run` matches (a power of two), pairs of
 * neighbours into one: an element lands at its rank in its own run plus the
 * sibling's elements before it.  A run without a sibling copies */
__global__ __launch_bounds__(SD_BLOCK) void lzf_order_merge_kernel(LzfOrderArgs a, const uint32_t *src, uint32_t *dst,
                                                                   uint64_t run)
{
    if (a.w_state[OD_STATUS] != (uint64_t)LZF_ORDER_OK) return;
    const uint64_t live = a.w_state[OD_LIVE], step = (uint64_t)gridDim.x * SD_BLOCK;
    for (uint64_t q = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; q < live; q += step) {
        const uint32_t e = src[q];
        const uint64_t pair = q & ~(2ull * run - 1ull);
        const bool right = (q & run) != 0ull;
        const uint64_t own = right ? pair + run : pair, sib = right ? pair : pair + run;
        uint64_t lo = sib < live ? sib : live, hi = sib + run < live ? sib + run : live;
        while (lo < hi) {                 /* the first of the sibling's that e is not after */
            const uint64_t mid = lo + (hi - lo) / 2u;
            if (od_before(a, src[mid], e)) lo = mid + 1u;
            else hi = mid;
        }
        const uint64_t sib0 = sib < live ? sib : live;
        dst[pair + (q - own) + (lo - sib0)] = e;
    }
}

/* ---- emit ---------------------------------------------------------------------------- */

__global__ __launch_bounds__(SD_BLOCK) void lzf_order_emit_kernel(LzfOrderArgs a, const uint32_t *sorted)
{
    const bool ok = a.w_state[OD_STATUS] == (uint64_t)LZF_ORDER_OK;
    uint64_t n = ok ? a.w_state[OD_LIVE] : 0ull;
    if (a.limit > 0 && (uint64_t)a.limit < n) n = (uint64_t)a.limit;            /* src/trie.c:162 */
    if (a.cap < n) n = a.cap;
    const uint64_t step = (uint64_t)gridDim.x * SD_BLOCK;
    for (uint64_t r = (uint64_t)blockIdx.x * SD_BLOCK + threadIdx.x; r < a.cap; r += step)
        a.sel[r] = r < n ? a.w_live[sorted[r]] : SD_PAD;
    if (blockIdx.x == 0u && threadIdx.x == 0u) a.result[0] = n;
}

}  // namespace

hipError_t lzf_launch_store_select_ordered(LzfOrderArgs &a, hipStream_t s)
{
    const uint32_t nt = sd_tiles(a.count), ct = sd_tiles(a.cand_cap), sweep = sd_sweep_grid(a.cand_cap);
    hipLaunchKernelGGL(lzf_order_match_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_order_carry_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, nt);
    hipLaunchKernelGGL(lzf_order_clear_kernel, dim3(sd_sweep_grid(a.slots)), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_order_cands_kernel, dim3(nt), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_order_births_kernel, dim3(sweep), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_order_live_kernel, dim3(ct), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_order_live_carry_kernel, dim3(1), dim3(SD_BLOCK), 0, s, a, ct);
    hipLaunchKernelGGL(lzf_order_lists_kernel, dim3(ct), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_order_rows_kernel, dim3(sweep), dim3(SD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(lzf_order_tile_sort_kernel, dim3(ct), dim3(SD_BLOCK), 0, s, a);
    /* the pass count from cand_cap: the real length is known on the device only */
    uint32_t from = 0u;
    for (uint64_t run = SD_TILE; run < a.cand_cap; run <<= 1, from ^= 1u)
        hipLaunchKernelGGL(lzf_order_merge_kernel, dim3(sweep), dim3(SD_BLOCK), 0, s, a,
                           (const uint32_t *)a.w_sort[from], a.w_sort[from ^ 1u], run);
    hipLaunchKernelGGL(lzf_order_emit_kernel, dim3(sd_sweep_grid(a.cap)), dim3(SD_BLOCK), 0, s, a,
                       (const uint32_t *)a.w_sort[from]);
    return hipGetLastError();
}
