/*
 * lzf_lane_diag.hip -- the lane generation's cross-check forms: compiled into
 * the diagnostic library only (csrc/Makefile, DIAG_OBJ), selected by the
 * LZF_GPU_* variables of INTEGRATION.md §5, never the default.
 * All of them run ONE LANE or ONE WAVE per value:
 *
 *   decompress  lzf_decompress_lane_kernel: one lane decodes one stream with
 *               the reference's checks in the reference's order; literal runs
 *               and back-references move as unaligned 16-byte pieces.
 *   kernel 1    lzf_cand_small_kernel (values <= 4 KiB, and <= 8 KiB with a
 *               3-bit identity), lzf_cand_ring_kernel (to 64 KiB) and
 *               lzf_cand_mid_kernel (to 64 KiB, opt-in): one wave per value,
 *               the cand words of lzf_lane.hip from bucket heads and skip
 *               links in LDS instead of the stream kernel's exact table.
 *   kernel 2    lzf_parse_wave_kernel: the parse as one wave per value, 64
 *               positions per step over LDS-resident data.
 *
 * lzf_lane.hip's launcher reaches them through the hooks of lzf_lane_dev.h.
 */
#include "lzf_lane_dev.h"

__device__ __forceinline__ uint32_t ln_ab(uint32_t hi, uint32_t lo)    /* (hi:lo) >> 8 */
{
    return __builtin_amdgcn_alignbyte(hi, lo, 1u);
}

/* ======================================================================== */
/* decompress: one lane per stream                                          */
/* ======================================================================== */

#define LD_THREADS 256u

/* Back-reference copy of L bytes from distance `back` (src/lzf_d.c:137-142
 * copies byte-serially, so an overlapping source replicates a period of
 * `back` bytes).  Pieces of up to 16 bytes; while the period is shorter than
 * 16 the copy distance doubles (any multiple of the period is a valid source
 * once that many bytes exist), so a run of 264 takes 5 + 16 pieces. */
__device__ __forceinline__ void ln_copy_back(uint8_t *out, uint32_t o, uint32_t back, uint32_t L,
                                             uint32_t cap)
{
    uint32_t D = back, t = 0;
    do {
        uint32_t c = L - t;
        if (c > 16u) c = 16u;
        if (c > D) c = D;
        const uint32_t s = o + t - D;
        const uint4 v = dv_ld16_safe_w(out + s, cap - s);
        dv_st_exact(out + o + t, v, c);
        t += c;
        if (D < 16u) D <<= 1;
    } while (t < L);
}

__global__ __launch_bounds__(LD_THREADS) void lzf_decompress_lane_kernel(LzfBatch bt)
{
    const uint32_t v = blockIdx.x * LD_THREADS + threadIdx.x;
    if (v >= bt.count) return;
    if (bt.skip && bt.skip[v]) return;
    const uint32_t in_len = bt.in_len[v];
    const uint32_t cap = bt.out_cap[v];
    const uint8_t *in = bt.in + bt.in_off[v];
    uint8_t *out = bt.out + bt.out_off[v];
    /* as the reference (do-while, src/lzf_d.c:64), a 0-length stream still
     * reads its first control byte */
    const uint32_t avail = in_len ? in_len : 1u;
    uint32_t i = 0, o = 0;
    int32_t err = 0;
    do {
        uint4 w0, w1;
        if (i + 32u <= avail) {
            w0 = dv_ld16(in + i);
            w1 = dv_ld16(in + i + 16u);
        } else {
            w0 = dv_ld16_safe_w(in + i, avail - i);
            w1 = i + 16u < avail ? dv_ld16_tail_w(in + i + 16u, avail - i - 16u) : make_uint4(0, 0, 0, 0);
        }
        const uint32_t c = w0.x & 0xFFu;
        if (c < 32u) {                                               /* literal run */
            const uint32_t cnt = c + 1u;
            if ((uint64_t)o + cnt > cap) { err = 7; break; }         /* E2BIG  src/lzf_d.c:72 */
            if ((uint64_t)i + 1u + cnt > in_len) { err = 22; break; }/* EINVAL src/lzf_d.c:79 */
            const uint4 lo = make_uint4(ln_ab(w0.y, w0.x), ln_ab(w0.z, w0.y), ln_ab(w0.w, w0.z),
                                        ln_ab(w1.x, w0.w));
            dv_st_exact(out + o, lo, cnt);
            if (cnt > 16u) {
                const uint32_t b32 = cnt == 32u ? (uint32_t)in[i + 32u] : 0u;
                const uint4 hi = make_uint4(ln_ab(w1.y, w1.x), ln_ab(w1.z, w1.y), ln_ab(w1.w, w1.z),
                                            ln_ab(b32, w1.w));
                dv_st_exact(out + o + 16u, hi, cnt - 16u);
            }
            o += cnt;
            i += 1u + cnt;
        } else {                                                     /* back-reference */
            uint32_t len = c >> 5, ob = (w0.x >> 8) & 0xFFu, tsz = 2u;
            if (i + 1u >= in_len) { err = 22; break; }               /* src/lzf_d.c:101 */
            if (len == 7u) {
                len += ob;
                ob = (w0.x >> 16) & 0xFFu;
                tsz = 3u;
                if (i + 2u >= in_len) { err = 22; break; }           /* src/lzf_d.c:111 */
            }
            const uint32_t back = ((c & 31u) << 8) + 1u + ob;
            if ((uint64_t)o + len + 2u > cap) { err = 7; break; }    /* src/lzf_d.c:121 */
            if (back > o) { err = 22; break; }                       /* src/lzf_d.c:127 */
            ln_copy_back(out, o, back, len + 2u, cap);
            o += len + 2u;
            i += tsz;
        }
    } while (i < in_len);
    bt.out_len[v] = err ? 0u : o;
    bt.err[v] = err;
}

hipError_t lzf_launch_decompress_lane(const LzfBatch &b, hipStream_t s)
{
    const uint32_t grid = (b.count + LD_THREADS - 1u) / LD_THREADS;
    const size_t lds = lane_lds_for("LZF_LANE_DEC_BLOCKS", 0u);
    if (lds) {
        hipError_t e = hipFuncSetAttribute((const void *)lzf_decompress_lane_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lzf_decompress_lane_kernel, dim3(grid), dim3(LD_THREADS), lds, s, b);
    return hipGetLastError();
}

/* ======================================================================== */
/* compress, kernel 1: same-slot predecessor of every position              */
/* ======================================================================== */

#define K1_WIN      4u            /* windows of 64 positions resolved per step */
#ifndef KS_WIN
#define KS_WIN      4u            /* small class: windows per step (exchange form, json4k compress: 4: 48.6 ms, 3: 49.1, 2: 49.8, 1: 52.2) */
#endif
#ifndef KS8_WIN
#define KS8_WIN     2u            /* 8 KiB small class: windows per step */
#endif
#define KM_BUCKETS  2048u         /* mid class */

/* agreement of the bytes at p and q (q < p), at most 8 and at most n - p */
__device__ __forceinline__ uint32_t k1_agree(const uint8_t *src, uint32_t n, uint32_t p, uint32_t q)
{
    const uint32_t avail = n - p;
    uint32_t a0, a1, b0, b1;
    if (avail >= 8u) {
        const uint2 a = dv_ld8(src + p), b = dv_ld8(src + q);
        a0 = a.x; a1 = a.y; b0 = b.x; b1 = b.y;
    } else {
        const uint4 a = dv_ld16_tail_w(src + p, avail), b = dv_ld16_tail_w(src + q, avail);
        a0 = a.x; a1 = a.y; b0 = b.x; b1 = b.y;
    }
    uint32_t k;
    if (a0 != b0) k = (uint32_t)__builtin_ctz(a0 ^ b0) >> 3;
    else if (a1 != b1) k = 4u + ((uint32_t)__builtin_ctz(a1 ^ b1) >> 3);
    else k = 8u;
    return k < avail ? k : avail;
}

/* Lane-order check of the bucket-head atomics: a returned head from a later
 * position means the LDS did not serialise the wave's same-address atomics in
 * lane order; then the predecessors are rebuilt from the keys (the head before
 * the step is the smallest value any lane of the bucket got back). */
template <uint32_t BSHIFT>
__device__ __noinline__ void k1_fix_order(uint32_t (&r)[K1_WIN], const uint32_t (&key)[K1_WIN],
                                          const bool (&act)[K1_WIN])
{
    const uint32_t lane = threadIdx.x;
    uint32_t fixed[K1_WIN];
#pragma unroll
    for (uint32_t j = 0; j < K1_WIN; j++) {
        const uint32_t myb = (key[j] & 0xFFFFu) >> BSHIFT;
        uint32_t mn = 0xFFFFFFFFu, mx = 0u;
        for (uint32_t t = 0; t < 64u * K1_WIN; t++) {
            const uint32_t tj = t >> 6, tl = t & 63u;
            uint32_t kt = 0u, rt = 0u, at = 0u;
#pragma unroll
            for (uint32_t jj = 0; jj < K1_WIN; jj++) {
                const uint32_t kk = (uint32_t)__shfl((int)key[jj], (int)tl);
                const uint32_t rr = (uint32_t)__shfl((int)r[jj], (int)tl);
                const uint32_t aa = (uint32_t)__shfl(act[jj] ? 1 : 0, (int)tl);
                if (jj == tj) { kt = kk; rt = rr; at = aa; }
            }
            if (at && ((kt & 0xFFFFu) >> BSHIFT) == myb) {
                mn = rt < mn ? rt : mn;
                if (t < 64u * j + lane && kt > mx) mx = kt;
            }
        }
        fixed[j] = mn > mx ? mn : mx;
    }
#pragma unroll
    for (uint32_t j = 0; j < K1_WIN; j++)
        if (act[j]) r[j] = fixed[j];
}

/* Small class (every value <= MAXN <= 8 KiB bytes: all positions inside one
 * 8 KiB window, so no window test).  Persistent workgroups of one wave walk the batch; the next
 * value's bytes are loaded into registers while the current one is
 * processed and then staged in LDS, so the position loop reads only LDS.
 *
 * Slot-mix m = mix(slot) (bijective): bucket = m >> IDB, identity = the low
 * IDB bits (IDB = 4 for values <= 4 KiB, 3 for values <= 8 KiB, so that an
 * entry [pos+1 | identity] fits 16 bits).
 * Per position the kernel keeps, in LDS, the bucket head (latest position of
 * the bucket) and a skip link: the latest earlier position of the bucket
 * with ANOTHER identity.  Per window of 64 positions one lane-ordered 16-bit
 * exchange on the heads (ds_mskor_rtn_b32) gives each lane its latest
 * earlier same-bucket position, the head's or an earlier lane's; the
 * same-slot predecessor follows the skip links from there until the
 * identity matches (one hop per change of identity, not per position).
 * Entries are [pos+1:16-IDB | identity:IDB].  LDS at 4 KiB: heads 8 KiB,
 * links 8 KiB, bytes 4 KiB; at 8 KiB: heads 16 KiB, links 16 KiB, bytes
 * 8 KiB. */
__device__ __forceinline__ uint32_t ks_rd4(const uint32_t *w, uint32_t x)
{
    return __builtin_amdgcn_alignbyte(w[(x >> 2) + 1u], w[x >> 2], x & 3u);
}

/* highest set bit of a 64-bit mask (mask != 0) */
__device__ __forceinline__ uint32_t ks_hibit(uint64_t m)
{
    return 63u - (uint32_t)__builtin_clzll(m);
}

/* WIN lane-ordered 16-bit exchanges (ds_mskor_rtn_b32), issued in order, one wait */
template <uint32_t WIN>
__device__ __forceinline__ void ks_xchg(uint32_t (&r)[WIN], const uint32_t (&a)[WIN], const uint32_t (&m)[WIN],
                                        const uint32_t (&d)[WIN])
{
    static_assert(WIN >= 1u && WIN <= 4u, "1..4 windows per step");
    if constexpr (WIN == 1u) {
        asm volatile("ds_mskor_rtn_b32 %0, %1, %2, %3\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(r[0]) : "v"(a[0]), "v"(m[0]), "v"(d[0]) : "memory");
    } else if constexpr (WIN == 2u) {
        asm volatile("ds_mskor_rtn_b32 %0, %2, %3, %4\n\tds_mskor_rtn_b32 %1, %5, %6, %7\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(r[0]), "=&v"(r[1])
                     : "v"(a[0]), "v"(m[0]), "v"(d[0]), "v"(a[1]), "v"(m[1]), "v"(d[1]) : "memory");
    } else if constexpr (WIN == 3u) {
        asm volatile("ds_mskor_rtn_b32 %0, %3, %4, %5\n\tds_mskor_rtn_b32 %1, %6, %7, %8\n\t"
                     "ds_mskor_rtn_b32 %2, %9, %10, %11\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2])
                     : "v"(a[0]), "v"(m[0]), "v"(d[0]), "v"(a[1]), "v"(m[1]), "v"(d[1]), "v"(a[2]), "v"(m[2]),
                       "v"(d[2]) : "memory");
    } else {
        asm volatile("ds_mskor_rtn_b32 %0, %4, %5, %6\n\tds_mskor_rtn_b32 %1, %7, %8, %9\n\t"
                     "ds_mskor_rtn_b32 %2, %10, %11, %12\n\tds_mskor_rtn_b32 %3, %13, %14, %15\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(r[0]), "=&v"(r[1]), "=&v"(r[2]), "=&v"(r[3])
                     : "v"(a[0]), "v"(m[0]), "v"(d[0]), "v"(a[1]), "v"(m[1]), "v"(d[1]), "v"(a[2]), "v"(m[2]),
                       "v"(d[2]), "v"(a[3]), "v"(m[3]), "v"(d[3]) : "memory");
    }
}

template <uint32_t IDB, uint32_t MAXN, uint32_t WIN>
__global__ __launch_bounds__(64) void lzf_cand_small_kernel(LzfBatch bt, LzfLaneScratch sc)
{
    static_assert(MAXN <= LZF_WINDOW && ((MAXN - 1u) >> (16u - IDB)) == 0u, "entry [pos+1 | id] must fit 16 bits");
    constexpr uint32_t BUCKETS = 1u << (16u - IDB), IDM = (1u << IDB) - 1u;
    constexpr uint32_t PF = MAXN / 1024u;                /* 16-byte loads per lane per value */
    __shared__ __attribute__((aligned(16))) uint16_t H[BUCKETS + 64u];   /* + one dummy per lane */
    __shared__ uint16_t E[MAXN];
    __shared__ __attribute__((aligned(16))) uint32_t Bw[MAXN / 4u + 4u];
    const uint32_t lane = threadIdx.x;
    uint32_t v = blockIdx.x;
    if (v >= bt.count) return;
    uint4 pf[PF];
    uint32_t pn = bt.in_len[v];
    {
        const uint8_t *s0 = bt.in + bt.in_off[v];
#pragma unroll
        for (uint32_t k = 0; k < PF; k++) {
            const uint32_t at = 16u * (64u * k + lane);
            pf[k] = at < pn ? dv_ld16_safe_w(s0 + at, pn - at) : make_uint4(0, 0, 0, 0);
        }
    }
    while (v < bt.count) {
        const uint32_t n = pn;
        uint16_t *cand = sc.cand + (uint64_t)v * sc.cstride;
#pragma unroll
        for (uint32_t k = 0; k < PF; k++) ((uint4 *)Bw)[64u * k + lane] = pf[k];
        const uint32_t vn = v + gridDim.x;
        if (vn < bt.count) {                       /* next value's bytes, in flight */
            pn = bt.in_len[vn];
            const uint8_t *s1 = bt.in + bt.in_off[vn];
#pragma unroll
            for (uint32_t k = 0; k < PF; k++) {
                const uint32_t at = 16u * (64u * k + lane);
                pf[k] = at < pn ? dv_ld16_safe_w(s1 + at, pn - at) : make_uint4(0, 0, 0, 0);
            }
        }
        if (n >= 3u && n <= MAXN) {          /* a longer value: refused by the parse (n > max_len) */
            for (uint32_t k = lane; k < BUCKETS / 8u; k += 64u) ((uint4 *)H)[k] = make_uint4(0, 0, 0, 0);
            dv_wave_fence();
            const uint32_t np = n - 2u;               /* positions 0 .. n-3 */
            for (uint32_t P = 0; P < np; P += 64u * WIN) {
                uint32_t p[WIN], m[WIN], tri[WIN];
                bool act[WIN];
                /* the step's byte reads first, in one LDS round trip */
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++) {
                    p[j] = P + 64u * j + lane;
                    act[j] = p[j] < np;
                    tri[j] = ks_rd4(Bw, act[j] ? p[j] : 0u);
                }
                /* one lane-ordered 16-bit exchange per window on the bucket's
                 * head (ds_mskor_rtn_b32, tools/lds_mskor_order.hip): each lane
                 * gets the latest earlier position of its bucket -- the
                 * head's or an earlier lane's of the window -- and the
                 * highest lane's key stays.  The skip link of p is that
                 * predecessor when its identity differs, else the
                 * predecessor's own link (an earlier lane's: resolved by
                 * pointer doubling over the window's lanes); the same-slot
                 * predecessor follows the links from it until the identity
                 * matches.  Windows go in order: window j's links are in E
                 * before window j+1 exchanges. */
                uint32_t q1[WIN], cur[WIN];
                bool need = false;
                const uint32_t hb = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)H;
                /* the windows' exchanges in window order, then one wait (the
                 * results are outputs of the same asm statement) */
                uint32_t xa[WIN], xm[WIN], xd[WIN], xr[WIN], xs[WIN];
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++) {
                    m[j] = dv_mix(dv_slot(tri[j]));
                    const uint32_t h = act[j] ? (m[j] >> IDB) : BUCKETS + lane;
                    xs[j] = (h & 1u) << 4;
                    xa[j] = hb + 4u * (h >> 1);
                    xm[j] = 0xFFFFu << xs[j];
                    xd[j] = ((((p[j] + 1u) << IDB) | (m[j] & IDM)) & 0xFFFFu) << xs[j];
                }
                ks_xchg<WIN>(xr, xa, xm, xd);
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++) {
                    const uint32_t id = m[j] & IDM;
                    const uint32_t sh = xs[j], rv = xr[j];
                    const uint32_t prev = act[j] ? (rv >> sh) & 0xFFFFu : 0u;
                    const uint32_t ppos = (prev >> IDB) - 1u;            /* prev != 0 */
                    const uint32_t w0 = P + 64u * j;                      /* the window's first position */
                    const bool same = prev && (prev & IDM) == id;
                    /* link entry: resolved (bit 16 | link) or pending (the lane of
                     * an earlier same-slot position of this window) */
                    const uint32_t lprev = same && ppos < w0 ? (uint32_t)E[ppos] : 0u;
                    uint32_t le = !same ? (0x10000u | prev) : ppos >= w0 ? (ppos - w0) : (0x10000u | lprev);
                    /* six doublings resolve any chain inside 64 lanes; the cap bounds
                     * the loop even if the lane order failed (then lzf_selfcheck.hip
                     * has already routed compress batches away from this kernel) */
                    for (uint32_t r_ = 0; r_ < 6u && __ballot(!(le & 0x10000u)); r_++)
                        le = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((le & 0x10000u) ? lane : le) << 2), (int)le);
                    if (act[j]) E[p[j]] = (uint16_t)le;
                    dv_wave_fence();
                    /* same-slot predecessor: prev if its identity is mine, else
                     * along the links from prev's own link */
                    q1[j] = same ? (prev >> IDB) : 0u;                    /* pos+1 */
                    cur[j] = (prev && !same) ? (uint32_t)E[ppos] : 0u;
                    if (cur[j] && (cur[j] & IDM) == id) { q1[j] = cur[j] >> IDB; cur[j] = 0u; }
                    need |= cur[j] != 0u;
                }
                dv_wave_fence();
                while (__ballot(need)) {
                    need = false;
#pragma unroll
                    for (uint32_t j = 0; j < WIN; j++) {
                        if (cur[j]) {
                            /* links go to earlier positions; anything else ends the walk */
                            const uint32_t e0 = E[(cur[j] >> IDB) - 1u];
                            const uint32_t e = (e0 >> IDB) < (cur[j] >> IDB) ? e0 : 0u;
                            cur[j] = e;
                            if (e && (e & IDM) == (m[j] & IDM)) { q1[j] = e >> IDB; cur[j] = 0u; }
                            need |= cur[j] != 0u;
                        }
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++) {
                    if (!act[j]) continue;
                    uint32_t w = 0u;
                    if (q1[j] > 1u) {                    /* q = q1 - 1 > 0 */
                        const uint32_t q = q1[j] - 1u;
                        /* agreement of the bytes at p and q, <= 8, <= n - p:
                         * both dwords read at once (one LDS round trip) */
                        const uint32_t x0 = tri[j] ^ ks_rd4(Bw, q);
                        const uint32_t x1 = ks_rd4(Bw, p[j] + 4u) ^ ks_rd4(Bw, q + 4u);
                        const uint64_t xx = ((uint64_t)x1 << 32) | x0;
                        uint32_t k = xx ? (uint32_t)__builtin_ctzll(xx) >> 3 : 8u;
                        const uint32_t avail = n - p[j];
                        if (k > avail) k = avail;
                        w = (dv_code(k) << 13) | (p[j] - q - 1u);
                    }
                    cand[p[j]] = (uint16_t)w;
                }
            }
        }
        dv_wave_fence();
        v = vn;
    }
}

/* Small class, 16 KiB ("ring" form: values <= 16 KiB, so positions reach
 * 8 KiB past the window).  The value's bytes are staged whole as above; the
 * bucket heads are u32 [pos+1 | identity:4] (4096 buckets, 16 KiB) and the
 * skip links are kept only for the last 8192 positions, which is all a
 * candidate inside the window can reach, in a ring of u16 (16 KiB): a link
 * is [d:13 | identity bits 0-2], d = distance back to the target (0: none;
 * a target 8192 or more back is outside every later window).  A target whose
 * three stored identity bits match is confirmed from its bytes (its full slot
 * mix, read in the same LDS round trip as its own link).  A head or
 * link whose position is more than 8192 before p is outside p's window
 * (src/lzf_c.c:153 off < MAX_OFF) and ends the lookup: so is every older one.
 * The links of the step in flight go to S first and join the ring after the
 * step's walks, so that a walk never reads a ring slot the step overwrote.
 * LDS 50.6 KiB: 3 values per CU (u32 links: 66.8 KiB, 2 per CU).
 *
 * Against window64 at 1 M values of 16 KiB (tools/crossover.py): mixed
 * entropy (BASELINE configs[4]) 570 vs 648 ms, Zipf text 437 vs 938 ms,
 * sentence text 473 vs 676 ms.  With u32 links (2 values per CU) it was
 * 702 / 523 / 549 ms. */
#ifndef KR_WIN
#define KR_WIN  2u
#endif
template <uint32_t MAXN, uint32_t WIN>
__global__ __launch_bounds__(64) void lzf_cand_ring_kernel(LzfBatch bt, LzfLaneScratch sc)
{
    constexpr uint32_t IDB = 4u, IDM = 15u, BUCKETS = 4096u, RING = LZF_WINDOW;
    constexpr uint32_t T0 = 0u, T1 = 64u, T2 = 128u, TN = 144u;   /* digits as at 4 KiB */
    /* values past 16 KiB stream their bytes through a 16 KiB LDS ring in 1 KiB
     * chunks, one chunk in flight in registers: a step reads positions from
     * P - 8192 (the window) to P + 64*WIN + 12, and a chunk is stored only
     * once P + 64*WIN + 16 passes the bytes staged, so it never overwrites a
     * byte the window still reaches */
    constexpr bool STREAM = MAXN > KR_MAXN;
    constexpr uint32_t RB = 16384u, WM = RB / 4u - 1u;
    constexpr uint32_t PF = STREAM ? 1u : MAXN / 1024u;
    __shared__ __attribute__((aligned(16))) uint32_t H[BUCKETS];
    __shared__ uint16_t E[RING];
    __shared__ uint16_t S[64u * WIN];
    __shared__ __attribute__((aligned(16))) uint32_t Bw[STREAM ? RB / 4u : MAXN / 4u + 4u];
    __shared__ unsigned long long T[WIN][TN];
    const auto rd4 = [&](uint32_t x) -> uint32_t {
        if constexpr (STREAM) {
            const uint32_t w = x >> 2;
            return __builtin_amdgcn_alignbyte(Bw[(w + 1u) & WM], Bw[w & WM], x & 3u);
        } else {
            return ks_rd4(Bw, x);
        }
    };
    const uint32_t lane = threadIdx.x;
    const unsigned long long mine = 1ull << lane, below = mine - 1ull;
    uint32_t v = blockIdx.x;
    if (v >= bt.count) return;
    for (uint32_t k = lane; k < WIN * TN; k += 64u) (&T[0][0])[k] = 0ull;
    uint4 pf[PF];
    uint32_t pn = bt.in_len[v];
    if (!STREAM) {
        const uint8_t *s0 = bt.in + bt.in_off[v];
#pragma unroll
        for (uint32_t k = 0; k < PF; k++) {
            const uint32_t at = 16u * (64u * k + lane);
            pf[k] = at < pn ? dv_ld16_safe_w(s0 + at, pn - at) : make_uint4(0, 0, 0, 0);
        }
    }
    while (v < bt.count) {
        const uint32_t n = pn;
        uint16_t *cand = sc.cand + (uint64_t)v * sc.cstride;
        const uint8_t *src = bt.in + bt.in_off[v];
        uint32_t L = 0u;                           /* STREAM: bytes staged in the ring */
        if (!STREAM) {
#pragma unroll
            for (uint32_t k = 0; k < PF; k++) ((uint4 *)Bw)[64u * k + lane] = pf[k];
        } else {                                   /* the first chunk */
            pf[0] = 16u * lane < n ? dv_ld16_safe_w(src + 16u * lane, n - 16u * lane) : make_uint4(0, 0, 0, 0);
        }
        const uint32_t vn = v + gridDim.x;
        if (vn < bt.count) pn = bt.in_len[vn];
        if (!STREAM && vn < bt.count) {            /* next value's bytes, in flight */
            pn = bt.in_len[vn];
            const uint8_t *s1 = bt.in + bt.in_off[vn];
#pragma unroll
            for (uint32_t k = 0; k < PF; k++) {
                const uint32_t at = 16u * (64u * k + lane);
                pf[k] = at < pn ? dv_ld16_safe_w(s1 + at, pn - at) : make_uint4(0, 0, 0, 0);
            }
        }
        if (n >= 3u) {
            for (uint32_t k = lane; k < BUCKETS / 4u; k += 64u) ((uint4 *)H)[k] = make_uint4(0, 0, 0, 0);
            dv_wave_fence();
            const uint32_t np = n - 2u;               /* positions 0 .. n-3 */
            for (uint32_t P = 0; P < np; P += 64u * WIN) {
                if (STREAM && L < n && L < P + 64u * WIN + 16u) {
                    ((uint4 *)Bw)[((L >> 4) + lane) & (RB / 16u - 1u)] = pf[0];
                    L += 1024u;
                    const uint32_t at = L + 16u * lane;
                    pf[0] = at < n ? dv_ld16_safe_w(src + at, n - at) : make_uint4(0, 0, 0, 0);
                    dv_wave_fence();
                }
                uint32_t p[WIN], m[WIN], tri[WIN];
                bool act[WIN];
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++) {
                    p[j] = P + 64u * j + lane;
                    act[j] = p[j] < np;
                    tri[j] = rd4(act[j] ? p[j] : 0u);
                }
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++) {
                    m[j] = dv_mix(dv_slot(tri[j]));
                    if (act[j]) {
                        __hip_atomic_fetch_or(&T[j][T0 + ((m[j] >> IDB) & 63u)], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_or(&T[j][T1 + (m[j] >> (IDB + 6u))], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        __hip_atomic_fetch_or(&T[j][T2 + (m[j] & IDM)], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                dv_wave_fence();
                unsigned long long MB[WIN], MS[WIN];
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++) {
                    MB[j] = T[j][T0 + ((m[j] >> IDB) & 63u)] & T[j][T1 + (m[j] >> (IDB + 6u))];
                    MS[j] = MB[j] & T[j][T2 + (m[j] & IDM)];
                    if (!act[j]) MB[j] = MS[j] = 0ull;
                }
                dv_wave_fence();
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++) {
                    if (act[j]) {
                        T[j][T0 + ((m[j] >> IDB) & 63u)] = 0ull;
                        T[j][T1 + (m[j] >> (IDB + 6u))] = 0ull;
                        T[j][T2 + (m[j] & IDM)] = 0ull;
                    }
                }
                /* a head x = [y+1 | id] is inside p's window iff y + 8192 >= p;
                 * the link of position y is in S while y belongs to this step */
#define KR_INW(x_, p_) ((x_) != 0u && ((x_) >> IDB) + (RING - 1u) >= (p_))
#define KR_LINK(y_) ((uint32_t)((y_) >= P ? S[(y_) - P] : E[(y_) & (RING - 1u)]))
                uint32_t q1[WIN], cp[WIN], ci[WIN];   /* candidate: pos+1 (0: none), id bits 0-2 */
                bool need = false;
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++) {
                    const uint32_t bk = m[j] >> IDB, id = m[j] & IDM;
                    const uint32_t key = ((p[j] + 1u) << IDB) | id;
                    const unsigned long long ss = MS[j] & below, sb = MB[j] & ~MS[j] & below;
                    const uint32_t h0 = act[j] ? H[bk] : 0u;
                    const uint32_t h = KR_INW(h0, p[j]) ? h0 : 0u;
                    /* the head's link: target pos+1 (0: none or out of window), id bits */
                    uint32_t ey = 0u, ei = 0u;
                    if (h) {
                        const uint32_t e = KR_LINK((h >> IDB) - 1u);
                        ey = e ? (h >> IDB) - (e >> 3) : 0u;
                        if (ey + (RING - 1u) < p[j]) ey = 0u;
                        ei = e & 7u;
                    }
                    /* skip link: latest earlier bucket position with another identity */
                    const uint32_t lsb = sb ? ks_hibit(sb) : lane;
                    const uint32_t ksb = (uint32_t)__shfl((int)key, (int)lsb);
                    uint32_t ty, ti;                                  /* link target pos+1, id bits */
                    if (sb) { ty = ksb >> IDB; ti = ksb & 7u; }
                    else if (h && (h & IDM) != id) { ty = h >> IDB; ti = h & 7u; }
                    else { ty = ey; ti = ei; }
                    const uint32_t d = p[j] + 1u - ty;                /* >= 1 when ty != 0 */
                    if (act[j]) S[p[j] - P] = (uint16_t)((ty && d < RING) ? ((d << 3) | ti) : 0u);
                    if (act[j] && (MB[j] >> lane) == 1ull) H[bk] = key;
                    /* same-slot predecessor (pos+1), inside the window */
                    q1[j] = ss ? P + 64u * j + ks_hibit(ss) + 1u : 0u;
                    cp[j] = 0u;
                    ci[j] = ei;
                    if (act[j] && !ss && h) {
                        if ((h & IDM) == id) q1[j] = h >> IDB;
                        else cp[j] = ey;                              /* walk from the head's link */
                    }
                    need |= cp[j] != 0u;
                }
                dv_wave_fence();
                /* per hop: the candidate's link and bytes in one LDS round trip;
                 * it is the same-slot predecessor iff its slot mix equals mine */
                while (__ballot(need)) {
                    need = false;
#pragma unroll
                    for (uint32_t j = 0; j < WIN; j++) {
                        if (cp[j]) {
                            const uint32_t y = cp[j] - 1u;
                            const uint32_t e = KR_LINK(y);
                            const uint32_t ty = rd4(y);
                            if (ci[j] == (m[j] & 7u) && dv_mix(dv_slot(ty)) == m[j]) {
                                q1[j] = cp[j];
                                cp[j] = 0u;
                            } else {
                                uint32_t ny = e ? cp[j] - (e >> 3) : 0u;
                                if (ny + (RING - 1u) < p[j]) ny = 0u;
                                cp[j] = ny;
                                ci[j] = e & 7u;
                                need |= ny != 0u;
                            }
                        }
                    }
                }
#undef KR_INW
#undef KR_LINK
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++) {
                    if (!act[j]) continue;
                    uint32_t w = 0u;
                    if (q1[j] > 1u) {                    /* q = q1 - 1 > 0, p - q - 1 < 8192 */
                        const uint32_t q = q1[j] - 1u;
                        const uint32_t x0 = tri[j] ^ rd4(q);
                        const uint32_t x1 = rd4(p[j] + 4u) ^ rd4(q + 4u);
                        const uint64_t xx = ((uint64_t)x1 << 32) | x0;
                        uint32_t k = xx ? (uint32_t)__builtin_ctzll(xx) >> 3 : 8u;
                        const uint32_t avail = n - p[j];
                        if (k > avail) k = avail;
                        w = (dv_code(k) << 13) | (p[j] - q - 1u);
                    }
                    cand[p[j]] = (uint16_t)w;
                }
                /* the step's links join the ring (every walk of the step is done) */
#pragma unroll
                for (uint32_t j = 0; j < WIN; j++)
                    if (act[j]) E[p[j] & (RING - 1u)] = S[64u * j + lane];
                dv_wave_fence();
            }
        }
        dv_wave_fence();
        v = vn;
    }
}

/* Mid class (values <= 64 KiB).  LDS: bucket heads [pos+1:16 | mix:16]
 * (8 KiB), a ring of the head each position displaced (its bucket
 * predecessor's key) over the last 8192 positions (32 KiB), and the keys of
 * the step in flight, which join the ring only after the step's walks. */
__global__ __launch_bounds__(64) void lzf_cand_mid_kernel(LzfBatch bt, LzfLaneScratch sc)
{
    __shared__ __attribute__((aligned(16))) uint32_t H[KM_BUCKETS];
    __shared__ uint32_t R[LZF_WINDOW];
    __shared__ uint32_t S[64u * K1_WIN];
    const uint32_t lane = threadIdx.x, v = blockIdx.x;
    const uint32_t n = bt.in_len[v];
    const uint8_t *src = bt.in + bt.in_off[v];
    uint16_t *cand = sc.cand + (uint64_t)v * sc.cstride;
    if (n < 3u) return;
    for (uint32_t k = lane; k < KM_BUCKETS / 4u; k += 64u) ((uint4 *)H)[k] = make_uint4(0, 0, 0, 0);
    dv_wave_fence();
    const uint32_t np = n - 2u;
    for (uint32_t P = 0; P < np; P += 64u * K1_WIN) {
        uint32_t p[K1_WIN], m[K1_WIN], key[K1_WIN], r[K1_WIN];
        bool act[K1_WIN];
#pragma unroll
        for (uint32_t j = 0; j < K1_WIN; j++) {
            p[j] = P + 64u * j + lane;
            act[j] = p[j] < np;
            m[j] = act[j] ? dv_mix(dv_slot(dv_tri(src, n, p[j]))) : 0u;
            key[j] = ((p[j] + 1u) << 16) | m[j];
        }
#pragma unroll
        for (uint32_t j = 0; j < K1_WIN; j++)
            r[j] = act[j] ? atomicMax(&H[m[j] >> 5], key[j]) : 0u;
        bool bad = sc.force_fix != 0u;
#pragma unroll
        for (uint32_t j = 0; j < K1_WIN; j++) bad |= act[j] && (r[j] >> 16) > p[j];
        if (__ballot(bad)) k1_fix_order<5>(r, key, act);
#pragma unroll
        for (uint32_t j = 0; j < K1_WIN; j++) S[64u * j + lane] = r[j];
        dv_wave_fence();
        uint32_t cur[K1_WIN];
        bool fd[K1_WIN], need = false;
#pragma unroll
        for (uint32_t j = 0; j < K1_WIN; j++) {
            cur[j] = r[j];
            /* an entry is usable while inside the window: p - q - 1 < 8192 */
            if (cur[j] && p[j] - (cur[j] >> 16) >= LZF_WINDOW) cur[j] = 0u;
            fd[j] = cur[j] != 0u && (cur[j] & 0xFFFFu) == m[j];
            need |= act[j] && !fd[j] && cur[j] != 0u;
        }
        while (__ballot(need)) {
            need = false;
#pragma unroll
            for (uint32_t j = 0; j < K1_WIN; j++) {
                if (act[j] && !fd[j] && cur[j] != 0u) {
                    const uint32_t x = (cur[j] >> 16) - 1u;
                    uint32_t e = x >= P ? S[x - P] : R[x & (LZF_WINDOW - 1u)];
                    if (e && p[j] - (e >> 16) >= LZF_WINDOW) e = 0u;
                    cur[j] = e;
                    fd[j] = e != 0u && (e & 0xFFFFu) == m[j];
                    need |= !fd[j] && e != 0u;
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < K1_WIN; j++) {
            if (!act[j]) continue;
            uint32_t w = 0u;
            if (fd[j] && (cur[j] >> 16) > 1u) {
                const uint32_t q = (cur[j] >> 16) - 1u;
                w = (dv_code(k1_agree(src, n, p[j], q)) << 13) | (p[j] - q - 1u);
            }
            cand[p[j]] = (uint16_t)w;
        }
        dv_wave_fence();
#pragma unroll
        for (uint32_t j = 0; j < K1_WIN; j++)
            if (act[j]) R[p[j] & (LZF_WINDOW - 1u)] = r[j];
        dv_wave_fence();
    }
}

/* ======================================================================== */
/* compress, kernel 2 (wave form): the parse 64 positions at a time         */
/* ======================================================================== */

/* One wave per value of the small class; the value's bytes, its cand words
 * and an inserted-bitmap live in LDS.  Per window of 64 positions from the
 * parse position P every lane decides its position as if the parse visited
 * it: its ref is the first inserted position on the cand chain, literal or
 * match, and the match length (cand agreement, else an 8-byte probe).  A
 * candidate before P is checked in the bitmap (decided); one inside the
 * window is assumed inserted.  The scalar unit then follows the parse's
 * orbit P -> P + step -> ... jumping over runs of literal lanes; lanes it
 * stops at that still need work get it there, so only visited positions pay
 * for it: a candidate found skipped is walked back along its cand chain, a
 * match longer than the probe is measured by the whole wave (256 bytes at
 * once).  A visited lane whose in-window candidate turns out to lie in a
 * match interior (not inserted: src/lzf_c.c:227-247) ends the window there,
 * so every emitted token is the reference's.  Emission is closed form over
 * the window's tokens (prefix sum of output sizes; a run's header is written
 * when the run closes) with the reference's out-of-space checks. */
/* -DKW_PHASES: cycles per phase of the wave-form parse, summed in k2_sites[0..7] */
#ifdef KW_PHASES
#define KW_PH(i) do { const uint64_t t_ = clock64(); ph_[i] += t_ - ph_t; ph_t = t_; } while (0)
#else
#define KW_PH(i) ((void)0)
#endif

/* lane states of a window */
#define KW_LIT   0u    /* literal */
#define KW_MATCH 1u    /* match of length m */
#define KW_LONG  2u    /* match of length >= k (k < lim), to be measured */
#define KW_WALK  3u    /* candidate q not inserted: walk the chain first */

/* literal or match at x given the ref q and its rel code (src/lzf_c.c:151-209) */
__device__ __forceinline__ void kw_decide(const uint32_t *Bw, uint32_t n, uint32_t x, bool act, uint32_t rel,
                                          uint32_t q, uint32_t &st, uint32_t &m, uint32_t &k, uint32_t &lim)
{
    st = KW_LIT;
    m = 1u;
    if (!(act && rel >= 2u && x + 4u < n)) return;
    uint32_t maxlen = n - x - 2u;                                     /* src/lzf_c.c:169-170 */
    if (maxlen > LZF_MAX_REF) maxlen = LZF_MAX_REF;
    lim = (maxlen > 16u && maxlen < 19u) ? 19u : maxlen;
    st = KW_MATCH;
    if (rel <= 6u) {
        m = rel + 1u < lim ? rel + 1u : lim;
        return;
    }
    k = rel == 7u ? 8u : 3u;
    const uint32_t d0 = ks_rd4(Bw, x + k) ^ ks_rd4(Bw, q + k);
    const uint32_t d1 = ks_rd4(Bw, x + k + 4u) ^ ks_rd4(Bw, q + k + 4u);
    if (d0) k += (uint32_t)__builtin_ctz(d0) >> 3;
    else if (d1) k += 4u + ((uint32_t)__builtin_ctz(d1) >> 3);
    else k += 8u;
    if (!(d0 | d1) && k < lim) st = KW_LONG;
    m = k < lim ? k : lim;
}

/* one link back along the cand chain from a skipped q */
__device__ __forceinline__ bool kw_hop(const uint16_t *Cw, uint32_t x, uint32_t &rel, uint32_t &q)
{
    K2_SITE(12);
    const uint32_t c2 = Cw[q], r2 = c2 >> 13, q2 = q - 1u - (c2 & 0x1FFFu);
    if (!r2 || x - q2 - 1u >= LZF_WINDOW) {
        rel = 0u;
        return false;
    }
    const bool e1 = rel >= 2u && rel <= 8u, e2 = r2 >= 2u;
    rel = rel == 9u ? 9u : (e1 && e2) ? 8u : (e1 != e2) ? 1u : 9u;
    q = q2;
    return true;
}

/* first inserted position on the cand chain from q (q < P: the bitmap is
 * final there); rel follows it: 8 equal (length unknown), 1 differ, 0 none.
 * A skipped position below P is never visited, so its cand word serves only
 * walks through it: the walk's start q0 is pointed straight at the result
 * (path compression; code 2 = 3 bytes equal, 1 = differ, 0 = none). */
__device__ __forceinline__ void kw_walk(const uint32_t *Bw, uint16_t *Cw, const uint32_t *IB, uint32_t x,
                                        uint32_t &rel, uint32_t &q, uint32_t q0)
{
    while (!((IB[q >> 5] >> (q & 31u)) & 1u)) {
        if (!kw_hop(Cw, x, rel, q)) {
            Cw[q0] = 0u;
            return;
        }
    }
    if (q != q0) {
        const bool eq = ((ks_rd4(Bw, q0) ^ ks_rd4(Bw, q)) & 0xFFFFFFu) == 0u;
        Cw[q0] = (uint16_t)(((eq ? 2u : 1u) << 13) | (q0 - q - 1u));
    }
    if (rel == 9u) rel = ((ks_rd4(Bw, x) ^ ks_rd4(Bw, q)) & 0xFFFFFFu) == 0u ? 8u : 1u;
}
__device__ __forceinline__ unsigned long long kw_range(uint32_t a, uint32_t b)   /* bits [a, b), a < 64 */
{
    const unsigned long long hi = b >= 64u ? ~0ull : (1ull << b) - 1ull;
    return hi & ~((1ull << a) - 1ull);
}

__global__ __launch_bounds__(64) void lzf_parse_wave_kernel(LzfBatch bt, LzfLaneScratch sc)
{
    __shared__ __attribute__((aligned(16))) uint32_t Bw[KW_MAXN / 4u + 8u];
    __shared__ __attribute__((aligned(16))) uint16_t Cw[KW_MAXN + 64u];
    __shared__ uint32_t IB[KW_MAXN / 32u + 4u];
    const uint32_t lane = threadIdx.x, v = blockIdx.x;
    const unsigned long long mine = 1ull << lane, lt = mine - 1ull;
    const uint32_t n = bt.in_len[v], cap = bt.out_cap[v];
    if (n == 0u || cap == 0u) {                                       /* src/lzf_c.c:131 */
        if (lane == 0u) bt.out_len[v] = 0u;
        return;
    }
    const uint8_t *src = bt.in + bt.in_off[v];
    uint8_t *dst = bt.out + bt.out_off[v];
    const uint32_t np = n >= 3u ? n - 2u : 0u;                        /* positions 0 .. n-3 */
#ifdef KW_PHASES
    uint64_t ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ph_t = clock64();
#endif
    {
        const uint4 *cand = (const uint4 *)(sc.cand + (uint64_t)v * sc.cstride);
        for (uint32_t k = lane; k < (KW_MAXN / 4u + 8u) / 4u; k += 64u) {
            const uint32_t at = 16u * k;
            ((uint4 *)Bw)[k] = at < n ? dv_ld16_safe_w(src + at, n - at) : make_uint4(0, 0, 0, 0);
        }
        for (uint32_t k = lane; k < (np + 7u) / 8u; k += 64u) ((uint4 *)Cw)[k] = cand[k];
        for (uint32_t k = lane; k < KW_MAXN / 32u + 4u; k += 64u) IB[k] = 0u;
    }
    __syncthreads();
    KW_PH(0);
#define KW_BYTE(x_) ((Bw[(x_) >> 2] >> (8u * ((x_) & 3u))) & 0xFFu)
    uint32_t P = 0u, o = 1u, run = 0u;                                /* op, lit of the reference */
    bool ok = true;
    while (P < np) {
        if (lane == 0u) K2_SITE(11);
        const uint32_t x = P + lane;
        const bool act = x < np;
        const uint32_t c = act ? (uint32_t)Cw[x] : 0u;
        /* rel: 0 no ref; 1 ref with other bytes; 2..6 equal for rel+1 bytes;
         * 7 equal >= 8; 8 equal 3 bytes, length unknown; 9 unknown */
        uint32_t rel = c >> 13;
        uint32_t q = x - 1u - (c & 0x1FFFu);
        const bool spec = rel != 0u && q >= P;                        /* assumed inserted */
        uint32_t st = KW_LIT, m = 1u, k = 0u, lim = 0u;
        const uint32_t q1 = q;
        bool walk = rel != 0u && !spec && !((IB[q >> 5] >> (q & 31u)) & 1u);
        if (walk) {                                                   /* one link back, all lanes */
            walk = kw_hop(Cw, x, rel, q) && !((IB[q >> 5] >> (q & 31u)) & 1u);
            if (!walk && rel == 9u) rel = ((ks_rd4(Bw, x) ^ ks_rd4(Bw, q)) & 0xFFFFFFu) == 0u ? 8u : 1u;
        }
        if (walk) st = KW_WALK;
        else kw_decide(Bw, n, x, act, rel, q, st, m, k, lim);
        KW_PH(1);
        /* the orbit of the parse through the window: runs of literal lanes
         * are taken at once, the scalar loop stops at the other lanes */
        const uint32_t end = np - P < 64u ? np - P : 64u;             /* lanes that are positions */
        unsigned long long STOP = __ballot(st != KW_LIT), V = 0ull;
        uint32_t t = 0u;
        while (true) {
            const unsigned long long rest = STOP & ~((1ull << t) - 1ull);
            const uint32_t u = rest ? (uint32_t)__builtin_ctzll(rest) : 64u;
            if (u >= end) {
                V |= kw_range(t, end);
                t = end;
                break;
            }
            V |= kw_range(t, u + 1u);
            if (lane == 0u) K2_SITE(15);
            uint32_t su = (uint32_t)__builtin_amdgcn_readlane((int)st, (int)u);
            if (su == KW_WALK) {                                      /* skipped candidate */
                KW_PH(2);
                if (lane == 0u) K2_SITE(10);
                if (lane == u) {
                    kw_walk(Bw, Cw, IB, x, rel, q, q1);
                    kw_decide(Bw, n, x, act, rel, q, st, m, k, lim);
                }
                su = (uint32_t)__builtin_amdgcn_readlane((int)st, (int)u);
                KW_PH(6);
            }
            if (su == KW_LONG) {                                      /* the wave measures it */
                KW_PH(2);
                if (lane == 0u) K2_SITE(13);
                const uint32_t xu = P + u;
                const uint32_t qu = (uint32_t)__builtin_amdgcn_readlane((int)q, (int)u);
                const uint32_t ku = (uint32_t)__builtin_amdgcn_readlane((int)k, (int)u);
                const uint32_t lu = (uint32_t)__builtin_amdgcn_readlane((int)lim, (int)u);
                const uint32_t at = ku + 4u * lane;
                const uint32_t dd = at < lu ? ks_rd4(Bw, xu + at) ^ ks_rd4(Bw, qu + at) : 0xFFu;
                const unsigned long long dm = __ballot(dd != 0u);
                uint32_t mu = lu;
                if (dm) {
                    const uint32_t j = (uint32_t)__builtin_ctzll(dm);
                    const uint32_t dj = (uint32_t)__builtin_amdgcn_readlane((int)dd, (int)j);
                    const uint32_t e = ku + 4u * j + ((uint32_t)__builtin_ctz(dj) >> 3);
                    mu = e < lu ? e : lu;
                }
                if (lane == u) {
                    m = mu;
                    st = KW_MATCH;
                }
                su = KW_MATCH;
                KW_PH(7);
            }
            t = su == KW_LIT ? u + 1u : u + (uint32_t)__builtin_amdgcn_readlane((int)m, (int)u);
            if (t >= end) break;
        }
        KW_PH(2);
        const bool hit = st != KW_LIT;                                /* every visited lane is final */
        const unsigned long long HITm = __ballot(hit);
        const bool isv = (V >> lane) & 1ull;
        const uint32_t s = ks_hibit(V & (lt | mine));                 /* latest token <= lane */
        const uint32_t m_s = (uint32_t)__shfl((int)m, (int)s);
        const bool inm = !isv && ((HITm >> s) & 1ull);                /* inside s's match */
        const unsigned long long IM = __ballot(inm && lane + 2u < s + m_s);
        const unsigned long long INV = V & __ballot(spec && ((IM >> (q - P)) & 1ull));
        const uint32_t f = INV ? (uint32_t)__builtin_ctzll(INV) : 64u;
        if (lane == 0u && f < 64u) K2_SITE(14);
        const unsigned long long keep = f < 64u ? (1ull << f) - 1ull : ~0ull;
        const unsigned long long TK = V & keep;
        const unsigned long long INS = __ballot(isv || (inm && lane + 2u >= s + m_s)) & keep;
        KW_PH(3);

        /* emission (src/lzf_c.c:172-224, 258-273) */
        const bool tok = (TK >> lane) & 1ull;
        const unsigned long long Mb = TK & HITm, Lb = TK & ~HITm, mlt = Mb & lt;
        const unsigned long long seg = mlt ? lt & ~((2ull << ks_hibit(mlt)) - 1ull) : lt;
        const uint32_t lb = (uint32_t)__builtin_popcountll(Lb & seg);
        const uint32_t r0 = (mlt ? 0u : run) + lb;                    /* open run before lane */
        const uint32_t rl = r0 & 31u;
        /* output bytes of a token: literal 1 (+1 on a rollover); match 3
         * (+1 long form, -1 when it undoes an empty run): prefix sums as
         * lane-mask popcounts */
        const unsigned long long RL = __ballot(tok && !hit && ((r0 + 1u) & 31u) == 0u);
        const unsigned long long BG = __ballot(tok && hit && m - 2u >= 7u);
        const unsigned long long UD = __ballot(tok && hit && rl == 0u);
#define KW_MB(M_) __builtin_amdgcn_mbcnt_hi((uint32_t)((M_) >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)(M_), 0u))
        const uint32_t ob = o + KW_MB(TK) + KW_MB(RL) + 2u * KW_MB(Mb) + KW_MB(BG) - KW_MB(UD);
#undef KW_MB
        const uint32_t osum = (uint32_t)(__builtin_popcountll(TK) + __builtin_popcountll(RL) +
                                         2 * __builtin_popcountll(Mb) + __builtin_popcountll(BG) -
                                         __builtin_popcountll(UD));
        const uint32_t om = ob - (rl == 0u ? 1u : 0u);
        const bool bad = tok && (hit ? om + 4u >= cap : ob >= cap);   /* src/lzf_c.c:176, 263 */
        KW_PH(4);
        if (__ballot(bad)) {
            ok = false;
            break;
        }
        if (tok) {
            if (!hit) {
                dst[ob] = (uint8_t)KW_BYTE(x);
                if (((r0 + 1u) & 31u) == 0u) dst[ob - LZF_MAX_LIT] = (uint8_t)(LZF_MAX_LIT - 1u);
            } else {
                const uint32_t off = x - q - 1u, L = m - 2u;
                if (rl) dst[ob - rl - 1u] = (uint8_t)(rl - 1u);       /* close the run */
                if (L < 7u) {
                    dst[om] = (uint8_t)((off >> 8) | (L << 5));
                    dst[om + 1u] = (uint8_t)off;
                } else {
                    dst[om] = (uint8_t)(0xE0u | (off >> 8));
                    dst[om + 1u] = (uint8_t)(L - 7u);
                    dst[om + 2u] = (uint8_t)off;
                }
            }
        }
        /* inserted positions of the window; a match past the window inserts
         * its two last positions (src/lzf_c.c:227-247) */
        if (lane < 3u) {
            const uint32_t sh = P & 31u;
            const unsigned long long lo = INS << sh;
            const uint32_t w = lane == 0u ? (uint32_t)lo : lane == 1u ? (uint32_t)(lo >> 32)
                                                                      : (sh ? (uint32_t)(INS >> (64u - sh)) : 0u);
            if (w) IB[(P >> 5) + lane] |= w;
        }
        const uint32_t last = ks_hibit(TK);
        if (f == 64u && lane == last && hit && lane + m > 64u) {
            const uint32_t t1 = x + m - 2u, t2 = t1 + 1u;
            if (lane + m - 2u >= 64u) IB[t1 >> 5] |= 1u << (t1 & 31u);
            IB[t2 >> 5] |= 1u << (t2 & 31u);
        }
        o += osum;
        run = ((HITm >> last) & 1ull) ? 0u : (((uint32_t)__builtin_amdgcn_readlane((int)r0, (int)last) + 1u) & 31u);
        P = f < 64u ? P + f : P + t;
        KW_PH(5);
        dv_wave_fence();
    }
#ifdef KW_PHASES
    if (lane == 0u)
        for (uint32_t i = 0; i < 8u; i++) atomicAdd(&k2_sites[i], (unsigned long long)ph_[i]);
#endif
    if (lane == 0u) {
        if (!ok || o + 3u > cap) {                                    /* src/lzf_c.c:276 */
            bt.out_len[v] = 0u;
        } else {
            for (uint32_t p = P; p < n; p++) {                        /* src/lzf_c.c:279-288 */
                dst[o++] = (uint8_t)KW_BYTE(p);
                if (++run == LZF_MAX_LIT) {
                    dst[o - LZF_MAX_LIT - 1u] = (uint8_t)(LZF_MAX_LIT - 1u);
                    run = 0u;
                    o++;
                }
            }
            if (run) dst[o - run - 1u] = (uint8_t)(run - 1u);
            else o--;
            bt.out_len[v] = o;
        }
    }
#undef KW_BYTE
}

/* ---- the launcher's hooks (lzf_lane_dev.h) -------------------------------- */

bool lzf_lane_diag_cand_small(void)
{
    const char *e = getenv("LZF_GPU_CAND");
    return e && !strcmp(e, "small");
}

static bool lane_ring_enabled()
{
    const char *r = getenv("LZF_GPU_LANE_RING");     /* "0" turns the ring class off */
    return !(r && *r == '0');
}

/* LZF_GPU_CAND=small takes the small and ring classes (values <= 64 KiB;
 * LZF_GPU_LANE_RING=0 stops it at 8 KiB, and LZF_GPU_LANE_MID=1 then routes
 * values up to 64 KiB through the mid-class kernel). */
bool lzf_lane_diag_supported(uint32_t max_len)
{
    if (max_len <= KS8_MAXN) return true;
    if (max_len <= KR64_MAXN && lane_ring_enabled()) return true;
    const char *e = getenv("LZF_GPU_LANE_MID");
    return max_len <= KM_MAXN && e && *e == '1';
}

bool lzf_lane_diag_cand(const LzfBatch &c, const LzfLaneScratch &sc, uint32_t max_len, hipStream_t s)
{
    if (!lzf_lane_diag_cand_small()) return false;
    const bool ring = max_len > KS8_MAXN && max_len <= KR64_MAXN && lane_ring_enabled();
    if (max_len > KS8_MAXN && !ring) {
        hipLaunchKernelGGL(lzf_cand_mid_kernel, dim3(c.count), dim3(64), 0, s, c, sc);
        return true;
    }
    /* the small and ring kernels are persistent: as many one-wave workgroups
     * as stay resident (LDS-bound), each walking the batch */
    const void *fn = max_len <= KS_MAXN    ? (const void *)lzf_cand_small_kernel<4u, KS_MAXN, KS_WIN>
                     : max_len <= KS8_MAXN ? (const void *)lzf_cand_small_kernel<3u, KS8_MAXN, KS8_WIN>
                     : max_len <= KR_MAXN  ? (const void *)lzf_cand_ring_kernel<KR_MAXN, KR_WIN>
                                           : (const void *)lzf_cand_ring_kernel<KR64_MAXN, KR_WIN>;
    uint32_t grid = 256u * 8u;
    int dev = 0, cus = 0;
    hipFuncAttributes fa;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        hipFuncGetAttributes(&fa, fn) == hipSuccess && cus > 0 && fa.sharedSizeBytes > 0) {
        uint32_t per = (uint32_t)(160u * 1024u / fa.sharedSizeBytes);   /* LDS-bound residency */
        const char *pe = getenv("LZF_LANE_CAND_PER");                 /* residency override */
        if (pe && atoi(pe) > 0) per = (uint32_t)atoi(pe);
        if (per > 32u) per = 32u;
        if (per < 1u) per = 1u;
        grid = (uint32_t)cus * per;
    }
    const uint32_t g = c.count < grid ? c.count : grid;
    if (max_len <= KS_MAXN)
        hipLaunchKernelGGL((lzf_cand_small_kernel<4u, KS_MAXN, KS_WIN>), dim3(g), dim3(64), 0, s, c, sc);
    else if (max_len <= KS8_MAXN)
        hipLaunchKernelGGL((lzf_cand_small_kernel<3u, KS8_MAXN, KS8_WIN>), dim3(g), dim3(64), 0, s, c, sc);
    else if (max_len <= KR_MAXN)
        hipLaunchKernelGGL((lzf_cand_ring_kernel<KR_MAXN, KR_WIN>), dim3(g), dim3(64), 0, s, c, sc);
    else
        hipLaunchKernelGGL((lzf_cand_ring_kernel<KR64_MAXN, KR_WIN>), dim3(g), dim3(64), 0, s, c, sc);
    return true;
}

bool lzf_lane_diag_parse(const LzfBatch &c, const LzfLaneScratch &sc, uint32_t max_len, hipStream_t s)
{
    const char *pe = getenv("LZF_GPU_LANE_PARSE");
    if (!(max_len <= KW_MAXN && pe && pe[0] == 'w')) return false;
    hipLaunchKernelGGL(lzf_parse_wave_kernel, dim3(c.count), dim3(64), 0, s, c, sc);
    return true;
}

int lzf_lane_diag_sites(unsigned long long *out16, int reset)
{
#if defined(K2_COUNT_SITES) || defined(KW_PHASES) || defined(K2_WAVE_SITES)
    return k2_sites_add(out16, reset);
#else
    (void)out16;
    (void)reset;
    return 0;
#endif
}
