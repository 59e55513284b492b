/*
 * lzf_lane.hip -- the "lane" generation of the LZF compressor for gfx950: what
 * the product library runs for values of at most 64 KiB (the routing of
 * lzf_api.cpp takes it up to 16 KiB).  Two kernels per batch, chunked by the
 * scratch size:
 *
 *   1. lzf_cand_stream_kernel (lzf_stream.hip), position-parallel: for every
 *      position p the nearest earlier position q with the same 16-bit slot
 *      (src/lzf_c.c:47-57, HLOG 16) -- whether or not the parse will insert q
 *      -- and how far the bytes at p and q agree (<= 8), packed into a u16
 *      per position in HBM scratch (the "cand" word: offset and dv_code,
 *      lzf_dev.h).
 *   2. lzf_parse_lane_kernel (here), ONE LANE PER VALUE: the reference's
 *      greedy parse and emission (src/lzf_c.c:145-290), bit-exact.  A wave
 *      advances 64 values at once, so one VALU instruction does the work of
 *      64 scalar steps.  The reference's ref at p is the latest INSERTED
 *      position of p's slot (src/lzf_c.c:147-149); every position the parse
 *      visits is inserted, plus the last two positions of each match
 *      (src/lzf_c.c:227-247), so ref(p) is the first position on the cand
 *      chain from p that is not inside an earlier match.  The lane keeps an
 *      inserted-bitmap of its value (the last 32 words in LDS, older words in
 *      HBM scratch) and walks the chain only past skipped positions.  Every
 *      wave memory instruction touches one line per lane, so the kernel is
 *      shaped to issue few of them.  Its output cursor is
 *      lzf_emit.h, shared with lzf_cand.hip's record parse.
 *
 * Scratch per value: 2 B/position (cand) + 1 bit/position (bitmap).
 *
 * The diagnostic library adds cross-check forms of both kernels and a lane
 * decoder (lzf_lane_diag.hip); the launcher below hands a launch to them
 * through the two hooks of lzf_lane_dev.h.
 */
#include "lzf_lane_dev.h"

#ifndef K2_THREADS
#define K2_THREADS 256u
#endif
#ifndef K2_CB
#define K2_CB      32u          /* cand words per parse block: 8, 16 or 32 (16 B each 8) */
#endif
#ifndef K2_RW
#define K2_RW      32u          /* bitmap words kept in LDS per lane (power of two) */
#endif

/* Debug builds (tools/build_variant.sh): -DK2_COUNT_SITES, per-site event
 * counts of the parse kernel's global memory accesses (K2_SITE,
 * lzf_lane_dev.h); with the diagnostic file's own (-DKW_PHASES) */
#if defined(K2_COUNT_SITES) || defined(KW_PHASES) || defined(K2_WAVE_SITES)
extern "C" int lzf_gpu_debug_sites(unsigned long long *out16, int reset)
{
    memset(out16, 0, 16 * sizeof(*out16));
    const int r = k2_sites_add(out16, reset);
    return r ? r : lzf_lane_diag_sites(out16, reset);
}
#endif
/* -DK2_WAVE_SITES: how often the WAVE runs each section of the lane parse
 * (once per wave pass, whatever its active lanes), in k2_sites[0..15] */
#ifdef K2_WAVE_SITES
#define K2_WS(i)                                                                   \
    do {                                                                           \
        const uint64_t b_ = __ballot(1);                                           \
        if ((b_ & (~b_ + 1ull)) == (1ull << (threadIdx.x & 63u))) wsc_[i]++;       \
    } while (0)
#else
#define K2_WS(i) ((void)0)
#endif

/* The lanes of a wave are at different points of their values, so the loop
 * is a state machine in which every lane does at most ONE unit of each kind
 * of work per iteration -- take the cand word of p, test one candidate for
 * insertion (or hop one link back), compare one 16-byte piece of a long
 * match, emit one literal or one back-reference -- and a long walk or match
 * of one lane costs the others only the small blocks it runs through. */
/* one trip taken when 6 lanes gain from it: with the persistent lanes, 2 trips
 * / 8 lanes cost json4k, mixed16k and text8k 1.6-2.7 % (profiles/r06/v) */
/* candidate tests per iteration.  Two, the record parse's setting, were not
 * kept (profiles/r03/INDEX.md); the one-trip loop stays because the kernel's
 * instruction stream depends on it (without it the same parse compiles to 12
 * more instructions, profiles/r16/toolkit/isa.md) */
#ifndef K2_NRES
#define K2_NRES 1u
#endif
#ifndef K2_LITMIN
#define K2_LITMIN   6u       /* lanes of the wave that must take a free-literal trip for it to run */
#endif
#ifndef K2_LITX
#define K2_LITX 1u       /* free-literal trips after a literal in the same iteration (0: none) */
#endif
#ifndef K2_LITB
#define K2_LITB 1        /* a trip takes up to 4 free literals (0: one) */
#endif
enum { K2_STEP = 0, K2_RESOLVE = 1, K2_DECIDE = 2, K2_EXTEND = 3, K2_EMIT = 4, K2_DONE = 5 };


/* the shared output cursor and bitmap ring (lzf_emit.h), with this parse's
 * site counter, ring index (a mask: K2_RW is a power of two) and input byte:
 * its window W is loaded at the first byte outside it, from that byte on */
#define EMIT_SITE(i) K2_SITE(i)
#define EMIT_RW K2_RW
#define EMIT_THREADS K2_THREADS
#define EMIT_RING_AT(w_) ((w_) & (K2_RW - 1u))
#define EMIT_BYTE(pos_, out_)                                                      \
    do {                                                                           \
        uint32_t d_ = (pos_) - wb;                                                 \
        if (d_ >= 16u) {                                                           \
            K2_SITE(6);                                                            \
            W = dv_ld16_safe_w(src + (pos_), n - (pos_));                          \
            wb = (pos_);                                                           \
            d_ = 0u;                                                               \
        }                                                                          \
        (out_) = (dv_sel4_bits(W, d_ >> 2) >> (8u * (d_ & 3u))) & 0xFFu;           \
    } while (0)
#include "lzf_emit.h"

__global__ __launch_bounds__(K2_THREADS) void lzf_parse_lane_kernel(LzfBatch bt, LzfLaneScratch sc)
{
    /* Persistent lanes: as many blocks as stay resident, lane l parsing
     * values l, l + G, l + 2G, ... (G lanes in the grid), so a wave stays
     * full while values remain: a wave's pass costs its instructions whatever
     * its active lanes, and one value's chain can be ~2x another's (mixed
     * data: 6.1 k wave passes for 3.4 k per value, profiles/r06/o).  A queue
     * handing out values as lanes finish balanced mixed data ~3 % better and
     * cost text and json 5-7 %: a load waits behind its lane's atomic
     * (profiles/r06/p-r). */
    uint32_t v = blockIdx.x * K2_THREADS + threadIdx.x;
    uint32_t n = 0u, cap = 0u;
    const uint8_t *src = nullptr;
    uint8_t *dst = nullptr;
    const uint16_t *cand = nullptr;
    uint32_t *bits = nullptr;

    /* output: aligned dwords at da; acc holds the bytes from dword fw on */
    uint32_t dm = 0u;
    uint8_t *da = nullptr;
    uint64_t acc = 0;
    uint32_t accn = 0u, fw = 0;
    uint32_t hx = 0u;                   /* header byte of the open run (index from da) */
    /* completed dwords [fs, fw) wait in pb0..2 and go out as one 16-byte
     * store: every store instruction of the wave touches 64 lines (one
     * per lane's value), so fewer, wider stores */
    uint32_t pb0 = 0u, pb1 = 0u, pb2 = 0u, fs = 0u;
    /* input: the 16 bytes from position wb; loaded at the first byte that
     * falls outside it (a literal, or a match extension's own piece) */
    uint32_t wb = 0xFFFFFFF0u;          /* none yet */
    uint4 W = make_uint4(0, 0, 0, 0);

    uint32_t o = 1u, run = 0u, p = 0u; /* o, run: the reference's op and lit */
    /* cand words [cb, cb+32): one 64-byte, line-aligned block.  A wave load
     * costs one line fetch per lane; the four loads of a block share it */
    uint32_t cb = 0xFFFFFFE0u;         /* none yet (p - cb >= 32 for every p) */
    uint4 C0 = W, C1 = W, C2 = W, C3 = W;
    uint32_t cw = 0u, curw = 0u;       /* inserted-bitmap word of p, in flight */
    /* the last K2_RW bitmap words of the value in LDS (word w at slot w % K2_RW,
     * lane-interleaved: conflict-free), older words in the scratch array;
     * only words [fl, cw) of the current value are ever read from it */
    __shared__ uint32_t k2_ring[K2_RW][K2_THREADS];
    uint32_t *const ring = &k2_ring[0][threadIdx.x];
    /* words [0, fl) are in the scratch array (EMIT_FLUSH_TO) */
    uint32_t fl = 0u;
    uint32_t ms = 0u, me = 0u;         /* the last match: [ms, me) */
    uint32_t rel = 0u, q = 0u, k = 0u, lim = 0u, m = 0u;
    bool ok = true, live = false;
    uint32_t mode = K2_DONE;
    [[maybe_unused]] uint32_t fm = 0u, fmb = 0xFFFFFFE0u;   /* K2_LITB: candidate mask of block fmb */
    /* the lane's next value */
#define K2_NEXT() (v + gridDim.x * K2_THREADS)
    /* The value after this one: its lengths and offsets are loaded when the
     * parse of v passes 31/32 of it, so a lane that finishes rarely waits */
    uint32_t nv = v, nn = 0u, ncap = 0u, rsv = 2u, tr2 = 0u;
    uint64_t nio = 0u, noo = 0u;
#define K2_LOAD_AHEAD()                                                            \
    do {                                                                           \
        if (nv < bt.count) {                                                       \
            nn = bt.in_len[nv];                                                    \
            ncap = bt.out_cap[nv];                                                 \
            nio = bt.in_off[nv];                                                   \
            noo = bt.out_off[nv];                                                  \
        }                                                                          \
        rsv = 2u;                                                                  \
    } while (0)
    /* take the value ahead, or the first after it that the parse does not
     * refuse (src/lzf_c.c:131; past the stated max_len, the scratch stride),
     * with its state fresh; none left: the lane idles */
#define K2_START()                                                                 \
    do {                                                                           \
        live = false;                                                              \
        for (;;) {                                                                 \
            if (rsv != 2u) K2_LOAD_AHEAD();                                        \
            if (nv >= bt.count) break;                                             \
            v = nv;                                                                \
            n = nn;                                                                \
            cap = ncap;                                                            \
            src = bt.in + nio;                                                     \
            dst = bt.out + noo;                                                    \
            nv = K2_NEXT();                                                        \
            rsv = 0u;                                                              \
            if (n != 0u && cap != 0u && n <= bt.max_len) {                         \
                live = true;                                                       \
                break;                                                             \
            }                                                                      \
            bt.out_len[v] = 0u;                                                    \
        }                                                                          \
        if (live) {                                                                \
            cand = sc.cand + (uint64_t)v * sc.cstride;                             \
            bits = sc.bits + (uint64_t)v * sc.bstride;                             \
            dm = (uint32_t)((uintptr_t)dst & 3u);                                  \
            da = dst - dm;                                                         \
            acc = 0;                                                               \
            accn = dm;                                                             \
            fw = 0u;                                                               \
            hx = dm;                                                               \
            pb0 = pb1 = pb2 = fs = 0u;                                             \
            wb = 0xFFFFFFF0u;                                                      \
            o = 1u;                                                                \
            run = p = 0u;                                                          \
            cb = 0xFFFFFFE0u;                                                      \
            cw = curw = fl = 0u;                                                   \
            ms = me = 0u;                                                          \
            ok = true;                                                             \
            fmb = 0xFFFFFFE0u;                                                     \
            tr2 = n - (n >> 5);                                                    \
            mode = n >= 3u ? K2_STEP : K2_DONE;                                    \
        } else {                                                                   \
            mode = K2_DONE;                                                        \
        }                                                                          \
    } while (0)
#ifdef K2_WAVE_SITES
    uint32_t wsc_[16] = {0u};
#endif

    K2_LOAD_AHEAD();                   /* nv = v: the lane's first value */
    K2_START();
    while (__ballot(live)) {
        if (mode != K2_DONE) K2_SITE(0);
        K2_WS(0);
        /* the next value's lengths and offsets */
        if (live && rsv != 2u && p >= tr2) K2_LOAD_AHEAD();
        /* ---- the cand word of p ------------------------------------------ */
        if (mode == K2_STEP) {                                            /* src/lzf_c.c:145 */
            if (p >= n - 2u) {
                mode = K2_DONE;
            } else {
                uint32_t d = p - cb;
                K2_SITE(10);
                K2_WS(1);
                if (d >= K2_CB) {
                    K2_SITE(1);
                    K2_WS(2);
                    cb = p & ~(K2_CB - 1u);
                    d = p - cb;
                    const uint4 *cp = (const uint4 *)(cand + cb);
                    C0 = cp[0];
                    if (K2_CB >= 16u) C1 = cp[1];
                    if (K2_CB >= 32u) {
                        C2 = cp[2];
                        C3 = cp[3];
                    }
                }
                const uint32_t dw = d >> 1;
                const uint4 Cq = dw < 8u ? (dw < 4u ? C0 : C1) : (dw < 12u ? C2 : C3);
                const uint32_t c = (dv_sel4_bits(Cq, dw & 3u) >> (16u * (d & 1u))) & 0xFFFFu;
                /* rel: 0 no ref; 1 ref with other bytes; 2..6 equal for rel+1
                 * bytes; 7 equal >= 8; 8 equal 3 bytes, length unknown; 9 unknown */
                rel = c >> 13;
                q = p - 1u - (c & 0x1FFFu);
                mode = rel ? K2_RESOLVE : K2_DECIDE;
            }
        }
        /* ---- is the candidate inserted? else one link back: up to K2_NRES
         * tests per iteration ---------------------------------------------- */
#pragma unroll
        for (uint32_t rt_ = 0; rt_ < K2_NRES; rt_++) {
            if (mode == K2_RESOLVE) {
                K2_WS(3);
                uint32_t word;
                if (q >= ms) {
                    word = (q > ms && q + 3u <= me) ? 0u : 0xFFFFFFFFu;         /* last match's interior */
                } else {
                    const uint32_t d = cw - (q >> 5);
                    if (d != 0u && (q >> 5) < fl) K2_SITE(3);
                    word = d == 0u ? curw : (q >> 5) >= fl ? EMIT_RING(q >> 5) : bits[q >> 5];
                }
                if ((word >> (q & 31u)) & 1u) {                              /* q is the ref */
                    if (rel == 9u) K2_SITE(5);
                    if (rel == 9u) {
                        /* one 4-byte load per side (q + 3 <= p + 2 < n, p >= 1):
                         * one memory wait instead of up to three */
                        const uint32_t x_ = dv_ld4(src + q) ^ (dv_ld4(src + p - 1u) >> 8);
                        rel = (x_ & 0xFFFFFFu) == 0u ? 8u : 1u;
                    }
                    mode = K2_DECIDE;
                } else {
                    K2_SITE(4);
                    const uint32_t c2 = cand[q];
                    const uint32_t r2 = c2 >> 13;
                    const uint32_t q2 = q - 1u - (c2 & 0x1FFFu);
                    if (!r2 || p - q2 - 1u >= LZF_WINDOW) {
                        rel = 0u;
                        mode = K2_DECIDE;
                    } else {
                        /* 3-byte agreements combine, exact ones do not: this parse's
                         * chains are short and the rule gained nothing here
                         * (profiles/r05/INDEX.md) */
                        rel = dv_comb(rel, r2, false);
                        q = q2;
                    }
                }
            }
        }
        /* ---- literal, or the start of a back-reference ------------------- */
        if (mode == K2_DECIDE) {
            K2_WS(4);
            curw |= 1u << (p & 31u);                                     /* p is inserted */
            if (!(rel >= 2u && p + 4u < n)) {                            /* src/lzf_c.c:151-166 */
                K2_WS(5);
                if (o >= cap) {                                          /* src/lzf_c.c:263 */
                    ok = false;
                    mode = K2_DONE;
                } else {
                    EMIT_LITERAL(p);
                    p++;
                    if ((p & 31u) == 0u) {
                        EMIT_FLUSH_TO(cw);
                        EMIT_RING(cw) = curw;
                        cw++;
                        curw = 0u;
                    }
                    mode = K2_STEP;
#if K2_LITX
                    /* free literals: while the next positions have no
                     * candidate at all (cand code 0: no earlier position with
                     * their slot in the window, so no inserted one either,
                     * src/lzf_c.c:153-158), and their cand word and byte are
                     * already in registers, they are literals with no memory
                     * access -- up to K2_LITX more per iteration */
                    /* only when enough lanes of the wave are at a literal at
                     * all (one ballot of the branch's lanes): on text, where
                     * few are, the wave skips the path */
                    bool go = true;
#if K2_LITB
                    /* K2_LITB: up to 4 free literals per trip.  fm: bit j set
                     * when cand word cb + j has a candidate (code != 0), made
                     * once per block on the path's first use of it */
                    if ((uint32_t)__builtin_popcountll(__ballot(true)) >= K2_LITMIN) {
                        K2_WS(6);
                        if (fmb != cb) {
                            K2_WS(7);
                            fm = 0u;
#pragma unroll
                            for (uint32_t k_ = 0; k_ < 8u; k_++) {
                                const uint4 Ck_ = k_ < 2u ? C0 : k_ < 4u ? C1 : k_ < 6u ? C2 : C3;
                                const uint32_t lo_ = dv_sel4_bits(Ck_, (2u * k_) & 3u), hi_ = dv_sel4_bits(Ck_, (2u * k_ + 1u) & 3u);
                                /* the high bytes of cand words 4k..4k+3 (their codes in bits 5-7) */
                                const uint32_t x_ = __builtin_amdgcn_perm(hi_, lo_, 0x07050301u);
                                /* bit 7 of each byte: its code is nonzero; the multiply gathers
                                 * bits 7, 15, 23, 31 into bits 28-31 (no carries reach them) */
                                const uint32_t t_ = (x_ | (x_ << 1) | (x_ << 2)) & 0x80808080u;
                                fm |= ((t_ * 0x00204081u) >> 28) << (4u * k_);
                            }
                            fmb = cb;
                        }
#pragma unroll
                        for (uint32_t e_ = 0; e_ < K2_LITX; e_++) {
                            const uint32_t d_ = p - cb, x_ = p - wb;
                            uint32_t r_ = 0u;
                            if (go && p < n - 2u && d_ < K2_CB && x_ < 16u && o < cap) {
                                const uint32_t z_ = fm >> d_;
                                r_ = z_ ? (uint32_t)__builtin_ctz(z_) : 32u;
                                r_ = min(r_, min(K2_CB - d_, 16u - x_));
                                r_ = min(r_, min(n - 2u - p, cap - o));
                                r_ = min(r_, min(LZF_MAX_LIT - run, 32u - (p & 31u)));
                                r_ = min(r_, run == 0u ? 3u : 4u);     /* acc: at most 4 new bytes per put */
                            }
                            go = r_ != 0u;
                            if ((uint32_t)__builtin_popcountll(__ballot(go)) < K2_LITMIN) break;
                            K2_WS(8);
                            if (go) {
                                K2_SITE(9);
                                curw |= ((1u << r_) - 1u) << (p & 31u);
                                const uint32_t lo_ = dv_sel4_bits(W, x_ >> 2), hi_ = dv_sel4_bits(W, (x_ >> 2) + 1u);
                                const uint32_t by_ = __builtin_amdgcn_alignbit(hi_, lo_, 8u * (x_ & 3u)) &
                                                     (r_ == 4u ? 0xFFFFFFFFu : (1u << (8u * r_)) - 1u);
                                const bool first_ = run == 0u;
                                hx = first_ ? 4u * fw + accn : hx;
                                EMIT_PUT(first_ ? (uint64_t)by_ << 8 : (uint64_t)by_, first_ ? r_ + 1u : r_);
                                o += r_;
                                run += r_;
                                if (run == LZF_MAX_LIT) { EMIT_PATCH(hx, LZF_MAX_LIT - 1u); run = 0u; o++; }
                                p += r_;
                                if ((p & 31u) == 0u) {
                                    EMIT_FLUSH_TO(cw);
                                    EMIT_RING(cw) = curw;
                                    cw++;
                                    curw = 0u;
                                }
                            }
                        }
                    }
#else
                    if ((uint32_t)__builtin_popcountll(__ballot(true)) >= K2_LITMIN)
#pragma unroll
                    for (uint32_t e_ = 0; e_ < K2_LITX; e_++) {
                        const uint32_t d_ = p - cb, x_ = p - wb;
                        go = go && p < n - 2u && d_ < K2_CB && x_ < 16u && o < cap;
                        if (go) {
                            const uint32_t dw_ = d_ >> 1;
                            const uint4 Cq_ = dw_ < 8u ? (dw_ < 4u ? C0 : C1) : (dw_ < 12u ? C2 : C3);
                            go = ((dv_sel4_bits(Cq_, dw_ & 3u) >> (16u * (d_ & 1u))) & 0xE000u) == 0u;
                        }
                        /* a trip the wave takes only when enough lanes gain
                         * from it: on text, where few do, the others would
                         * wait through it */
                        if ((uint32_t)__builtin_popcountll(__ballot(go)) < K2_LITMIN) break;
                        if (go) {
                            K2_SITE(9);
                            curw |= 1u << (p & 31u);
                            const uint32_t byte_ = (dv_sel4_bits(W, x_ >> 2) >> (8u * (x_ & 3u))) & 0xFFu;
                            const bool first_ = run == 0u;
                            hx = first_ ? 4u * fw + accn : hx;
                            EMIT_PUT(first_ ? byte_ << 8 : byte_, first_ ? 2u : 1u);
                            o++;
                            if (++run == LZF_MAX_LIT) { EMIT_PATCH(hx, LZF_MAX_LIT - 1u); run = 0u; o++; }
                            p++;
                            if ((p & 31u) == 0u) {
                                EMIT_FLUSH_TO(cw);
                                EMIT_RING(cw) = curw;
                                cw++;
                                curw = 0u;
                            }
                        }
                    }
#endif  /* K2_LITB */
#endif
                }
            } else {
                K2_WS(9);
                uint32_t maxlen = n - p - 2u;                            /* src/lzf_c.c:169-170 */
                if (maxlen > LZF_MAX_REF) maxlen = LZF_MAX_REF;
                lim = (maxlen > 16u && maxlen < 19u) ? 19u : maxlen;
                if (rel <= 6u) {
                    m = rel + 1u < lim ? rel + 1u : lim;
                    mode = K2_EMIT;
                } else {
                    k = rel == 7u ? 8u : 3u;
                    mode = K2_EXTEND;
                }
            }
        }
        /* ---- one 16-byte piece of a long match --------------------------- */
        if (mode == K2_EXTEND) {
            K2_WS(10);
            if (k < lim) {
                K2_SITE(7);
                const uint32_t avail = n - (p + k);
                const uint4 a = dv_ld16_safe_w(src + p + k, avail), b = dv_ld16_safe_w(src + q + k, avail);
                W = a;                                   /* literals after the match read it */
                wb = p + k;
                const uint32_t d = dv_first_diff(a, b);
                k += d;
                if (d < 16u) lim = k < lim ? k : lim;
            }
            if (k >= lim) {
                m = lim;
                mode = K2_EMIT;
            }
        }
        /* ---- the back-reference ------------------------------------------ */
        if (mode == K2_EMIT) {
            K2_WS(11);
            const uint32_t off = p - q - 1u;
            if (run) EMIT_PATCH(hx, run - 1u);                             /* close the run */
            else o--;                                                    /* undo empty run */
            if (o + 4u >= cap) {                                         /* src/lzf_c.c:176 */
                ok = false;
                mode = K2_DONE;
            } else {
                const uint32_t L = m - 2u;
                const bool two = L < 7u;
                EMIT_PUT(two ? ((off >> 8) | (L << 5)) | ((off & 0xFFu) << 8)
                           : (0xE0u | (off >> 8)) | ((L - 7u) << 8) | ((off & 0xFFu) << 16),
                       two ? 2u : 3u);
                o += two ? 2u : 3u;
                run = 0u;
                o++;                                                     /* reserve a header */
                ms = p;
                p += m;
                me = p;
                if (p >= n - 2u) {                                       /* src/lzf_c.c:229 */
                    mode = K2_DONE;
                } else {
                    /* the two last positions of the match are inserted, its interior not */
                    const uint32_t nw = p >> 5, t1 = p - 2u, t2 = p - 1u;
                    const uint32_t b1 = 1u << (t1 & 31u), b2 = 1u << (t2 & 31u);
                    if (nw == cw) {
                        curw |= b1 | b2;
                    } else {
                        K2_WS(12);
                        uint32_t wo = curw, wm = 0u, wn = 0u;
                        if ((t1 >> 5) == cw) wo |= b1; else if ((t1 >> 5) == nw) wn |= b1; else wm |= b1;
                        if ((t2 >> 5) == cw) wo |= b2; else if ((t2 >> 5) == nw) wn |= b2; else wm |= b2;
                        EMIT_FLUSH_TO(cw);
                        EMIT_RING(cw) = wo;
                        /* words cw+1 .. nw-2 are all interior (0), nw-1 holds tails */
                        for (uint32_t w = cw + 1u; w < nw; w++) {
                            EMIT_FLUSH_TO(w);
                            EMIT_RING(w) = w + 1u == nw ? wm : 0u;
                        }
                        curw = wn;
                        cw = nw;
                    }
                    mode = K2_STEP;
                }
            }
        }
        /* ---- a finished value: its tail (src/lzf_c.c:276-290), then the next */
        if (live && mode == K2_DONE) {
            if (!ok || o + 3u > cap) {                                    /* src/lzf_c.c:276 */
                bt.out_len[v] = 0u;
            } else {
                while (p < n) {                                           /* src/lzf_c.c:279-288 */
                    EMIT_LITERAL(p);
                    p++;
                }
                EMIT_FINISH();
                bt.out_len[v] = o;
            }
            K2_START();
        }
    }
#ifdef K2_WAVE_SITES
    for (uint32_t i_ = 0; i_ < 16u; i_++)
        if (wsc_[i_]) atomicAdd(&k2_sites[i_], (unsigned long long)wsc_[i_]);
#endif
#undef K2_NEXT
#undef K2_LOAD_AHEAD
#undef K2_START
}

/* ---- launcher ------------------------------------------------------------ */

/* cand words per value: a multiple of 64 (128 bytes), so the parse's 64-byte
 * blocks never straddle a line, plus slack for the last block */
static uint64_t lane_cstride(uint32_t max_len) { return (((uint64_t)max_len + 63u) & ~63ull) + 64u; }
static uint64_t lane_bstride(uint32_t max_len) { return ((((uint64_t)max_len + 31u) >> 5) + 3u) & ~3ull; }

size_t lzf_lane_scratch_per_value(uint32_t max_len)
{
    return (size_t)(lane_cstride(max_len) * 2u + lane_bstride(max_len) * 4u);
}

/* kernel 1 of the lane generation is the stream form (lzf_stream.hip: the
 * exact table, values back to back in one pipeline per CU; any value the
 * parse's 13-bit offsets and 16-bit positions cover).  The diagnostic build
 * can take its small, ring or mid class instead (LZF_GPU_CAND=small, read per
 * launch, a cross-check): json4k 1 M x 4 KiB runs 45.9 ms with the stream
 * form, 48.7 with the small class (cand 17.3 vs 19.9 ms, rocprof). */
const char *lzf_lane_cand_name(void) { return lzf_lane_diag_cand_small() ? "cand_small" : "cand_stream"; }

bool lzf_lane_compress_supported(uint32_t max_len)
{
    return lzf_lane_diag_cand_small() ? lzf_lane_diag_supported(max_len) : max_len <= LZF_SLOTS;
}

/* blocks of the lane parse resident on the whole device at once (0: unknown);
 * LZF_GPU_PARSE_RESIDENT overrides it (diagnostics) */
static uint32_t parse_resident(size_t lds)
{
    if (const char *e = getenv("LZF_GPU_PARSE_RESIDENT")) return (uint32_t)strtoul(e, nullptr, 10);
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void *)lzf_parse_lane_kernel, (int)K2_THREADS,
                                                     lds) != hipSuccess ||
        cus <= 0 || per <= 0) {
        (void)hipGetLastError();
        return 0u;
    }
    return (uint32_t)cus * (uint32_t)per;
}

hipError_t lzf_launch_compress_lane(const LzfBatch &b, hipStream_t s, void *scratch,
                                    size_t scratch_bytes, uint32_t force_fix, hipStream_t aux,
                                    hipEvent_t *ev, uint32_t *chunks)
{
    if (!lzf_lane_compress_supported(b.max_len)) return hipErrorInvalidValue;
    const uint64_t cstride = lane_cstride(b.max_len), bstride = lane_bstride(b.max_len);
    /* with an aux stream: two scratch halves, kernel 1 of chunk i+1 on s
     * overlaps kernel 2 of chunk i on aux */
    const bool pipe = aux != nullptr && ev != nullptr &&
                      scratch_bytes / 2u >= lzf_lane_scratch_per_value(b.max_len) + 512u && b.count >= 4u;
    const size_t half = pipe ? (scratch_bytes / 2u) & ~(size_t)255 : scratch_bytes;
    uint64_t chunk = half / lzf_lane_scratch_per_value(b.max_len);
    const auto bits_at = [&](uint64_t ch) { return ((ch * cstride * 2u) + 255u) & ~255ull; };
    while (chunk && bits_at(chunk) + chunk * bstride * 4u > half) chunk--;
    if (chunk == 0) return hipErrorInvalidValue;
    if (pipe) {                       /* at least 4 chunks so the stages overlap */
        const uint64_t quarter = (b.count + 3u) / 4u;
        if (quarter < chunk) chunk = quarter < 1024u ? (b.count < 1024u ? b.count : 1024u) : quarter;
    }
    if (chunks) *chunks = (uint32_t)((b.count + chunk - 1u) / chunk);
    LzfLaneScratch sc[2];
    for (int h = 0; h < 2; h++) {
        uint8_t *base = (uint8_t *)scratch + (pipe ? h * half : 0);
        sc[h].cand = (uint16_t *)base;
        sc[h].bits = (uint32_t *)(base + bits_at(chunk));
        sc[h].cstride = cstride;
        sc[h].bstride = bstride;
        sc[h].force_fix = force_fix;
    }
    const size_t parse_lds = lane_lds_for("LZF_LANE_PARSE_BLOCKS", 0u);
    if (parse_lds) {
        hipError_t e = hipFuncSetAttribute((const void *)lzf_parse_lane_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)parse_lds);
        if (e != hipSuccess) return e;
    }
    /* diagnostics: LZF_GPU_LANE_STAGE=1 runs kernel 1 only (its own time) */
    const char *stg = getenv("LZF_GPU_LANE_STAGE");
    const bool cand_only = stg && *stg == '1';
    hipError_t e;
    uint32_t i = 0;
    for (uint64_t first = 0; first < b.count; first += chunk, i++) {
        const uint32_t cnt = (uint32_t)((b.count - first) < chunk ? (b.count - first) : chunk);
        const int h = pipe ? (int)(i & 1u) : 0;
        LzfBatch c = b;
        c.in_off = b.in_off + first;
        c.in_len = b.in_len + first;
        c.out_off = b.out_off + first;
        c.out_cap = b.out_cap + first;
        c.out_len = b.out_len + first;
        c.count = cnt;
        /* scratch half h is free once kernel 2 of chunk i-2 is done */
        if (pipe && i >= 2u && (e = hipStreamWaitEvent(s, ev[2 + h], 0)) != hipSuccess) return e;
        /* kernel 1: the stream form, unless the diagnostic build took another */
        if (!lzf_lane_diag_cand(c, sc[h], b.max_len, s) &&
            (e = lzf_launch_cand_stream(c, sc[h], s)) != hipSuccess)
            return e;
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (cand_only) continue;
        hipStream_t s2 = s;
        if (pipe) {
            if ((e = hipEventRecord(ev[h], s)) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(aux, ev[h], 0)) != hipSuccess) return e;
            s2 = aux;
        }
        /* kernel 2: one lane per value (the diagnostic build's wave form is
         * slower today) */
        if (!lzf_lane_diag_parse(c, sc[h], b.max_len, s2)) {
            /* persistent lanes: as many blocks as stay resident */
            uint32_t grid = (cnt + K2_THREADS - 1u) / K2_THREADS;
            const uint32_t res = parse_resident(parse_lds);
            if (res && grid > res) grid = res;
            hipLaunchKernelGGL(lzf_parse_lane_kernel, dim3(grid), dim3(K2_THREADS), parse_lds, s2, c, sc[h]);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (pipe && (e = hipEventRecord(ev[2 + h], aux)) != hipSuccess) return e;
    }
    if (pipe) {                       /* join: s waits for the last kernel 2 of both halves */
        for (uint32_t h = 0; h < 2u && h < i; h++)
            if ((e = hipStreamWaitEvent(s, ev[2 + h], 0)) != hipSuccess) return e;
    }
    return hipSuccess;
}
