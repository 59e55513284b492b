/*
 * lzf_emit.h -- the output cursor and the inserted-bitmap ring of the two
 * one-lane-per-value parses (lzf_parse_lane_kernel, lzf_lane.hip;
 * lzf_parse_rec_kernel, lzf_cand.hip): the reference's emission
 * (src/lzf_c.c:172-224, 258-290) written once.
 *
 * Macros over the kernel's own locals, not a struct with members: both parses
 * are register-bound state machines whose instruction streams are pinned
 * (profiles/r16/toolkit/isa.md), and the same text compiles to the same code
 * by construction.  The kernel declares, with these names:
 *
 *   uint8_t *da; uint32_t dm;   dst rounded down to a dword, and dst - da
 *   uint64_t acc; uint32_t accn the bytes from dword fw on, and how many
 *   uint32_t fw, fs             completed dwords [fs, fw) wait in pb0..2
 *   uint32_t pb0, pb1, pb2      (slot fw - fs) and leave with the fourth as
 *                               one 16-byte store: every store instruction of
 *                               the wave touches one line per lane's value,
 *                               so fewer, wider stores
 *   uint32_t hx                 header byte of the open run (index from da)
 *   uint32_t o, run             the reference's op and lit
 *   uint32_t *ring, *bits; uint32_t fl
 *                               the last EMIT_RW bitmap words of the value in
 *                               LDS (lane-interleaved: conflict-free), words
 *                               [0, fl) in the scratch array
 *
 * and defines what differs between the two before it includes this file:
 *
 *   EMIT_SITE(i)          a debug build's event counter, else ((void)0)
 *   EMIT_BYTE(pos_, out_) out_ = the input byte at pos_, from the kernel's
 *                         16-byte window (each parse refills it its own way)
 *   EMIT_RING_AT(w_)      ring row of bitmap word w_: w_ & (RW - 1) or w_ % RW
 *   EMIT_RW, EMIT_THREADS ring words per lane, lanes per block
 *
 * Slot and patch selects instead of branches: every branch costs the wave its
 * exec-mask juggling.
 */
#ifndef GIBSON_AMD_LZF_EMIT_H
#define GIBSON_AMD_LZF_EMIT_H

#define EMIT_RING(w_) ring[EMIT_RING_AT(w_) * EMIT_THREADS]
/* a word goes to the scratch array, four at a time in one 16-byte store,
 * before its ring slot is reused: afterwards words [fl, w_] fit the ring */
#define EMIT_FLUSH_TO(w_)                                                          \
    do {                                                                           \
        while (fl + EMIT_RW <= (w_)) {                                             \
            *(uint4 *)(bits + fl) = make_uint4(EMIT_RING(fl), EMIT_RING(fl + 1u),  \
                                               EMIT_RING(fl + 2u), EMIT_RING(fl + 3u)); \
            fl += 4u;                                                              \
        }                                                                          \
    } while (0)
#define EMIT_STORE16(w_)                                                           \
    do {                                                                           \
        if (fs == 0u && dm != 0u) {        /* dst's first dword: bytes before dst are not ours */ \
            for (uint32_t t_ = dm; t_ < 4u; t_++) da[t_] = (uint8_t)(pb0 >> (8u * t_)); \
            const uint2 m_ = make_uint2(pb1, pb2);                                 \
            __builtin_memcpy(da + 4u, &m_, 8);                                     \
            const uint32_t l_ = (w_);                                              \
            __builtin_memcpy(da + 12u, &l_, 4);                                    \
        } else {                                                                   \
            const uint4 v_ = make_uint4(pb0, pb1, pb2, (w_));                      \
            __builtin_memcpy(da + 4u * fs, &v_, 16);                               \
        }                                                                          \
        EMIT_SITE(8);                                                              \
    } while (0)
/* cnt_ (<= 4) more output bytes */
#define EMIT_PUT(bytes_, cnt_)                                                     \
    do {                                                                           \
        acc |= (uint64_t)(bytes_) << (8u * accn);                                  \
        accn += (cnt_);                                                            \
        if (accn >= 4u) {                                                          \
            const uint32_t w_ = (uint32_t)acc, np_ = fw - fs;                      \
            pb0 = np_ == 0u ? w_ : pb0;                                            \
            pb1 = np_ == 1u ? w_ : pb1;                                            \
            pb2 = np_ == 2u ? w_ : pb2;                                            \
            if (np_ == 3u) {                                                       \
                EMIT_STORE16(w_);                                                  \
                fs = fw + 1u;                                                      \
            }                                                                      \
            fw++;                                                                  \
            acc >>= 32;                                                            \
            accn -= 4u;                                                            \
        }                                                                          \
    } while (0)
/* output byte x_ (a run header behind the cursor): still in acc, waiting in
 * pb0..2, or already stored */
#define EMIT_PATCH(x_, byte_)                                                      \
    do {                                                                           \
        if ((x_) >= 4u * fw) {                                                     \
            const uint32_t sh_ = 8u * ((x_) - 4u * fw);                            \
            acc = (acc & ~(0xFFull << sh_)) | ((uint64_t)(byte_) << sh_);          \
        } else if ((x_) >= 4u * fs) {                                              \
            const uint32_t i_ = ((x_) >> 2) - fs, sh_ = 8u * ((x_) & 3u);          \
            const uint32_t mk_ = ~(0xFFu << sh_), b_ = (uint32_t)(byte_) << sh_;  \
            pb0 = i_ == 0u ? (pb0 & mk_) | b_ : pb0;                               \
            pb1 = i_ == 1u ? (pb1 & mk_) | b_ : pb1;                               \
            pb2 = i_ == 2u ? (pb2 & mk_) | b_ : pb2;                               \
        } else {                                                                   \
            da[(x_)] = (uint8_t)(byte_);                                           \
        }                                                                          \
    } while (0)
/* one literal (src/lzf_c.c:258-273, 279-288) */
#define EMIT_LITERAL(pos_)                                                         \
    do {                                                                           \
        uint32_t byte_;                                                            \
        EMIT_BYTE(pos_, byte_);                                                    \
        const bool first_ = run == 0u;             /* the run's header slot first */ \
        hx = first_ ? 4u * fw + accn : hx;                                         \
        EMIT_PUT(first_ ? byte_ << 8 : byte_, first_ ? 2u : 1u);                   \
        o++;                                                                       \
        if (++run == LZF_MAX_LIT) { EMIT_PATCH(hx, LZF_MAX_LIT - 1u); run = 0u; o++; } \
    } while (0)
/* the value's end: close the run, then the dwords and bytes still held */
#define EMIT_FINISH()                                                              \
    do {                                                                           \
        if (run) EMIT_PATCH(hx, run - 1u);                                         \
        else o--;                                                                  \
        for (uint32_t i = fs; i < fw; i++) {                                       \
            const uint32_t wv = i == fs ? pb0 : i == fs + 1u ? pb1 : pb2;          \
            if (i == 0u && dm != 0u)                                               \
                for (uint32_t t = dm; t < 4u; t++) da[t] = (uint8_t)(wv >> (8u * t)); \
            else                                                                   \
                *(uint32_t *)(da + 4u * i) = wv;                                   \
        }                                                                          \
        for (uint32_t t = 0; t < accn; t++)                                        \
            if (4u * fw + t >= dm) da[4u * fw + t] = (uint8_t)(acc >> (8u * t));   \
    } while (0)

#endif
