/*
 * carve_check.cpp -- every work-area layout of the device store against its
 * size (`make carve_check`, run by tests/test_work_sizes.py).  A stand-alone
 * host program: its own main, no kernel, not linked to the library; it is
 * built with the host sanitizers together with lzf_layout.cpp.
 *
 * For every layout, every n in (1, 63, 1023, 1024, 1025, 4097) -- mset also
 * over vlen in (1, 15, 16, 4096), set_store over in_bytes in (1, 65536) -- and
 * every misalignment 0 .. 15 of the work pointer: a buffer of exactly
 * work_size bytes is carved at its start plus the misalignment (the size's
 * slack is what lets a caller align, so the buffer grows by the misalignment),
 * every byte of every array the layout hands out is written, and every
 * pointer is checked for its element type's alignment.  A layout that hands
 * out more than its size is a heap overflow under AddressSanitizer; arrays
 * that overlap show as a wrong fill byte.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lzf_store_layout.h"

static int g_bad = 0;
static unsigned g_arrays = 0;

struct Span {
    uint8_t *p;
    uint64_t bytes;
};

static Span g_span[32];
static unsigned g_nspan;
static const char *g_layout[32];          /* the layouts settled so far, each name once */
static unsigned g_nlayout;

template <typename T>
static void fill(const char *what, T *p, uint64_t count)
{
    if ((uintptr_t)p % alignof(T)) {
        fprintf(stderr, "carve_check: %s at %p is not aligned to %zu\n", what, (void *)p, alignof(T));
        g_bad = 1;
        return;
    }
    memset((void *)p, (int)(0x11u + g_nspan), count * sizeof(T));
    g_span[g_nspan++] = Span{(uint8_t *)p, count * sizeof(T)};
    g_arrays++;
}

/* after all the fills: every array still holds its own byte, so no two overlap */
static void settle(const char *what, uint64_t n)
{
    for (unsigned k = 0; k < g_nspan; k++)
        for (uint64_t j = 0; j < g_span[k].bytes; j++)
            if (g_span[k].p[j] != (uint8_t)(0x11u + k)) {
                fprintf(stderr, "carve_check: %s n=%llu: array %u was overwritten at byte %llu\n", what,
                        (unsigned long long)n, k, (unsigned long long)j);
                g_bad = 1;
                j = g_span[k].bytes - 1u;
            }
    g_nspan = 0;
    for (unsigned k = 0; k < g_nlayout; k++)
        if (!strcmp(g_layout[k], what)) return;
    g_layout[g_nlayout++] = what;
}

/* run `use` on a buffer of exactly `size` bytes at every misalignment */
template <typename F>
static void at_every_misalignment(uint64_t size, F use)
{
    for (unsigned mis = 0; mis < 16u; mis++) {
        uint8_t *buf = (uint8_t *)malloc(size + mis);
        if (!buf) {
            fprintf(stderr, "carve_check: out of memory\n");
            exit(2);
        }
        use(buf + mis);
        free(buf);
    }
}

int main()
{
    static const uint32_t ns[] = {1u, 63u, 1023u, 1024u, 1025u, 4097u};
    static const uint32_t vlens[] = {1u, 15u, 16u, 4096u};
    static const uint64_t in_bytes[] = {1u, 65536u};
    for (const uint32_t n : ns) {
        const uint64_t nt = sd_tiles(n);
        at_every_misalignment(lzf_frame_work_bytes(n), [&](void *work) {
            LzfFrameArgs a{};
            a.count = n;
            lzf_frame_carve(a, work);
            fill("frame.w_off", a.w_off, n);
            fill("frame.w_voff", a.w_voff, n);
            fill("frame.w_bsum", a.w_bsum, sd_frame_tiles(n));
            fill("frame.w_state", a.w_state, 2);
            fill("frame.w_len", a.w_len, n);
            fill("frame.w_err", a.w_err, n);
            fill("frame.w_skip", a.w_skip, n);
            settle("frame", n);
        });
        for (const uint64_t ib : in_bytes)
            at_every_misalignment(lzf_store_work_bytes(n, ib), [&](void *work) {
                LzfStoreArgs a{};
                a.count = n;
                a.in_bytes = ib;
                lzf_store_carve(a, work);
                fill("store.w_state", a.w_state, SD_STATE_WORDS);
                fill("store.w_slot_off", a.w_slot_off, n);
                fill("store.w_tile", a.w_tile, nt);
                fill("store.w_len", a.w_len, n);
                fill("store.w_cap", a.w_cap, n);
                fill("store.w_out", a.w_out, n);
                fill("store.w_slots", a.w_slots, sd_slot_room(ib, n) + 16u);   /* and the realigning loads' 16 */
                settle("store", n);
            });
        at_every_misalignment(lzf_compact_work_bytes(n), [&](void *work) {
            LzfCompactArgs a{};
            a.count = n;
            lzf_compact_carve(a, work);
            fill("compact.w_state", a.w_state, SD_STATE_WORDS);
            fill("compact.w_tile_n", a.w_tile_n, nt);
            fill("compact.w_tile_b", a.w_tile_b, nt);
            fill("compact.w_tile_d", a.w_tile_d, nt);
            fill("compact.w_live_dst", a.w_live_dst, n);
            fill("compact.w_live_src", a.w_live_src, n);
            settle("compact", n);
        });
        at_every_misalignment(lzf_renumber_work_bytes(n), [&](void *work) {
            LzfRenumberArgs a{};
            a.count = n;
            lzf_renumber_carve(a, work);
            fill("renumber.w_state", a.w_state, SD_STATE_WORDS);
            fill("renumber.w_tile_n", a.w_tile_n, nt);
            fill("renumber.w_tile_b", a.w_tile_b, nt);
            fill("renumber.w_tile_d", a.w_tile_d, nt);
            settle("renumber", n);
        });
        at_every_misalignment(lzf_append_work_bytes(n), [&](void *work) {
            LzfAppendArgs a{};
            a.n = n;
            lzf_append_carve(a, work);
            fill("append.w_state", a.w_state, SD_STATE_WORDS);
            fill("append.w_tile_n", a.w_tile_n, nt);
            fill("append.w_tile_b", a.w_tile_b, nt);
            settle("append", n);
        });
        at_every_misalignment(lzf_bucket_work_bytes(n), [&](void *work) {
            LzfBucketArgs a{};
            a.n = n;
            lzf_bucket_carve(a, work);
            fill("bucket.w_table", a.w_table, (uint64_t)LZF_RQ_NCLASS * nt);
            settle("bucket", n);
        });
        at_every_misalignment(lzf_select_work_bytes(n), [&](void *work) {
            LzfSelectArgs a{};
            a.count = n;
            lzf_select_carve(a, work);
            fill("select.w_mask", a.w_mask, nt * SD_WORDS);
            fill("select.w_tile", a.w_tile, nt);
            settle("select", n);
        });
        /* select_ordered: the candidate cap below, at and above n; the node cap small and large */
        for (const uint32_t cn : {1u, n, n + 1000u})
            for (const uint64_t nodes : {(uint64_t)1u, (uint64_t)3u * n, (uint64_t)4096u})
                at_every_misalignment(lzf_order_work_bytes(n, cn, nodes, 7u), [&](void *work) {
                    LzfOrderArgs a{};
                    a.count = n;
                    a.cand_cap = cn;
                    a.node_cap = nodes;
                    lzf_order_carve(a, work);
                    const uint64_t ct = sd_tiles(cn);
                    if (a.slots < 2u * nodes || (a.slots & (a.slots - 1u))) {
                        fprintf(stderr, "carve_check: order.slots %llu for %llu node words\n",
                                (unsigned long long)a.slots, (unsigned long long)nodes);
                        g_bad = 1;
                    }
                    fill("order.w_state", a.w_state, SD_STATE_WORDS);
                    fill("order.w_mask", a.w_mask, nt * SD_WORDS);
                    fill("order.w_tile_n", a.w_tile_n, nt);
                    fill("order.w_tile_b", a.w_tile_b, nt);
                    fill("order.w_tile_m", a.w_tile_m, nt);
                    fill("order.w_table", a.w_table, a.slots);
                    fill("order.w_ctile_n", a.w_ctile_n, ct);
                    fill("order.w_ctile_b", a.w_ctile_b, ct);
                    fill("order.w_row_off", a.w_row_off, cn);
                    fill("order.w_rows", a.w_rows, nodes);
                    fill("order.w_cand", a.w_cand, cn);
                    fill("order.w_live", a.w_live, cn);
                    fill("order.w_row_len", a.w_row_len, cn);
                    fill("order.w_sort0", a.w_sort[0], cn);
                    fill("order.w_sort1", a.w_sort[1], cn);
                    settle("order", n);
                });
        at_every_misalignment(lzf_mget_work_bytes(n), [&](void *work) {
            LzfMgetArgs a{};
            a.n = n;
            lzf_mget_carve(a, work);
            fill("mget.w_state", a.w_state, SD_STATE_WORDS);
            fill("mget.g_key_off", a.g_key_off, n);
            fill("mget.g_val_off", a.g_val_off, n);
            fill("mget.w_off", a.w_off, n);
            fill("mget.w_voff", a.w_voff, n);
            fill("mget.w_tile", a.w_tile, nt);
            fill("mget.w_tcnt", a.w_tcnt, nt);
            fill("mget.g_key_len", a.g_key_len, n);
            fill("mget.g_val_size", a.g_val_size, n);
            fill("mget.g_val_len", a.g_val_len, n);
            fill("mget.g_null", a.g_null, n);
            fill("mget.w_len", a.w_len, n);
            fill("mget.w_err", a.w_err, n);
            fill("mget.g_enc", a.g_enc, n);
            fill("mget.w_skip", a.w_skip, n);
            settle("mget", n);
        });
        at_every_misalignment(lzf_reply_work_bytes(n), [&](void *work) {
            LzfReplyArgs a{};
            a.n = n;
            lzf_reply_carve(a, work);
            fill("reply.w_state", a.w_state, SD_STATE_WORDS);
            fill("reply.g_val_off", a.g_val_off, n);
            fill("reply.w_off", a.w_off, n);
            fill("reply.w_voff", a.w_voff, n);
            fill("reply.w_tile", a.w_tile, nt);
            fill("reply.w_tcnt", a.w_tcnt, nt);
            fill("reply.g_val_size", a.g_val_size, n);
            fill("reply.g_val_len", a.g_val_len, n);
            fill("reply.g_null", a.g_null, n);
            fill("reply.w_len", a.w_len, n);
            fill("reply.w_err", a.w_err, n);
            fill("reply.g_enc", a.g_enc, n);
            fill("reply.g_code", a.g_code, n);
            fill("reply.g_cls", a.g_cls, n);
            fill("reply.w_skip", a.w_skip, (uint64_t)n * LZF_DECODE_NCLASS);
            settle("reply", n);
        });
        at_every_misalignment(lzf_minc_work_bytes(n), [&](void *work) {
            LzfMincArgs a{};
            a.n = n;
            lzf_minc_carve(a, work);
            fill("minc.w_state", a.w_state, SD_STATE_WORDS);
            fill("minc.w_val", a.w_val, n);
            fill("minc.w_tile", a.w_tile, nt);
            fill("minc.w_cls", a.w_cls, n);
            settle("minc", n);
        });
        for (const uint32_t vlen : vlens)
            at_every_misalignment(lzf_mset_work_bytes(n, vlen), [&](void *work) {
                LzfMsetArgs a{};
                a.n = n;
                a.vlen = vlen;
                lzf_mset_carve(a, work);
                fill("mset.w_state", a.w_state, SD_STATE_WORDS);
                fill("mset.c_off", a.c_off, 2);
                fill("mset.c_len", a.c_len, 3);
                if ((uintptr_t)a.w_slot % 16u) {
                    fprintf(stderr, "carve_check: mset.w_slot is not 16-byte aligned\n");
                    g_bad = 1;
                }
                fill("mset.w_slot", a.w_slot, sd_mset_slot_bytes(vlen));
                fill("mset.w_tile", a.w_tile, nt);
                fill("mset.w_cls", a.w_cls, ((uint64_t)n + 15u) & ~15ull);
                settle("mset", n);
            });
        at_every_misalignment(lzf_keys_work_bytes(n), [&](void *work) {
            LzfKeysArgs a{};
            a.n = n;
            lzf_keys_carve(a, work);
            fill("keys.w_state", a.w_state, SD_STATE_WORDS);
            fill("keys.w_tile_n", a.w_tile_n, nt);
            fill("keys.w_tile_b", a.w_tile_b, nt);
            settle("keys", n);
        });
    }
    if (g_bad) return 1;
    printf("carve_check: ok, %u arrays written; layouts:", g_arrays);
    for (unsigned k = 0; k < g_nlayout; k++) printf(" %s", g_layout[k]);
    printf("\n");
    return 0;
}
