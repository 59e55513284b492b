/*
 * lzf_internal.h -- shared definitions between the HIP kernels and the
 * C-ABI layer (lzf_api.cpp).  Not installed; the public boundary is
 * include/lzf.h and include/lzf_gpu.h.
 */
#ifndef GIBSON_AMD_LZF_INTERNAL_H
#define GIBSON_AMD_LZF_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* LZF format constants (reference src/lzf_c.c:74-76, src/lzfP.h:55) */
#define LZF_MAX_LIT   32u
#define LZF_WINDOW    8192u
#define LZF_MAX_REF   264u
#define LZF_SLOTS     65536u

/* one batch, device pointers */
struct LzfBatch {
    const uint8_t *in;
    const uint64_t *in_off;
    const uint32_t *in_len;
    uint8_t *out;
    const uint64_t *out_off;
    const uint32_t *out_cap;
    uint32_t *out_len;
    int32_t *err;          /* decompress only */
    uint32_t count;
    uint32_t max_len;      /* max in_len (compress) / max out_cap (decompress) */
    const uint8_t *skip;   /* decompress: values with skip[i] != 0 are left alone (NULL: none) */
};

/* the store's item arrays as one view, device pointers: what every index-list
 * operator and sweep reads and writes of an item besides its value.  A NULL
 * member means what it meant as a loose argument: no time arrays (item_time
 * and item_ttl NULL together), nothing expires; no item_lock, nothing is
 * locked; no last_access, none is kept.  The members are not const, as some
 * operator writes each of them; an operator that only reads an array says so
 * where its view is built (lzf_api.cpp) */
struct LzfItems {
    uint8_t *enc;
    uint32_t count;
    int64_t *item_time;
    int32_t *item_ttl;
    int64_t *item_lock;
    int64_t *last_access;
    int64_t now;
};

/* the decode size classes (the rule: lzf_size_class_of, lzf_dev.h); here
 * because the reply work area holds one skip list per class */
#define LZF_DECODE_NCLASS 3u
#define LZF_DECODE_EDGE0  4096u
#define LZF_DECODE_EDGE1  16384u

/* the MGET reply frame (lzf_frame.hip); device pointers */
struct LzfFrameArgs {
    const uint8_t *keys;
    const uint64_t *key_off;
    const uint32_t *key_len;
    const uint8_t *vals;
    const uint64_t *val_off;
    const uint32_t *val_size;
    const uint8_t *enc;
    const uint32_t *val_len;
    uint32_t count, elements;
    uint32_t max_val_len;
    int reply_header;
    uint64_t max_response;
    uint8_t *frame;
    uint64_t *frame_len;
    /* work area (lzf_frame_layout, lzf_store_layout.h) */
    uint64_t *w_off, *w_voff, *w_bsum, *w_state;
    uint32_t *w_len;
    int32_t *w_err;
    uint8_t *w_skip;
};

/* the device SET path (lzf_store.hip); device pointers */
struct LzfStoreArgs {
    const uint8_t *in;
    const uint64_t *in_off;
    const uint32_t *in_len;
    uint32_t count, max_in_len, compression;
    uint64_t in_bytes;
    uint8_t *store;
    uint64_t store_cap;
    uint64_t *store_used;
    uint64_t *val_off;
    uint32_t *val_size;
    uint8_t *enc;
    uint32_t *status;
    /* work area (lzf_store_layout) */
    uint64_t *w_state, *w_slot_off, *w_tile;
    uint32_t *w_len, *w_cap, *w_out;
    uint8_t *w_slots;
};

/* the store's lifecycle (lzf_store.hip): usage and the semispace compaction;
 * device pointers.  Usage alone: val_off, src, dst, dst_used, status NULL */
struct LzfCompactArgs {
    const uint8_t *src;
    uint64_t src_cap;
    uint64_t *val_off;
    uint32_t *val_size;
    const uint8_t *enc;
    uint32_t count;
    uint8_t *dst;
    uint64_t dst_cap;
    uint64_t *dst_used;
    uint64_t *report;
    uint32_t *status;
    /* work area (lzf_compact_layout): per scan tile the live count (top bit: a
     * live item out of range), the live bytes and the dead bytes; the dense
     * list of the live items, destination and source offset per live rank */
    uint64_t *w_state, *w_tile_n, *w_tile_b, *w_tile_d, *w_live_dst, *w_live_src;
};

/* one set of the store's ten item arrays, device pointers, member for member
 * the public lzf_store_items: the renumbering reads one set and writes another.
 * item_time and item_ttl are given or NULL together; item_lock and last_access
 * may be NULL */
struct LzfItemArrays {
    uint64_t *val_off;
    uint32_t *val_size;
    uint8_t *enc;
    uint32_t *val_len;
    uint64_t *key_off;
    uint32_t *key_len;
    int64_t *item_time;
    int32_t *item_ttl;
    int64_t *item_lock;
    int64_t *last_access;
};

/* the renumbering of the live items into a second set of arrays and a second
 * key arena (lzf_renumber.hip); device pointers.  src is only read */
struct LzfRenumberArgs {
    LzfItemArrays src, dst;
    uint32_t count, dst_cap;
    const uint8_t *src_keys;
    uint64_t src_keys_cap;
    uint8_t *dst_keys;
    uint64_t dst_keys_cap;
    uint64_t *dst_keys_used;
    uint32_t *remap;
    uint64_t *report;
    uint32_t *status;
    /* work area (lzf_renumber_layout): per scan tile the live count (top bit:
     * a live key out of range), the live key bytes and the dead items' key
     * bytes; after the carry the first two hold the sums of the tiles before */
    uint64_t *w_state, *w_tile_n, *w_tile_b, *w_tile_d;
};

/* the key append of a parsed SET batch (lzf_request.hip); device pointers.
 * The rq_* arrays are the parse's outputs, n entries; key_off .. last_access
 * the store's, `count` entries, written at [first, first + n) */
struct LzfAppendArgs {
    const uint8_t *req;
    uint64_t req_bytes;
    const uint8_t *op, *status;
    const uint64_t *rq_key_off;
    const uint32_t *rq_key_len, *rq_val_len;
    const int64_t *num;
    uint32_t n, first;
    uint8_t *keys;
    uint64_t keys_cap;
    uint64_t *keys_used;
    uint64_t *key_off;
    uint32_t *key_len;
    int64_t *item_time;
    int32_t *item_ttl;
    int64_t *item_lock, *last_access;
    int64_t now;
    int32_t max_item_ttl;
    uint32_t *set_len, *void_idx;
    uint64_t *result;
    /* work area (lzf_append_layout): per scan tile the accepted count and the
     * accepted key bytes; after the carry the latter holds the sum of the tiles
     * before */
    uint64_t *w_state, *w_tile_n, *w_tile_b;
};

/* the bucket of a parsed batch by operator class (lzf_dispatch.hip); device
 * pointers.  The first seven arrays are the parse's outputs, n entries; b_*
 * their copies in bucket order */
struct LzfBucketArgs {
    const uint8_t *op, *status;
    const uint64_t *key_off, *val_off;
    const uint32_t *key_len, *val_len;
    const int64_t *num;
    uint32_t n;
    uint32_t *perm, *slot, *class_first;
    uint8_t *b_op, *b_status;
    uint64_t *b_key_off, *b_val_off;
    uint32_t *b_key_len, *b_val_len;
    int64_t *b_num;
    /* work area (lzf_bucket_layout): the classes x tiles table, class-major:
     * per tile its requests of each class, after the scan the position in perm
     * of the tile's first request of the class */
    uint64_t *w_table;
};

/* the prefix select over the store's keys (lzf_mget.hip); device pointers */
struct LzfSelectArgs {
    const uint8_t *keys;
    const uint64_t *key_off;
    const uint32_t *key_len;
    const uint8_t *enc;
    uint32_t count;
    const uint8_t *prefix;
    uint32_t prefix_len;
    uint32_t *sel;
    uint32_t cap;
    uint32_t *result;
    /* work area (lzf_select_layout): one 64-bit match word per 64 items, and
     * per tile its match count, then the matches before it */
    uint64_t *w_mask, *w_tile;
};

/* the ordered prefix select (lzf_order.hip); device pointers.  Candidates are
 * the items whose key starts with the prefix, dead ones included; matches are
 * the live candidates */
struct LzfOrderArgs {
    const uint8_t *keys;
    const uint64_t *key_off;
    const uint32_t *key_len;
    const uint8_t *enc;
    uint32_t count;
    const uint8_t *prefix;
    uint32_t prefix_len;
    int64_t limit;
    uint32_t cand_cap;
    uint64_t node_cap;
    uint32_t *sel;
    uint32_t cap;
    uint64_t *result;
    /* work area (lzf_order_layout).  w_state: the OD_* words of lzf_order.hip.
     * w_mask / w_tile_n / w_tile_b / w_tile_m: per 64 items the candidates'
     * ballot, per item tile [live:32 | candidates:32], the candidates' node
     * words and their longest key.  w_table: the node table, `slots` words.
     * w_cand: the candidate list.  w_ctile_n / w_ctile_b: per tile of the
     * candidate list its matches and their row words.  w_live, w_row_off,
     * w_row_len: per match its item, and its row in w_rows.  w_sort: the two
     * index buffers of the sort */
    uint64_t slots;
    uint64_t *w_state, *w_mask, *w_tile_n, *w_tile_b, *w_tile_m, *w_table, *w_ctile_n, *w_ctile_b, *w_row_off;
    uint32_t *w_cand, *w_live, *w_row_len, *w_rows, *w_sort[2];
};

/* MGET over an index list (lzf_mget.hip); device pointers */
struct LzfMgetArgs {
    const uint32_t *idx;
    uint32_t n;
    const uint8_t *keys;
    const uint64_t *key_off;
    const uint32_t *key_len;
    const uint8_t *store;
    const uint64_t *val_off;
    const uint32_t *val_size;
    const uint32_t *val_len;
    LzfItems it;
    uint32_t max_val_len;
    int reply_header;
    uint8_t *frame;
    uint64_t max_response;
    uint64_t *frame_len;
    uint64_t *result;
    /* work area (lzf_mget_layout).  g_*: the entries' descriptors in list order
     * (a dropped entry: g_enc NULL; g_null: the item an expired entry nulls);
     * w_*: as LzfFrameArgs, and per tile the frame bytes and the three counts */
    uint64_t *w_state, *g_key_off, *g_val_off, *w_off, *w_voff, *w_tile, *w_tcnt;
    uint32_t *g_key_len, *g_val_size, *g_val_len, *g_null, *w_len;
    int32_t *w_err;
    uint8_t *g_enc, *w_skip;
};

/* the per-request replies over an index list (lzf_reply.hip); device pointers.
 * op_status: VALUE mode only */
struct LzfReplyArgs {
    const uint32_t *idx;
    uint32_t n;
    int mode;
    const uint8_t *op_status;
    const uint8_t *store;
    const uint64_t *val_off;
    const uint32_t *val_size;
    const uint32_t *val_len;
    LzfItems it;
    uint32_t max_val_len;
    uint8_t *replies;
    uint64_t rep_cap;
    uint64_t *rep_used;
    uint64_t *rep_off;
    uint32_t *rep_len;
    uint8_t *entry_status;
    uint64_t *result;
    /* work area (lzf_reply_layout).  g_*: the entries' descriptors in list order
     * (g_code: the entry's LZF_REPL_* code; g_cls: its decode class, RP_NO_CLASS
     * when the decoder has nothing to do for it; g_null: the item an expired
     * entry nulls); w_off: the slot's offset inside its tile; per tile the slot
     * bytes, then the bytes before it, and the packed counts; w_voff, w_len,
     * w_err: the decoder's out_off, out_len, err; w_skip: one skip list per
     * decode class */
    uint64_t *w_state, *g_val_off, *w_off, *w_voff, *w_tile, *w_tcnt;
    uint32_t *g_val_size, *g_val_len, *g_null, *w_len;
    int32_t *w_err;
    uint8_t *g_enc, *g_code, *g_cls, *w_skip;
};

/* the key index over the store's keys (lzf_kidx.hip); device pointers.  The
 * lookup reads table, slots, the key arrays, enc, count and result only */
struct LzfKidxArgs {
    void *table;
    uint32_t slots;
    uint32_t *used;
    const uint8_t *keys;
    const uint64_t *key_off;
    const uint32_t *key_len;
    uint8_t *enc;
    uint32_t count, first, n;
    uint64_t *result;
    uint32_t *status;
};

/* the lock operators over an index list (lzf_ops.hip); device pointers.
 * lock_time: MLOCK only; the view's item_ttl / item_lock / last_access and
 * entry_status may be NULL where the call allows it */
struct LzfLockArgs {
    const uint32_t *idx;
    uint32_t n;
    int64_t lock_time;
    LzfItems it;
    uint8_t *entry_status;
    uint64_t *result;
};

/* INC / DEC over an index list (lzf_ops.hip); device pointers */
struct LzfMincArgs {
    const uint32_t *idx;
    uint32_t n;
    int64_t delta;
    int single;
    uint8_t *store;
    uint64_t store_cap;
    uint64_t *store_used;
    uint64_t *val_off;
    uint32_t *val_size;
    LzfItems it;
    uint8_t *entry_status;
    int64_t *entry_value;
    uint64_t *result;
    uint32_t *status;
    /* work area (lzf_minc_layout): the call's base and status; per entry its
     * new number and its LZF_ENT_* class; per tile its converted entries, then
     * the converted entries before it */
    uint64_t *w_state, *w_tile;
    int64_t *w_val;
    uint8_t *w_cls;
};

/* MSET over an index list (lzf_mset.hip); device pointers */
struct LzfMsetArgs {
    const uint32_t *idx;
    uint32_t n;
    const uint8_t *value;
    uint32_t vlen, compression;
    uint8_t *store;
    uint64_t store_cap;
    uint64_t *store_used;
    uint64_t *val_off;
    uint32_t *val_size;
    uint32_t *val_len;
    LzfItems it;
    uint8_t *entry_status;
    uint64_t *result;
    uint32_t *status;
    /* work area (lzf_mset_layout): the call's base, status and stored form; the
     * descriptors of the one-value compress batch (c_off: in_off, out_off;
     * c_len: in_len, out_cap, out_len); per tile its DONE entries, then the
     * DONE entries before it; per entry its LZF_ENT_* class; the compress slot */
    uint64_t *w_state, *c_off, *w_tile;
    uint32_t *c_len;
    uint8_t *w_cls, *w_slot;
};

/* META over an index list (lzf_meta.hip); device pointers */
struct LzfMetaArgs {
    const uint32_t *idx;
    uint32_t n;
    int field;
    const uint32_t *val_size;
    LzfItems it;
    uint8_t *entry_status;
    int64_t *entry_value;
    uint64_t *result;
};

/* the KEYS reply frame over an index list (lzf_meta.hip); device pointers */
struct LzfKeysArgs {
    const uint32_t *idx;
    uint32_t n;
    const uint8_t *keys;
    const uint64_t *key_off;
    const uint32_t *key_len;
    const uint8_t *enc;
    uint32_t count;
    int reply_header;
    uint8_t *frame;
    uint64_t max_response;
    uint64_t *frame_len;
    uint64_t *result;
    /* work area (lzf_keys_layout): found, payload, status; per tile its
     * participating entries and their key bytes, then those before it */
    uint64_t *w_state, *w_tile_n, *w_tile_b;
};

/* compress scratch of the lane generation (lzf_lane.hip), device pointers:
 * per value cstride u16 cand words and bstride u32 inserted-bitmap words */
struct LzfLaneScratch {
    uint16_t *cand;
    uint32_t *bits;
    uint64_t cstride;
    uint64_t bstride;
    uint32_t force_fix;    /* diagnostics: take the atomic-order repair path */
};

/* compress scratch of the table generation (lzf_cand.hip), device pointers:
 * per value rstride u32 records and bstride u32 inserted-bitmap words */
struct LzfRecScratch {
    uint32_t *rec;
    uint32_t *bits;
    uint64_t rstride;
    uint64_t bstride;
};

/* a batch whose inputs arrive in parts (the registered host path): part p is
 * values [end[p-1], end[p]) (end[-1] = 0), in once ev[p] has fired on its
 * stream; kernel 1 of a part may start then, the parse after all of them */
struct LzfParts {
    uint32_t n;
    const uint32_t *end;
    const hipEvent_t *ev;
};

/* launchers, defined next to their kernels; return hipSuccess or the error.
 * The store's lzf_X_work_bytes / lzf_X_carve pairs are defined together in
 * lzf_layout.cpp, each pair from the one layout of lzf_store_layout.h */
hipError_t lzf_launch_compress_table(const LzfBatch &b, hipStream_t s, void *scratch, size_t scratch_bytes,
                                     uint32_t *chunks, const LzfParts *parts = nullptr);
size_t lzf_table_scratch_per_value(uint32_t max_len);
bool lzf_table_compress_supported(uint32_t max_len);
hipError_t lzf_launch_compress_wtab(const LzfBatch &b, hipStream_t s, void *scratch, size_t scratch_bytes,
                                    uint32_t *chunks);
size_t lzf_wtab_scratch_per_value(uint32_t max_len);
bool lzf_wtab_compress_supported(uint32_t max_len);
hipError_t lzf_launch_decompress_lane(const LzfBatch &b, hipStream_t s);
hipError_t lzf_launch_dsize(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t *out_size,
                            int32_t *err, uint32_t count, uint32_t limit, hipStream_t s);
/* aux / ev (4 events) optional: chunks pipelined over s (kernel 1) and aux
 * (kernel 2); s is joined with aux before returning */
hipError_t lzf_launch_compress_lane(const LzfBatch &b, hipStream_t s, void *scratch,
                                    size_t scratch_bytes, uint32_t force_fix, hipStream_t aux,
                                    hipEvent_t *ev, uint32_t *chunks);
size_t lzf_lane_scratch_per_value(uint32_t max_len);
hipError_t lzf_launch_cand_stream(const LzfBatch &b, const LzfLaneScratch &sc, hipStream_t s);
hipError_t lzf_launch_cand_stream_rec(const LzfBatch &b, const LzfRecScratch &sc, hipStream_t s);
const char *lzf_lane_cand_name(void);
bool lzf_lane_compress_supported(uint32_t max_len);
hipError_t lzf_launch_compress(const LzfBatch &b, hipStream_t s);
hipError_t lzf_launch_decompress(const LzfBatch &b, hipStream_t s);
hipError_t lzf_launch_synth(int kind, uint64_t seed, uint64_t first, uint64_t stride,
                            uint32_t count, uint32_t n, uint8_t *out, hipStream_t s);
hipError_t lzf_launch_frame(LzfFrameArgs &a, hipStream_t s,
                            hipError_t (*decode)(const LzfBatch &, hipStream_t));
size_t lzf_frame_work_bytes(uint32_t count);
void lzf_frame_carve(LzfFrameArgs &a, void *work);
const char *lzf_compress_kernel_name(void);
/* the device SET path: plan, `compress` over the candidates' scratch slots,
 * sizes and the store decision, the dense pack (lzf_store.hip) */
hipError_t lzf_launch_store(LzfStoreArgs &a, hipStream_t s,
                            hipError_t (*compress)(const LzfBatch &, hipStream_t));
uint64_t lzf_store_work_bytes(uint32_t count, uint64_t in_bytes);
void lzf_store_carve(LzfStoreArgs &a, void *work);
/* the store's lifecycle (lzf_store.hip): items nulled by index and by TTL,
 * the usage report, and the compaction of the live items into a second arena */
hipError_t lzf_launch_store_delete(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count, hipStream_t s);
hipError_t lzf_launch_store_expire(const LzfItems &it, uint32_t *expired, hipStream_t s);
hipError_t lzf_launch_store_usage(LzfCompactArgs &a, hipStream_t s);
hipError_t lzf_launch_store_compact(LzfCompactArgs &a, hipStream_t s);
uint64_t lzf_compact_work_bytes(uint32_t count);
void lzf_compact_carve(LzfCompactArgs &a, void *work);
/* the renumbering (lzf_renumber.hip): the live items, dense and in order, into
 * a second set of item arrays with their keys packed into a second arena; and
 * an index list from before it translated through its remap */
hipError_t lzf_launch_store_renumber(LzfRenumberArgs &a, hipStream_t s);
hipError_t lzf_launch_store_remap(uint32_t *idx, uint32_t n, const uint32_t *remap, uint32_t count, hipStream_t s);
uint64_t lzf_renumber_work_bytes(uint32_t count);
void lzf_renumber_carve(LzfRenumberArgs &a, void *work);
/* request ingest (lzf_request.hip): the parse of a batch of raw requests (the
 * grammar: lzf_request.h), and the key append of a parsed SET batch */
struct LzfRequestArgs;
hipError_t lzf_launch_request_parse(const LzfRequestArgs &a, hipStream_t s);
hipError_t lzf_launch_store_append_keys(LzfAppendArgs &a, hipStream_t s);
uint64_t lzf_append_work_bytes(uint32_t n);
void lzf_append_carve(LzfAppendArgs &a, void *work);
/* request dispatch (lzf_dispatch.hip): the stable partition of a parsed batch
 * by operator class (the rule: lzf_request_class_of, lzf_request.h) with the
 * seven arrays gathered into bucket order, and the reply table of a bucketed
 * batch in request order */
struct LzfStitchArgs;
hipError_t lzf_launch_request_bucket(const LzfBucketArgs &a, hipStream_t s);
hipError_t lzf_launch_request_stitch(const LzfStitchArgs &a, hipStream_t s);
uint64_t lzf_bucket_work_bytes(uint32_t n);
void lzf_bucket_carve(LzfBucketArgs &a, void *work);
/* the operators over the store (lzf_mget.hip): the prefix select into an
 * index list, and MGET (`decode` over the gathered entries, in place in the
 * frame), COUNT and MTTL over an index list */
hipError_t lzf_launch_store_select(LzfSelectArgs &a, hipStream_t s);
uint64_t lzf_select_work_bytes(uint32_t count);
void lzf_select_carve(LzfSelectArgs &a, void *work);
/* the ordered prefix select (lzf_order.hip): the live matches in the
 * reference's trie order */
hipError_t lzf_launch_store_select_ordered(LzfOrderArgs &a, hipStream_t s);
uint64_t lzf_order_work_bytes(uint32_t count, uint32_t cand_cap, uint64_t node_cap, uint32_t cap);
void lzf_order_carve(LzfOrderArgs &a, void *work);
hipError_t lzf_launch_store_mget(LzfMgetArgs &a, hipStream_t s, hipError_t (*decode)(const LzfBatch &, hipStream_t));
uint64_t lzf_mget_work_bytes(uint32_t n);
void lzf_mget_carve(LzfMgetArgs &a, void *work);
hipError_t lzf_launch_store_count(const uint32_t *idx, uint32_t n, const LzfItems &it, uint64_t *result,
                                  hipStream_t s);
hipError_t lzf_launch_store_mttl(const uint32_t *idx, uint32_t n, int32_t ttl, const LzfItems &it, uint64_t *result,
                                 hipStream_t s);
/* one reply frame per entry of an index list (lzf_reply.hip): classify, scan,
 * write, `decode` once per decode size class (one_route: once, with
 * max_val_len) over the gathered entries, in place in the arena, check; and
 * the reply code of an entry status on the host */
hipError_t lzf_launch_store_replies(LzfReplyArgs &a, hipStream_t s,
                                    hipError_t (*decode)(const LzfBatch &, hipStream_t), bool one_route);
uint64_t lzf_reply_work_bytes(uint32_t n);
void lzf_reply_carve(LzfReplyArgs &a, void *work);
int lzf_reply_code(int ent_status);
/* the lock-aware operators over an index list (lzf_ops.hip): MLOCK, MUNLOCK
 * and MDEL in one pass each, INC / DEC in three launches, the SET guard over
 * a lookup's output, and the number parse on the host */
hipError_t lzf_launch_store_mlock(const LzfLockArgs &a, hipStream_t s);
hipError_t lzf_launch_store_munlock(const LzfLockArgs &a, hipStream_t s);
hipError_t lzf_launch_store_mdel(const LzfLockArgs &a, hipStream_t s);
hipError_t lzf_launch_store_minc(LzfMincArgs &a, hipStream_t s);
uint64_t lzf_minc_work_bytes(uint32_t n);
void lzf_minc_carve(LzfMincArgs &a, void *work);
hipError_t lzf_launch_store_set_guard(const uint32_t *occ, uint32_t first, uint32_t n, const LzfItems &it,
                                      uint8_t *refused, uint64_t *result, hipStream_t s);
int lzf_ops_parse_long(const uint8_t *v, uint32_t len, int64_t *out);
/* MSET over an index list (lzf_mset.hip): classify, `compress` over the one
 * value, the decision, the descriptors, the replicated stored bytes */
hipError_t lzf_launch_store_mset(LzfMsetArgs &a, hipStream_t s,
                                 hipError_t (*compress)(const LzfBatch &, hipStream_t));
uint64_t lzf_mset_work_bytes(uint32_t n, uint32_t vlen);
void lzf_mset_carve(LzfMsetArgs &a, void *work);
/* the memory sweep, META and the KEYS frame (lzf_meta.hip), and META's field
 * name on the host */
hipError_t lzf_launch_store_gc(const LzfItems &it, int64_t gc_ratio, const uint32_t *val_size, const uint64_t *gate,
                               uint64_t max_bytes, uint64_t *result, hipStream_t s);
hipError_t lzf_launch_store_meta(const LzfMetaArgs &a, hipStream_t s);
int lzf_meta_field(const uint8_t *m, uint32_t mlen);
hipError_t lzf_launch_store_keys(LzfKeysArgs &a, hipStream_t s);
uint64_t lzf_keys_work_bytes(uint32_t n);
void lzf_keys_carve(LzfKeysArgs &a, void *work);
/* the key index (lzf_kidx.hip): the table's geometry and a key's home slot on
 * the host, the upsert of the items [first, first + n) and the lookup of nq
 * query keys into idx */
bool lzf_kidx_slots_ok(uint32_t slots);
uint64_t lzf_kidx_table_bytes(uint32_t slots);
uint32_t lzf_kidx_home(const uint8_t *key, uint32_t len, uint32_t slots);
hipError_t lzf_launch_kidx_insert(LzfKidxArgs &a, hipStream_t s);
/* the table and *used cleared, then the insert of [0, count), FULL judged on
 * the items the insert will not skip */
hipError_t lzf_launch_kidx_rebuild(LzfKidxArgs &a, hipStream_t s);
hipError_t lzf_launch_kidx_lookup(LzfKidxArgs &a, const uint8_t *qkeys, const uint64_t *q_off, const uint32_t *q_len,
                                  uint32_t nq, uint32_t *idx, hipStream_t s);
/* value moves between mapped host memory and device arenas (lzf_hostio.hip):
 * len[k] (at least min_len) bytes from src + src_off[k] to dst + dst_off[k] */
hipError_t lzf_launch_move(const uint8_t *src, const uint64_t *src_off, uint8_t *dst, const uint64_t *dst_off,
                           const uint32_t *len, uint32_t min_len, uint32_t count, hipStream_t s);
/* zero bytes [len[k], cap[k]) of every value's slot at dst + dst_off[k] (the
 * bytes past a decoded value that a DMA of abutting slots would carry) */
hipError_t lzf_launch_clear_tail(uint8_t *dst, const uint64_t *dst_off, const uint32_t *len, const uint32_t *cap,
                                 uint32_t count, hipStream_t s);
/* size classes of a mixed-size batch (lzf_mixed.hip): the stable partition of
 * `count` lengths into perm / class_count / class_max (work:
 * lzf_partition_work_bytes, 4-byte aligned), the four descriptor arrays
 * gathered through perm, and the results scattered back (the refused values
 * get out_len 0 and err EINVAL; err / c_err NULL for compress) */
size_t lzf_partition_work_bytes(uint32_t count);
hipError_t lzf_launch_size_partition(const uint32_t *len, uint32_t count, uint32_t bound, int kind, uint32_t *perm,
                                     uint32_t *class_count, uint32_t *class_max, void *work, hipStream_t s);
hipError_t lzf_launch_mixed_gather(const uint32_t *perm, uint32_t count, const uint64_t *in_off,
                                   const uint32_t *in_len, const uint64_t *out_off, const uint32_t *out_cap,
                                   uint64_t *c_in_off, uint32_t *c_in_len, uint64_t *c_out_off, uint32_t *c_out_cap,
                                   hipStream_t s);
hipError_t lzf_launch_mixed_scatter(const uint32_t *perm, uint32_t count, const uint32_t *class_count,
                                    const uint32_t *c_out_len, const int32_t *c_err, uint32_t *out_len, int32_t *err,
                                    hipStream_t s);
/* lzf_api.cpp, for the host-memory paths of lzf_host.cpp: the routed
 * launches, the routing's batch threshold, the device check, the scratch */
hipError_t lzf_route_compress(const LzfBatch &b, hipStream_t s);
hipError_t lzf_route_decompress(const LzfBatch &b, hipStream_t s);
uint32_t lzf_route_min_count(uint32_t max_len);
bool lzf_device_ok(int dev);
void lzf_scratch_release_all(void);
/* compress with the routed generations whatever the batch size, on a private
 * scratch (lzf_scratch_create): the host pipeline's side-by-side chunks */
hipError_t lzf_route_compress_bulk(const LzfBatch &b, hipStream_t s, void *scratch,
                                   const LzfParts *parts = nullptr);
/* window64 (one wave per value), and whether the default routing is in
 * force (no LZF_GPU_KERNEL override, the LDS lane order held) */
hipError_t lzf_route_compress_window(const LzfBatch &b, hipStream_t s);
bool lzf_route_default(void);
/* a private scratch holding 1/share of the cap (the host pipeline's slots) */
void *lzf_scratch_create(unsigned share);
void lzf_scratch_release(void *scratch);
void lzf_scratch_destroy(void *scratch);
const char *lzf_decompress_kernel_name(void);

#endif
