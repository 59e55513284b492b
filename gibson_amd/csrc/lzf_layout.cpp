/*
 * lzf_layout.cpp -- the sizes and the carves of the device store's thirteen work
 * areas, each from its one layout (lzf_store_layout.h): the size is the layout
 * measured plus the slack for aligning the caller's pointer (64 bytes for the
 * frame, 16 for the others, as ever), the carve is the layout over that
 * pointer.  Host code only, no kernel: csrc/carve_check.cpp compiles this file
 * with the host sanitizers.
 */
#include "lzf_store_layout.h"

namespace {

template <typename A>
uint64_t measured(A a, void (*layout)(A &, LzfCarver &), uint64_t slack)
{
    LzfCarver c;
    layout(a, c);
    c.pad(slack);
    return c.bytes();
}

template <typename A>
void carved(A &a, void (*layout)(A &, LzfCarver &), void *work)
{
    LzfCarver c(work);
    layout(a, c);
}

}  // namespace

size_t lzf_frame_work_bytes(uint32_t count)
{
    LzfFrameArgs a{};
    a.count = count;
    return (size_t)measured(a, lzf_frame_layout, 64u);
}

void lzf_frame_carve(LzfFrameArgs &a, void *work) { carved(a, lzf_frame_layout, work); }

uint64_t lzf_store_work_bytes(uint32_t count, uint64_t in_bytes)
{
    LzfStoreArgs a{};
    a.count = count;
    a.in_bytes = in_bytes;
    return measured(a, lzf_store_layout, 16u);
}

void lzf_store_carve(LzfStoreArgs &a, void *work) { carved(a, lzf_store_layout, work); }

uint64_t lzf_compact_work_bytes(uint32_t count)
{
    LzfCompactArgs a{};
    a.count = count;
    return measured(a, lzf_compact_layout, 16u);
}

void lzf_compact_carve(LzfCompactArgs &a, void *work) { carved(a, lzf_compact_layout, work); }

uint64_t lzf_renumber_work_bytes(uint32_t count)
{
    LzfRenumberArgs a{};
    a.count = count;
    return measured(a, lzf_renumber_layout, 16u);
}

void lzf_renumber_carve(LzfRenumberArgs &a, void *work) { carved(a, lzf_renumber_layout, work); }

uint64_t lzf_append_work_bytes(uint32_t n)
{
    LzfAppendArgs a{};
    a.n = n;
    return measured(a, lzf_append_layout, 16u);
}

void lzf_append_carve(LzfAppendArgs &a, void *work) { carved(a, lzf_append_layout, work); }

uint64_t lzf_bucket_work_bytes(uint32_t n)
{
    LzfBucketArgs a{};
    a.n = n;
    return measured(a, lzf_bucket_layout, 16u);
}

void lzf_bucket_carve(LzfBucketArgs &a, void *work) { carved(a, lzf_bucket_layout, work); }

uint64_t lzf_select_work_bytes(uint32_t count)
{
    LzfSelectArgs a{};
    a.count = count;
    return measured(a, lzf_select_layout, 16u);
}

void lzf_select_carve(LzfSelectArgs &a, void *work) { carved(a, lzf_select_layout, work); }

/* cap sizes nothing: sel is the caller's, and the sort works on cand_cap */
uint64_t lzf_order_work_bytes(uint32_t count, uint32_t cand_cap, uint64_t node_cap, uint32_t cap)
{
    (void)cap;
    LzfOrderArgs a{};
    a.count = count;
    a.cand_cap = cand_cap;
    a.node_cap = node_cap;
    return measured(a, lzf_order_layout, 16u);
}

void lzf_order_carve(LzfOrderArgs &a, void *work) { carved(a, lzf_order_layout, work); }

uint64_t lzf_mget_work_bytes(uint32_t n)
{
    LzfMgetArgs a{};
    a.n = n;
    return measured(a, lzf_mget_layout, 16u);
}

void lzf_mget_carve(LzfMgetArgs &a, void *work) { carved(a, lzf_mget_layout, work); }

uint64_t lzf_reply_work_bytes(uint32_t n)
{
    LzfReplyArgs a{};
    a.n = n;
    return measured(a, lzf_reply_layout, 16u);
}

void lzf_reply_carve(LzfReplyArgs &a, void *work) { carved(a, lzf_reply_layout, work); }

uint64_t lzf_minc_work_bytes(uint32_t n)
{
    LzfMincArgs a{};
    a.n = n;
    return measured(a, lzf_minc_layout, 16u);
}

void lzf_minc_carve(LzfMincArgs &a, void *work) { carved(a, lzf_minc_layout, work); }

uint64_t lzf_mset_work_bytes(uint32_t n, uint32_t vlen)
{
    LzfMsetArgs a{};
    a.n = n;
    a.vlen = vlen;
    return measured(a, lzf_mset_layout, 16u);
}

void lzf_mset_carve(LzfMsetArgs &a, void *work) { carved(a, lzf_mset_layout, work); }

uint64_t lzf_keys_work_bytes(uint32_t n)
{
    LzfKeysArgs a{};
    a.n = n;
    return measured(a, lzf_keys_layout, 16u);
}

void lzf_keys_carve(LzfKeysArgs &a, void *work) { carved(a, lzf_keys_layout, work); }
