/*
 * lzf_order.h -- the host form of the ordered prefix select
 * (lzf_host_store_select_ordered, include/lzf_gpu.h), free of kernels: the
 * reference's trie itself, built over the candidates in index order, and its
 * pre-order walk.  lzf_order.hip reaches the same list by another route
 * (births in a hash table, rows, a sort), so the two check each other;
 * csrc/order_check.cpp runs this one under the host sanitizers against a
 * std::sort over rows.
 *
 * The trie.  Below the prefix's node, a node per distinct key prefix of a
 * candidate, dead candidates included: tr_remove leaves the nodes in place
 * (src/trie.c:382-414).  A node's children are a list in arrival order, as
 * tr_insert appends them (src/trie.c:74-95); a child is found by a scan of
 * that list (tr_find_next_node, src/trie.c:39-56).  The live items whose key
 * ends at a node hang off it in index order: the reference holds one, a store
 * with two live items of one key yields both.  The walk is tr_recurse
 * (src/trie.c:154-176) with an explicit stack: the node, then its children,
 * oldest first; it ends when `limit` items are out (src/trie.c:162).
 */
#ifndef GIBSON_AMD_LZF_ORDER_H
#define GIBSON_AMD_LZF_ORDER_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/lzf_gpu.h"

static inline int lzf_order_host(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                                 const uint8_t *enc, uint32_t count, const uint8_t *prefix, uint32_t plen,
                                 int64_t limit, uint32_t cand_cap, uint64_t node_cap, uint32_t *sel, uint32_t cap,
                                 uint64_t *result)
{
    const uint32_t NIL = 0xFFFFFFFFu;
    uint64_t cands = 0ull, words = 0ull, live = 0ull;
    for (uint32_t i = 0; i < count; i++) {
        if (key_len[i] < plen || memcmp(keys + key_off[i], prefix, plen)) continue;
        cands++;
        words += key_len[i] - plen;
        live += enc[i] != (uint8_t)LZF_ENC_NULL;
    }
    for (uint32_t r = 0; r < cap; r++) sel[r] = NIL;
    result[0] = 0ull;
    result[1] = live;
    result[2] = cands;
    result[3] = words;
    result[4] = LZF_ORDER_OK;
    if (cands > cand_cap || words > node_cap) {
        result[4] = LZF_ORDER_EWORK;
        return LZF_GPU_OK;
    }
    if (words >= NIL) return LZF_GPU_EARG;                /* the nodes are numbered in 32 bits here */
    /* node 0 is the prefix's */
    struct Node {
        uint32_t first, last, next;       /* children, oldest first; the next sibling */
        uint32_t item, item_last;         /* the live items that end here, by index */
        uint8_t value;
    };
    std::vector<Node> node(1, Node{NIL, NIL, NIL, NIL, NIL, 0});
    std::vector<uint32_t> item_next(count, NIL);
    node.reserve((size_t)(words < (1ull << 26) ? words + 1u : (1ull << 26)));
    for (uint32_t i = 0; i < count; i++) {
        if (key_len[i] < plen || memcmp(keys + key_off[i], prefix, plen)) continue;
        const uint8_t *key = keys + key_off[i];
        uint32_t at = 0u;
        for (uint32_t d = plen; d < key_len[i]; d++) {
            uint32_t c = node[at].first;
            while (c != NIL && node[c].value != key[d]) c = node[c].next;
            if (c == NIL) {
                c = (uint32_t)node.size();
                node.push_back(Node{NIL, NIL, NIL, NIL, NIL, key[d]});
                if (node[at].last == NIL) node[at].first = c;
                else node[node[at].last].next = c;
                node[at].last = c;
            }
            at = c;
        }
        if (enc[i] == (uint8_t)LZF_ENC_NULL) continue;
        if (node[at].item_last == NIL) node[at].item = i;
        else item_next[node[at].item_last] = i;
        node[at].item_last = i;
    }
    const uint64_t want = limit > 0 && (uint64_t)limit < live ? (uint64_t)limit : live;
    const uint64_t n = want < cap ? want : cap;
    uint64_t out = 0ull;
    std::vector<uint32_t> stack(1, 0u);
    while (!stack.empty() && out < n) {
        const uint32_t at = stack.back();
        stack.pop_back();
        for (uint32_t i = node[at].item; i != NIL && out < n; i = item_next[i]) sel[out++] = i;
        /* the children pushed youngest first, so that the oldest is walked next */
        const size_t base = stack.size();
        for (uint32_t c = node[at].first; c != NIL; c = node[c].next) stack.push_back(c);
        for (size_t lo = base, hi = stack.size(); lo + 1u < hi; lo++, hi--) {
            const uint32_t t = stack[lo];
            stack[lo] = stack[hi - 1u];
            stack[hi - 1u] = t;
        }
    }
    result[0] = out;
    return LZF_GPU_OK;
}

#endif
