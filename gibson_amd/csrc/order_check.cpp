/*
 * order_check.cpp -- the host form of the ordered prefix select (lzf_order.h)
 * under the host sanitizers (`make order_check`, run by
 * tests/test_select_ordered.py).  A stand-alone host program: its own main, no
 * kernel, not linked to the library, never loaded into Python.
 *
 * Every array lives in a heap block of exactly its size -- the key bytes end
 * with the last key -- so a read or write of the host form past an array is an
 * AddressSanitizer report.  The host form walks a trie; it is compared with
 * the rule of include/lzf_gpu.h stated the other way: births by a scan over
 * all the items, rows of births, a std::sort over the rows.  Seeded stores of
 * 1-400 items over small alphabets (so that siblings, dead births, keys that
 * are prefixes of others and duplicates of live keys all occur), every limit
 * class, caps below, at and above the result, and both refusals.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "lzf_order.h"

static int g_bad = 0;
static unsigned g_cases = 0;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 32) % n);
}

/* count elements in a heap block of exactly that size */
template <typename T>
struct Block {
    T *p;
    uint64_t count;
    explicit Block(uint64_t n) : p((T *)malloc(n ? n * sizeof(T) : 1u)), count(n)
    {
        if (!p) exit(2);
        memset((void *)p, 0xA5, n * sizeof(T));
    }
    ~Block() { free(p); }
    Block(const Block &) = delete;
    T &operator[](uint64_t i) { return p[i]; }
};

typedef std::vector<uint8_t> Key;

/* the rule: birth(P) is the first item whose key starts with P */
static std::vector<uint32_t> naive(const std::vector<Key> &key, const std::vector<uint8_t> &enc, const Key &prefix,
                                   uint64_t *cands, uint64_t *words)
{
    const size_t plen = prefix.size();
    auto starts = [](const Key &k, const uint8_t *p, size_t n) { return k.size() >= n && !memcmp(k.data(), p, n); };
    std::vector<std::pair<std::vector<uint32_t>, uint32_t>> rows;
    *cands = *words = 0ull;
    for (uint32_t i = 0; i < key.size(); i++) {
        if (!starts(key[i], prefix.data(), plen)) continue;
        *cands += 1u;
        *words += key[i].size() - plen;
        if (enc[i] == (uint8_t)LZF_ENC_NULL) continue;
        std::vector<uint32_t> row;
        for (size_t d = plen + 1u; d <= key[i].size(); d++) {
            uint32_t b = 0u;
            while (!starts(key[b], key[i].data(), d)) b++;
            row.push_back(b);
        }
        rows.push_back({row, i});
    }
    std::sort(rows.begin(), rows.end());      /* a vector that is a prefix of another compares less */
    std::vector<uint32_t> out;
    for (const auto &r : rows) out.push_back(r.second);
    return out;
}

static void one_store(uint32_t count, uint32_t letters, uint32_t max_len)
{
    std::vector<Key> key(count);
    std::vector<uint8_t> enc(count);
    uint64_t bytes = 0ull;
    for (uint32_t i = 0; i < count; i++) {
        if (i && !rnd(6u)) key[i] = key[rnd(i)];                     /* an overwrite, or a duplicate */
        else
            for (uint32_t n = 1u + rnd(max_len); n; n--) key[i].push_back((uint8_t)('a' + rnd(letters)));
        enc[i] = rnd(4u) ? (uint8_t)LZF_ENC_PLAIN : (uint8_t)LZF_ENC_NULL;
        bytes += key[i].size();
    }
    Block<uint8_t> keys(bytes), e(count);
    Block<uint64_t> off(count);
    Block<uint32_t> len(count);
    uint64_t at = 0ull;
    for (uint32_t i = 0; i < count; i++) {
        off[i] = at;
        len[i] = (uint32_t)key[i].size();
        e[i] = enc[i];
        memcpy(keys.p + at, key[i].data(), key[i].size());
        at += key[i].size();
    }
    for (uint32_t trial = 0; trial < 6u; trial++) {
        Key prefix = key[rnd(count)];
        prefix.resize(1u + rnd((uint32_t)prefix.size()));
        if (trial == 5u) prefix.push_back((uint8_t)'~');              /* no candidate */
        Block<uint8_t> pre(prefix.size());
        memcpy(pre.p, prefix.data(), prefix.size());
        uint64_t cands, words;
        const std::vector<uint32_t> want = naive(key, enc, prefix, &cands, &words);
        const int64_t limits[] = {-1, 0, 1, (int64_t)want.size() / 2, (int64_t)want.size(), (int64_t)want.size() + 1};
        for (const int64_t limit : limits) {
            const uint64_t kept = limit > 0 && (uint64_t)limit < want.size() ? (uint64_t)limit : want.size();
            const uint32_t caps[] = {(uint32_t)(kept > 1u ? kept - 1u : 1u), (uint32_t)(kept ? kept : 1u),
                                     (uint32_t)kept + 3u};
            for (const uint32_t cap : caps)
                for (int refuse = 0; refuse < 3; refuse++) {
                    /* the caps exact, or one of them one short */
                    if ((refuse == 1 && !cands) || (refuse == 2 && !words)) continue;
                    const uint64_t cand_cap = refuse == 1 ? cands - 1u : cands, node_cap = refuse == 2 ? words - 1u : words;
                    if ((refuse == 1 && !cand_cap) || (refuse == 2 && !node_cap)) continue;
                    Block<uint32_t> sel(cap);
                    Block<uint64_t> result(5);
                    const int rc = lzf_order_host(keys.p, off.p, len.p, e.p, count, pre.p, (uint32_t)prefix.size(), limit,
                                                  (uint32_t)(cand_cap ? cand_cap : 1u), node_cap ? node_cap : 1u, sel.p,
                                                  cap, result.p);
                    const uint64_t n = refuse ? 0ull : (kept < cap ? kept : cap);
                    bool same = rc == LZF_GPU_OK && result[0] == n && result[1] == want.size() && result[2] == cands &&
                                result[3] == words && result[4] == (uint64_t)(refuse ? LZF_ORDER_EWORK : LZF_ORDER_OK);
                    for (uint32_t r = 0; same && r < cap; r++) same = sel[r] == (r < n ? want[r] : 0xFFFFFFFFu);
                    if (!same) {
                        fprintf(stderr, "order_check: count %u, prefix of %zu bytes, limit %lld, cap %u, refuse %d\n",
                                count, prefix.size(), (long long)limit, cap, refuse);
                        g_bad = 1;
                    }
                    g_cases++;
                }
        }
    }
}

int main()
{
    static const uint32_t counts[] = {1u, 2u, 3u, 7u, 64u, 200u, 400u};
    for (const uint32_t count : counts)
        for (uint32_t letters = 1u; letters <= 3u; letters++)
            for (uint32_t round = 0; round < 4u; round++) one_store(count, letters, round < 2u ? 4u : 9u);
    if (g_bad) return 1;
    printf("order_check: ok, %u calls\n", g_cases);
    return 0;
}
