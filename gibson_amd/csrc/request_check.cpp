/*
 * request_check.cpp -- the request grammar (lzf_request.h) on the host, under
 * the host sanitizers (`make request_check`, run by
 * tests/test_request_ingest.py).  A stand-alone host program: its own main, no
 * kernel, not linked to the library, never loaded into Python.
 *
 * Every request lives in a heap block of exactly req_len bytes, so a read of
 * the host form past a request is an AddressSanitizer report.  The crafted
 * table pins the statuses, spans and numbers of the cases include/lzf_gpu.h
 * names; the fuzz compares lzf_request_parse_one with a byte-at-a-time
 * transcription of src/query.c:229-373 that keeps the reference's wrapped
 * size_t subtraction and only then tells SHORT from OK.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lzf_request.h"

static int g_bad = 0;
static unsigned g_cases = 0;

/* a request of exactly 2 + strlen(payload) bytes on the heap (len < 2: that many bytes of the opcode) */
static uint8_t *request(uint32_t op, const uint8_t *payload, uint32_t plen, int cut, uint32_t *len)
{
    *len = cut >= 0 ? (uint32_t)cut : 2u + plen;
    uint8_t *r = (uint8_t *)malloc(*len ? *len : 1u);
    if (!r) exit(2);
    const uint8_t head[2] = {(uint8_t)op, (uint8_t)(op >> 8)};
    for (uint32_t i = 0; i < *len; i++) r[i] = i < 2u ? head[i] : payload[i - 2u];
    if (!*len) {                                             /* a block of 0 bytes: nothing may be read */
        free(r);
        r = (uint8_t *)malloc(0);
    }
    return r;
}

struct Want {
    uint32_t op;            /* the opcode sent */
    const char *payload;
    uint32_t max_key, max_value, expect_op;
    uint32_t status;
    const char *key, *val;  /* the spans' bytes; NULL: no span */
    int64_t num;
};

static void crafted(const Want &w)
{
    uint32_t len;
    uint8_t *r = request(w.op, (const uint8_t *)w.payload, (uint32_t)strlen(w.payload), -1, &len);
    const LzfRequest o = lzf_request_parse_one(r, len, w.max_key, w.max_value, w.expect_op);
    const uint32_t klen = w.key ? (uint32_t)strlen(w.key) : 0u, vlen = w.val ? (uint32_t)strlen(w.val) : 0u;
    int ok = o.status == w.status && o.key_len == klen && o.val_len == vlen && o.num == w.num;
    ok = ok && (!klen || (o.key_at + klen <= len && !memcmp(r + o.key_at, w.key, klen)));
    ok = ok && (!vlen || (o.val_at + vlen <= len && !memcmp(r + o.val_at, w.val, vlen)));
    if (!ok) {
        fprintf(stderr, "request_check: op %u \"%s\" max_key %u max_value %u: status %u key %u+%u val %u+%u num %lld\n",
                w.op, w.payload, w.max_key, w.max_value, o.status, o.key_at, o.key_len, o.val_at, o.val_len,
                (long long)o.num);
        g_bad = 1;
    }
    free(r);
    g_cases++;
}

/* src/query.c:229-373 and the handlers' use of it, a byte at a time */
static LzfRequest model(const uint8_t *r, uint32_t len, uint64_t max_key, uint64_t max_value, uint32_t expect_op)
{
    LzfRequest o = {0u, (uint32_t)LZF_REQ_BADOP, 0u, 0u, 0u, 0u, 0};
    if (len < 2u) return o;
    const uint32_t op = r[0] | ((uint32_t)r[1] << 8);
    const int g = lzf_request_grammar(op);
    if (g == LZF_RQ_BAD) return o;
    o.op = op;
    o.status = LZF_REQ_OTHER;
    if (expect_op && op != expect_op) return o;
    o.status = LZF_REQ_OK;
    if (g == LZF_RQ_EMPTY) return o;
    const uint8_t *buffer = r + 2, *p = buffer;
    const uint64_t size = len - 2u, end = size < max_key ? size : max_key;
    uint64_t i = 0, ttllen = 0, klen, vlen = 0;
    const uint8_t *ttl = p, *key, *value = NULL;
    if (g == LZF_RQ_SET) {
        while (i++ < end && *p != ' ') ++p;
        ttllen = (uint64_t)(p++ - ttl);
    }
    key = p;
    while (i++ < end && *p != ' ') ++p;
    klen = (uint64_t)(p++ - key);
    int ret = 1;
    if (g == LZF_RQ_SET) {
        value = p;
        vlen = size - ttllen - klen - 2u;                    /* wraps */
        vlen = vlen < max_value ? vlen : max_value;
        ret = size && ttllen && klen && vlen;
    } else if (g == LZF_RQ_KEYOPT) {
        const uint64_t left = size - klen;
        if (left > 0) {
            value = p;
            vlen = left - 1u;
            vlen = vlen < max_value ? vlen : max_value;
        }
        ret = klen && !(value && !vlen);
    } else if (g != LZF_RQ_KEY) {
        value = p;
        vlen = size - klen - 1u;                             /* wraps */
        vlen = vlen < max_value ? vlen : max_value;
        ret = klen && vlen;
    } else {
        ret = klen != 0;
    }
    o.status = LZF_REQ_ERR;
    if (!ret) return o;
    o.status = LZF_REQ_SHORT;                                /* the departure: the value must lie inside the request */
    if (value && vlen && (uint64_t)(value - r) + vlen > len) return o;
    o.key_at = (uint32_t)(key - r);
    o.key_len = (uint32_t)klen;
    if (value && vlen) {
        o.val_at = (uint32_t)(value - r);
        o.val_len = (uint32_t)vlen;
    }
    int ok = 1;
    if (g == LZF_RQ_SET) ok = lzf_parse_long(ttl, (uint32_t)ttllen, &o.num);
    else if (g == LZF_RQ_KEYNUM) ok = lzf_parse_long(value, (uint32_t)vlen, &o.num);
    else if (g == LZF_RQ_KEYOPT) {
        o.num = -1;
        if (value && vlen) ok = lzf_parse_long(value, (uint32_t)vlen, &o.num);
    }
    o.status = ok ? LZF_REQ_OK : LZF_REQ_NAN;
    if (!ok) o.num = 0;
    return o;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 32) % n);
}

int main()
{
    const uint32_t SET = LZF_OP_SET, TTL = LZF_OP_TTL, GET = LZF_OP_GET, MGET = LZF_OP_MGET, MSET = LZF_OP_MSET;
    const Want table[] = {
        {SET, "10 key v", 512, 4096, 0, LZF_REQ_OK, "key", "v", 10},
        {SET, "10 key", 512, 4096, 0, LZF_REQ_SHORT, NULL, NULL, 0},
        {SET, "10 key ", 512, 4096, 0, LZF_REQ_ERR, NULL, NULL, 0},
        {SET, "10", 512, 4096, 0, LZF_REQ_ERR, NULL, NULL, 0},
        {SET, "10 ", 512, 4096, 0, LZF_REQ_ERR, NULL, NULL, 0},
        {SET, " key v", 512, 4096, 0, LZF_REQ_ERR, NULL, NULL, 0},
        {SET, "", 512, 4096, 0, LZF_REQ_ERR, NULL, NULL, 0},
        {SET, "0x k v", 512, 4096, 0, LZF_REQ_OK, "k", "v", 0},
        {SET, "- k v", 512, 4096, 0, LZF_REQ_OK, "k", "v", 0},
        {SET, "-7 k v", 512, 4096, 0, LZF_REQ_OK, "k", "v", -7},
        {SET, "1x k v", 512, 4096, 0, LZF_REQ_NAN, "k", "v", 0},
        {SET, "10 abcdefgh value", 8, 4096, 0, LZF_REQ_OK, "abcde", "gh value", 10},   /* the budget ends inside the key */
        {SET, "10 abcdefghijklmnopqrstuvwxyz 0123456789", 512, 4, 0, LZF_REQ_OK, "abcdefghijklmnopqrstuvwxyz", "0123", 10},
        {TTL, "abc", 512, 4096, 0, LZF_REQ_SHORT, NULL, NULL, 0},
        {TTL, "abc ", 512, 4096, 0, LZF_REQ_ERR, NULL, NULL, 0},
        {TTL, "abc x", 512, 4096, 0, LZF_REQ_NAN, "abc", "x", 0},
        {TTL, "abc 12", 512, 4096, 0, LZF_REQ_OK, "abc", "12", 12},
        {TTL, "abcd", 4, 4096, 0, LZF_REQ_SHORT, NULL, NULL, 0},
        {TTL, "abcde", 4, 4096, 0, LZF_REQ_ERR, NULL, NULL, 0},
        {TTL, "abcdef", 4, 4096, 0, LZF_REQ_NAN, "abcd", "f", 0},
        {MGET, "abc", 512, 4096, 0, LZF_REQ_OK, "abc", NULL, -1},
        {MGET, "abc ", 512, 4096, 0, LZF_REQ_ERR, NULL, NULL, 0},
        {MGET, "abc 5", 512, 4096, 0, LZF_REQ_OK, "abc", "5", 5},
        {MGET, "abc z", 512, 4096, 0, LZF_REQ_NAN, "abc", "z", 0},
        {GET, "abc def", 512, 4096, 0, LZF_REQ_OK, "abc", NULL, 0},
        {GET, "", 512, 4096, 0, LZF_REQ_ERR, NULL, NULL, 0},
        {GET, "0123456789abcdefXYZ rest", 512, 4096, 0, LZF_REQ_OK, "0123456789abcdefXYZ", NULL, 0},
        {MSET, "pre value bytes", 512, 4096, 0, LZF_REQ_OK, "pre", "value bytes", 0},
        {0, "abc", 512, 4096, 0, LZF_REQ_BADOP, NULL, NULL, 0},
        {22, "abc", 512, 4096, 0, LZF_REQ_BADOP, NULL, NULL, 0},
        {0x0101, "abc", 512, 4096, 0, LZF_REQ_BADOP, NULL, NULL, 0},
        {0x00FF, "abc", 512, 4096, 0, LZF_REQ_OK, NULL, NULL, 0},
        {LZF_OP_PING, "", 512, 4096, 0, LZF_REQ_OK, NULL, NULL, 0},
        {GET, "abc", 512, 4096, SET, LZF_REQ_OTHER, NULL, NULL, 0},
        {SET, "10 key v", 512, 4096, GET, LZF_REQ_OTHER, NULL, NULL, 0},
        {22, "abc", 512, 4096, GET, LZF_REQ_BADOP, NULL, NULL, 0},
    };
    for (const Want &w : table) crafted(w);
    for (int cut = 0; cut < 2; cut++) {                       /* 0 and 1 bytes: BADOP, and nothing to read */
        uint32_t len;
        uint8_t *r = request(GET, NULL, 0, cut, &len);
        const LzfRequest o = lzf_request_parse_one(r, len, 512, 4096, 0);
        if (o.status != LZF_REQ_BADOP || o.op || o.key_len || o.val_len || o.num) {
            fprintf(stderr, "request_check: a request of %d bytes: status %u\n", cut, o.status);
            g_bad = 1;
        }
        free(r);
        g_cases++;
    }

    static const uint32_t ops[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 200, 255};
    static const char alphabet[] = "  09-ab";
    static const uint32_t max_keys[] = {1, 4, 8, 9, 16, 512}, max_values[] = {1, 3, 4096};
    unsigned seen[LZF_REQ_NSTATUS] = {0};
    for (unsigned it = 0; it < 200000u; it++) {
        uint8_t payload[40];
        const uint32_t plen = rnd(it % 4u ? 25u : 41u);
        for (uint32_t i = 0; i < plen; i++) payload[i] = (uint8_t)alphabet[rnd(7)];
        const uint32_t op = ops[rnd(sizeof ops / sizeof *ops)];
        const uint32_t mk = max_keys[rnd(6)], mv = max_values[rnd(3)], expect = rnd(8) ? 0u : ops[1 + rnd(21)];
        uint32_t len;
        uint8_t *r = request(op, payload, plen, rnd(50) ? -1 : (int)rnd(2), &len);
        const LzfRequest a = lzf_request_parse_one(r, len, mk, mv, expect), b = model(r, len, mk, mv, expect);
        if (a.op != b.op || a.status != b.status || a.key_at != b.key_at || a.key_len != b.key_len ||
            a.val_at != b.val_at || a.val_len != b.val_len || a.num != b.num) {
            fprintf(stderr, "request_check: fuzz %u: op %u len %u max_key %u max_value %u: status %u, the model %u\n", it,
                    op, len, mk, mv, a.status, b.status);
            g_bad = 1;
        }
        if (a.status != LZF_REQ_OK && a.status != LZF_REQ_NAN && (a.key_at || a.key_len || a.val_at || a.val_len || a.num))
            g_bad = 1;
        seen[a.status]++;
        free(r);
        g_cases++;
    }
    for (unsigned s = 0; s < LZF_REQ_NSTATUS; s++)
        if (s != LZF_REQ_ERANGE && !seen[s]) {
            fprintf(stderr, "request_check: the fuzz never produced status %u\n", s);
            g_bad = 1;
        }
    if (lzf_request_reply_code_of(LZF_REQ_OK) != -1 || lzf_request_reply_code_of(LZF_REQ_BADOP) != -2 ||
        lzf_request_reply_code_of(LZF_REQ_NAN) != LZF_REPL_ERR_NAN || lzf_request_reply_code_of(LZF_REQ_SHORT) != LZF_REPL_ERR)
        g_bad = 1;
    if (g_bad) return 1;
    printf("request_check: ok, %u requests\n", g_cases);
    return 0;
}
