/*
 * lzf_request.h -- the request grammar of the reference server in one place:
 * what gbProcessQuery (src/query.c:1393-1485) and the three parse functions
 * around it (gbParseKeyAndOptionalValue, gbParseKeyValue, gbParseTtlKeyValue,
 * src/query.c:229-373) make of one request buffer, and gbQueryParseLong
 * (src/query.c:39-76) for the number in it.  One copy, host and device: the
 * parse kernel (lzf_request.hip), lzf_host_request_parse (lzf_api.cpp) and
 * csrc/request_check.cpp all run lzf_request_entry.  The file needs no HIP
 * header: a plain host compiler reads it too.
 *
 * A request is client->buffer, buffer_size bytes: [i16 opcode LE][payload],
 * size = buffer_size - 2.  The scan rules, quirk for quirk:
 *   - the key scan stops at the first ' ' or after end = min(size, max_key)
 *     bytes; SET's ttl token and key share ONE budget of end, because
 *     gbParseTtlKeyValue does not reset its counter between them (:334-347);
 *   - one byte is skipped after each token, space or not;
 *   - vlen = size - ttllen - klen - 2 (SET), size - klen - 1 (key and value),
 *     left - 1 (MGET's optional value), each then clamped to max_value;
 *   - the checks run in the reference's order: ttl token, key, value.
 *
 * LZF_REQ_SHORT is the one deliberate departure from the reference.  Where
 * the payload ends with the key ("10 key" for SET, "abc" for TTL, a key that
 * fills max_key exactly with nothing behind it) the reference's unsigned
 * subtraction wraps, min() turns it into maxvaluesize, the parse function
 * returns 1 and the handler reads past its buffer.  Here such a request is
 * refused -- no byte outside it is ever read -- and the reply is REPL_ERR.
 *
 * No byte outside [r, r + len) is read, whatever the load width: words are
 * loaded whole only where 8 bytes of the payload are left, the tail comes from
 * a load moved back inside the payload or, for a payload below 8 bytes, from
 * byte loads.
 */
#ifndef GIBSON_AMD_LZF_REQUEST_H
#define GIBSON_AMD_LZF_REQUEST_H

#include <stdint.h>

#include "../../include/lzf_gpu.h"

#if defined(__HIPCC__)
#define LZF_HD __host__ __device__
#else
#define LZF_HD
#endif

/* gbQueryParseLong (src/query.c:39-76), quirk for quirk: a first byte '0'
 * yields 0 whatever follows; a leading '-' negates and a lone "-" is 0; every
 * other byte must be a digit; no length limit, the accumulation n * 10 + d and
 * the negation modulo 2^64 (what the reference's x86-64 build computes where C
 * leaves the signed overflow undefined).  len == 0: not a number (the
 * reference asserts vlen > 0) */
LZF_HD inline int lzf_parse_long(const uint8_t *v, uint32_t len, int64_t *out)
{
    if (!len) return 0;
    if (v[0] == (uint8_t)'0') {
        *out = 0;
        return 1;
    }
    const uint32_t neg = v[0] == (uint8_t)'-' ? 1u : 0u;
    uint64_t n = 0ull;
    for (uint32_t i = neg; i < len; i++) {
        const uint32_t d = (uint32_t)v[i] - (uint32_t)'0';
        if (d > 9u) return 0;
        n = n * 10ull + d;
    }
    *out = (int64_t)(neg ? 0ull - n : n);
    return 1;
}

/* the grammar rows of the operator table */
enum {
    LZF_RQ_BAD = 0,     /* no branch in gbProcessQuery */
    LZF_RQ_KEY,         /* gbParseKeyValue, value == NULL */
    LZF_RQ_KEYVAL,      /* key and required value */
    LZF_RQ_KEYNUM,      /* key and required number */
    LZF_RQ_KEYOPT,      /* gbParseKeyAndOptionalValue: MGET's limit */
    LZF_RQ_SET,         /* gbParseTtlKeyValue */
    LZF_RQ_EMPTY        /* no payload read */
};

LZF_HD inline int lzf_request_grammar(uint32_t op)
{
    switch (op) {
    case LZF_OP_SET: return LZF_RQ_SET;
    case LZF_OP_TTL:
    case LZF_OP_LOCK:
    case LZF_OP_MTTL:
    case LZF_OP_MLOCK: return LZF_RQ_KEYNUM;
    case LZF_OP_MSET:
    case LZF_OP_META: return LZF_RQ_KEYVAL;
    case LZF_OP_MGET: return LZF_RQ_KEYOPT;
    case LZF_OP_GET:
    case LZF_OP_DEL:
    case LZF_OP_INC:
    case LZF_OP_DEC:
    case LZF_OP_UNLOCK:
    case LZF_OP_MDEL:
    case LZF_OP_MINC:
    case LZF_OP_MDEC:
    case LZF_OP_MUNLOCK:
    case LZF_OP_COUNT:
    case LZF_OP_KEYS: return LZF_RQ_KEY;
    case LZF_OP_STATS:
    case LZF_OP_PING:
    case LZF_OP_END: return LZF_RQ_EMPTY;
    default: return LZF_RQ_BAD;
    }
}

/* `while( i++ < end && *p != ' ' ) ++p` from index `from`: the index of the
 * first ' ' in p[from, end), or end; `from` itself when from >= end (the shared
 * budget is spent).  Eight bytes a step; reads p[from, end) only */
LZF_HD inline uint32_t lzf_request_span(const uint8_t *p, uint32_t from, uint32_t end)
{
    uint32_t i = from;
    while (i < end) {
        const uint32_t left = end - i;
        uint64_t w = 0ull;
        if (left >= 8u) {
            __builtin_memcpy(&w, p + i, 8);
        } else if (end >= 8u) {                               /* the last 8 bytes of the scan, moved into place */
            __builtin_memcpy(&w, p + (end - 8u), 8);
            w >>= 8u * (8u - left);
        } else {
            for (uint32_t k = 0; k < left; k++) w |= (uint64_t)p[i + k] << (8u * k);
        }
        /* a zero byte of x is a space; bytes past `left` are 0x00 in w, 0x20 in
         * x, and a false positive of the borrow lies above a true one */
        const uint64_t x = w ^ 0x2020202020202020ull;
        const uint64_t z = (x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull;
        if (z) return i + ((uint32_t)__builtin_ctzll(z) >> 3);
        i += left < 8u ? left : 8u;
    }
    return i;
}

/* one request's parse; offsets count from the request's first byte */
struct LzfRequest {
    uint32_t op, status;
    uint32_t key_at, key_len, val_at, val_len;
    int64_t num;
};

LZF_HD inline LzfRequest lzf_request_parse_one(const uint8_t *r, uint32_t len, uint32_t max_key, uint32_t max_value,
                                               uint32_t expect_op)
{
    LzfRequest o = {0u, (uint32_t)LZF_REQ_BADOP, 0u, 0u, 0u, 0u, 0};
    if (len < 2u) return o;
    const uint32_t op = (uint32_t)r[0] | ((uint32_t)r[1] << 8);
    const int g = lzf_request_grammar(op);
    if (g == LZF_RQ_BAD) return o;
    o.op = op;
    if (expect_op && op != expect_op) {
        o.status = LZF_REQ_OTHER;
        return o;
    }
    o.status = LZF_REQ_OK;
    if (g == LZF_RQ_EMPTY) return o;
    o.status = LZF_REQ_ERR;
    const uint8_t *p = r + 2;
    const uint32_t size = len - 2u;
    const uint32_t end = size < max_key ? size : max_key;
    uint32_t kat = 0u;
    if (g == LZF_RQ_SET) {                                    /* the ttl token; size == 0, where the reference asserts: t == 0 */
        const uint32_t t = lzf_request_span(p, 0u, end);
        if (!t) return o;
        kat = t + 1u;
    }
    const uint32_t k = lzf_request_span(p, kat, end) - kat;
    if (!k) return o;
    uint32_t vat = 0u, vlen = 0u;
    if (g != LZF_RQ_KEY) {
        /* size - klen - 1, for SET size - ttllen - klen - 2: -1 where the
         * reference's size_t wraps */
        const int64_t left = (int64_t)size - (int64_t)kat - (int64_t)k - 1;
        if (g == LZF_RQ_KEYOPT && left < 0) {                 /* `left > 0` fails: no value, limit -1 */
            o.num = -1;
        } else {
            if (left == 0) return o;
            if (left < 0) {
                o.status = LZF_REQ_SHORT;
                return o;
            }
            vat = kat + k + 1u;
            vlen = left < (int64_t)max_value ? (uint32_t)left : max_value;
        }
    }
    o.status = LZF_REQ_OK;
    o.key_at = 2u + kat;
    o.key_len = k;
    if (vlen) {
        o.val_at = 2u + vat;
        o.val_len = vlen;
    }
    int ok = 1;
    if (g == LZF_RQ_SET) ok = lzf_parse_long(p, kat - 1u, &o.num);
    else if (vlen && (g == LZF_RQ_KEYNUM || g == LZF_RQ_KEYOPT)) ok = lzf_parse_long(p + vat, vlen, &o.num);
    if (!ok) {
        o.status = LZF_REQ_NAN;
        o.num = 0;
    }
    return o;
}

/* a batch of requests and the arrays its parse fills; device pointers for the
 * kernel, host pointers for lzf_host_request_parse */
struct LzfRequestArgs {
    const uint8_t *req;
    uint64_t req_bytes;
    const uint64_t *req_off;
    const uint32_t *req_len;
    uint32_t n, max_key, max_value, expect_op;
    uint8_t *op, *status;
    uint64_t *key_off, *val_off;
    uint32_t *key_len, *val_len;
    int64_t *num;
    uint64_t *result;
};

/* request k of the batch: the range test, the parse, the seven outputs with
 * their offsets absolute into req; -> the status */
LZF_HD inline uint32_t lzf_request_entry(const LzfRequestArgs &a, uint64_t k)
{
    const uint64_t off = a.req_off[k];
    const uint32_t len = a.req_len[k];
    LzfRequest o = {0u, (uint32_t)LZF_REQ_ERANGE, 0u, 0u, 0u, 0u, 0};
    if (off <= a.req_bytes && len <= a.req_bytes - off)
        o = lzf_request_parse_one(a.req + off, len, a.max_key, a.max_value, a.expect_op);
    a.op[k] = (uint8_t)o.op;
    a.status[k] = (uint8_t)o.status;
    a.key_off[k] = o.key_len ? off + o.key_at : 0ull;
    a.key_len[k] = o.key_len;
    a.val_off[k] = o.val_len ? off + o.val_at : 0ull;
    a.val_len[k] = o.val_len;
    a.num[k] = o.num;
    return o.status;
}

/* what the host replies for a status: -1 the operator replies, -2 close the
 * connection (gbProcessQuery returns GB_ERR), else the REPL_* code */
LZF_HD inline int lzf_request_reply_code_of(int status)
{
    switch (status) {
    case LZF_REQ_OK: return -1;
    case LZF_REQ_BADOP: return -2;
    case LZF_REQ_NAN: return LZF_REPL_ERR_NAN;
    default: return LZF_REPL_ERR;
    }
}

/* The reply code of an operator's entry status, the single-key replies of
 * gbQueryIncDecHandler and its kin (src/query.c:853-886): REPL_VAL for an
 * entry the operator applied to, the error code of the others.  One rule for
 * the reply kernels, the stitch and lzf_host_reply_code */
LZF_HD inline int lzf_reply_code_of(int ent_status)
{
    switch (ent_status) {
    case LZF_ENT_DONE:
    case LZF_ENT_CONVERTED: return LZF_REPL_VAL;
    case LZF_ENT_DEAD:
    case LZF_ENT_EXPIRED: return LZF_REPL_ERR_NOT_FOUND;
    case LZF_ENT_LOCKED: return LZF_REPL_ERR_LOCKED;
    case LZF_ENT_NAN:
    case LZF_ENT_UNCHANGED: return LZF_REPL_ERR_NAN;
    default: return LZF_REPL_ERR;
    }
}

/* ---- dispatch: the class rule, the bucket on the host, the stitch rule ------------
 * (lzf_dispatch.hip has the kernels, lzf_api.cpp the calls, csrc/dispatch_check.cpp
 * runs the host forms under the host sanitizers) */

/* the class of a parsed request: 0 refused -- every status but OK and NAN, and
 * an op the parse cannot yield; the operator itself, 1 .. 21, NAN travelling
 * with it; LZF_RQ_NCLASS - 1 for END */
LZF_HD inline uint32_t lzf_request_class_of(uint32_t op, uint32_t status)
{
    if (status != (uint32_t)LZF_REQ_OK && status != (uint32_t)LZF_REQ_NAN) return 0u;
    if (op == (uint32_t)LZF_OP_END) return (uint32_t)LZF_RQ_NCLASS - 1u;
    return op >= (uint32_t)LZF_OP_SET && op <= (uint32_t)LZF_OP_KEYS ? op : 0u;
}

/* lzf_host_request_bucket: a counting sort by class, stable; host pointers */
inline void lzf_request_bucket_host(const uint8_t *op, const uint8_t *status, const uint64_t *key_off,
                                    const uint32_t *key_len, const uint64_t *val_off, const uint32_t *val_len,
                                    const int64_t *num, uint32_t n, uint32_t *perm, uint32_t *slot,
                                    uint32_t *class_first, uint8_t *b_op, uint8_t *b_status, uint64_t *b_key_off,
                                    uint32_t *b_key_len, uint64_t *b_val_off, uint32_t *b_val_len, int64_t *b_num)
{
    uint64_t at[LZF_RQ_NCLASS] = {0ull};
    for (uint64_t k = 0; k < n; k++) at[lzf_request_class_of(op[k], status[k])]++;
    uint64_t x = 0ull;
    for (uint32_t c = 0; c < (uint32_t)LZF_RQ_NCLASS; c++) {
        const uint64_t cnt = at[c];
        class_first[c] = (uint32_t)x;
        at[c] = x;
        x += cnt;
    }
    class_first[LZF_RQ_NCLASS] = n;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t j = at[lzf_request_class_of(op[k], status[k])]++;
        perm[j] = (uint32_t)k;
        slot[k] = (uint32_t)j;
        b_op[j] = op[k];
        b_status[j] = status[k];
        b_key_off[j] = key_off[k];
        b_key_len[j] = key_len[k];
        b_val_off[j] = val_off[k];
        b_val_len[j] = val_len[k];
        b_num[j] = num[k];
    }
}

/* the stitch of a bucketed batch's replies; device pointers for the kernel,
 * host pointers for lzf_host_request_stitch.  class_mode and class_base travel
 * by value */
struct LzfStitchArgs {
    const uint8_t *op, *status;
    const uint32_t *slot, *class_first;
    uint32_t n;
    uint8_t class_mode[LZF_RQ_NCLASS];
    uint64_t class_base[LZF_RQ_NCLASS];
    const uint64_t *b_rep_off;
    const uint32_t *b_rep_len;
    const uint8_t *b_ent, *b_refused;
    uint8_t *replies;
    uint64_t rep_cap, code_base;
    uint64_t *out_off;
    uint32_t *out_len;
    uint8_t *out_kind;
    uint64_t *result;
};

/* what a request's reply is counted as: result[0 .. 3]; BAD is a code reply
 * that also counts in result[4] */
enum { LZF_ST_ARENA = 0, LZF_ST_CODE = 1, LZF_ST_CLOSE = 2, LZF_ST_HOST = 3, LZF_ST_BAD = 4, LZF_ST_NTALLY = 5 };

#define LZF_STITCH_CODES 64u              /* the bytes of the code area */

/* byte t of the code area: the frames of the codes 0 .. 6, [i16 code][u8
 * PLAIN][u32 1][0x00] each (gbClientEnqueueCode, as lzf_reply.hip writes it),
 * then 8 zero bytes */
LZF_HD inline uint8_t lzf_stitch_code_byte(uint32_t t)
{
    const uint32_t code = t >> 3, b = t & 7u;
    if (code > 6u) return 0u;
    return b == 0u ? (uint8_t)code : b == 3u ? (uint8_t)1u : (uint8_t)0u;
}

/* request k's row of the reply table, the seven rules of include/lzf_gpu.h in
 * their order; -> LZF_ST_* */
LZF_HD inline uint32_t lzf_stitch_entry(const LzfStitchArgs &a, uint64_t k)
{
    const uint32_t op = a.op[k], st = a.status[k];
    uint64_t off = 0ull;
    uint32_t len = 0u, kind = LZF_OUT_REPLY, tally = LZF_ST_CODE;
    int code = LZF_REPL_ERR;
    if (st == (uint32_t)LZF_REQ_BADOP) {
        kind = LZF_OUT_CLOSE;
        tally = LZF_ST_CLOSE;
    } else if (st == (uint32_t)LZF_REQ_OK || st == (uint32_t)LZF_REQ_NAN) {
        const uint32_t c = lzf_request_class_of(op, st), mode = a.class_mode[c];
        const uint64_t j = a.slot[k];
        if (j < a.class_first[c] || j >= a.class_first[c + 1u] || j >= a.n) {
            tally = LZF_ST_BAD;                               /* a table that contradicts itself: no b_* entry is read */
        } else if (st == (uint32_t)LZF_REQ_NAN) {
            const uint32_t ent = mode == (uint32_t)LZF_STITCH_CODE ? a.b_ent[j] : (uint32_t)LZF_ENT_DONE;
            code = ent == (uint32_t)LZF_ENT_DEAD || ent == (uint32_t)LZF_ENT_EXPIRED ? LZF_REPL_ERR_NOT_FOUND
                                                                                   : LZF_REPL_ERR_NAN;
        } else if (mode == (uint32_t)LZF_STITCH_HOST) {
            kind = LZF_OUT_HOST;
            tally = LZF_ST_HOST;
        } else if (op == (uint32_t)LZF_OP_SET && a.b_refused && a.b_refused[j]) {
            code = LZF_REPL_ERR_LOCKED;
        } else if (mode == (uint32_t)LZF_STITCH_ARENA) {
            const uint64_t base = a.class_base[c], o = base + a.b_rep_off[j];
            const uint32_t l = a.b_rep_len[j];
            if (o >= base && o <= a.rep_cap && l <= a.rep_cap - o) {
                off = o;
                len = l;
                tally = LZF_ST_ARENA;
            } else {
                tally = LZF_ST_BAD;
            }
        } else {
            const int ent = a.b_ent[j];
            code = ent == LZF_ENT_DONE || ent == LZF_ENT_CONVERTED ? LZF_REPL_OK : lzf_reply_code_of(ent);
        }
    }
    if (tally == LZF_ST_CODE || tally == LZF_ST_BAD) {
        off = a.code_base + 8ull * (uint32_t)code;
        len = 8u;
    }
    a.out_off[k] = off;
    a.out_len[k] = len;
    a.out_kind[k] = (uint8_t)kind;
    return tally;
}

/* lzf_host_request_stitch: the code area, then the same entry in a loop */
inline void lzf_request_stitch_host(const LzfStitchArgs &a)
{
    for (uint32_t c = 0; c < LZF_ST_NTALLY; c++) a.result[c] = 0ull;
    for (uint32_t t = 0; t < LZF_STITCH_CODES; t++) a.replies[a.code_base + t] = lzf_stitch_code_byte(t);
    for (uint64_t k = 0; k < a.n; k++) {
        const uint32_t t = lzf_stitch_entry(a, k);
        a.result[t == LZF_ST_BAD ? LZF_ST_CODE : t]++;
        if (t == LZF_ST_BAD) a.result[LZF_ST_BAD]++;
    }
}

#endif
