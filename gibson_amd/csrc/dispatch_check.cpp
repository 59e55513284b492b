/*
 * dispatch_check.cpp -- the host forms of the request bucket and stitch
 * (lzf_request.h) under the host sanitizers (`make dispatch_check`, run by
 * tests/test_request_dispatch.py).  A stand-alone host program: its own main,
 * no kernel, not linked to the library, never loaded into Python.
 *
 * Every array lives in a heap block of exactly its size, so a read or write
 * of the host forms past an array is an AddressSanitizer report.  The bucket
 * is compared with a stable sort by class, the stitch with a second statement
 * of the seven rules of include/lzf_gpu.h written as a list, first over a
 * crafted table that pins one request per rule and then over a seeded fuzz.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "lzf_request.h"

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
    explicit Block(uint64_t n) : p((T *)malloc(n * sizeof(T))), count(n)
    {
        if (!p) exit(2);
        memset((void *)p, 0xA5, n * sizeof(T));
    }
    ~Block() { free(p); }
    Block(const Block &) = delete;
    T &operator[](uint64_t i) { return p[i]; }
};

static void fail(const char *what, uint64_t n, uint64_t at)
{
    fprintf(stderr, "dispatch_check: %s: n %llu, entry %llu\n", what, (unsigned long long)n, (unsigned long long)at);
    g_bad = 1;
}

/* the class rule once more, as a table lookup over the statement of the header */
static uint32_t naive_class(uint32_t op, uint32_t status)
{
    if (status == LZF_REQ_ERR || status == LZF_REQ_BADOP || status == LZF_REQ_SHORT || status == LZF_REQ_ERANGE ||
        status == LZF_REQ_OTHER || status >= LZF_REQ_NSTATUS)
        return 0u;
    if (op == 0xFFu) return 22u;
    for (uint32_t c = 1; c <= 21u; c++)
        if (op == c) return c;
    return 0u;
}

struct Parsed {
    Block<uint8_t> op, status;
    Block<uint64_t> key_off, val_off;
    Block<uint32_t> key_len, val_len;
    Block<int64_t> num;
    explicit Parsed(uint32_t n) : op(n), status(n), key_off(n), val_off(n), key_len(n), val_len(n), num(n) {}
};

/* pick: 0 uniform over the classes, 1 one class, 2 alternating pair, 3 runs, 4 realistic */
static void fill_parsed(Parsed &p, uint32_t n, int pick)
{
    static const uint8_t ops[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 200, 255};
    const uint32_t one = rnd(23), run = 64u + rnd(2);
    for (uint32_t k = 0; k < n; k++) {
        uint32_t op, st = LZF_REQ_OK;
        switch (pick) {
        case 0:
            op = ops[rnd(sizeof ops)];
            st = rnd(4) ? LZF_REQ_OK : rnd(LZF_REQ_NSTATUS + 1u);
            break;
        case 1: op = one == 22u ? 0xFFu : one; st = one ? LZF_REQ_OK : LZF_REQ_ERR; break;
        case 2: op = k & 1u ? LZF_OP_GET : LZF_OP_SET; break;
        case 3: op = 1u + (k / run) % 21u; break;
        default: {
            const uint32_t x = rnd(100);
            op = x < 70u ? LZF_OP_GET : x < 90u ? LZF_OP_SET : ops[1u + rnd(21)];
            st = rnd(100) < 3u ? (uint32_t)LZF_REQ_ERR + rnd(6) : LZF_REQ_OK;
        }
        }
        p.op[k] = (uint8_t)op;
        p.status[k] = (uint8_t)st;
        p.key_off[k] = ((uint64_t)rnd(1u << 31) << 20) + k;
        p.key_len[k] = rnd(1u << 16);
        p.val_off[k] = ~(uint64_t)k;
        p.val_len[k] = rnd(1u << 31);
        p.num[k] = (int64_t)(((uint64_t)rnd(1u << 31) << 33) ^ k);
    }
}

static void check_bucket(uint32_t n, int pick)
{
    Parsed p(n), b(n);
    fill_parsed(p, n, pick);
    Block<uint32_t> perm(n), slot(n), first(LZF_RQ_NCLASS + 1u);
    lzf_request_bucket_host(p.op.p, p.status.p, p.key_off.p, p.key_len.p, p.val_off.p, p.val_len.p, p.num.p, n, perm.p,
                            slot.p, first.p, b.op.p, b.status.p, b.key_off.p, b.key_len.p, b.val_off.p, b.val_len.p,
                            b.num.p);
    std::vector<uint32_t> want(n);
    for (uint32_t k = 0; k < n; k++) want[k] = k;
    std::stable_sort(want.begin(), want.end(), [&](uint32_t x, uint32_t y) {
        return naive_class(p.op[x], p.status[x]) < naive_class(p.op[y], p.status[y]);
    });
    uint32_t count[LZF_RQ_NCLASS] = {0u};
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t c = naive_class(p.op[k], p.status[k]);
        if (c != lzf_request_class_of(p.op[k], p.status[k])) fail("class rule", n, k);
        count[c]++;
    }
    uint32_t x = 0u;
    for (uint32_t c = 0; c < LZF_RQ_NCLASS; c++) {
        if (first[c] != x) fail("class_first", n, c);
        x += count[c];
    }
    if (first[LZF_RQ_NCLASS] != n) fail("class_first end", n, LZF_RQ_NCLASS);
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t k = want[j];
        if (perm[j] != k || slot[k] != j) fail("perm / slot", n, j);
        if (b.op[j] != p.op[k] || b.status[j] != p.status[k] || b.key_off[j] != p.key_off[k] ||
            b.key_len[j] != p.key_len[k] || b.val_off[j] != p.val_off[k] || b.val_len[j] != p.val_len[k] ||
            b.num[j] != p.num[k])
            fail("gather", n, j);
    }
    g_cases++;
}

/* ---- the stitch ------------------------------------------------------------------ */

struct Row {
    uint64_t off;
    uint32_t len;
    uint8_t kind;
};

struct Stitch {
    uint32_t n;
    Block<uint8_t> op, status;
    Block<uint32_t> slot, first;
    uint8_t mode[LZF_RQ_NCLASS];
    uint64_t base[LZF_RQ_NCLASS];
    Block<uint64_t> rep_off;
    Block<uint32_t> rep_len;
    Block<uint8_t> ent, refused;
    uint64_t rep_cap, code_base;
    explicit Stitch(uint32_t n_) : n(n_), op(n_), status(n_), slot(n_), first(LZF_RQ_NCLASS + 1u), rep_off(n_),
                                   rep_len(n_), ent(n_), refused(n_), rep_cap(0), code_base(0) {}
};

/* the seven rules as the header lists them; the tallies in t[5] */
static Row naive_row(Stitch &s, uint32_t k, bool with_refused, uint64_t *t)
{
    const uint32_t op = s.op[k], st = s.status[k];
    const Row err = {s.code_base + 8u * LZF_REPL_ERR, 8u, LZF_OUT_REPLY};
    if (st == LZF_REQ_BADOP) {                                                   /* 1 */
        t[2]++;
        return Row{0, 0, LZF_OUT_CLOSE};
    }
    t[1]++;
    if (st != LZF_REQ_OK && st != LZF_REQ_NAN) return err;                       /* 2 */
    const uint32_t c = naive_class(op, st), j = s.slot[k];
    if (j < s.first[c] || j >= s.first[c + 1u] || j >= s.n) {                    /* the table contradicts itself */
        t[4]++;
        return err;
    }
    if (st == LZF_REQ_NAN) {                                                     /* 3 */
        const bool gone = s.mode[c] == LZF_STITCH_CODE && (s.ent[j] == LZF_ENT_DEAD || s.ent[j] == LZF_ENT_EXPIRED);
        return Row{s.code_base + 8u * (gone ? LZF_REPL_ERR_NOT_FOUND : LZF_REPL_ERR_NAN), 8u, LZF_OUT_REPLY};
    }
    if (s.mode[c] == LZF_STITCH_HOST) {                                          /* 4 */
        t[1]--;
        t[3]++;
        return Row{0, 0, LZF_OUT_HOST};
    }
    if (op == LZF_OP_SET && with_refused && s.refused[j])                        /* 5 */
        return Row{s.code_base + 8u * LZF_REPL_ERR_LOCKED, 8u, LZF_OUT_REPLY};
    if (s.mode[c] == LZF_STITCH_ARENA) {                                         /* 6 */
        const unsigned __int128 o = (unsigned __int128)s.base[c] + s.rep_off[j];
        if (o + s.rep_len[j] > s.rep_cap) {
            t[4]++;
            return err;
        }
        t[1]--;
        t[0]++;
        return Row{(uint64_t)o, s.rep_len[j], LZF_OUT_REPLY};
    }
    int code;                                                                    /* 7 */
    switch (s.ent[j]) {
    case LZF_ENT_DONE:
    case LZF_ENT_CONVERTED: code = LZF_REPL_OK; break;
    case LZF_ENT_DEAD:
    case LZF_ENT_EXPIRED: code = LZF_REPL_ERR_NOT_FOUND; break;
    case LZF_ENT_LOCKED: code = LZF_REPL_ERR_LOCKED; break;
    case LZF_ENT_NAN:
    case LZF_ENT_UNCHANGED: code = LZF_REPL_ERR_NAN; break;
    default: code = LZF_REPL_ERR;
    }
    return Row{s.code_base + 8u * (uint32_t)code, 8u, LZF_OUT_REPLY};
}

/* the host form's arguments over s and the output blocks, as lzf_api.cpp fills
 * them once its checks have passed (those are tests/test_request_dispatch.py's) */
static LzfStitchArgs args_of(Stitch &s, bool with_ent, bool with_refused, uint8_t *replies, uint64_t *off, uint32_t *len,
                             uint8_t *kind, uint64_t *result)
{
    LzfStitchArgs a{};
    a.op = s.op.p; a.status = s.status.p; a.slot = s.slot.p; a.class_first = s.first.p; a.n = s.n;
    memcpy(a.class_mode, s.mode, sizeof a.class_mode);
    memcpy(a.class_base, s.base, sizeof a.class_base);
    a.b_rep_off = s.rep_off.p; a.b_rep_len = s.rep_len.p;
    a.b_ent = with_ent ? s.ent.p : nullptr; a.b_refused = with_refused ? s.refused.p : nullptr;
    a.replies = replies; a.rep_cap = s.rep_cap; a.code_base = s.code_base;
    a.out_off = off; a.out_len = len; a.out_kind = kind; a.result = result;
    return a;
}

/* run the host form over s -- b_ent / b_refused NULL when asked -- and compare */
static void run_stitch(Stitch &s, bool with_ent, bool with_refused, uint64_t *seen)
{
    const uint32_t n = s.n;
    Block<uint8_t> replies(s.rep_cap), kind(n);
    Block<uint64_t> off(n), result(LZF_ST_NTALLY);
    Block<uint32_t> len(n);
    lzf_request_stitch_host(args_of(s, with_ent, with_refused, replies.p, off.p, len.p, kind.p, result.p));
    uint64_t t[5] = {0, 0, 0, 0, 0};
    for (uint32_t k = 0; k < n; k++) {
        const Row w = naive_row(s, k, with_refused, t);
        if (off[k] != w.off || len[k] != w.len || kind[k] != w.kind) fail("stitch row", n, k);
        if (seen && w.kind == LZF_OUT_REPLY && w.len == 8u && w.off >= s.code_base && w.off < s.code_base + 64u)
            seen[(w.off - s.code_base) / 8u]++;
    }
    for (uint32_t c = 0; c < 5u; c++)
        if (result[c] != t[c]) fail("stitch result", n, c);
    if (t[0] + t[1] + t[2] + t[3] != n) fail("stitch result sum", n, 0);
    for (uint64_t i = 0; i < s.rep_cap; i++) {
        uint8_t want = 0xA5;
        if (i >= s.code_base && i < s.code_base + 64u) {
            const uint32_t code = (uint32_t)(i - s.code_base) / 8u, b = (uint32_t)(i - s.code_base) % 8u;
            const uint8_t frame[8] = {(uint8_t)code, 0, LZF_ENC_PLAIN, 1, 0, 0, 0, 0};
            want = code <= 6u ? frame[b] : 0u;
        }
        if (replies[i] != want) fail("reply bytes", n, i);
    }
    if (seen) {
        seen[8] += t[0];
        seen[9] += t[2];
        seen[10] += t[3];
        seen[11] += t[4];
    }
    g_cases++;
}

/* a consistent bucketed batch: op / status drawn, slot and class_first from a
 * stable sort, the b_* arrays random */
static void fill_stitch(Stitch &s, bool code_classes)
{
    static const uint8_t ops[] = {1, 1, 1, 3, 3, 3, 4, 4, 7, 8, 2, 19, 18, 255, 11, 21, 5, 0, 22};
    static const uint8_t sts[] = {0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 1, 3, 4, 5, 6};
    const uint32_t n = s.n;
    for (uint32_t k = 0; k < n; k++) {
        s.op[k] = ops[rnd(sizeof ops)];
        s.status[k] = sts[rnd(sizeof sts)];
    }
    std::vector<uint32_t> perm(n);
    for (uint32_t k = 0; k < n; k++) perm[k] = k;
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) {
        return naive_class(s.op[x], s.status[x]) < naive_class(s.op[y], s.status[y]);
    });
    uint32_t count[LZF_RQ_NCLASS] = {0u};
    for (uint32_t j = 0; j < n; j++) {
        s.slot[perm[j]] = j;
        count[naive_class(s.op[perm[j]], s.status[perm[j]])]++;
    }
    uint32_t x = 0u;
    for (uint32_t c = 0; c <= LZF_RQ_NCLASS; c++) {
        s.first[c] = x;
        if (c < LZF_RQ_NCLASS) x += count[c];
    }
    for (uint32_t c = 0; c < LZF_RQ_NCLASS; c++) {
        s.mode[c] = LZF_STITCH_HOST;
        s.base[c] = 100u * c;
    }
    s.mode[LZF_OP_SET] = s.mode[LZF_OP_GET] = s.mode[LZF_OP_INC] = LZF_STITCH_ARENA;
    if (code_classes) s.mode[LZF_OP_DEL] = s.mode[LZF_OP_LOCK] = s.mode[LZF_OP_UNLOCK] = s.mode[LZF_OP_TTL] = LZF_STITCH_CODE;
    s.rep_cap = 4096u;
    s.code_base = 8u * rnd(400);
    s.base[LZF_OP_INC] = ~0ull - 50u;                          /* wraps for most offsets */
    for (uint32_t j = 0; j < n; j++) {
        s.rep_off[j] = rnd(8) ? rnd(3000) : rnd(6000);
        s.rep_len[j] = rnd(8) ? rnd(300) : rnd(2000);
        s.ent[j] = (uint8_t)rnd(9);
        s.refused[j] = rnd(4) ? 0u : (uint8_t)(1u + rnd(255));
    }
}

int main()
{
    /* the class rule over every pair */
    for (uint32_t op = 0; op < 256u; op++)
        for (uint32_t st = 0; st < 9u; st++)
            if (lzf_request_class_of(op, st) != naive_class(op, st) || lzf_request_class_of(op, st) >= LZF_RQ_NCLASS)
                fail("class rule", op, st);

    static const uint32_t ns[] = {1, 2, 63, 64, 65, 255, 1023, 1024, 1025, 3079, 20011};
    for (const uint32_t n : ns)
        for (int pick = 0; pick < 5; pick++) check_bucket(n, pick);
    for (unsigned it = 0; it < 300u; it++) check_bucket(1u + rnd(700), (int)rnd(5));

    /* the crafted table: one request per rule, classes of one or two requests */
    {
        /*                 BADOP ERR  NAN/del  NAN/del  NAN/get PING SET-locked SET  GET   GET-bad DEL  DEL   DEL  */
        const uint8_t op[] = {0, 3, 4, 4, 3, 19, 1, 1, 3, 3, 4, 4, 4};
        const uint8_t st[] = {3, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0};
        const uint32_t n = sizeof op;
        Stitch s(n);
        memcpy(s.op.p, op, n);
        memcpy(s.status.p, st, n);
        /* bucket order: class 0: 0 1 | SET: 6 7 | GET: 4 8 9 | DEL: 2 3 10 11 12 | PING: 5 */
        const uint32_t slot[] = {0, 1, 7, 8, 4, 12, 2, 3, 5, 6, 9, 10, 11};
        memcpy(s.slot.p, slot, sizeof slot);
        for (uint32_t c = 0; c <= LZF_RQ_NCLASS; c++)
            s.first[c] = c <= 1u ? 2u * c : c <= 3u ? 4u : c == 4u ? 7u : c <= 19u ? 12u : 13u;
        s.first[0] = 0u;
        for (uint32_t c = 0; c < LZF_RQ_NCLASS; c++) {
            s.mode[c] = LZF_STITCH_HOST;
            s.base[c] = 0u;
        }
        s.mode[1] = s.mode[3] = LZF_STITCH_ARENA;
        s.mode[4] = LZF_STITCH_CODE;
        s.base[1] = 100u;
        s.base[3] = 200u;
        s.rep_cap = 364u;
        s.code_base = 300u;
        for (uint32_t j = 0; j < n; j++) {
            s.rep_off[j] = 10u * j;
            s.rep_len[j] = 9u;
            s.ent[j] = LZF_ENT_DONE;
            s.refused[j] = 0u;
        }
        s.refused[2] = 1u;                                     /* request 6 */
        s.rep_off[6] = 160u;                                   /* request 9: 200 + 160 + 9 > 364 */
        s.ent[7] = LZF_ENT_DEAD;                               /* request 2: NAN on a missing key */
        s.ent[8] = LZF_ENT_LOCKED;                             /* request 3: NAN on a present key */
        s.ent[10] = LZF_ENT_EXPIRED;                           /* request 11 */
        s.ent[11] = LZF_ENT_LOCKED;                            /* request 12 */
        run_stitch(s, true, true, nullptr);
        Block<uint8_t> replies(s.rep_cap), kind(n);
        Block<uint64_t> off(n), result(5);
        Block<uint32_t> len(n);
        lzf_request_stitch_host(args_of(s, true, true, replies.p, off.p, len.p, kind.p, result.p));
        const int want_code[] = {-1, LZF_REPL_ERR, LZF_REPL_ERR_NOT_FOUND, LZF_REPL_ERR_NAN, LZF_REPL_ERR_NAN, -2,
                                 LZF_REPL_ERR_LOCKED, -3, -3, LZF_REPL_ERR, LZF_REPL_OK, LZF_REPL_ERR_NOT_FOUND,
                                 LZF_REPL_ERR_LOCKED};
        for (uint32_t k = 0; k < n; k++) {
            bool ok;
            if (want_code[k] == -1) ok = kind[k] == LZF_OUT_CLOSE && !off[k] && !len[k];
            else if (want_code[k] == -2) ok = kind[k] == LZF_OUT_HOST && !off[k] && !len[k];
            else if (want_code[k] == -3) ok = kind[k] == LZF_OUT_REPLY && len[k] == 9u &&
                                              off[k] == s.base[op[k]] + 10u * slot[k];
            else ok = kind[k] == LZF_OUT_REPLY && len[k] == 8u && off[k] == 300u + 8u * (uint32_t)want_code[k];
            if (!ok) fail("crafted stitch", n, k);
        }
        if (result[0] != 2u || result[1] != 9u || result[2] != 1u || result[3] != 1u || result[4] != 1u)
            fail("crafted stitch result", n, 0);
    }

    /* the fuzz: codes 0 1 2 4 5, arena, close, host and bad slices all occur */
    uint64_t seen[12] = {0};
    for (unsigned it = 0; it < 400u; it++) {
        Stitch s(1u + rnd(it % 8u ? 300u : 3000u));
        const bool code_classes = rnd(4) != 0;
        fill_stitch(s, code_classes);
        run_stitch(s, code_classes || rnd(2), rnd(2) != 0, seen);
        if (it % 16u == 0u) {                                  /* a slot that leaves its class: no b_* entry is read */
            const uint32_t k = rnd(s.n);
            s.slot[k] = rnd(2) ? s.n + rnd(5) : s.n - 1u - s.slot[k];
            run_stitch(s, code_classes || rnd(2), true, seen);
        }
    }
    static const unsigned need[] = {0, 1, 2, 4, 5, 8, 9, 10, 11};
    for (const unsigned c : need)
        if (seen[c] < 100u) {
            fprintf(stderr, "dispatch_check: the fuzz produced outcome %u only %llu times\n", c, (unsigned long long)seen[c]);
            g_bad = 1;
        }
    if (seen[3] || seen[6] || seen[7]) fail("a code frame that no rule yields", 0, 0);
    if (g_bad) return 1;
    printf("dispatch_check: ok, %u cases\n", g_cases);
    return 0;
}
