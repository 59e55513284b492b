"""Request ingest (lzf_gpu_request_parse, lzf_host_request_parse,
lzf_gpu_store_append_keys): raw request buffers become the descriptors of the
device store's calls, against a Python transcription of the reference.

The model follows src/query.c:229-373 and the handlers' use of it line by
line, the wrapped size_t subtraction included, and only then tells
LZF_REQ_SHORT -- the one departure, a value span that would leave the request
-- from OK.  It shares no logic with csrc/lzf_request.h.  The bar is bit-exact.

On the GPU every output is a view into a larger tensor whose excess, in front
and behind, holds a guard byte that is checked afterwards."""
import ctypes
import os
import random
import struct
import subprocess

import numpy as np
import pytest

try:                                    # before liblzf_hip.so loads: one HIP runtime in the process
    import torch as _torch  # noqa: F401
except ImportError:
    _torch = None

import gibson_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("lzf_gpu_request_parse", "lzf_host_request_parse", "lzf_host_request_reply_code",
             "lzf_gpu_store_append_keys_work_size", "lzf_gpu_store_append_keys")
OK, ERR, NAN, BADOP, SHORT, ERANGE, OTHER = range(7)
SET, TTL, GET, MSET, MGET, PING, END = 1, 2, 3, 9, 11, 19, 0xFF
ENC_PLAIN, ENC_LZF, ENC_NULL = 0, 1, 0xFF
STORE_OK, STORE_FULL = 0, 1
PAD = 0xFFFFFFFF
M64 = (1 << 64) - 1
FIELDS = ("op", "status", "key_off", "key_len", "val_off", "val_len", "num")
DTYPE = {"op": np.uint8, "status": np.uint8, "key_off": np.uint64, "key_len": np.uint32, "val_off": np.uint64,
         "val_len": np.uint32, "num": np.int64}

# the grammar rows of gbProcessQuery's operator table (src/query.c:1393-1485)
ROW_KEY = (3, 4, 5, 6, 8, 12, 13, 14, 16, 17, 21)
ROW_KEYVAL = (9, 20)
ROW_KEYNUM = (2, 10, 7, 15)
ROW_OPT = (11,)
ROW_SET = (1,)
ROW_EMPTY = (18, 19, 0xFF)


# ---- the model: src/query.c, line by line ---------------------------------------

def ref_parse_long(v):
    """gbQueryParseLong (src/query.c:39-76); long arithmetic modulo 2^64"""
    assert len(v) > 0
    n, sign, start = 0, 1, 0
    c = v[0]
    if c == ord("0"):
        return 1, 0
    elif c == ord("-"):
        sign, start = -1, 1
    for i in range(start, len(v)):
        c = v[i]
        if ord("0") <= c <= ord("9"):
            n = (n * 10 + (c - ord("0"))) & M64
        else:
            return 0, None
    n = (n * sign) & M64
    return 1, n - (1 << 64) if n >> 63 else n


def ref_scan(buf, p, i, end):
    """while( i++ < end && *p != ' ' ) ++p;  -> p, i"""
    while True:
        go = i < end
        i += 1
        if not (go and buf[p] != 0x20):
            return p, i
        p += 1


def ref_key_opt(buf, size, maxkey, maxvalue):
    """gbParseKeyAndOptionalValue (:229-278) -> ret, key, klen, value, vlen"""
    p, i = 0, 0
    key = p
    end = min(size, maxkey)
    p, i = ref_scan(buf, p, i, end)
    klen = p - key
    p += 1
    left = (size - klen) & M64
    if left > 0:
        value = p
        vlen = min((left - 1) & M64, maxvalue)
    else:
        value, vlen = None, 0
    if klen <= 0:
        return 0, key, klen, value, vlen
    elif value is not None and vlen <= 0:
        return 0, key, klen, value, vlen
    return 1, key, klen, value, vlen


def ref_key_value(buf, size, maxkey, maxvalue, want_value):
    """gbParseKeyValue (:280-318)"""
    p, i = 0, 0
    key = p
    end = min(size, maxkey)
    p, i = ref_scan(buf, p, i, end)
    klen = p - key
    p += 1
    value, vlen = None, 0
    if want_value:
        value = p
        vlen = min((size - klen - 1) & M64, maxvalue)
    if klen <= 0:
        return 0, key, klen, value, vlen
    elif value is not None and vlen <= 0:
        return 0, key, klen, value, vlen
    return 1, key, klen, value, vlen


def ref_ttl_key_value(buf, size, maxkey, maxvalue):
    """gbParseTtlKeyValue (:320-373): one counter i for both scans"""
    p, i = 0, 0
    ttl = p
    end = min(size, maxkey)
    p, i = ref_scan(buf, p, i, end)
    ttllen = p - ttl
    p += 1
    key = p
    end = min(size, maxkey)
    p, i = ref_scan(buf, p, i, end)
    klen = p - key
    p += 1
    value = p
    vlen = min((size - ttllen - klen - 2) & M64, maxvalue)
    if ttllen <= 0:
        ret = 0
    elif klen <= 0:
        ret = 0
    elif vlen <= 0:
        ret = 0
    else:
        ret = 1
    return ret, ttllen, key, klen, value, vlen


def model_one(r, maxkey, maxvalue, expect_op=0):
    """one request -> (op, status, key_at, key_len, val_at, val_len, num),
    offsets from the request's first byte"""
    bad = (0, BADOP, 0, 0, 0, 0, 0)
    if len(r) < 2:
        return bad
    op = struct.unpack("<h", r[:2])[0]
    if op not in ROW_KEY + ROW_KEYVAL + ROW_KEYNUM + ROW_OPT + ROW_SET + ROW_EMPTY:
        return bad
    if expect_op and op != expect_op:
        return (op, OTHER, 0, 0, 0, 0, 0)
    if op in ROW_EMPTY:
        return (op, OK, 0, 0, 0, 0, 0)
    buf, size = r[2:], len(r) - 2
    err = (op, ERR, 0, 0, 0, 0, 0)
    ttllen = 0
    if op in ROW_SET:
        if size == 0:                                   # assert( size > 0 )
            return err
        ret, ttllen, key, klen, value, vlen = ref_ttl_key_value(buf, size, maxkey, maxvalue)
    elif op in ROW_OPT:
        ret, key, klen, value, vlen = ref_key_opt(buf, size, maxkey, maxvalue)
    else:
        ret, key, klen, value, vlen = ref_key_value(buf, size, maxkey, maxvalue, op not in ROW_KEY)
    if not ret:
        return err
    if value is not None and vlen and value + vlen > size:
        return (op, SHORT, 0, 0, 0, 0, 0)               # the reference reads past its buffer here
    num, ok = 0, 1
    if op in ROW_SET:
        ok, num = ref_parse_long(buf[:ttllen])
    elif op in ROW_KEYNUM:
        ok, num = ref_parse_long(buf[value:value + vlen])
    elif op in ROW_OPT:
        num = -1
        if value is not None and vlen:
            ok, num = ref_parse_long(buf[value:value + vlen])
    has_val = value is not None and vlen > 0
    return (op, OK if ok else NAN, 2 + key, klen, 2 + value if has_val else 0, vlen if has_val else 0,
            num if ok else 0)


def model_batch(arena, off, ln, req_bytes, maxkey, maxvalue, expect_op=0, cache=None):
    """-> {field: array} and the per-status counts"""
    out = {f: np.zeros(len(ln), DTYPE[f]) for f in FIELDS}
    counts = [0] * 7
    for k in range(len(ln)):
        o, n = int(off[k]), int(ln[k])
        if o + n > req_bytes:
            t = (0, ERANGE, 0, 0, 0, 0, 0)
        else:
            r = bytes(arena[o:o + n])
            key = (r, maxkey, maxvalue, expect_op)
            t = cache.get(key) if cache is not None else None
            if t is None:
                t = model_one(r, maxkey, maxvalue, expect_op)
                if cache is not None:
                    cache[key] = t
        counts[t[1]] += 1
        out["op"][k], out["status"][k], out["num"][k] = t[0], t[1], t[6]
        out["key_off"][k], out["key_len"][k] = (o + t[2] if t[3] else 0), t[3]
        out["val_off"][k], out["val_len"][k] = (o + t[4] if t[5] else 0), t[5]
    return out, counts


def request(op, payload):
    return struct.pack("<H", op) + payload


def pack(reqs):
    """requests back to back -> arena, off, len"""
    ln = np.array([len(r) for r in reqs], np.uint32)
    off = (np.cumsum(ln.astype(np.int64)) - ln).astype(np.uint64)
    return np.frombuffer(b"".join(reqs), np.uint8), off, ln


# (op, payload, max_key, max_value, expect_op, status, key, value, num)
CRAFTED = [
    (SET, b"10 key v", 512, 4096, 0, OK, b"key", b"v", 10),
    (SET, b"10 key", 512, 4096, 0, SHORT, b"", b"", 0),
    (SET, b"10 key ", 512, 4096, 0, ERR, b"", b"", 0),
    (SET, b"10", 512, 4096, 0, ERR, b"", b"", 0),
    (SET, b"10 ", 512, 4096, 0, ERR, b"", b"", 0),
    (SET, b" key v", 512, 4096, 0, ERR, b"", b"", 0),
    (SET, b"", 512, 4096, 0, ERR, b"", b"", 0),
    (SET, b"0x k v", 512, 4096, 0, OK, b"k", b"v", 0),
    (SET, b"- k v", 512, 4096, 0, OK, b"k", b"v", 0),
    (SET, b"1x k v", 512, 4096, 0, NAN, b"k", b"v", 0),
    (TTL, b"abc", 512, 4096, 0, SHORT, b"", b"", 0),
    (TTL, b"abc ", 512, 4096, 0, ERR, b"", b"", 0),
    (TTL, b"abc x", 512, 4096, 0, NAN, b"abc", b"x", 0),
    (TTL, b"abc 77", 512, 4096, 0, OK, b"abc", b"77", 77),
    (MGET, b"abc", 512, 4096, 0, OK, b"abc", b"", -1),
    (MGET, b"abc ", 512, 4096, 0, ERR, b"", b"", 0),
    (MGET, b"abc 9", 512, 4096, 0, OK, b"abc", b"9", 9),
    (GET, b"abc def", 512, 4096, 0, OK, b"abc", b"", 0),
    (TTL, b"abcd", 4, 4096, 0, SHORT, b"", b"", 0),
    (TTL, b"abcde", 4, 4096, 0, ERR, b"", b"", 0),
    (TTL, b"abcdef", 4, 4096, 0, NAN, b"abcd", b"f", 0),
    (SET, b"10 abcdefgh value", 8, 4096, 0, OK, b"abcde", b"gh value", 10),        # the budget ends inside the key
    (SET, b"5 key 0123456789", 512, 4, 0, OK, b"key", b"0123", 5),                 # clamped to max_value
    (MSET, b"pre some value", 512, 4096, 0, OK, b"pre", b"some value", 0),
    (0, b"abc", 512, 4096, 0, BADOP, b"", b"", 0),
    (22, b"abc", 512, 4096, 0, BADOP, b"", b"", 0),
    (0x0101, b"abc", 512, 4096, 0, BADOP, b"", b"", 0),
    (0x00FF, b"abc", 512, 4096, 0, OK, b"", b"", 0),
    (PING, b"", 512, 4096, 0, OK, b"", b"", 0),
    (GET, b"abc", 512, 4096, SET, OTHER, b"", b"", 0),
    (SET, b"10 key v", 512, 4096, GET, OTHER, b"", b"", 0),
    (22, b"abc", 512, 4096, GET, BADOP, b"", b"", 0),
    (GET, b"abc", 512, 4096, GET, OK, b"abc", b"", 0),
]
CRAFTED_REQS = [request(c[0], c[1]) for c in CRAFTED] + [b"", b"\x03"]   # and 0 and 1 bytes: BADOP

FUZZ_SEED, FUZZ_N = 20261021, 20000
FUZZ_OPS = list(range(23)) + [200, 255]
FUZZ_ALPHABET = b"  09-ab"
FUZZ_KEYS, FUZZ_VALUES = (1, 4, 8, 512), (1, 3, 4096)


def fuzz_batch():
    rnd = random.Random(FUZZ_SEED)
    reqs, limits = [], []
    for _ in range(FUZZ_N):
        payload = bytes(rnd.choice(FUZZ_ALPHABET) for _ in range(rnd.randint(0, 24)))
        reqs.append(request(rnd.choice(FUZZ_OPS), payload))
        limits.append((rnd.choice(FUZZ_KEYS), rnd.choice(FUZZ_VALUES)))
    return reqs, limits


_FUZZ = []


def fuzz():
    if not _FUZZ:
        _FUZZ.append(fuzz_batch())
    return _FUZZ[0]


# ---- CPU ---------------------------------------------------------------------

def test_library_exports_the_ingest_calls():
    L = gibson_amd.lib()
    for n in NEW_NAMES:
        assert hasattr(L, n), n
        assert n in gibson_amd.lzf.EXPORTS
    for n in ("request_parse", "host_request_parse", "request_reply_code", "store_append_keys",
              "store_append_keys_work", "ParsedRequests"):
        assert callable(getattr(gibson_amd, n)), n
    assert [gibson_amd.REQ_OK, gibson_amd.REQ_ERR, gibson_amd.REQ_NAN, gibson_amd.REQ_BADOP, gibson_amd.REQ_SHORT,
            gibson_amd.REQ_ERANGE, gibson_amd.REQ_OTHER, gibson_amd.REQ_NSTATUS] == list(range(8))
    assert (gibson_amd.OP_SET, gibson_amd.OP_GET, gibson_amd.OP_MGET, gibson_amd.OP_KEYS, gibson_amd.OP_END) == \
        (1, 3, 11, 21, 0xFF)


def test_ingest_calls_reject_bad_arguments_without_device():
    # argument validation happens before any HIP call, so this runs on CPU;
    # only calls that must be refused are made (the pointers are host memory)
    L = gibson_amd.lib()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(4096)
    p = lambda k: ctypes.c_void_p(ctypes.addressof(buf) + 64 * k)

    def parse(fn, drop=None, n=1, max_key=8, max_value=8, tail=()):
        ptrs = {k: p(i) for i, k in enumerate(("req", "off", "len", "op", "status", "koff", "klen", "voff", "vlen",
                                               "num", "result"))}
        if drop:
            ptrs[drop] = null
        return fn(ptrs["req"], 64, ptrs["off"], ptrs["len"], n, max_key, max_value, 0, ptrs["op"], ptrs["status"],
                  ptrs["koff"], ptrs["klen"], ptrs["voff"], ptrs["vlen"], ptrs["num"], ptrs["result"], *tail)

    for fn, tail in ((L.lzf_gpu_request_parse, (null,)), (L.lzf_host_request_parse, ())):
        for d in ("req", "off", "len", "op", "status", "koff", "klen", "voff", "vlen", "num", "result"):
            assert parse(fn, drop=d, tail=tail) == -1, d
        assert parse(fn, n=0, tail=tail) == -1
        assert parse(fn, max_key=0, tail=tail) == -1
        assert parse(fn, max_value=0, tail=tail) == -1

    names = ("req", "op", "status", "rkoff", "rklen", "rvlen", "num", "keys", "used", "koff", "klen", "time", "ttl",
             "lock", "access", "set_len", "void", "result", "work")

    def append(drop=(), n=1, first=0, count=1, keys_cap=64):
        a = {k: (null if k in drop else p(i)) for i, k in enumerate(names)}
        return L.lzf_gpu_store_append_keys(a["req"], 64, a["op"], a["status"], a["rkoff"], a["rklen"], a["rvlen"],
                                           a["num"], n, a["keys"], keys_cap, a["used"], a["koff"], a["klen"],
                                           a["time"], a["ttl"], a["lock"], a["access"], first, count, 0, 100,
                                           a["set_len"], a["void"], a["result"], a["work"], null)

    for d in names:
        if d not in ("time", "ttl", "lock", "access"):
            assert append(drop=(d,)) == -1, d
    assert append(drop=("time",)) == -1 and append(drop=("ttl",)) == -1       # both or neither
    assert append(n=0) == -1 and append(count=0) == -1 and append(keys_cap=0) == -1
    assert append(n=2, first=0, count=1) == -1 and append(n=1, first=1, count=1) == -1
    assert append(n=2**32 - 1, first=2**32 - 1, count=2**32 - 1) == -1        # first + n in 64 bits


def test_request_reply_code():
    f = gibson_amd.request_reply_code
    assert f(OK) == -1 and f(BADOP) == -2 and f(NAN) == gibson_amd.REPL_ERR_NAN
    for s in (ERR, SHORT, ERANGE, OTHER, 7, 200, -1):
        assert f(s) == gibson_amd.REPL_ERR, s


def test_append_keys_work_size():
    ws = gibson_amd.lib().lzf_gpu_store_append_keys_work_size
    prev = 0
    for n in (1, 2, 1023, 1024, 1025, 3079, 300000, 1 << 20, (1 << 31) + 5, 2**32 - 1):
        w = ws(n)
        assert w >= prev and w >= 16 * ((n + 1023) // 1024) + 64, n
        prev = w
    assert 16 * (2**32 // 1024) <= ws(2**32 - 1) < 2**32                       # 64-bit arithmetic: no wrap
    # 16 bytes of slack, 8 state words, two u64 per scan tile
    assert {n: int(ws(n)) for n in (1, 1024, 1025, 4097)} == {1: 96, 1024: 96, 1025: 112, 4097: 160}


def host_parse(reqs, maxkey, maxvalue, expect_op=0, req_bytes=None, off=None):
    arena, o, ln = pack(reqs)
    if off is not None:
        o = np.array(off, np.uint64)
    if req_bytes is not None:
        arena = arena[:req_bytes]
    out, result = gibson_amd.host_request_parse(arena, o, ln, maxkey, maxvalue, expect_op)
    return {f: getattr(out, f) for f in FIELDS}, result.tolist(), (arena, o, ln)


def same(got, want):
    for f in FIELDS:
        assert got[f].dtype == DTYPE[f] and (got[f] == want[f]).all(), (f, np.nonzero(got[f] != want[f])[0][:8])


def test_crafted_requests_on_the_host():
    for op, payload, mk, mv, exp, status, key, val, num in CRAFTED:
        r = request(op, payload)
        t = model_one(r, mk, mv, exp)
        # what the table claims is what the model yields
        assert t[1] == status and r[t[2]:t[2] + t[3]] == key and r[t[4]:t[4] + t[5]] == val and t[6] == num, (op, payload, t)
        assert t[0] == (0 if status == BADOP else op & 0xFF)
        if status not in (OK, NAN):
            assert t[2:] == (0, 0, 0, 0, 0)
        # a neighbour on either side, so that the offsets are not 0
        got, result, (arena, off, ln) = host_parse([b"\x03\x00left", r, b"\x03\x00right"], mk, mv, exp)
        want, counts = model_batch(arena, off, ln, len(arena), mk, mv, exp)
        same(got, want)
        assert result == counts and got["status"][1] == status
    got, result, _ = host_parse([b"", b"\x03", b"\x03\x00k"], 512, 4096)
    assert got["status"].tolist() == [BADOP, BADOP, OK] and got["op"].tolist() == [0, 0, 3] and result[BADOP] == 2
    # a request past req_bytes, one that ends exactly at it, and an offset that wraps
    reqs = [request(GET, b"abc"), request(GET, b"defg")]
    got, result, _ = host_parse(reqs, 512, 4096, req_bytes=10)
    assert got["status"].tolist() == [OK, ERANGE] and got["key_len"].tolist() == [3, 0] and result[ERANGE] == 1
    got, result, _ = host_parse(reqs, 512, 4096, req_bytes=11)
    assert got["status"].tolist() == [OK, OK] and got["key_off"].tolist() == [2, 7]
    got, result, _ = host_parse(reqs, 512, 4096, off=[2**64 - 2, 12])
    assert got["status"].tolist() == [ERANGE, ERANGE] and got["op"].tolist() == [0, 0]


def row_of(op):
    for name, row in (("key", ROW_KEY), ("keyval", ROW_KEYVAL), ("keynum", ROW_KEYNUM), ("opt", ROW_OPT),
                      ("set", ROW_SET), ("empty", ROW_EMPTY)):
        if op in row:
            return name
    return "bad"


def test_host_parse_equals_the_model_on_the_fuzz():
    reqs, limits = fuzz()
    pairs = {}
    for r, (mk, mv) in zip(reqs, limits):
        pair = (row_of(struct.unpack("<h", r[:2])[0]), model_one(r, mk, mv)[1])
        pairs[pair] = pairs.get(pair, 0) + 1
    print("fuzz pairs", sorted(pairs.items()))
    # from the model alone: every (grammar row, status) pair that can occur is there
    need = [("set", s) for s in (OK, ERR, NAN, SHORT)] + [("keynum", s) for s in (OK, ERR, NAN, SHORT)] + \
        [("keyval", s) for s in (OK, ERR, SHORT)] + [("opt", s) for s in (OK, ERR, NAN)] + \
        [("key", s) for s in (OK, ERR)] + [("empty", OK), ("bad", BADOP)]
    for p in need:
        assert pairs.get(p, 0) >= 10, (p, pairs.get(p, 0))
    assert set(pairs) == set(need)                              # and no pair that cannot occur
    for mk in FUZZ_KEYS:
        for mv in FUZZ_VALUES:
            sub = [r for r, lim in zip(reqs, limits) if lim == (mk, mv)]
            assert len(sub) > 1000
            got, result, (arena, off, ln) = host_parse(sub, mk, mv)
            want, counts = model_batch(arena, off, ln, len(arena), mk, mv)
            same(got, want)
            assert result == counts
    # the operator buckets: every opcode as expect_op over one slice
    sub = reqs[:1500]
    for exp in (SET, GET, MGET, TTL, END):
        got, result, (arena, off, ln) = host_parse(sub, 8, 4096, exp)
        want, counts = model_batch(arena, off, ln, len(arena), 8, 4096, exp)
        same(got, want)
        assert result == counts and counts[OTHER] > 500


def test_request_check_under_the_host_sanitizers():
    csrc = os.path.join(ROOT, "gibson_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "build/request_check"])
    out = subprocess.run([os.path.join(csrc, "build", "request_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "request_check: ok" in out.stdout


# ---- GPU ---------------------------------------------------------------------

FILL = 0xA5
GUARD = 0x5A
BAND = 64                                # guard bytes in front of and behind every output


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    gibson_amd.lib()
    return t


def dev(torch, a):
    """a numpy array on the device, unsigned types as the signed tensor of their width"""
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


class Guarded:
    """cap elements of dtype on the device, filled with FILL, at byte `mis` past
    a band of GUARD bytes and followed by another"""

    def __init__(self, torch, cap, dtype, mis=0):
        size = np.dtype(dtype).itemsize
        self.lo, self.n = BAND + mis, cap * size
        self.buf = torch.full((self.lo + self.n + BAND,), GUARD, dtype=torch.uint8, device="cuda")
        self.buf[self.lo:self.lo + self.n] = FILL
        self.dtype = dtype
        tdt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[size]
        body = self.buf[self.lo:self.lo + self.n]
        self.t = body if size == 1 else body.view(tdt)

    def read(self):
        """the body as numpy, after checking both bands"""
        raw = self.buf.cpu().numpy()
        assert (raw[:self.lo] == GUARD).all() and (raw[self.lo + self.n:] == GUARD).all()
        return raw[self.lo:self.lo + self.n].view(self.dtype)


def filled(dtype, n):
    """what n untouched elements of a Guarded read as"""
    return np.full(n * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)


def spaced(reqs, gaps, filler):
    """the requests with gaps[k] filler bytes in front of request k (and 3
    behind the last) -> arena, off, len"""
    parts, off, at = [], [], 0
    for r, g in zip(reqs, gaps):
        parts.append(bytes(filler[(at + j) % len(filler)] for j in range(g)))
        at += g
        off.append(at)
        parts.append(r)
        at += len(r)
    parts.append(bytes(filler[(at + j) % len(filler)] for j in range(3)))
    return (np.frombuffer(b"".join(parts), np.uint8), np.array(off, np.uint64),
            np.array([len(r) for r in reqs], np.uint32))


PARSE_NS = (1, 63, 64, 65, 1023, 1024, 1025, 4097)
ERANGE_AT = (40, 50)


@pytest.fixture(scope="module")
def parse_batch():
    """the crafted requests among the first 4097 - len(crafted) of the fuzz,
    shuffled, and one model cache for every layout of it"""
    reqs = CRAFTED_REQS + fuzz()[0][:max(PARSE_NS) - len(CRAFTED_REQS) - 2]
    random.Random(7).shuffle(reqs)
    for at in ERANGE_AT:                                  # two places for requests past req_bytes
        reqs.insert(at, request(GET, b"moved"))
    assert len(reqs) == max(PARSE_NS)
    return reqs, {}


@pytest.mark.gpu
@pytest.mark.parametrize("limits", [(512, 4096, 0), (4, 3, 0), (8, 1, 0), (1, 4096, 0), (512, 4096, SET)])
def test_parse_equals_the_model(torch, parse_batch, limits):
    reqs, cache = parse_batch
    mk, mv, exp = limits
    rs = np.random.RandomState(11)
    total = [0] * 7
    for spacing in ("packed", "spaced"):
        gaps = np.zeros(len(reqs), int) if spacing == "packed" else rs.randint(1, 8, len(reqs))
        per_filler = []
        for filler in (b" 0 9 1 ", b"\xaa"):
            arena, off, ln = spaced(reqs, gaps, filler)
            # two requests past req_bytes: one that ends a byte late, one whose offset wraps
            off, ln = off.copy(), ln.copy()
            late, wrap = ERANGE_AT
            off[late], ln[late] = len(arena) - 3, 4
            off[wrap], ln[wrap] = 2**64 - 2, 8
            runs = []
            for mis in (0, 1):
                whole = torch.full((len(arena) + 1,), 0x20, dtype=torch.uint8, device="cuda")
                d_req = whole[mis:mis + len(arena)]
                d_req.copy_(dev(torch, arena))
                d_off, d_len = dev(torch, off), dev(torch, ln)
                for n in PARSE_NS:
                    out = {f: Guarded(torch, n, DTYPE[f]) for f in FIELDS}
                    result = torch.full((8,), -7, dtype=torch.int64, device="cuda")
                    gibson_amd.request_parse(d_req, d_off[:n], d_len[:n], mk, mv,
                                             gibson_amd.ParsedRequests(*(out[f].t for f in FIELDS)), result[:7], exp)
                    runs.append((n, out, result))
            torch.cuda.synchronize()
            want, _ = model_batch(arena, off, ln, len(arena), mk, mv, exp, cache)
            assert want["status"][late] == ERANGE and want["status"][wrap] == ERANGE
            for n, out, result in runs:
                got = {f: out[f].read() for f in FIELDS}
                same(got, {f: want[f][:n] for f in FIELDS})
                counts = np.bincount(want["status"][:n], minlength=7).tolist()
                assert result.cpu().numpy().tolist() == counts + [-7], n
            per_filler.append(want)
            total = [a + b for a, b in zip(total, np.bincount(want["status"], minlength=7).tolist())]
        # the bytes between the requests do not reach the outputs
        for f in FIELDS:
            assert (per_filler[0][f] == per_filler[1][f]).all(), f
    print("parse", limits, "statuses", total)
    assert total[ERANGE] == 8 and all(total[s] for s in ((OK, OTHER, BADOP) if exp else (OK, ERR, NAN, BADOP, SHORT)))


# ---- the key append ----------------------------------------------------------------

NOW, MAX_TTL = 1_700_000_000, 100
REASONS = ("op", "err", "nan", "short", "other", "past", "late", "wrap")


def make_parsed(seed, key_len, refuse, gap=(3, 70)):
    """a request arena with one key span per request, `gap` bytes apart, and
    the parse outputs that name them; refuse[k]: None, or one of REASONS"""
    rs = np.random.RandomState(seed)
    n = len(key_len)
    key_len = np.array(key_len, np.int64)
    step = rs.randint(gap[0], gap[1], n) + key_len
    off = 5 + np.cumsum(step) - key_len
    arena = rs.randint(0, 256, int(off[-1] + key_len[-1] + 9)).astype(np.uint8)
    p = {"op": np.full(n, SET, np.uint8), "status": np.zeros(n, np.uint8), "key_off": off.astype(np.uint64),
         "key_len": key_len.astype(np.uint32), "val_off": np.zeros(n, np.uint64),
         "val_len": rs.randint(1, 5000, n).astype(np.uint32),
         "num": rs.choice(np.array([-1, 0, 1, 5, 99, 100, 101, 10**12, -10**12, 2**62], np.int64), n)}
    for k, why in enumerate(refuse):
        if why == "op":
            p["op"][k] = rs.choice([0, GET, MSET, 0xFF])
        elif why in ("err", "nan", "short", "other"):
            p["status"][k] = {"err": ERR, "nan": NAN, "short": SHORT, "other": OTHER}[why]
        elif why == "past":
            p["key_off"][k] = len(arena) + 1
        elif why == "late":
            p["key_off"][k] = len(arena) - int(key_len[k]) + 1
        elif why == "wrap":
            p["key_off"][k] = 2**64 - 4
    return arena, p


def append_model(arena, p, first, base, keys_cap):
    """-> result, the new items' members, set_len, void_idx, the appended bytes"""
    n = len(p["op"])
    ok = (p["op"] == SET) & (p["status"] == OK)
    for k in np.nonzero(ok)[0]:
        o, ln = int(p["key_off"][k]), int(p["key_len"][k])
        ok[k] = o <= len(arena) and ln <= len(arena) - o
    klen = np.where(ok, p["key_len"], 0).astype(np.int64)
    total = int(klen.sum())
    full = base + total > M64 or base + total > keys_cap
    if full:
        ok[:], klen[:], total = False, 0, 0
    before = (np.cumsum(klen) - klen).astype(np.uint64)
    m = {"key_off": np.full(n, base, np.uint64) + before, "key_len": klen.astype(np.uint32),
         "item_time": np.full(n, NOW, np.int64), "last_access": np.full(n, NOW, np.int64),
         "item_lock": np.zeros(n, np.int64),
         "item_ttl": np.where(ok & (p["num"] > 0), np.minimum(p["num"], MAX_TTL), -1).astype(np.int32)}
    set_len = np.where(ok, p["val_len"], 0).astype(np.uint32)
    void = np.where(ok, PAD, first + np.arange(n)).astype(np.uint32)
    pos = np.concatenate([np.arange(int(p["key_off"][k]), int(p["key_off"][k]) + int(klen[k])) for k in range(n)
                          if klen[k]] or [np.zeros(0, np.int64)]).astype(np.int64)
    result = [int(ok.sum()), n - int(ok.sum()), total, STORE_FULL if full else STORE_OK]
    return result, m, set_len, void, arena[pos]


ITEM = (("key_off", np.uint64), ("key_len", np.uint32), ("item_time", np.int64), ("item_ttl", np.int32),
        ("item_lock", np.int64), ("last_access", np.int64))


class Append:
    """one lzf_gpu_store_append_keys call on the device; no synchronisation"""

    def __init__(self, torch, arena, p, base=0, first=3, tail=2, keys_cap=None, mis=0,
                 members=("item_time", "item_ttl", "item_lock", "last_access")):
        self.torch, self.arena, self.p, self.base, self.first = torch, arena, p, base, first
        n = self.n = len(p["op"])
        self.count = first + n + tail
        need = int(np.where((p["op"] == SET) & (p["status"] == OK), p["key_len"], 0).sum())
        self.keys_cap = (base % 2**32) + need + 21 if keys_cap is None else keys_cap
        self.members = ("key_off", "key_len") + tuple(members)
        self.d_req = dev(torch, arena)
        self.parsed = gibson_amd.ParsedRequests(*(dev(torch, p[f]) for f in FIELDS))
        self.keys = Guarded(torch, self.keys_cap, np.uint8, mis)
        self.used = dev(torch, np.array([base, 0x1111], np.uint64))
        self.items = {f: Guarded(torch, self.count, dt) for f, dt in ITEM if f in self.members}
        self.set_len, self.void = Guarded(torch, n, np.uint32), Guarded(torch, n, np.uint32)
        self.result = torch.full((5,), -7, dtype=torch.int64, device="cuda")
        opt = {f: self.items[f].t for f in members}
        self.work = gibson_amd.store_append_keys(self.d_req, self.parsed, self.keys.t, self.used[:1],
                                                 self.items["key_off"].t, self.items["key_len"].t, first, NOW, MAX_TTL,
                                                 self.set_len.t, self.void.t, self.result[:4], **opt)

    def check(self, expect=None):
        self.torch.cuda.synchronize()
        n, first, base = self.n, self.first, self.base
        result, m, set_len, void, packed = append_model(self.arena, self.p, first, base, self.keys_cap)
        got = self.result.cpu().numpy().tolist()
        print("append n", n, "base", base, "cap", self.keys_cap, "result", got[:4], "expected", result)
        if expect is not None:
            assert result[3] == expect                      # the model holds the case the test claims
        assert got == result + [-7]
        used = self.used.cpu().numpy().view(np.uint64).tolist()
        assert used == [(base + result[2]) if result[3] == STORE_OK else base, 0x1111]
        for f, dt in ITEM:
            if f not in self.members:
                continue
            want = filled(dt, self.count)                   # entries outside [first, first + n) keep their fill
            want[first:first + n] = m[f]
            assert (self.items[f].read() == want).all(), f
        assert (self.set_len.read() == set_len).all() and (self.void.read() == void).all()
        keys = self.keys.read()
        lo = base if result[3] == STORE_OK and base <= self.keys_cap else 0
        if result[3] == STORE_OK:
            assert (keys[:lo] == FILL).all() and (keys[lo + result[2]:] == FILL).all()
            assert (keys[lo:lo + result[2]] == packed).all()
        else:
            assert (keys == FILL).all()                     # a refusal is whole
        assert (self.d_req.cpu().numpy() == self.arena).all()
        return result


def third_refused(rs, n, reasons=REASONS):
    return [reasons[rs.randint(len(reasons))] if rs.rand() < 1 / 3 else None for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 3079])
def test_append_against_the_model(torch, n):
    rs = np.random.RandomState(0xA99 + n)
    runs = []
    for base in (0, 1, 15, 16, 17):
        arena, p = make_parsed(100 * n + base, rs.randint(16, 41, n), third_refused(rs, n))
        runs.append(Append(torch, arena, p, base=base, mis=(base * 5 + n) % 16))
    arena, p = make_parsed(n, rs.randint(16, 41, n), [None] * n)                       # none refused
    runs.append(Append(torch, arena, p, base=7, first=0, tail=0))
    for r in runs:
        assert r.check(STORE_OK)[3] == STORE_OK


@pytest.mark.gpu
def test_append_key_shapes(torch):
    rs = np.random.RandomState(0x5A9E)
    runs = []
    ones = make_parsed(1, np.ones(1500, int), third_refused(rs, 1500), gap=(1, 4))
    runs += [Append(torch, *ones, base=b, mis=b) for b in (0, 15)]
    lens = np.concatenate([np.array([255, 256, 257, 511, 512, 1, 3, 4, 15, 16, 17, 4096, 70001] * 2),
                           rs.randint(16, 41, 1100)])
    rs.shuffle(lens)
    refuse = third_refused(rs, len(lens))
    for k in np.nonzero(lens >= 255)[0][::2]:
        refuse[k] = None                                                                # both sides of the wave path live
    mixed = make_parsed(2, lens, refuse)
    acc = np.array([r is None for r in refuse])
    assert set(lens[acc]) >= {255, 256, 257, 511, 512} and len(lens) > 1024
    runs += [Append(torch, *mixed, base=b, mis=m) for b, m in ((0, 0), (9, 1), (17, 7), (16, 15))]
    forty = make_parsed(3, np.full(1024, 40), [None] * 1024)                            # one tile past one window
    assert 1024 * 40 > 32768
    runs += [Append(torch, *forty, base=b) for b in (0, 5)]
    hole = [None if k < 1024 or k >= 2048 else REASONS[k % len(REASONS)] for k in range(3072)]
    hole[5] = hole[2500] = "err"
    runs.append(Append(torch, *make_parsed(4, rs.randint(16, 41, 3072), hole), base=3))  # an empty tile between two
    runs.append(Append(torch, *make_parsed(5, rs.randint(16, 41, 1500), third_refused(rs, 1500, REASONS[:1] * 3 + REASONS)),
                       base=1))
    for r in runs:
        r.check(STORE_OK)


@pytest.mark.gpu
def test_append_refusal_reasons_and_optional_members(torch):
    rs = np.random.RandomState(0x4EF)
    runs = []
    for why in REASONS:                                                                 # a third refused, per reason
        arena, p = make_parsed(len(runs), rs.randint(16, 41, 1300), third_refused(rs, 1300, (why,)))
        runs.append(Append(torch, arena, p, base=len(runs)))
    everything = make_parsed(77, rs.randint(16, 41, 1300), [REASONS[k % len(REASONS)] for k in range(1300)])
    runs.append(Append(torch, *everything, base=11))                                    # every request refused
    some = make_parsed(78, rs.randint(16, 41, 1300), third_refused(rs, 1300))
    runs += [Append(torch, *some, members=("item_lock", "last_access")),                # no time / ttl
             Append(torch, *some, members=("item_time", "item_ttl")),                   # no lock, no last_access
             Append(torch, *some, members=())]
    results = [r.check(STORE_OK) for r in runs]
    assert results[len(REASONS)][:3] == [0, 1300, 0]
    assert all(r[1] > 300 for r in results[:len(REASONS)])


@pytest.mark.gpu
def test_append_whole_call_refusal(torch):
    rs = np.random.RandomState(0xF011)
    arena, p = make_parsed(9, rs.randint(16, 41, 1500), third_refused(rs, 1500))
    need = append_model(arena, p, 3, 0, 1 << 40)[0][2]
    cases = [(Append(torch, arena, p, base=9, keys_cap=9 + need - 1), STORE_FULL),       # one byte short
             (Append(torch, arena, p, base=9, keys_cap=9 + need), STORE_OK),             # exactly the need
             (Append(torch, arena, p, base=2**64 - 3, keys_cap=need + 64), STORE_FULL),  # the end wraps
             (Append(torch, arena, p, base=0, keys_cap=1), STORE_FULL)]
    for r, want in cases:
        res = r.check(want)
        if want == STORE_FULL:
            assert res == [0, 1500, 0, STORE_FULL]


# ---- end to end ----------------------------------------------------------------------

def code_frame(code):
    """gbClientEnqueueCode: [i16 code][u8 PLAIN][u32 1][0x00]"""
    return struct.pack("<hBI", code, ENC_PLAIN, 1) + b"\0"


def value_frame(value):
    return struct.pack("<hBI", gibson_amd.REPL_VAL, ENC_PLAIN, len(value)) + value


class Server:
    """the reference's handlers over a dict, one request at a time"""

    def __init__(self, maxkey, maxvalue, max_ttl):
        self.items, self.maxkey, self.maxvalue, self.max_ttl = {}, maxkey, maxvalue, max_ttl

    def request(self, r, now, expect_op):
        """-> the reply frame; None: the connection is closed"""
        op, status, kat, klen, vat, vlen, num = model_one(r, self.maxkey, self.maxvalue, expect_op)
        if status != OK:
            code = {BADOP: None, NAN: gibson_amd.REPL_ERR_NAN}.get(status, gibson_amd.REPL_ERR)
            return None if code is None else code_frame(code)
        key = r[kat:kat + klen]
        if op == SET:
            value = r[vat:vat + vlen]
            self.items[key] = {"value": value, "time": now, "ttl": min(self.max_ttl, num) if num > 0 else -1}
            return value_frame(value)
        assert op == GET
        it = self.items.get(key)
        if it is not None and it["ttl"] > 0 and now - it["time"] >= it["ttl"]:
            del self.items[key]
            it = None
        return code_frame(gibson_amd.REPL_ERR_NOT_FOUND) if it is None else value_frame(it["value"])


class DeviceStore:
    def __init__(self, torch, cap, val_room, key_room, slots):
        self.torch, self.cap, self.n = torch, cap, 0
        z = lambda dt: torch.zeros(cap, dtype=dt, device="cuda")
        self.arena = torch.zeros(val_room, dtype=torch.uint8, device="cuda")
        self.used = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.keys = torch.zeros(key_room, dtype=torch.uint8, device="cuda")
        self.keys_used = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.val_off, self.val_size, self.val_len = z(torch.int64), z(torch.int32), z(torch.int32)
        self.key_off, self.key_len = z(torch.int64), z(torch.int32)
        self.item_time, self.item_ttl = z(torch.int64), z(torch.int32)
        self.item_lock, self.last_access = z(torch.int64), z(torch.int64)
        self.enc = torch.full((cap,), ENC_NULL, dtype=torch.uint8, device="cuda")
        self.table = torch.full((gibson_amd.key_index_bytes(slots),), 0xFF, dtype=torch.uint8, device="cuda")
        self.kused = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.keep = []                                   # work areas, until the stream is idle

    def frames(self, idx, now, room, statuses):
        """store_replies (GET) over idx, refused requests overridden on the host
        from their status -> one frame (or None) per entry"""
        torch, n = self.torch, idx.numel()
        rep = torch.zeros(room, dtype=torch.uint8, device="cuda")
        used = torch.zeros(1, dtype=torch.int64, device="cuda")
        off, ln = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        est = torch.zeros(n, dtype=torch.uint8, device="cuda")
        res = torch.zeros(6, dtype=torch.int64, device="cuda")
        self.keep.append(gibson_amd.store_replies(idx, gibson_amd.REPLY_GET, self.arena, self.val_off, self.val_size,
                                                  self.enc, self.val_len, self.item_time, self.item_ttl, now, 256,
                                                  rep, used, off, ln, est, res, last_access=self.last_access))

        def read():
            assert int(res[3].item()) == gibson_amd.REPLY_OK and int(res[5].item()) == 0
            raw, o, l = rep.cpu().numpy(), off.cpu().numpy(), ln.cpu().numpy()
            out = []
            for k, st in enumerate(statuses().tolist()):
                code = gibson_amd.request_reply_code(st)
                out.append(bytes(raw[o[k]:o[k] + l[k]]) if code == -1 else None if code == -2 else code_frame(code))
            return out
        return read

    def set_batch(self, reqs, now, max_ttl):
        """the eight steps of one SET batch, no host wait -> a reader of its replies"""
        torch, first, n = self.torch, self.n, len(reqs)
        arena, off, ln = pack(reqs)
        d_req, d_off, d_len = dev(torch, arena), dev(torch, off), dev(torch, ln)
        parsed = gibson_amd.ParsedRequests.empty(n, "cuda")
        pres, ares = torch.zeros(7, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")
        set_len, void = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        gibson_amd.request_parse(d_req, d_off, d_len, 512, 4096, parsed, pres, expect_op=SET)               # 1
        self.keep.append(gibson_amd.store_append_keys(d_req, parsed, self.keys, self.keys_used, self.key_off,  # 2
                                                      self.key_len, first, now, max_ttl, set_len, void, ares,
                                                      item_time=self.item_time, item_ttl=self.item_ttl,
                                                      item_lock=self.item_lock, last_access=self.last_access))
        status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        sl = slice(first, first + n)
        self.keep.append(gibson_amd.set_store(d_req, parsed.val_off, set_len, 64, 256, len(arena), self.arena,  # 3
                                              self.used, self.val_off[sl], self.val_size[sl], self.enc[sl], status))
        self.val_len[sl] = set_len
        gibson_amd.store_delete(void, self.enc)                                                             # 4
        occ = torch.zeros(n, dtype=torch.int32, device="cuda")
        lres = torch.zeros(3, dtype=torch.int64, device="cuda")
        gibson_amd.key_index_lookup(self.table, self.keys, self.key_off, self.key_len, self.enc, self.keys,    # 5
                                    self.key_off[sl], self.key_len[sl], occ, lres)
        gres, refused = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
        gibson_amd.store_set_guard(occ, first, self.enc, self.item_time, self.item_lock, now, gres, refused)  # 6
        idx = torch.arange(first, first + n, dtype=torch.int32, device="cuda")
        read = self.frames(idx, now, 2 * len(arena) + 16 * n, lambda: parsed.status.cpu().numpy())         # 7
        kres, kst = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
        gibson_amd.key_index_insert(self.table, self.kused, self.keys, self.key_off, self.key_len, self.enc,  # 8
                                    first, n, kres, kst)
        self.keep.append((d_req, d_off, d_len, parsed, set_len, void, occ))
        self.n += n

        def done():
            assert int(status.item()) == STORE_OK and int(kst.item()) == 0 and int(ares[3].item()) == STORE_OK
            assert int(gres.item()) == 0 and not bool(refused.any())
            return read(), pres.cpu().numpy().tolist(), ares.cpu().numpy().tolist()
        return done

    def get_batch(self, reqs, now):
        torch, n = self.torch, len(reqs)
        arena, off, ln = pack(reqs)
        d_req = dev(torch, arena)
        parsed = gibson_amd.ParsedRequests.empty(n, "cuda")
        pres = torch.zeros(7, dtype=torch.int64, device="cuda")
        gibson_amd.request_parse(d_req, dev(torch, off), dev(torch, ln), 512, 4096, parsed, pres, expect_op=GET)
        idx = torch.zeros(n, dtype=torch.int32, device="cuda")
        lres = torch.zeros(3, dtype=torch.int64, device="cuda")
        gibson_amd.key_index_lookup(self.table, self.keys, self.key_off, self.key_len, self.enc, d_req,
                                    parsed.key_off, parsed.key_len, idx, lres)
        read = self.frames(idx, now, 512 * n, lambda: parsed.status.cpu().numpy())
        self.keep.append((d_req, parsed, idx))
        return read


@pytest.mark.gpu
def test_set_and_get_from_raw_requests_against_a_server_model(torch):
    rnd = random.Random(0x16E57)
    names = [b"user:%04d:" % i + bytes(rnd.choice(b"abcdef") for _ in range(rnd.randint(0, 24))) for i in range(600)]
    assert len(set(names)) == 600 and max(map(len, names)) <= 40

    def value():
        size = rnd.randint(1, 256)
        if rnd.random() < 0.5:
            return (b"the quick brown fox " * 13)[rnd.randint(0, 7):][:size]
        return bytes(rnd.randrange(256) for _ in range(size))

    def bad_set():
        k = rnd.choice(names)
        return rnd.choice([request(SET, b"10 " + k), request(SET, b"10 " + k + b" "), request(SET, b"1x " + k + b" v"),
                           request(GET, k), request(0, k), request(SET, b""), request(SET, b" " + k + b" v")])

    sets = []
    for _ in range(2000):
        if rnd.random() < 0.05:
            sets.append(bad_set())
        else:
            sets.append(request(SET, b"%d " % rnd.choice([-1, 0, 5, 10**12]) + rnd.choice(names) + b" " + value()))
    gets = []
    for _ in range(500):
        x = rnd.random()
        gets.append(request(GET, rnd.choice(names)) if x < 0.7 else request(GET, b"absent:%d" % rnd.randrange(99))
                    if x < 0.9 else rnd.choice([request(GET, b""), request(SET, b"1 k v"), request(22, b"k"), b"\x03"]))

    now = 1_000_000
    server = Server(512, 4096, 100)
    want_sets = [server.request(r, now, SET) for r in sets]
    want_gets = [[server.request(r, t, GET) for r in gets] for t in (now, now + 50, now + 200)]
    # what the batch claims to hold, from the model alone
    codes = [None if f is None else struct.unpack("<h", f[:2])[0] for f in want_sets]
    assert codes.count(gibson_amd.REPL_VAL) > 1800 and codes.count(gibson_amd.REPL_ERR) >= 20
    assert codes.count(gibson_amd.REPL_ERR_NAN) >= 5 and codes.count(None) >= 5
    for g in want_gets:
        assert sum(f is None for f in g) >= 5
    found = [sum(f is not None and f[:2] == b"\x06\x00" for f in g) for g in want_gets]
    assert found[0] > found[1] > found[2] > 50

    store = DeviceStore(torch, 2200, 1 << 20, 1 << 17, 8192)
    done = [store.set_batch(sets[a:a + 500], now, 100) for a in range(0, 2000, 500)]
    reads = [store.get_batch(gets, t) for t in (now, now + 50, now + 200)]
    torch.cuda.synchronize()
    got_sets, accepted = [], 0
    for d in done:
        frames, pres, ares = d()
        got_sets += frames
        accepted += ares[0]
        assert pres[OK] == ares[0] and sum(pres) == 500 == ares[0] + ares[1]
    assert accepted == codes.count(gibson_amd.REPL_VAL)
    assert got_sets == want_sets
    for r, want in zip(reads, want_gets):
        assert r() == want
    enc = store.enc.cpu().numpy()
    assert (enc == ENC_LZF).sum() > 50 and (enc == ENC_PLAIN).sum() > 50          # both encodings were stored
    assert int(store.keys_used.item()) == sum(len(model_key(r)) for r, f in zip(sets, want_sets)
                                              if f is not None and f[:2] == b"\x06\x00")


def model_key(r):
    t = model_one(r, 512, 4096, SET)
    return r[t[2]:t[2] + t[3]]
