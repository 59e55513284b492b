"""The memory sweep, META and the KEYS frame over the device store:
lzf_gpu_store_gc, lzf_gpu_store_meta, lzf_host_meta_field and
lzf_gpu_store_keys against Python models that transcribe gbMemoryFreeHandler
(src/server.c:311-327, the cron's gate :401-411), gbGetItemMeta and
gbQueryMetaHandler (src/query.c:1255-1339) and gbQueryKeysHandler (:1341-1391)
over the KVAL frame of src/net.c:1256-1342.  The KEYS frame is also held
against lzf_gpu_kv_frame over pair arrays built on the host.  The bar is exact
equality of every array, result word, per-entry output and frame byte.

Every buffer a test hands over with a size is allocated larger and the excess
filled with a guard value, which is checked afterwards."""
import ctypes
import random
import struct

import numpy as np
import pytest

try:                                    # before liblzf_hip.so loads: one HIP runtime in the process
    import torch as _torch  # noqa: F401
except ImportError:
    _torch = None

import gibson_amd

ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL = 0, 1, 2, 0xFF
DONE, DEAD, EXPIRED = 0, 1, 2
MGET_OK, MGET_NOT_FOUND, MGET_TOO_BIG = 0, 1, 2
PAD = 0xFFFFFFFF
NAMES = (b"size", b"encoding", b"access", b"created", b"ttl", b"left", b"lock")
NEW_NAMES = ("lzf_gpu_store_gc", "lzf_host_meta_field", "lzf_gpu_store_meta", "lzf_gpu_store_keys_work_size",
             "lzf_gpu_store_keys")
I64_MAX, I64_MIN = 2**63 - 1, -2**63


def wrap(x):
    """x modulo 2^64 as a signed 64-bit number"""
    x &= 2**64 - 1
    return x - 2**64 if x >= 2**63 else x


def strncmp(a, b, n):
    """C's strncmp over two NUL-terminated strings: 0 when equal"""
    a, b = a + b"\0", b + b"\0"
    for k in range(n):
        if a[k] != b[k]:
            return a[k] - b[k]
        if a[k] == 0:
            return 0
    return 0


def field_model(m):
    """gbGetItemMeta's chain (src/query.c:1263-1297) -> the field's index, or None"""
    if not m:
        return None
    for f, name in enumerate(NAMES):
        if strncmp(m, name, min(len(m), len(name))) == 0:
            return f
    return None


# ---- CPU ---------------------------------------------------------------------

def test_library_exports_the_gc_meta_and_keys_calls():
    L = gibson_amd.lib()
    for n in NEW_NAMES:
        assert hasattr(L, n), n
        assert n in gibson_amd.lzf.EXPORTS
    for n in ("store_gc", "store_meta", "meta_field", "store_keys", "store_keys_work"):
        assert callable(getattr(gibson_amd, n)), n
    assert (gibson_amd.META_SIZE, gibson_amd.META_ENCODING, gibson_amd.META_ACCESS, gibson_amd.META_CREATED,
            gibson_amd.META_TTL, gibson_amd.META_LEFT, gibson_amd.META_LOCK) == (0, 1, 2, 3, 4, 5, 6)


def test_gc_meta_and_keys_reject_bad_arguments_without_device():
    # argument validation happens before any HIP call, so this runs on CPU;
    # only calls that must be refused are made (the pointers are host memory)
    L = gibson_amd.lib()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(512)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def gc(ptrs, count=1):
        last, enc, vsize, gate, result = ptrs
        return L.lzf_gpu_store_gc(last, 5, 1, enc, vsize, count, gate, 0, result, null)

    for k in (0, 1, 2, 4):                           # the gate may be NULL
        ptrs = [p] * 5
        ptrs[k] = null
        assert gc(ptrs) == -1, k
    assert gc([p] * 5, count=0) == -1

    def meta(ptrs, n=1, field=0, count=1):
        idx, enc, vsize, time, ttl, lock, last, est, ev, result = ptrs
        return L.lzf_gpu_store_meta(idx, n, field, enc, vsize, count, time, ttl, lock, 5, last, est, ev, result, null)

    for k in (0, 1, 2, 3, 4, 8, 9):                  # item_lock, last_access, entry_status may be NULL
        ptrs = [p] * 10
        ptrs[k] = null
        assert meta(ptrs) == -1, k
    assert meta([p] * 10, n=0) == -1
    assert meta([p] * 10, count=0) == -1
    for field in (-1, 7, 100, -2**31):
        assert meta([p] * 10, field=field) == -1, field
    ptrs = [p] * 10
    ptrs[6] = null
    assert meta(ptrs, field=2) == -1                 # ACCESS reads last_access

    def keys(ptrs, n=1, count=1):
        idx, ks, koff, klen, enc, frame, flen, result, work = ptrs
        return L.lzf_gpu_store_keys(idx, n, ks, koff, klen, enc, count, 1, frame, 64, flen, result, work, null)

    for k in range(9):
        ptrs = [p] * 9
        ptrs[k] = null
        assert keys(ptrs) == -1, k
    assert keys([p] * 9, n=0) == -1
    assert keys([p] * 9, count=0) == -1


def test_keys_work_size():
    ws = gibson_amd.lib().lzf_gpu_store_keys_work_size
    prev = 0
    for n in (1, 2, 1023, 1024, 1025, 3000, 262145, 1 << 20, (1 << 31) + 5, 2**32 - 2, 2**32 - 1):
        w = ws(n)
        assert w >= 16 * ((n + 1023) // 1024) and w >= prev, n     # two u64 per tile of 1024 entries
        prev = w
    assert 16 * (2**32 // 1024) <= ws(2**32 - 1) < 2**32


def test_meta_field_matches_the_strncmp_chain():
    cases = [b"l", b"le", b"lo", b"sizeXYZ", b"t", b"x", b"s\0ize", b"si\0", b"\0", b"size\0", b"lock\0x", b"loc\0k",
             b"tt", b"ttlx", b"encodingencoding", b"LOCK", b"Size", b" size", b"\xff", b"e", b"a", b"c"]
    for name in NAMES:
        cases += [name[:k] for k in range(1, len(name) + 1)] + [name + b"!", name + name]
    rnd = random.Random(0x3E7A)
    alphabet = bytes(sorted(set(b"".join(NAMES)))) + b"\0"
    cases += [bytes(rnd.choice(alphabet) for _ in range(rnd.randint(1, 9))) for _ in range(300)]
    hits = 0
    for m in cases:
        exp = field_model(m)
        hits += exp is not None
        assert gibson_amd.meta_field(m) == exp, m
    assert 60 <= hits <= len(cases) - 60                 # both outcomes are well covered
    # by hand, from the chain's order: a prefix goes to the first name it fits
    assert [gibson_amd.meta_field(m) for m in (b"s", b"sizeXYZ", b"l", b"le", b"lo", b"t", b"x")] == \
           [0, 0, 5, 5, 6, 4, None]
    assert [gibson_amd.meta_field(n) for n in NAMES] == list(range(7))
    assert gibson_amd.meta_field(b"s\0ize") is None and gibson_amd.meta_field(b"size\0") == 0
    assert gibson_amd.meta_field(b"") is None
    L = gibson_amd.lib()
    assert L.lzf_host_meta_field(None, 4) == -1 and L.lzf_host_meta_field(ctypes.c_char_p(b"size"), 0) == -1


# ---- GPU ---------------------------------------------------------------------

GUARD = 0x5A
UNSET = -7
ROOM = 4096                              # guard bytes past every size
EXTRA = 16                               # guard elements past every per-item array
NOW = 1_700_000_000


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    gibson_amd.lib()
    return t


def _padded(torch, a, guard):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(np.concatenate([a, np.full(EXTRA, guard, a.dtype)])).cuda()


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _check(t, a, guard, what):
    """tensor t is the array a followed by EXTRA guard elements"""
    got = t.cpu().numpy()
    exp = np.concatenate([np.ascontiguousarray(a).astype(got.dtype), np.full(EXTRA, guard, got.dtype)])
    bad = np.nonzero(got != exp)[0]
    assert not len(bad), (what, len(bad), "first at", int(bad[0]), int(got[bad[0]]), int(exp[bad[0]]))


# ---- gc

def gc_store(count, gc_ratio, seed):
    """last_access at every distance from NOW that the rule tells apart"""
    rs = np.random.RandomState(seed)
    eta = rs.choice([0, 1, gc_ratio - 1, gc_ratio, gc_ratio + 1, 10 * gc_ratio, -1, -gc_ratio, I64_MIN, I64_MAX,
                     I64_MAX - 5], count)
    last = np.array([wrap(NOW - int(e)) for e in eta], np.int64)
    enc = rs.choice([ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL], count, p=[0.3, 0.3, 0.2, 0.2]).astype(np.uint8)
    size = rs.randint(0, 2**31, count).astype(np.uint32) * 2 + 1           # sums past 2^32
    return last, enc, size


def model_gc(last, enc, size, now, gc_ratio):
    """gbMemoryFreeHandler over every live item -> (enc after, freed, bytes)"""
    out, freed, total = enc.copy(), 0, 0
    for i in range(len(enc)):
        if enc[i] == ENC_NULL:
            continue
        eta = wrap(now - int(last[i]))
        if eta and eta >= gc_ratio:
            out[i] = ENC_NULL
            freed += 1
            total += int(size[i])
    return out, freed, total


# 1
@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 65, 1025, 3000])
def test_gc_frees_by_last_access_alone(torch, count):
    gc_ratio = 3600
    last, enc, size = gc_store(count, gc_ratio, 0x6C + count)
    exp_enc, freed, total = model_gc(last, enc, size, NOW, gc_ratio)
    if count >= 1025:
        assert 0 < freed < count - (enc == ENC_NULL).sum() and total > 2**32
    for gate, max_bytes, runs in ((None, 0, True), (100, 99, True), (100, 100, False), (100, 2**63, False),
                                  (2**64 - 1, 2**64 - 2, True)):
        d_last, d_enc, d_size = _padded(torch, last, UNSET), _padded(torch, enc, GUARD), \
            _padded(torch, size.view(np.int32), UNSET)
        result = torch.full((3 + 4,), UNSET, dtype=torch.int64, device="cuda")
        d_gate = None if gate is None else torch.from_numpy(np.array([gate], np.uint64).view(np.int64)).cuda()
        gibson_amd.store_gc(d_last[:count], NOW, gc_ratio, d_enc[:count], d_size[:count], result[:3], gate=d_gate,
                            max_bytes=max_bytes)
        torch.cuda.synchronize()
        got = result.cpu().numpy().tolist()
        print("count", count, "gate", gate, max_bytes, "result", got[:3], "expected", freed, total)
        assert got == ([freed, total, 1] if runs else [0, 0, 0]) + [UNSET] * 4
        _check(d_enc, exp_enc if runs else enc, GUARD, "enc")
        _check(d_last, last, UNSET, "last_access")
        _check(d_size, size.view(np.int32), UNSET, "val_size")
    # by hand: eta 0 stays, eta == gc_ratio goes, a negative eta stays
    one = lambda e: model_gc(np.array([NOW - e], np.int64), np.array([ENC_PLAIN], np.uint8), np.array([9], np.uint32),
                             NOW, gc_ratio)[1:]
    assert [one(0), one(gc_ratio - 1), one(gc_ratio), one(-1)] == [(0, 0), (0, 0), (1, 9), (0, 0)]


# ---- meta

class Items:
    """the arrays META reads, of every kind"""

    def __init__(self, count, seed):
        rs = np.random.RandomState(seed)
        self.n = count
        self.enc = rs.choice([ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL], count, p=[0.3, 0.3, 0.2, 0.2]).astype(np.uint8)
        self.size = rs.randint(0, 2**32, count, dtype=np.int64).astype(np.uint32)
        age = rs.randint(0, 1200, count).astype(np.int64)
        self.time = NOW - age
        self.time[rs.rand(count) < 0.05] = I64_MIN + 7       # now - time wraps
        self.ttl = rs.choice([-1, 0, 5, 600, 32767, 2**31 - 1], count).astype(np.int32)
        self.lock = rs.choice([0, -1, 30, -5, I64_MAX, I64_MIN], count).astype(np.int64)
        self.last = (NOW - rs.randint(0, 5000, count)).astype(np.int64)

    def validity(self, i, now):
        if i >= self.n or self.enc[i] == ENC_NULL:
            return DEAD
        if self.ttl[i] > 0 and wrap(now - int(self.time[i])) >= int(self.ttl[i]):
            return EXPIRED
        return DONE


def model_meta(s, idx, field, now, lock=True, last=True):
    """gbQueryMetaHandler per entry -> (entry_status, entry_value, result); s is updated"""
    st, val = [], []
    for i in map(int, idx):
        v = s.validity(i, now)
        x = 0
        if v == EXPIRED:
            s.enc[i] = ENC_NULL
        elif v == DONE:
            ttl = int(s.ttl[i])
            x = [int(s.size[i]), int(s.enc[i]), int(s.last[i]), int(s.time[i]), ttl,
                 -1 if ttl <= 0 else wrap(ttl - wrap(now - int(s.time[i]))), int(s.lock[i]) if lock else 0][field]
            if last:
                s.last[i] = now
        st.append(v)
        val.append(x)
    return st, val, [st.count(DONE), st.count(EXPIRED)]


def meta_list(s, n, seed):
    rs = np.random.RandomState(seed)
    junk = n // 10
    idx = rs.choice(s.n, n - junk, replace=False).astype(np.uint32)
    idx = np.concatenate([idx, rs.choice([PAD, s.n, s.n + 1, 2**31 + 3], junk).astype(np.uint32)])
    rs.shuffle(idx)
    return idx


# 2
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 65, 1025, 2500])
def test_meta_every_field_over_a_mixed_list(torch, n):
    import copy
    s0 = Items(3000, 0x3E7A)
    idx = meta_list(s0, n, 0x11 + n)
    d_idx = _i32(torch, idx)
    for field in range(7):
        # then the optional arrays left out; ACCESS cannot do without last_access
        for lock, last, est in ((True, True, True), (False, field == gibson_amd.META_ACCESS, False)):
            s = copy.deepcopy(s0)
            st, val, res = model_meta(s, idx, field, NOW, lock, last)
            if n >= 1025:
                assert min(st.count(c) for c in (DONE, DEAD, EXPIRED)) >= 40
            d_enc, d_size = _padded(torch, s0.enc, GUARD), _padded(torch, s0.size.view(np.int32), UNSET)
            d_time, d_ttl = _padded(torch, s0.time, UNSET), _padded(torch, s0.ttl, UNSET)
            d_lock, d_last = _padded(torch, s0.lock, UNSET), _padded(torch, s0.last, UNSET)
            d_est = torch.full((n + ROOM,), 0x77, dtype=torch.uint8, device="cuda")
            d_val = torch.full((n + EXTRA,), UNSET, dtype=torch.int64, device="cuda")
            result = torch.full((2 + 4,), UNSET, dtype=torch.int64, device="cuda")
            c = s0.n
            gibson_amd.store_meta(d_idx, field, d_enc[:c], d_size[:c], d_time[:c], d_ttl[:c],
                                  d_lock[:c] if lock else None, NOW, d_val[:n], result[:2],
                                  last_access=d_last[:c] if last else None, entry_status=d_est[:n] if est else None)
            torch.cuda.synchronize()
            got = result.cpu().numpy().tolist()
            print("n", n, "field", field, "result", got[:2], "expected", res)
            assert got == res + [UNSET] * 4
            assert d_val.cpu().numpy().tolist() == val + [UNSET] * EXTRA
            e = d_est.cpu().numpy()
            assert (e[:n] == (np.array(st, np.uint8) if est else 0x77)).all() and (e[n:] == 0x77).all()
            _check(d_enc, s.enc, GUARD, "enc")
            _check(d_last, s.last, UNSET, "last_access")
            for t, a, what in ((d_size, s0.size.view(np.int32), "size"), (d_time, s0.time, "time"),
                               (d_ttl, s0.ttl, "ttl"), (d_lock, s0.lock, "lock")):
                _check(t, a, UNSET, what)


# 3
@pytest.mark.gpu
def test_meta_by_hand(torch):
    # items: ttl -1, ttl 0, ttl 600 at age 100, ttl 50 at age 100 (expired), dead
    enc = np.array([ENC_LZF, ENC_PLAIN, ENC_NUMBER, ENC_PLAIN, ENC_NULL], np.uint8)
    size = np.array([11, 22, 8, 44, 55], np.uint32)
    time = np.array([NOW - 100] * 5, np.int64)
    ttl = np.array([-1, 0, 600, 50, 600], np.int32)
    lock = np.array([-1, 0, 77, 5, 5], np.int64)
    last = np.array([NOW - 9, NOW - 8, NOW - 7, NOW - 6, NOW - 5], np.int64)
    idx = _i32(torch, [4, 3, 2, 1, 0, PAD])
    want = {0: [0, 0, 8, 22, 11, 0], 1: [0, 0, ENC_NUMBER, ENC_PLAIN, ENC_LZF, 0],
            2: [0, 0, NOW - 7, NOW - 8, NOW - 9, 0], 3: [0, 0, NOW - 100, NOW - 100, NOW - 100, 0],
            4: [0, 0, 600, 0, -1, 0], 5: [0, 0, 500, -1, -1, 0], 6: [0, 0, 77, 0, -1, 0]}
    for field, exp in want.items():
        d_enc, d_last = torch.from_numpy(enc).cuda(), torch.from_numpy(last).cuda()
        val = torch.full((6,), UNSET, dtype=torch.int64, device="cuda")
        result = torch.full((2,), UNSET, dtype=torch.int64, device="cuda")
        est = torch.full((6,), 0x77, dtype=torch.uint8, device="cuda")
        gibson_amd.store_meta(idx, field, d_enc, _i32(torch, size), torch.from_numpy(time).cuda(),
                              torch.from_numpy(ttl).cuda(), torch.from_numpy(lock).cuda(), NOW, val, result,
                              last_access=d_last, entry_status=est)
        torch.cuda.synchronize()
        assert val.cpu().numpy().tolist() == exp, field
        assert est.cpu().numpy().tolist() == [DEAD, EXPIRED, DONE, DONE, DONE, DEAD]
        assert result.cpu().numpy().tolist() == [3, 1]
        assert d_enc.cpu().numpy().tolist() == [ENC_LZF, ENC_PLAIN, ENC_NUMBER, ENC_NULL, ENC_NULL]
        assert d_last.cpu().numpy().tolist() == [NOW, NOW, NOW, NOW - 6, NOW - 5]   # the locked item too


# ---- keys

def keys_model(keys, enc, idx, header, max_response):
    """gbQueryKeysHandler's reply -> (frame or b"", found, status, the participating items)"""
    idx = np.asarray(idx, np.uint32)
    part = [i for i in map(int, idx[idx < len(keys)]) if enc[i] != ENC_NULL and len(keys[i])]
    body = struct.pack("<I", len(part))
    for j, i in enumerate(part):
        d = b"%d" % j
        body += struct.pack("<I", len(d)) + d + struct.pack("<BI", ENC_PLAIN, len(keys[i])) + keys[i]
    if not part:
        return b"", 0, MGET_NOT_FOUND, part
    if len(body) > max_response:
        return b"", len(part), MGET_TOO_BIG, part
    return (struct.pack("<hBI", 7, ENC_PLAIN, len(body)) if header else b"") + body, len(part), MGET_OK, part


class KeyStore:
    def __init__(self, torch, count, seed):
        rnd = random.Random(seed)
        self.keys = [bytes(rnd.choice(b"abcdefghij:_0123456789") for _ in range(rnd.choice([0, 1, 2, 7, 40, 300])))
                     for _ in range(count)]
        self.klen = np.array([len(k) for k in self.keys], np.uint32)
        self.koff = np.concatenate([[0], np.cumsum(self.klen[:-1], dtype=np.int64)]).astype(np.int64)
        self.enc = np.array([rnd.choice([ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL]) for _ in range(count)], np.uint8)
        self.d_keys = torch.from_numpy(np.frombuffer(b"".join(self.keys) + b"\0", np.uint8).copy()).cuda()
        self.d_koff, self.d_klen = torch.from_numpy(self.koff).cuda(), _i32(torch, self.klen)
        self.d_enc = _padded(torch, self.enc, GUARD)
        self.takes = [i for i in range(count) if self.enc[i] != ENC_NULL and len(self.keys[i])]
        self.skipped = [i for i in range(count) if self.enc[i] == ENC_NULL or not len(self.keys[i])]


def run_keys(torch, ks, idx, header, max_response):
    n, count = len(idx), len(ks.keys)
    exp, found, status, part = keys_model(ks.keys, ks.enc, idx, header, max_response)
    hdr = 7 if header else 0
    frame = torch.full((hdr + max_response + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
    flen = torch.full((1 + 4,), UNSET, dtype=torch.int64, device="cuda")
    result = torch.full((2 + 4,), UNSET, dtype=torch.int64, device="cuda")
    wsize = int(gibson_amd.lib().lzf_gpu_store_keys_work_size(n))
    work = torch.full((wsize + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
    gibson_amd.store_keys(_i32(torch, idx), ks.d_keys, ks.d_koff, ks.d_klen, ks.d_enc[:count],
                          frame[:hdr + max_response], max_response, flen[:1], result[:2], work=work[:wsize],
                          reply_header=header)
    torch.cuda.synchronize()
    got = result.cpu().numpy().tolist()
    print("n", n, "header", header, "max_response", max_response, "result", got[:2], "expected", found, status,
          "frame_len", int(flen[0].item()), len(exp))
    assert got == [found, status] + [UNSET] * 4
    assert flen.cpu().numpy().tolist() == [len(exp)] + [UNSET] * 4
    f = frame.cpu().numpy().tobytes()
    assert f[:len(exp)] == exp
    assert f[len(exp):] == bytes([GUARD]) * (len(f) - len(exp))     # nothing past the frame; nothing at all when refused
    assert (work[wsize:].cpu().numpy() == GUARD).all()
    _check(ks.d_enc, ks.enc, GUARD, "enc")                          # nothing is nulled
    return exp, part


def kv_frame_of_pairs(torch, ks, part, header, max_response):
    """lzf_gpu_kv_frame over the pairs built on the host -> the frame"""
    digits = [b"%d" % j for j in range(len(part))]
    dl = np.array([len(d) for d in digits], np.uint32)
    do = np.concatenate([[0], np.cumsum(dl[:-1], dtype=np.int64)]).astype(np.int64)
    vl = ks.klen[part]
    n = len(part)
    frame = torch.full((7 + max_response,), GUARD, dtype=torch.uint8, device="cuda")
    flen = torch.zeros(1, dtype=torch.int64, device="cuda")
    w = gibson_amd.kv_frame(torch.from_numpy(np.frombuffer(b"".join(digits), np.uint8).copy()).cuda(),
                            torch.from_numpy(do).cuda(), _i32(torch, dl), ks.d_keys,
                            torch.from_numpy(ks.koff[part]).cuda(), _i32(torch, vl),
                            torch.zeros(n, dtype=torch.uint8, device="cuda"), _i32(torch, vl), n, int(vl.max()), frame,
                            max_response, flen, reply_header=header)
    torch.cuda.synchronize()
    del w
    return frame[:int(flen.item())].cpu().numpy().tobytes()


# 4
@pytest.mark.gpu
@pytest.mark.parametrize("found", [0, 1, 9, 10, 11, 100, 101, 1025])
def test_keys_frame_by_found(torch, found):
    ks = KeyStore(torch, 3000, 0x4E15)
    assert len(ks.takes) >= 1025 and len(ks.skipped) >= 300
    assert any(ks.enc[i] != ENC_NULL for i in ks.skipped) and any(ks.enc[i] == ENC_NULL for i in ks.skipped)
    rnd = random.Random(found)
    # `found` participating entries among dead ones, key-less ones, padding and out-of-range entries
    idx = rnd.sample(ks.takes, found) + rnd.sample(ks.skipped, 40) + [PAD, 3000, 3001, 2**31 + 3] * 3
    rnd.shuffle(idx)
    idx = np.array(idx, np.uint32)
    for header in (True, False):
        exp, part = run_keys(torch, ks, idx, header, 1 << 20)
        assert len(part) == found and (len(exp) > 0) == (found > 0)
        if not found:
            continue
        payload = len(exp) - (7 if header else 0)
        assert kv_frame_of_pairs(torch, ks, part, header, 1 << 20) == exp
        fit, _ = run_keys(torch, ks, idx, header, payload)           # exactly fitting
        assert fit == exp
        short, _ = run_keys(torch, ks, idx, header, payload - 1)     # one byte short: MGET_TOO_BIG, no byte written
        assert short == b""
        if found == 11 and header:                                   # by hand: the digit count changes inside the frame
            k = [ks.keys[i] for i in part]
            at = 7 + 4 + sum(4 + 1 + 5 + len(x) for x in k[:10])
            assert exp[:7] == struct.pack("<hBI", 7, 0, len(exp) - 7) and exp[7:11] == struct.pack("<I", 11)
            assert exp[at:at + 6] == struct.pack("<I", 2) + b"10" and exp[at + 6] == ENC_PLAIN


# 5
@pytest.mark.gpu
def test_keys_keeps_expired_items_and_list_order(torch):
    # KEYS makes no validity test (src/query.c:1353-1368): it is not even given the time arrays
    ks = KeyStore(torch, 200, 0x0E)
    idx = np.array(list(reversed(ks.takes)) + ks.skipped, np.uint32)
    exp, part = run_keys(torch, ks, idx, True, 1 << 20)
    assert part == list(reversed(ks.takes)) and len(part) >= 100
    first = ks.keys[part[0]]
    assert exp[11:11 + 4 + 1 + 1 + 4 + len(first)] == struct.pack("<I", 1) + b"0" + struct.pack("<BI", 0, len(first)) \
        + first


# 6
@pytest.mark.gpu
def test_keys_list_past_one_piece_of_the_tile_scan(torch):
    # 2 048 tiles of 1 024 entries are one piece of the scan over the tile sums; the carry between
    # pieces shows only past that.  Mostly padding, with entries at both ends and around the seam
    ks = KeyStore(torch, 3000, 0x4E15)
    n = 2048 * 1024 + 1025
    rnd = random.Random(0x5EA)
    idx = np.full(n, PAD, np.uint32)
    seam = 2048 * 1024
    where = sorted({0, 1, 1023, 1024, seam - 1, seam, seam + 1, n - 1} | set(rnd.sample(range(seam, n), 100))
                   | set(rnd.sample(range(seam), 300)))
    idx[where] = rnd.sample(range(3000), len(where))
    exp, part = run_keys(torch, ks, idx, True, 1 << 20)
    assert 150 < len(part) < len(where) and exp
    past = [int(i) for i in idx[seam:] if i != PAD and ks.enc[i] != ENC_NULL and len(ks.keys[i])]
    assert len(past) > 40 and part[-len(past):] == past     # pairs whose place needs the carry
