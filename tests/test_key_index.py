"""The device key index (lzf_gpu_key_index_insert / _lookup): exact-key upsert
and lookup over the device store's keys.  The model is a Python dict run over
each batch in request order; the bar is exact equality of idx, enc, result,
status and *used.  The slots a lookup examines are counted on the host from
the table as the device left it, by the two fixed points of the contract
(0xFF bytes: empty; linear probing from lzf_host_key_home) and the slot format
of DESIGN.md (the item index in the low 32 bits).

Every buffer a test hands over with a size is allocated larger and the excess
filled with a guard byte, which is checked afterwards."""
import ctypes
import random

import numpy as np
import pytest

from tests.oracle_lib import synth

try:                                    # before liblzf_hip.so loads: one HIP runtime in the process
    import torch as _torch  # noqa: F401
except ImportError:
    _torch = None

import gibson_amd

ENC_PLAIN, ENC_LZF, ENC_NULL = 0, 1, 0xFF
OK, FULL = 0, 1
PAD = 0xFFFFFFFF
EMPTY = 0xFFFFFFFFFFFFFFFF
NEW_NAMES = ("lzf_gpu_key_index_bytes", "lzf_host_key_home", "lzf_gpu_key_index_insert", "lzf_gpu_key_index_lookup")


# ---- CPU ---------------------------------------------------------------------

def test_library_exports_the_key_index_calls():
    L = gibson_amd.lib()
    for n in NEW_NAMES:
        assert hasattr(L, n), n
        assert n in gibson_amd.lzf.EXPORTS
    for n in ("key_index_bytes", "key_home", "key_index_insert", "key_index_lookup"):
        assert callable(getattr(gibson_amd, n)), n
    assert (gibson_amd.KIDX_OK, gibson_amd.KIDX_FULL) == (0, 1)


def test_key_index_calls_reject_bad_arguments_without_device():
    # argument validation happens before any HIP call, so this runs on CPU;
    # only calls that must be refused are made (the pointers are host memory)
    L = gibson_amd.lib()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(512)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def insert(ptrs, slots=16, count=8, first=0, n=8):
        table, used, keys, koff, klen, enc, result, status = ptrs
        return L.lzf_gpu_key_index_insert(table, slots, used, keys, koff, klen, enc, count, first, n, result, status,
                                          null)

    for k in range(8):                               # a NULL pointer in each position
        ptrs = [p] * 8
        ptrs[k] = null
        assert insert(ptrs) == -1, k
    assert insert([p] * 8, count=0, n=1) == -1
    assert insert([p] * 8, n=0) == -1
    assert insert([p] * 8, first=1) == -1            # first + n > count
    assert insert([p] * 8, count=8, first=8, n=1) == -1
    assert insert([p] * 8, count=2**32 - 1, first=2**32 - 2, n=2) == -1       # first + n wraps 32 bits to 0
    assert insert([p] * 8, count=2**32 - 1, first=2**31, n=2**31) == -1
    for slots in (0, 1, 8, 15, 17, 24, 4097, 2**31 + 1, 2**32 - 1):
        assert insert([p] * 8, slots=slots) == -1, slots

    def lookup(ptrs, slots=16, count=8, nq=1):
        table, keys, koff, klen, enc, qkeys, qoff, qlen, idx, result = ptrs
        return L.lzf_gpu_key_index_lookup(table, slots, keys, koff, klen, enc, count, qkeys, qoff, qlen, nq, idx,
                                          result, null)

    for k in range(10):
        ptrs = [p] * 10
        ptrs[k] = null
        assert lookup(ptrs) == -1, k
    assert lookup([p] * 10, count=0) == -1
    assert lookup([p] * 10, nq=0) == -1
    for slots in (0, 1, 8, 15, 17, 24, 4097, 2**31 + 1, 2**32 - 1):
        assert lookup([p] * 10, slots=slots) == -1, slots


def test_key_index_bytes():
    L = gibson_amd.lib()
    prev = 0
    for s in range(4, 32):
        b = L.lzf_gpu_key_index_bytes(1 << s)
        assert b >= 4 * (1 << s) and b > prev, s
        assert gibson_amd.key_index_bytes(1 << s) == b
        prev = b
    assert 4 * 2**31 <= L.lzf_gpu_key_index_bytes(2**31) < 2**40              # 64-bit arithmetic: no wrap
    for s in (0, 8, 24, 2**31 + 1):
        with pytest.raises(ValueError):
            gibson_amd.key_index_bytes(s)


def test_key_home():
    rnd = random.Random(0x4B1D)
    for slots in (16, 4096, 1 << 20, 2**31):
        homes = set()
        for _ in range(200):
            k = bytes(rnd.randrange(256) for _ in range(rnd.randint(1, 70)))
            h = gibson_amd.key_home(k, slots)
            assert h == gibson_amd.key_home(bytes(k), slots) and 0 <= h < slots
            homes.add(h)
        assert len(homes) > 8                        # it spreads
    # the length is part of the hash: over three table sizes, not one chance collision
    assert any(gibson_amd.key_home(b"a", s) != gibson_amd.key_home(b"a\0", s) for s in (1 << 20, 1 << 24, 2**31))
    assert any(gibson_amd.key_home(b"\0", s) != gibson_amd.key_home(b"\0\0", s) for s in (1 << 20, 1 << 24, 2**31))
    L = gibson_amd.lib()
    for slots in (0, 8, 17, 24, 2**31 + 1):
        assert L.lzf_host_key_home(ctypes.c_char_p(b"abc"), 3, slots) == 0xFFFFFFFF
        with pytest.raises(ValueError):
            gibson_amd.key_home(b"abc", slots)


# ---- GPU ---------------------------------------------------------------------

GUARD = 0x5A
GUARD32 = 0x5A5A5A5A
ROOM = 4096                              # guard bytes past every size
UNSET = -7
NOW = 1_700_000_000


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    gibson_amd.lib()
    return t


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _i64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _u8(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def key_arena(torch, keys, shift):
    """keys packed from byte ``shift`` of an arena: (arena, key_off, key_len)"""
    kl = np.array([len(k) for k in keys], np.uint32)
    off = shift + np.concatenate([[0], np.cumsum(kl[:-1], dtype=np.int64)])
    buf = np.frombuffer(bytes([GUARD]) * shift + b"".join(keys) + bytes([GUARD]) * 8, np.uint8)
    return _u8(torch, buf), _i64(torch, off), _i32(torch, kl)


class Index:
    """a store's keys and enc on the device, a key index over them, and the
    model: the dict, the enc bytes and the set of keys that hold a slot"""

    def __init__(self, torch, keys, slots, enc=None, shift=0, dev=None):
        self.t, self.keys, self.n, self.slots = torch, list(keys), len(keys), slots
        if dev is None:
            self.d_keys, self.d_koff, self.d_klen = key_arena(torch, self.keys, shift)
            enc = np.zeros(self.n, np.uint8) if enc is None else np.asarray(enc, np.uint8)
            self.enc_buf = _u8(torch, np.concatenate([enc, np.full(64, GUARD, np.uint8)]))
            self.enc = self.enc_buf[:self.n]
        else:                                                   # the arrays of an existing store
            self.d_keys, self.d_koff, self.d_klen, self.enc = dev
            self.enc_buf = None
        self.m_enc = self.enc.cpu().numpy().copy()
        self.bytes = gibson_amd.key_index_bytes(slots)
        self.table_buf = torch.full((self.bytes + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
        self.table = self.table_buf[:self.bytes]
        self.used = torch.full((9,), GUARD32, dtype=torch.int32, device="cuda")
        self.result = torch.full((8,), UNSET, dtype=torch.int64, device="cuda")
        self.status = torch.full((5,), UNSET, dtype=torch.int32, device="cuda")
        self.clear()

    def clear(self):
        self.table.fill_(0xFF)                                  # the documented clear
        self.used[:1] = 0
        self.map, self.claimed = {}, set()

    def table_words(self):
        return self.table.cpu().numpy().view(np.uint64)

    def model_insert(self, first, n):
        if len(self.claimed) + n > self.slots - self.slots // 4:
            return FULL, [0, 0, 0, 0]
        replaced = superseded = skipped = 0
        for i in range(first, first + n):
            key = self.keys[i]
            if self.m_enc[i] == ENC_NULL or not key:
                skipped += 1
                continue
            j = self.map.get(key)
            if j is not None and j != i and self.m_enc[j] != ENC_NULL:
                self.m_enc[j] = ENC_NULL
                if first <= j < first + n:
                    superseded += 1
                else:
                    replaced += 1
            self.map[key] = i
            self.claimed.add(key)
        mapped = sum(1 for i in range(first, first + n)
                     if self.m_enc[i] != ENC_NULL and self.keys[i] and self.map.get(self.keys[i]) == i)
        assert mapped + superseded + skipped == n
        return OK, [mapped, replaced, superseded, skipped]

    def check_guards(self):
        assert (self.table_buf[self.bytes:].cpu().numpy() == GUARD).all()
        assert (self.used[1:].cpu().numpy() == GUARD32).all()
        assert (self.status[1:].cpu().numpy() == UNSET).all()
        if self.enc_buf is not None:
            assert (self.enc_buf[self.n:].cpu().numpy() == GUARD).all()

    def insert(self, first, n):
        """one insert call and the model's; -> (status, result)"""
        torch = self.t
        self.result.fill_(UNSET)
        self.status.fill_(UNSET)
        before = self.table_words().copy()
        gibson_amd.key_index_insert(self.table, self.used, self.d_keys, self.d_koff, self.d_klen, self.enc, first, n,
                                    self.result, self.status)
        torch.cuda.synchronize()
        status, result = self.model_insert(first, n)
        got = self.result.cpu().numpy().tolist()
        print("insert", (first, n), "status", int(self.status[0].item()), "result", got[:4], "used",
              int(self.used[0].item()), "expected", status, result, len(self.claimed))
        assert int(self.status[0].item()) == status
        assert got[:4] == result and got[4:] == [UNSET] * 4
        assert int(self.used[0].item()) == len(self.claimed)
        assert (self.enc.cpu().numpy() == self.m_enc).all()
        if status == FULL:
            assert (self.table_words() == before).all()         # no table byte changed
        self.check_guards()
        return status, result

    def delete(self, idx):
        gibson_amd.store_delete(_i32(self.t, np.asarray(idx, np.uint32)), self.enc)
        self.m_enc[np.asarray(idx, np.int64)] = ENC_NULL

    def model_lookup(self, q):
        i = self.map.get(q) if q else None
        return PAD if i is None or self.m_enc[i] == ENC_NULL else i

    def examined(self, words, q):
        """the slots the walk for key q looks at in the table ``words``"""
        if not q:
            return 0
        pos, seen = gibson_amd.key_home(q, self.slots), 0
        for _ in range(self.slots):
            w = int(words[pos])
            seen += 1
            if w == EMPTY or ((w & PAD) < self.n and self.keys[w & PAD] == q):
                break
            pos = (pos + 1) & (self.slots - 1)
        return seen

    def lookup(self, qkeys, shift=1):
        """one lookup call against the model; -> idx as a device tensor (int32)"""
        torch = self.t
        nq = len(qkeys)
        d_q, d_qoff, d_qlen = key_arena(torch, qkeys, shift)
        idx_buf = torch.full((nq + 16,), 0x11111111, dtype=torch.int32, device="cuda")
        self.result.fill_(UNSET)
        gibson_amd.key_index_lookup(self.table, self.d_keys, self.d_koff, self.d_klen, self.enc, d_q, d_qoff, d_qlen,
                                    idx_buf[:nq], self.result)
        torch.cuda.synchronize()
        exp = [self.model_lookup(q) for q in qkeys]
        words = self.table_words()
        hits = sum(1 for e in exp if e != PAD)
        result = [hits, nq - hits, sum(self.examined(words, q) for q in qkeys)]
        got_idx = idx_buf.cpu().numpy().view(np.uint32)
        got = self.result.cpu().numpy().tolist()
        print("lookup", nq, "result", got[:3], "expected", result)
        assert got_idx[:nq].tolist() == exp
        assert (got_idx[nq:] == 0x11111111).all()
        assert got[:3] == result and got[3:] == [UNSET] * 5
        assert (self.enc.cpu().numpy() == self.m_enc).all()     # a lookup writes nothing
        self.check_guards()
        return idx_buf[:nq]


def keys_at_home(slots, home, n, tag=b"k"):
    out, i = [], 0
    while len(out) < n:
        k = tag + str(i).encode()
        if gibson_amd.key_home(k, slots) == home:
            out.append(k)
        i += 1
    return out


@pytest.mark.gpu
def test_one_chain_with_wrap_around(torch):
    # 12 keys whose home is the last slot: the chain is 15, 0, 1, .. 10.  Pins
    # linear probing, and that the host's and the device's home slots agree
    keys = keys_at_home(16, 15, 13)
    x = Index(torch, keys, 16)
    assert x.insert(0, 12) == (OK, [12, 0, 0, 0])
    words = x.table_words()
    assert [int(w) != EMPTY for w in words] == [True] * 11 + [False] * 4 + [True]
    x.lookup(keys[:12])
    assert x.result.cpu().numpy().tolist()[:3] == [12, 0, 78]          # 1 + .. + 12, whichever key won which slot
    x.lookup(keys[12:])                                                # absent, the same home
    assert x.result.cpu().numpy().tolist()[:3] == [0, 1, 13]


@pytest.mark.gpu
def test_load_bound(torch):
    rnd = random.Random(0x10AD)
    keys = [b"key:%d:%d" % (i, rnd.randrange(1 << 30)) for i in range(40)]
    x = Index(torch, keys, 16)
    assert x.insert(0, 12)[0] == OK                                    # 12 == 16 - 16 / 4
    assert x.insert(12, 1) == (FULL, [0, 0, 0, 0])                     # table, enc, used, result checked inside
    assert x.insert(0, 12) == (FULL, [0, 0, 0, 0])                     # n counts whole, for an indexed range too
    x.lookup(keys[:16])                                                # 12 present, 13th refused: a miss
    x.lookup(keys[20:40] + keys_at_home(16, 3, 4, b"absent"))          # absent keys in the table at its bound
    y = Index(torch, keys, 16)
    assert y.insert(0, 13) == (FULL, [0, 0, 0, 0])
    assert (y.table_words() == EMPTY).all()
    y.lookup(keys[:13])
    # n counts whole: 5 dead items among 13 are still refused
    z = Index(torch, keys, 16, enc=[ENC_NULL] * 5 + [0] * 35)
    assert z.insert(0, 13) == (FULL, [0, 0, 0, 0])
    assert z.insert(0, 12) == (OK, [7, 0, 0, 5])


@pytest.mark.gpu
def test_duplicates_inside_one_launch(torch):
    # 3000 items over 7 keys: equal keys share a wave, a workgroup and different workgroups
    rnd = random.Random(0xD0B1E)
    pool = [b"dup-key-%d" % i for i in range(7)]
    keys = [rnd.choice(pool) for _ in range(3000)]
    x = Index(torch, keys, 4096)
    assert x.insert(0, 3000) == (OK, [7, 0, 2993, 0])
    assert int(x.used[0].item()) == 7
    idx = x.lookup(pool).cpu().numpy().view(np.uint32).tolist()
    assert idx == [max(i for i, k in enumerate(keys) if k == p) for p in pool]
    assert (x.enc.cpu().numpy() != ENC_NULL).sum() == 7                # every other item is NULL


@pytest.mark.gpu
def test_overwrite_across_calls(torch):
    keys = [b"spare-%d" % i for i in range(120)]
    for i, k in enumerate((b"A", b"B", b"C", b"D")):
        keys[100 + i] = k
    keys[0:4] = [b"A", b"B", b"X", b"Y"]                               # two overwrites at lower indices
    keys[110:114] = [b"C", b"Y", b"C", b"Z"]                           # overwrites, and C twice in the batch
    x = Index(torch, keys, 64)
    assert x.insert(100, 4) == (OK, [4, 0, 0, 0])
    assert x.insert(0, 4) == (OK, [4, 2, 0, 0])                        # the new items win though their indices are lower
    idx = x.lookup([b"A", b"B", b"C", b"D", b"X", b"Y", b"Z"]).cpu().numpy().view(np.uint32).tolist()
    assert idx == [0, 1, 102, 103, 2, 3, PAD]
    assert x.enc.cpu().numpy()[[100, 101]].tolist() == [ENC_NULL, ENC_NULL]
    assert x.insert(110, 4) == (OK, [3, 2, 1, 0])                      # replaced 102 (C) and 3 (Y), superseded 110
    idx = x.lookup([b"A", b"B", b"C", b"D", b"X", b"Y", b"Z"]).cpu().numpy().view(np.uint32).tolist()
    assert idx == [0, 1, 112, 103, 2, 111, 113]
    assert int(x.used[0].item()) == 7


@pytest.mark.gpu
def test_dead_items(torch):
    keys = [b"live-%d" % i for i in range(20)] + [b"live-3", b"live-7"]
    x = Index(torch, keys, 64)
    assert x.insert(0, 20) == (OK, [20, 0, 0, 0])
    x.delete([3, 7, 9])
    idx = x.lookup(keys[:20]).cpu().numpy().view(np.uint32)
    assert idx[[3, 7, 9]].tolist() == [PAD] * 3 and (idx != PAD).sum() == 17
    assert x.insert(20, 2) == (OK, [2, 0, 0, 0])                       # nothing replaced: the occupants were dead
    assert int(x.used[0].item()) == 20                                 # their slots were taken over
    idx = x.lookup(keys[:20]).cpu().numpy().view(np.uint32)
    assert idx[[3, 7, 9]].tolist() == [20, 21, PAD]


@pytest.mark.gpu
def test_expired_item_is_a_hit(torch):
    keys = [b"ttl-%d" % i for i in range(12)]
    x = Index(torch, keys, 32)
    x.insert(0, 12)
    ttl = np.zeros(12, np.int32)
    ttl[[2, 5]] = 10                                                   # set 11 s ago: expired
    ttl[8] = 100
    time = _i64(torch, np.full(12, NOW - 11, np.int64))
    d_ttl = torch.from_numpy(ttl).cuda()
    idx = x.lookup(keys + [b"ttl-absent"])
    assert idx.cpu().numpy().view(np.uint32).tolist() == list(range(12)) + [PAD]     # tr_find_node returns them
    result = torch.full((2,), UNSET, dtype=torch.int64, device="cuda")
    gibson_amd.store_count(idx, x.enc, time, d_ttl, NOW, result)       # the operator applies the TTL rule
    torch.cuda.synchronize()
    assert result.cpu().numpy().tolist() == [10, 2]
    x.m_enc[[2, 5]] = ENC_NULL
    idx = x.lookup(keys).cpu().numpy().view(np.uint32)
    assert idx[[2, 5]].tolist() == [PAD, PAD] and (idx != PAD).sum() == 10


@pytest.mark.gpu
def test_skipped_items(torch):
    # a set_store batch refused for lack of room leaves every enc NULL
    values = [b"v" * 40, b"w" * 50, b"x" * 60]
    ln = np.array([len(v) for v in values], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.int64)])
    arena = torch.zeros(16, dtype=torch.uint8, device="cuda")
    used = torch.zeros(1, dtype=torch.int64, device="cuda")
    status = torch.full((1,), UNSET, dtype=torch.int32, device="cuda")
    vo = torch.zeros(3, dtype=torch.int64, device="cuda")
    vs = torch.zeros(3, dtype=torch.int32, device="cuda")
    keys = [b"r0", b"r1", b"r2"]
    d_keys, d_koff, d_klen = key_arena(torch, keys, 0)
    enc = torch.zeros(3, dtype=torch.uint8, device="cuda")
    w = gibson_amd.set_store(_u8(torch, np.frombuffer(b"".join(values), np.uint8)), _i64(torch, off), _i32(torch, ln),
                             64, int(ln.max()), int(ln.sum()), arena, used, vo, vs, enc, status)
    torch.cuda.synchronize()
    del w
    assert int(status.item()) == gibson_amd.STORE_FULL and (enc.cpu().numpy() == ENC_NULL).all()
    x = Index(torch, keys, 16, dev=(d_keys, d_koff, d_klen, enc))
    assert x.insert(0, 3) == (OK, [0, 0, 0, 3])
    assert (x.table_words() == EMPTY).all() and int(x.used[0].item()) == 0
    x.lookup(keys)
    # empty keys among live ones: the reference asserts klen > 0
    keys = [b"a", b"", b"b", b"", b""]
    y = Index(torch, keys, 16)
    assert y.insert(0, 5) == (OK, [2, 0, 0, 3])
    assert (y.table_words() != EMPTY).sum() == 2
    assert y.lookup(keys).cpu().numpy().view(np.uint32).tolist() == [0, PAD, 2, PAD, PAD]
    assert y.result.cpu().numpy().tolist()[2] == sum(y.examined(y.table_words(), k) for k in (b"a", b"b"))


@pytest.mark.gpu
def test_insert_is_idempotent(torch):
    rnd = random.Random(0x1DE)
    pool = [b"idem:%d" % i for i in range(150)]
    keys = [rnd.choice(pool) for _ in range(600)]
    x = Index(torch, keys, 1024)
    status, first = x.insert(0, 600)
    distinct = len(set(keys))
    assert (status, first) == (OK, [distinct, 0, 600 - distinct, 0])
    enc, words = x.enc.cpu().numpy().copy(), x.table_words().copy()
    assert x.insert(0, 600) == (OK, [distinct, 0, 0, 600 - distinct])  # the superseded ones are dead by now
    assert (x.enc.cpu().numpy() == enc).all() and (x.table_words() == words).all()
    assert int(x.used[0].item()) == distinct
    assert x.insert(100, 300)[0] == OK                                 # a part of the range
    assert (x.enc.cpu().numpy() == enc).all() and (x.table_words() == words).all()


@pytest.mark.gpu
def test_key_shapes(torch):
    rnd = random.Random(0x5AFE)
    keys = [bytes(rnd.randrange(256) for _ in range(n)) for n in (1, 2, 3, 4, 5, 63, 64, 65, 255, 4096)]
    keys += [b"abc"[:n] for n in (1, 2, 3)] + [b"abcdefghijklmnopqrstuvwxyz"[:n] for n in (7, 8, 9, 15, 16, 17, 24, 25)]
    long = bytes(rnd.randrange(256) for _ in range(300))
    keys += [long[:70] + bytes([c]) for c in (0, 1, 255)]              # equal but for the last byte
    keys += [long[:71 + n] for n in range(9)]                          # the tail bytes past the last whole word
    keys += [b"\0", b"\0\0", b"\0\0\0", b"a\0", b"a\0b", b"a\0\0b", b"\0a", b"z\0" * 8, b"z\0" * 8 + b"\0"]
    keys = list(dict.fromkeys(keys))
    absent = [keys[9][:-1] + bytes([keys[9][-1] ^ 1]), keys[9][:-1], keys[9] + b"\0", long[:70], long[:70] + b"\2",
              b"ab\0", b"\0" * 4, b"a", b"z\0" * 7, long[:80] + b"!"]
    absent = [k for k in absent if k not in keys]
    assert len(absent) >= 8
    for shift in (0, 1, 3):                                            # the arena offsets: even, odd
        x = Index(torch, keys, 256, shift=shift)
        assert x.insert(0, len(keys)) == (OK, [len(keys), 0, 0, 0])
        order = keys + absent
        rnd.shuffle(order)
        x.lookup(order, shift=(shift + 2) % 5)                         # a query arena of its own


def build_kv_store(torch):
    """a small set_store batch of PLAIN and LZF items, with the sizes at which
    the decoders change route, under distinct keys but for two duplicates"""
    from tests.test_store_mget import build_store
    rnd = random.Random(0xE2E)
    sizes = [rnd.randint(1, 200) for _ in range(48)]
    for i, n in zip(rnd.sample(range(48), 3), (4096, 4097, 16385)):
        sizes[i] = n
    values = [synth(1 if n > 4000 else i % 6, 0x5EEDE2E, i, n) for i, n in enumerate(sizes)]
    keys = [b"user:%d:%s" % (i, bytes(rnd.choice(b"abcxyz") for _ in range(rnd.randint(0, 20)))) for i in range(48)]
    big = [i for i, n in enumerate(sizes) if n > 4000]
    small = [i for i in range(48) if i not in big]
    keys[small[5]], keys[small[9]] = keys[small[20]], keys[small[30]]  # overwritten inside the batch
    h = build_store(torch, values, 64, keys)
    assert (h.enc == ENC_LZF).sum() >= 4 and (h.enc == ENC_PLAIN).sum() >= 4
    assert all(h.enc[i] == ENC_LZF for i in big)
    return h


@pytest.mark.gpu
def test_set_insert_lookup_mget_and_del_by_key(torch, oracle):
    from tests.test_store_mget import Dev, Mget, expect_frame
    h = build_kv_store(torch)
    d = Dev(torch, h, key_shift=1)
    x = Index(torch, h.keys, 128, dev=(d.keys, d.koff, d.klen, d.enc))
    distinct = len(set(h.keys))
    assert x.insert(0, h.n) == (OK, [distinct, 0, h.n - distinct, 0])
    rnd = random.Random(0xE2E2)
    query = list(dict.fromkeys(h.keys)) + [b"user:absent", b"user:", b"user:1:none"]
    rnd.shuffle(query)
    query.insert(7, h.keys[int(np.argmax(h.vlen))])                    # one key twice: the 16385-byte LZF item
    idx = x.lookup(query)
    valid = [x.model_lookup(q) for q in query if x.model_lookup(q) != PAD]
    assert len(valid) == distinct + 1
    exp = expect_frame(oracle, h, valid, 64 << 20, True)               # the same items in query order
    r = Mget(torch, d, idx, len(exp) + 5)                              # the list never leaves the device
    r.check(torch, exp, [len(valid), 0, len(query) - len(valid), 0])
    # DEL by key: lookup -> count -> delete
    gone = [query[k] for k in (0, 3, 7, 11, 30)] + [b"user:absent"]
    gone = list(dict.fromkeys(gone))
    idx = x.lookup(gone)
    hits = [x.model_lookup(q) for q in gone if x.model_lookup(q) != PAD]
    result = torch.full((2,), UNSET, dtype=torch.int64, device="cuda")
    gibson_amd.store_count(idx, d.enc, None, None, NOW, result)
    gibson_amd.store_delete(idx, d.enc)
    torch.cuda.synchronize()
    assert result.cpu().numpy().tolist() == [len(hits), 0]             # the reply of the DEL
    x.m_enc[np.asarray(hits, np.int64)] = ENC_NULL
    after = x.lookup(query).cpu().numpy().view(np.uint32)
    assert hits and all(after[k] == PAD for k, q in enumerate(query) if q in gone)


@pytest.mark.gpu
def test_rebuild_after_compaction(torch):
    from tests.test_store_mget import Dev
    h = build_kv_store(torch)
    d = Dev(torch, h)
    x = Index(torch, h.keys, 128, dev=(d.keys, d.koff, d.klen, d.enc))
    x.insert(0, h.n)
    rs = np.random.RandomState(0xC0DE)
    x.delete(rs.choice(h.n, 17, replace=False))
    dst = torch.zeros(int(h.arena.size) + 64, dtype=torch.uint8, device="cuda")
    dst_used = torch.zeros(1, dtype=torch.int64, device="cuda")
    report = torch.zeros(4, dtype=torch.int64, device="cuda")
    status = torch.full((1,), UNSET, dtype=torch.int32, device="cuda")
    w = gibson_amd.store_compact(d.arena[:int(h.arena.size)], d.off, d.size, d.enc, dst, dst_used, report, status)
    torch.cuda.synchronize()
    del w
    assert int(status.item()) == gibson_amd.STORE_OK
    live = int((x.m_enc != ENC_NULL).sum())
    assert report.cpu().numpy().tolist()[0] == live
    before = int(x.used[0].item())
    x.clear()
    assert x.insert(0, h.n) == (OK, [live, 0, 0, h.n - live])          # the live keys are distinct by now
    assert int(x.used[0].item()) == live < before
    x.lookup(list(dict.fromkeys(h.keys)) + [b"user:absent"])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_randomised_against_the_model(torch, seed):
    rnd = random.Random(0xABCD00 + seed)
    pool = [bytes(rnd.choice(b"abcdefgh:_01") for _ in range(rnd.randint(1, 40))) for _ in range(600)]
    pool = list(dict.fromkeys(pool))
    absent = [k + b"~" for k in pool[:80]] + [b"~" + k for k in pool[:40]]
    count = 2000
    keys = [rnd.choice(pool) for _ in range(count)]
    for i in rnd.sample(range(count), 12):
        keys[i] = b""
    x = Index(torch, keys, 4096, shift=seed)
    cuts = sorted(rnd.sample(range(200, count - 200, 50), 5 if seed & 1 else 4)) + [count]
    first = 0
    for end in cuts:
        assert x.insert(first, end - first)[0] == OK
        x.lookup(pool + absent + [b""])
        x.delete(rnd.sample(range(end), 60))                           # items of this batch and of earlier ones
        x.lookup(pool + absent)
        first = end
    assert len(x.claimed) == int(x.used[0].item()) <= len(pool)
