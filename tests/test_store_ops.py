"""Locks, the lock-aware DEL, INC / DEC and the SET guard over the device store:
lzf_gpu_store_mlock, _munlock, _mdel, _minc and _set_guard against a Python
model that transcribes the reference's callbacks (src/query.c:778-800,
853-886, 898-940, 1015-1036, 1097-1114, 446-451), the lock rule (:171-178),
the validity rule (:186-189) and gbQueryParseLong (:39-76).  The parse rule is
also held against tests/golden/parse_long.json, the reference's own answers.
The bar is exact equality of every array, result word and per-entry output.

Every buffer a test hands over with a size is allocated larger and the excess
filled with a guard value, which is checked afterwards."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

try:                                    # before liblzf_hip.so loads: one HIP runtime in the process
    import torch as _torch  # noqa: F401
except ImportError:
    _torch = None

import gibson_amd
from tests.oracle_lib import ROOT

ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL = 0, 1, 2, 0xFF
DONE, DEAD, EXPIRED, LOCKED, NAN, CONVERTED, UNCHANGED = range(7)
OK, FULL = 0, 1
PAD = 0xFFFFFFFF
NEW_NAMES = ("lzf_gpu_store_mlock", "lzf_gpu_store_munlock", "lzf_gpu_store_mdel", "lzf_gpu_store_minc_work_size",
             "lzf_gpu_store_minc", "lzf_host_parse_long", "lzf_gpu_store_set_guard")
I64_MAX, I64_MIN = 2**63 - 1, -2**63


def wrap(x):
    """x modulo 2^64 as a signed 64-bit number"""
    x &= 2**64 - 1
    return x - 2**64 if x >= 2**63 else x


def parse_model(v):
    """gbQueryParseLong (src/query.c:39-76): the number, or None"""
    if not v:
        return None
    if v[0] == 0x30:
        return 0
    neg = v[0] == 0x2D
    n = 0
    for c in v[1 if neg else 0:]:
        if not 0x30 <= c <= 0x39:
            return None
        n = (n * 10 + c - 0x30) % 2**64
    return wrap(-n if neg else n)


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "parse_long.json")) as f:
        return [(bytes.fromhex(c["hex"]), c["value"] if c["ok"] else None) for c in json.load(f)["cases"]]


# ---- CPU ---------------------------------------------------------------------

def test_library_exports_the_lock_and_inc_calls():
    L = gibson_amd.lib()
    for n in NEW_NAMES:
        assert hasattr(L, n), n
        assert n in gibson_amd.lzf.EXPORTS
    for n in ("store_mlock", "store_munlock", "store_mdel", "store_minc", "store_minc_work", "store_set_guard",
              "parse_long"):
        assert callable(getattr(gibson_amd, n)), n
    assert (gibson_amd.ENT_DONE, gibson_amd.ENT_DEAD, gibson_amd.ENT_EXPIRED, gibson_amd.ENT_LOCKED,
            gibson_amd.ENT_NAN, gibson_amd.ENT_CONVERTED, gibson_amd.ENT_UNCHANGED) == (0, 1, 2, 3, 4, 5, 6)


def test_lock_and_inc_calls_reject_bad_arguments_without_device():
    # argument validation happens before any HIP call, so this runs on CPU;
    # only calls that must be refused are made (the pointers are host memory)
    L = gibson_amd.lib()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(512)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def mlock(ptrs, n=1, count=1):
        idx, enc, time, ttl, lock, last, est, result = ptrs
        return L.lzf_gpu_store_mlock(idx, n, 30, enc, count, time, ttl, lock, 5, last, est, result, null)

    def munlock(ptrs, n=1, count=1):
        idx, enc, time, ttl, lock, last, est, result = ptrs
        return L.lzf_gpu_store_munlock(idx, n, enc, count, time, ttl, lock, 5, last, est, result, null)

    for f in (mlock, munlock):
        for k in (0, 1, 2, 3, 4, 7):                 # a NULL in each required position: all three time arrays
            ptrs = [p] * 8
            ptrs[k] = null
            assert f(ptrs) == -1, (f.__name__, k)
        assert f([p, p, null, null, null, p, p, p]) == -1
        assert f([p, p, null, null, p, p, p, p]) == -1    # item_lock without item_time
        assert f([p] * 8, n=0) == -1
        assert f([p] * 8, count=0) == -1

    def mdel(ptrs, n=1, count=1):
        idx, enc, time, ttl, lock, est, result = ptrs
        return L.lzf_gpu_store_mdel(idx, n, enc, count, time, ttl, lock, 5, est, result, null)

    for k in (0, 1, 6):
        ptrs = [p] * 7
        ptrs[k] = null
        assert mdel(ptrs) == -1, k
    for k in (2, 3):                                 # exactly one NULL time array
        ptrs = [p] * 7
        ptrs[k] = null
        assert mdel(ptrs) == -1, k
        ptrs[4] = null
        assert mdel(ptrs) == -1, k
    assert mdel([p, p, null, null, p, p, p]) == -1   # item_lock without item_time
    assert mdel([p] * 7, n=0) == -1
    assert mdel([p] * 7, count=0) == -1

    def minc(ptrs, n=1, count=1):
        idx, store, used, voff, vsize, enc, time, ttl, lock, last, est, ev, result, status, work = ptrs
        return L.lzf_gpu_store_minc(idx, n, 1, 0, store, 64, used, voff, vsize, enc, count, time, ttl, lock, 5, last,
                                    est, ev, result, status, work, null)

    for k in (0, 1, 2, 3, 4, 5, 12, 13, 14):
        ptrs = [p] * 15
        ptrs[k] = null
        assert minc(ptrs) == -1, k
    for k in (6, 7):
        ptrs = [p] * 15
        ptrs[k] = null
        assert minc(ptrs) == -1, k
        ptrs[8] = null
        assert minc(ptrs) == -1, k
    ptrs = [p] * 15
    ptrs[6] = ptrs[7] = null                         # item_lock without item_time
    assert minc(ptrs) == -1
    assert minc([p] * 15, n=0) == -1
    assert minc([p] * 15, count=0) == -1

    def guard(ptrs, first=0, n=1, count=1):
        occ, enc, time, lock, refused, result = ptrs
        return L.lzf_gpu_store_set_guard(occ, first, n, enc, count, time, lock, 5, refused, result, null)

    for k in (0, 1, 2, 3, 5):
        ptrs = [p] * 6
        ptrs[k] = null
        assert guard(ptrs) == -1, k
    assert guard([p] * 6, n=0) == -1
    assert guard([p] * 6, count=0) == -1
    assert guard([p] * 6, first=1, n=1, count=1) == -1
    assert guard([p] * 6, first=2**32 - 1, n=2**32 - 1, count=2**32 - 1) == -1   # 64-bit first + n


def test_minc_work_size():
    ws = gibson_amd.lib().lzf_gpu_store_minc_work_size
    prev = 0
    for n in (1, 2, 1023, 1024, 1025, 3000, 262145, 1 << 20, (1 << 31) + 5, 2**32 - 2, 2**32 - 1):
        w = ws(n)
        assert w >= 9 * n and w >= prev, n
        prev = w
    assert 9 * (2**32 - 1) <= ws(2**32 - 1) < 2**40       # 64-bit arithmetic: no wrap


def test_parse_long_matches_the_reference_fixture():
    cases = fixture()
    assert len(cases) >= 200
    have = {v for v, _ in cases}
    for v in (b"0", b"0abc", b"007", b"-", b"-0", b"--1", b"+5", b"12a", b"9223372036854775807",
              b"9223372036854775808", b"-9223372036854775809"):
        assert v in have, v
    assert any(len(v) == 40 and v.isdigit() for v in have) and any(len(v) == 4096 and v.isdigit() for v in have)
    assert any(max(v) >= 0x80 for v in have) and any(0 in v for v in have)
    for v, exp in cases:
        assert parse_model(v) == exp, v[:40]
        assert gibson_amd.parse_long(v) == exp, v[:40]
    # by hand, from the rule's text
    assert dict(cases)[b"9223372036854775808"] == I64_MIN and dict(cases)[b"-9223372036854775809"] == I64_MAX
    assert dict(cases)[b"0abc"] == 0 and dict(cases)[b"-"] == 0 and dict(cases)[b"+5"] is None
    assert gibson_amd.parse_long(b"") is None
    L = gibson_amd.lib()
    out = ctypes.c_int64(77)
    assert L.lzf_host_parse_long(None, 0, ctypes.byref(out)) == 0
    assert L.lzf_host_parse_long(ctypes.c_char_p(b"5"), 0, ctypes.byref(out)) == 0 and out.value == 77


# ---- GPU ---------------------------------------------------------------------

FILL = 0xA5
GUARD = 0x5A
UNSET = -7
ROOM = 4096                              # guard bytes past every size
EXTRA = 16                               # guard elements past every per-item array
NOW = 1_700_000_000
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2500]
COUNT = 3000


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    gibson_amd.lib()
    return t


class Store:
    """a store on the host, the model's state: the arena's bytes up to `used`,
    the per-item arrays, the time arrays"""

    def __init__(self, values, encs, base=7):
        self.n = len(values)
        self.size = np.array([len(v) for v in values], np.uint32)
        self.off = (base + np.concatenate([[0], np.cumsum(self.size[:-1], dtype=np.uint64)])).astype(np.uint64)
        self.arena = np.frombuffer(bytes([FILL]) * base + b"".join(values), np.uint8).copy()
        self.used = len(self.arena)
        self.enc = np.array(encs, np.uint8)
        self.time = np.full(self.n, NOW, np.int64)
        self.ttl = np.zeros(self.n, np.int32)
        self.lock = np.zeros(self.n, np.int64)
        self.last = np.full(self.n, -1, np.int64)

    def copy(self):
        s = Store.__new__(Store)
        s.n, s.used = self.n, self.used
        for k in ("size", "off", "arena", "enc", "time", "ttl", "lock", "last"):
            setattr(s, k, getattr(self, k).copy())
        return s

    def validity(self, i, now, ttl=True):
        if i >= self.n or self.enc[i] == ENC_NULL:
            return DEAD
        if ttl and self.ttl[i] > 0 and wrap(now - int(self.time[i])) >= int(self.ttl[i]):
            return EXPIRED
        return DONE

    def locked(self, i, now, lock=True):
        """gbItemIsLocked, src/query.c:171-178"""
        return lock and (int(self.lock[i]) == -1 or wrap(now - int(self.time[i])) < int(self.lock[i]))

    def stored(self, i):
        return bytes(self.arena[int(self.off[i]):int(self.off[i]) + int(self.size[i])])

    def grow(self, to):
        if to > len(self.arena):
            self.arena = np.concatenate([self.arena, np.full(to - len(self.arena), FILL, np.uint8)])


def model_mlock(s, idx, lock_time, now):
    st, res = [], [0, 0, 0]
    for i in map(int, idx):
        v = s.validity(i, now)
        if v == DEAD:
            st.append(DEAD)
        elif v == EXPIRED:
            s.enc[i] = ENC_NULL
            st.append(EXPIRED)
            res[1] += 1
        elif s.locked(i, now):
            st.append(LOCKED)
            res[2] += 1
        else:
            s.time[i] = s.last[i] = now
            s.lock[i] = lock_time
            st.append(DONE)
            res[0] += 1
    return st, res


def model_munlock(s, idx, now):
    st, res = [], [0, 0]
    for i in map(int, idx):
        v = s.validity(i, now)
        if v == DEAD:
            st.append(DEAD)
        elif v == EXPIRED:
            s.enc[i] = ENC_NULL
            st.append(EXPIRED)
            res[1] += 1
        else:
            s.lock[i] = 0
            s.last[i] = now
            st.append(DONE)
            res[0] += 1
    return st, res


def model_mdel(s, idx, now, ttl=True, lock=True):
    st, res = [], [0, 0, 0]
    for i in map(int, idx):
        v = s.validity(i, now, ttl)
        if v == DEAD:
            st.append(DEAD)
        elif s.locked(i, now, lock):
            st.append(LOCKED)
            res[2] += 1
        elif v == EXPIRED:
            s.enc[i] = ENC_NULL
            st.append(EXPIRED)
            res[1] += 1
        else:
            s.enc[i] = ENC_NULL
            st.append(DONE)
            res[0] += 1
    return st, res


def in_arena(off, size, cap):
    return off <= cap and size <= cap - off


def model_minc(s, idx, delta, single, now, cap, ttl=True, lock=True):
    """-> (status, result, entry_status, entry_value); the two last None on FULL"""
    cls, val = [], []
    for i in map(int, idx):
        v = s.validity(i, now, ttl)
        c, x = None, 0
        if v == DEAD:
            c = DEAD
        elif single:
            c = EXPIRED if v == EXPIRED else LOCKED if s.locked(i, now, lock) else None
        else:
            c = LOCKED if s.locked(i, now, lock) else EXPIRED if v == EXPIRED else None
        if c is None:
            e, off, size = int(s.enc[i]), int(s.off[i]), int(s.size[i])
            if e == ENC_NUMBER:
                if size == 8 and in_arena(off, 8, cap):
                    c, x = DONE, wrap(int.from_bytes(bytes(s.arena[off:off + 8]), "little", signed=True) + delta)
                else:
                    c = NAN
            elif e == ENC_PLAIN:
                p = parse_model(bytes(s.arena[off:off + size])) if size and in_arena(off, size, cap) else None
                c, x = (NAN, 0) if p is None else (CONVERTED, wrap(p + delta))
            else:
                c = NAN if single else UNCHANGED
        cls.append(c)
        val.append(x)
    conv = cls.count(CONVERTED)
    if s.used + 8 * conv > cap or s.used + 8 * conv >= 2**64:
        return FULL, [0] * 6, None, None
    base, rank = s.used, 0
    s.grow(base + 8 * conv)
    for i, c, x in zip(map(int, idx), cls, val):
        if c == EXPIRED:
            s.enc[i] = ENC_NULL
        if c in (DONE, CONVERTED, NAN, UNCHANGED):
            s.last[i] = now
        if c == DONE:
            o = int(s.off[i])
            s.arena[o:o + 8] = np.frombuffer(x.to_bytes(8, "little", signed=True), np.uint8)
        if c == CONVERTED:
            o = base + 8 * rank
            rank += 1
            s.arena[o:o + 8] = np.frombuffer(x.to_bytes(8, "little", signed=True), np.uint8)
            s.off[i], s.size[i], s.enc[i] = o, 8, ENC_NUMBER
    s.used = base + 8 * conv
    res = [cls.count(DONE) + conv + cls.count(UNCHANGED), cls.count(EXPIRED), cls.count(LOCKED), cls.count(NAN), conv,
           cls.count(UNCHANGED)]
    return OK, res, cls, val


def _padded(torch, a, guard):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(np.concatenate([a, np.full(EXTRA, guard, a.dtype)])).cuda()


class Dev:
    """the model's state on the device, every array followed by guard
    elements; `cap` is the arena's size as the calls are told it"""

    def __init__(self, torch, s, cap):
        self.t, self.n, self.cap = torch, s.n, cap
        s = s.copy()
        s.grow(cap)
        self.arena = torch.from_numpy(np.concatenate([s.arena[:cap], np.full(ROOM, GUARD, np.uint8)])).cuda()
        self.used = torch.tensor([s.used] + [UNSET] * 3, dtype=torch.int64, device="cuda")
        self.off = _padded(torch, s.off.view(np.int64), UNSET)
        self.size = _padded(torch, s.size.view(np.int32), UNSET)
        self.enc = _padded(torch, s.enc, GUARD)
        self.time = _padded(torch, s.time, UNSET)
        self.ttl = _padded(torch, s.ttl, UNSET)
        self.lock = _padded(torch, s.lock, UNSET)
        self.last = _padded(torch, s.last, UNSET)

    def a(self, name):
        """the array as the calls get it, without its guard elements"""
        return getattr(self, name)[:self.cap if name == "arena" else self.n]

    def check(self, s):
        """every array equals the model's, and every guard is intact"""
        self.t.cuda.synchronize()
        s = s.copy()
        s.grow(self.cap)
        exp = {"arena": np.concatenate([s.arena[:self.cap], np.full(ROOM, GUARD, np.uint8)]),
               "used": np.array([s.used] + [UNSET] * 3, np.int64)}
        for k, g in (("off", UNSET), ("size", UNSET), ("enc", GUARD), ("time", UNSET), ("ttl", UNSET),
                     ("lock", UNSET), ("last", UNSET)):
            a = getattr(s, k)
            a = a.view(np.int64) if k == "off" else a.view(np.int32) if k == "size" else a
            exp[k] = np.concatenate([a, np.full(EXTRA, g, a.dtype)])
        for k, e in exp.items():
            got = getattr(self, k).cpu().numpy()
            bad = np.nonzero(got != e)[0]
            assert not len(bad), (k, len(bad), "first at", int(bad[0]), int(got[bad[0]]), int(e[bad[0]]))


class Out:
    """the per-call outputs, guarded"""

    def __init__(self, torch, n, words):
        self.t, self.n, self.words = torch, n, words
        self.est = torch.full((n + ROOM,), 0x77, dtype=torch.uint8, device="cuda")
        self.ev = torch.full((n + EXTRA,), UNSET, dtype=torch.int64, device="cuda")
        self.result = torch.full((words + 4,), UNSET, dtype=torch.int64, device="cuda")
        self.status = torch.full((5,), UNSET, dtype=torch.int32, device="cuda")
        self.wsize = int(gibson_amd.lib().lzf_gpu_store_minc_work_size(n))
        self.work = torch.full((self.wsize + ROOM,), GUARD, dtype=torch.uint8, device="cuda")

    def check(self, result, st, val=None, status=None, tag=""):
        self.t.cuda.synchronize()
        got = self.result.cpu().numpy().tolist()
        print(tag, "n", self.n, "result", got[:self.words], "expected", result, "status",
              int(self.status[0].item()), status)
        assert got == list(result) + [UNSET] * 4
        est = self.est.cpu().numpy()
        assert (est[:self.n] == (np.array(st, np.uint8) if st is not None else 0x77)).all()
        assert (est[self.n:] == 0x77).all()
        ev = self.ev.cpu().numpy()
        assert ev[:self.n].tolist() == (list(val) if val is not None else [UNSET] * self.n)
        assert (ev[self.n:] == UNSET).all()
        assert self.status.cpu().numpy().tolist() == [UNSET if status is None else status] + [UNSET] * 4
        assert (self.work[self.wsize:].cpu().numpy() == GUARD).all()


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def le64(x):
    return int(x).to_bytes(8, "little", signed=True)


def mixed_store(seed=0x10C5):
    """COUNT items of every kind, densely packed from an odd offset, with TTLs
    and locks of every kind"""
    rnd = random.Random(seed)
    values, encs = [], []
    for _ in range(COUNT):
        kind = rnd.choice("NNNNNNddddddttzmLLLxxx")
        if kind == "N":
            values.append(le64(rnd.choice([0, 1, -1, I64_MAX, I64_MIN, rnd.randrange(I64_MIN, I64_MAX)])))
            encs.append(ENC_NUMBER)
        elif kind == "d":
            values.append(bytes(rnd.choice(b"123456789") for _ in range(rnd.choice([1, 2, 5, 9, 18, 19, 20, 30]))))
            encs.append(ENC_PLAIN)
        elif kind == "t":
            values.append(bytes(rnd.choice(b"abc 0123456789-+") for _ in range(rnd.randint(1, 24))))
            encs.append(ENC_PLAIN)
        elif kind == "z":
            values.append(rnd.choice([b"0", b"0abc", b"007", b"-", b"-0", b"-42", b"", b"--1"]))
            encs.append(ENC_PLAIN)
        elif kind == "m":                                # a number whose size is not 8: never read
            values.append(bytes(rnd.randrange(256) for _ in range(rnd.choice([0, 7, 9]))))
            encs.append(ENC_NUMBER)
        elif kind == "L":                                # the bytes of an LZF item are never looked at
            values.append(bytes(rnd.randrange(256) for _ in range(rnd.randint(1, 40))))
            encs.append(ENC_LZF)
        else:
            values.append(bytes(rnd.randrange(256) for _ in range(rnd.randint(0, 12))))
            encs.append(ENC_NULL)
    s = Store(values, encs)
    rs = np.random.RandomState(seed & 0xFFFF)
    age = rs.randint(0, 1200, COUNT).astype(np.int64)
    s.time = NOW - age
    s.ttl = rs.choice([-1, 0, 5, 600, 32767], COUNT).astype(np.int32)
    # unlocked; for good; a future lock; an elapsed lock; a negative value other than -1
    pick = rs.choice(5, COUNT, p=[0.4, 0.15, 0.15, 0.15, 0.15])
    s.lock = np.select([pick == 0, pick == 1, pick == 2, pick == 3], [0, -1, age + 1 + rs.randint(0, 90, COUNT), age],
                       -5 - rs.randint(0, 90, COUNT)).astype(np.int64)
    return s


@pytest.fixture(scope="module")
def mixed():
    s = mixed_store()
    every = list(range(COUNT))
    st = model_minc(s.copy(), every, 1, 0, NOW, 1 << 40)[2]
    assert min(st.count(c) for c in range(7)) >= 60, [st.count(c) for c in range(7)]
    both = [i for i in every if s.validity(i, NOW) == EXPIRED and s.locked(i, NOW)]
    assert len(both) >= 60                               # locked and expired: the order of the tests shows
    return s


def mixed_list(s, n, seed):
    """distinct items of every kind, with padding and out-of-range entries, shuffled"""
    rs = np.random.RandomState(seed)
    junk = n // 10
    idx = rs.choice(s.n, n - junk, replace=False).astype(np.uint32)
    idx = np.concatenate([idx, rs.choice([PAD, s.n, s.n + 1, 2**31 + 3], junk).astype(np.uint32)])
    rs.shuffle(idx)
    return idx


# 1
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_random_mix_of_every_operator(torch, mixed, n):
    idx = mixed_list(mixed, n, 0x51 + n)
    d_idx = _i32(torch, idx)
    cap = mixed.used + 8 * n + 5

    s, d, o = mixed.copy(), Dev(torch, mixed, cap), Out(torch, n, 3)
    st, res = model_mlock(s, idx, 300, NOW)
    gibson_amd.store_mlock(d_idx, 300, d.a("enc"), d.a("time"), d.a("ttl"), d.a("lock"), NOW, o.result[:3],
                           last_access=d.a("last"), entry_status=o.est[:n])
    o.check(res, st, tag="mlock")
    d.check(s)

    s, d, o = mixed.copy(), Dev(torch, mixed, cap), Out(torch, n, 2)
    st, res = model_munlock(s, idx, NOW)
    gibson_amd.store_munlock(d_idx, d.a("enc"), d.a("time"), d.a("ttl"), d.a("lock"), NOW, o.result[:2],
                             last_access=d.a("last"), entry_status=o.est[:n])
    o.check(res, st, tag="munlock")
    d.check(s)

    s, d, o = mixed.copy(), Dev(torch, mixed, cap), Out(torch, n, 3)
    st, res = model_mdel(s, idx, NOW)
    gibson_amd.store_mdel(d_idx, d.a("enc"), d.a("time"), d.a("ttl"), d.a("lock"), NOW, o.result[:3],
                          entry_status=o.est[:n])
    o.check(res, st, tag="mdel")
    d.check(s)

    for single, delta in ((False, 1), (True, -1)):
        s, d, o = mixed.copy(), Dev(torch, mixed, cap), Out(torch, n, 6)
        status, res, st, val = model_minc(s, idx, delta, single, NOW, cap)
        assert status == OK
        gibson_amd.store_minc(d_idx, delta, d.a("arena"), d.used[:1], d.a("off"), d.a("size"), d.a("enc"),
                              d.a("time"), d.a("ttl"), d.a("lock"), NOW, o.result[:6], o.status[:1], single=single,
                              last_access=d.a("last"), entry_status=o.est[:n], entry_value=o.ev[:n],
                              work=o.work[:o.wsize])
        o.check(res, st, val, OK, tag="minc single=%d" % single)
        d.check(s)

    # the optional outputs left out, and no lock and no time arrays
    s, d, o = mixed.copy(), Dev(torch, mixed, cap), Out(torch, n, 6)
    status, res, st, val = model_minc(s, idx, 7, False, NOW, cap, ttl=False, lock=False)
    s.last = mixed.last.copy()
    gibson_amd.store_minc(d_idx, 7, d.a("arena"), d.used[:1], d.a("off"), d.a("size"), d.a("enc"), None, None, None,
                          NOW, o.result[:6], o.status[:1], work=o.work[:o.wsize])
    o.check(res, None, None, OK, tag="minc bare")
    d.check(s)


def model_guard(s, occ, first, now):
    refused = []
    for k, j in enumerate(map(int, occ)):
        r = (j < s.n and not first <= j < first + len(occ) and s.enc[j] != ENC_NULL and s.locked(j, now))
        if r:
            s.enc[first + k] = ENC_NULL
        refused.append(1 if r else 0)
    return refused


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_random_mix_set_guard(torch, mixed, n):
    rs = np.random.RandomState(0x6A + n)
    first = int(rs.randint(0, COUNT - n + 1))
    occ = rs.choice(np.concatenate([np.arange(COUNT + 40), [PAD] * 300]), n).astype(np.uint32)
    s, d, o = mixed.copy(), Dev(torch, mixed, mixed.used), Out(torch, n, 1)
    s.enc[first:first + n] = ENC_PLAIN                   # the batch's own items are live
    d.enc[first:first + n] = ENC_PLAIN
    refused = model_guard(s, occ, first, NOW)
    if n > 60:
        assert 0 < sum(refused) < n
    gibson_amd.store_set_guard(_i32(torch, occ), first, d.a("enc"), d.a("time"), d.a("lock"), NOW, o.result[:1],
                               refused=o.est[:n])
    o.check([sum(refused)], refused, tag="set_guard")
    d.check(s)
    # without the optional output
    d2, o2 = Dev(torch, mixed, mixed.used), Out(torch, n, 1)
    d2.enc[first:first + n] = ENC_PLAIN
    gibson_amd.store_set_guard(_i32(torch, occ), first, d2.a("enc"), d2.a("time"), d2.a("lock"), NOW, o2.result[:1])
    o2.check([sum(refused)], None, tag="set_guard bare")
    d2.check(s)


# 2
@pytest.mark.gpu
def test_check_order_on_a_locked_and_expired_entry(torch):
    s0 = Store([le64(5), b"12", b"zz", le64(9)], [ENC_NUMBER, ENC_PLAIN, ENC_LZF, ENC_NUMBER])
    s0.time[:] = NOW - 100
    s0.ttl[:] = 50                                       # expired
    s0.lock[:] = [-1, 1000, -1, 0]                       # the first three locked as well
    idx = np.arange(4, dtype=np.uint32)
    d_idx = _i32(torch, idx)
    cap = s0.used + 64

    def run(op):
        s, d, o = s0.copy(), Dev(torch, s0, cap), Out(torch, 4, 6)
        if op == "mlock":
            st, res = model_mlock(s, idx, 7, NOW)
            gibson_amd.store_mlock(d_idx, 7, d.a("enc"), d.a("time"), d.a("ttl"), d.a("lock"), NOW, o.result[:3],
                                   last_access=d.a("last"), entry_status=o.est[:4])
        elif op == "munlock":
            st, res = model_munlock(s, idx, NOW)
            gibson_amd.store_munlock(d_idx, d.a("enc"), d.a("time"), d.a("ttl"), d.a("lock"), NOW, o.result[:2],
                                     last_access=d.a("last"), entry_status=o.est[:4])
        elif op == "mdel":
            st, res = model_mdel(s, idx, NOW)
            gibson_amd.store_mdel(d_idx, d.a("enc"), d.a("time"), d.a("ttl"), d.a("lock"), NOW, o.result[:3],
                                  entry_status=o.est[:4])
        else:
            single = op == "inc"
            _, res, st, _ = model_minc(s, idx, 1, single, NOW, cap)
            gibson_amd.store_minc(d_idx, 1, d.a("arena"), d.used[:1], d.a("off"), d.a("size"), d.a("enc"), d.a("time"),
                                  d.a("ttl"), d.a("lock"), NOW, o.result[:6], o.status[:1], single=single,
                                  last_access=d.a("last"), entry_status=o.est[:4], work=o.work[:o.wsize])
        torch.cuda.synchronize()
        got = o.est[:4].cpu().numpy().tolist()
        assert got == st
        assert o.result.cpu().numpy().tolist()[:len(res)] == res
        d.check(s)
        return got, d.enc[:4].cpu().numpy().tolist()

    # by hand: MDEL and MINC leave it, the others null it
    live = [ENC_NUMBER, ENC_PLAIN, ENC_LZF]
    assert run("mdel") == ([LOCKED, LOCKED, LOCKED, EXPIRED], live + [ENC_NULL])
    assert run("minc") == ([LOCKED, LOCKED, LOCKED, EXPIRED], live + [ENC_NULL])
    for op in ("mlock", "munlock", "inc"):
        assert run(op) == ([EXPIRED] * 4, [ENC_NULL] * 4), op


def run_minc(torch, s0, idx, delta, cap, single=False, status=OK):
    """one store_minc call over s0 against the model; -> (model state, classes, values, Dev)"""
    n = len(idx)
    s, d, o = s0.copy(), Dev(torch, s0, cap), Out(torch, n, 6)
    exp_status, res, st, val = model_minc(s, idx, delta, single, NOW, cap)
    assert exp_status == status
    gibson_amd.store_minc(_i32(torch, idx), delta, d.a("arena"), d.used[:1], d.a("off"), d.a("size"), d.a("enc"),
                          d.a("time"), d.a("ttl"), d.a("lock"), NOW, o.result[:6], o.status[:1], single=single,
                          last_access=d.a("last"), entry_status=o.est[:n], entry_value=o.ev[:n],
                          work=o.work[:o.wsize])
    o.check(res, st, val, status, tag="minc")
    d.check(s)
    return s, st, val, d


# 3
@pytest.mark.gpu
def test_parse_on_the_device_matches_the_fixture(torch):
    cases = fixture()
    s0 = Store([v for v, _ in cases], [ENC_PLAIN] * len(cases), base=3)
    idx = np.arange(len(cases), dtype=np.uint32)
    s, st, val, d = run_minc(torch, s0, idx, 0, s0.used + 8 * len(cases))
    arena = d.arena.cpu().numpy()
    off = d.off.cpu().numpy()
    for k, (v, exp) in enumerate(cases):
        assert st[k] == (NAN if exp is None else CONVERTED), v[:40]
        if exp is not None:
            assert val[k] == exp and bytes(arena[off[k]:off[k] + 8]) == le64(exp), v[:40]


# 4
@pytest.mark.gpu
def test_deltas_on_numbers_at_unaligned_offsets(torch):
    nums = [0, 1, -1, I64_MAX, I64_MIN, I64_MAX - 32766, I64_MIN + 32766, 0x0123456789ABCDEF, -0x0123456789ABCDEF]
    values, encs = [], []
    for k, x in enumerate(nums * 3):                     # odd gaps: every offset modulo 8
        values += [le64(x), b"x" * (1 + k % 3)]
        encs += [ENC_NUMBER, ENC_LZF]
    s0 = Store(values, encs, base=1)
    assert {int(o) % 8 for o in s0.off[::2]} == set(range(8))
    idx = np.arange(0, len(values), 2, dtype=np.uint32)
    for delta in (1, -1, 32767, -32767):
        s, st, val, _ = run_minc(torch, s0, idx, delta, s0.used)
        assert st == [DONE] * len(idx)
        assert val == [wrap(x + delta) for x in nums * 3]
    s, st, val, _ = run_minc(torch, s0, idx[3:5], 1, s0.used)
    assert val[0] == I64_MIN                             # INT64_MAX + 1 wraps
    s, st, val, _ = run_minc(torch, s0, idx[3:5], -1, s0.used)
    assert val[1] == I64_MAX


# 5
@pytest.mark.gpu
def test_lzf_items(torch):
    s0 = Store([b"\x01ab", le64(4), b"\x02xyz"], [ENC_LZF, ENC_NUMBER, ENC_LZF], base=2)
    idx = np.array([2, 1, 0], np.uint32)
    s, st, val, d = run_minc(torch, s0, idx, 1, s0.used)
    assert st == [UNCHANGED, DONE, UNCHANGED] and val == [0, 5, 0]      # counted as found: result[0] == 3 in the model
    assert s.last.tolist() == [NOW] * 3
    s, st, val, d = run_minc(torch, s0, idx, 1, s0.used, single=True)
    assert st == [NAN, DONE, NAN]
    assert s.last.tolist() == [NOW] * 3                  # :861 comes before the value test


# 6
@pytest.mark.gpu
def test_converted_offsets_follow_the_list_order(torch):
    rnd = random.Random(0x0FF5)
    values = [b"%d" % rnd.randrange(-10**9, 10**9) for _ in range(COUNT)]
    s0 = Store(values, [ENC_PLAIN] * COUNT)
    idx = np.random.RandomState(0x0FF5).permutation(COUNT)[:2500].astype(np.uint32)
    s, st, val, d = run_minc(torch, s0, idx, 3, s0.used + 8 * 2500)
    off = d.off.cpu().numpy()
    assert st == [CONVERTED] * 2500
    assert [int(off[i]) for i in idx] == [s0.used + 8 * r for r in range(2500)]
    assert val == [int(values[i]) + 3 for i in idx]
    assert int(d.used[0].item()) == s0.used + 8 * 2500
    # a list with NUMBER items and text between the converted ones: the rank counts the converted only
    s1 = s0.copy()
    s1.enc[::3] = ENC_LZF
    s, st, val, d = run_minc(torch, s1, idx, 3, s0.used + 8 * 2500)
    off = d.off.cpu().numpy()
    conv = [int(i) for i in idx if i % 3]
    assert 1024 < len(conv) < 2500
    assert [int(off[i]) for i in conv] == [s0.used + 8 * r for r in range(len(conv))]


@pytest.mark.gpu
def test_list_past_one_piece_of_the_tile_scan(torch):
    # 2 048 tiles of 1 024 entries are one piece of the scan over the tile counts; the carry between
    # pieces shows only past that.  Mostly padding, with entries at both ends and around the seam
    seam = 2048 * 1024
    n = seam + 1025
    rnd = random.Random(0x5EA2)
    where = {0, 1, 1023, 1024, seam - 1, seam, seam + 1, n - 1}
    where |= set(rnd.sample(range(2, seam - 1), 150)) | set(rnd.sample(range(seam + 2, n - 1), 150))
    where = np.array(sorted(where))
    values, encs = [], []
    for k in range(len(where)):
        kind = "numeric" if k < 8 else rnd.choice(["numeric"] * 4 + ["number", "text", "dead"])
        if kind == "numeric":
            values.append(b"%d" % rnd.randrange(-10**9, 10**9))
        elif kind == "number":
            values.append(le64(rnd.randrange(-10**9, 10**9)))
        else:
            values.append(b"x%d" % k)
        encs.append(ENC_NUMBER if kind == "number" else ENC_NULL if kind == "dead" else ENC_PLAIN)
    s0 = Store(values, encs)
    items = np.random.RandomState(0x5EA2).permutation(len(where)).astype(np.uint32)   # list order is not item order
    idx = np.full(n, PAD, np.uint32)
    idx[where] = items
    cap = s0.used + 8 * len(where)
    # the model over the real entries alone: a padding entry is DEAD, its value 0, and counts nowhere
    s = s0.copy()
    status, res, st, val = model_minc(s, items, 5, False, NOW, cap)
    assert status == OK and {DONE, CONVERTED, NAN, DEAD} <= set(st)
    conv = [k for k in range(len(where)) if st[k] == CONVERTED]
    assert sum(1 for k in conv if where[k] >= seam) > 50           # ranks that need the carry
    exp_st = np.full(n, DEAD, np.uint8)
    exp_st[where] = st
    exp_val = np.zeros(n, np.int64)
    exp_val[where] = val
    d, o = Dev(torch, s0, cap), Out(torch, n, 6)
    gibson_amd.store_minc(_i32(torch, idx), 5, d.a("arena"), d.used[:1], d.a("off"), d.a("size"), d.a("enc"),
                          d.a("time"), d.a("ttl"), d.a("lock"), NOW, o.result[:6], o.status[:1],
                          last_access=d.a("last"), entry_status=o.est[:n], entry_value=o.ev[:n], work=o.work[:o.wsize])
    d.check(s)                                                     # values, descriptors, *store_used, the guards
    off = d.off.cpu().numpy()
    assert [int(off[items[k]]) for k in conv] == [s0.used + 8 * r for r in range(len(conv))]
    assert int(d.used[0].item()) == s0.used + 8 * len(conv)
    assert o.result.cpu().numpy().tolist() == res + [UNSET] * 4
    assert o.status.cpu().numpy().tolist() == [OK] + [UNSET] * 4
    est, ev = o.est.cpu().numpy(), o.ev.cpu().numpy()
    assert (est[:n] == exp_st).all() and (est[n:] == 0x77).all()
    assert (ev[:n] == exp_val).all() and (ev[n:] == UNSET).all()
    assert (o.work[o.wsize:].cpu().numpy() == GUARD).all()


# 7
@pytest.mark.gpu
def test_full_boundary(torch, mixed):
    idx = mixed_list(mixed, 1025, 0xF011)
    conv = model_minc(mixed.copy(), idx, 1, False, NOW, 1 << 40)[2].count(CONVERTED)
    assert conv > 100
    run_minc(torch, mixed, idx, 1, mixed.used + 8 * conv)             # exactly fits
    # one byte less: refused whole.  run_minc holds every array, *store_used and the
    # optional outputs to their values before the call, and result to zero
    s, st, val, d = run_minc(torch, mixed, idx, 1, mixed.used + 8 * conv - 1, status=FULL)
    assert st is None and val is None and s.used == mixed.used
    assert (s.enc == mixed.enc).all() and (s.last == mixed.last).all()
    # *store_used already past the cap, and nothing to convert
    s0 = Store([le64(1)], [ENC_NUMBER])
    run_minc(torch, s0, np.array([0], np.uint32), 1, s0.used - 1, status=FULL)


# 8
@pytest.mark.gpu
def test_malformed_items_are_not_dereferenced(torch):
    s0 = Store([le64(1), le64(2)[:7], le64(3), b"1234", b"5678", le64(4), b"99"],
               [ENC_NUMBER, ENC_NUMBER, ENC_NUMBER, ENC_PLAIN, ENC_PLAIN, ENC_NUMBER, ENC_PLAIN], base=5)
    cap = s0.used + 32
    s0.off[2] = cap - 7                                  # a number whose last byte leaves the arena
    s0.off[4] = cap - 3                                  # text that does
    s0.off[5] = 2**64 - 4                                # off + 8 wraps
    s0.off[6] = cap + 1
    s0.size[6] = 0xFFFFFFFF
    idx = np.arange(7, dtype=np.uint32)
    for single in (False, True):
        s, st, val, d = run_minc(torch, s0, idx, 1, cap, single=single)
        assert st == [DONE, NAN, NAN, CONVERTED, NAN, NAN, NAN]
        assert val == [2, 0, 0, 1235, 0, 0, 0]
    # at the very end of the arena they are in range
    s1 = s0.copy()
    s1.off[2], s1.off[4] = cap - 8, cap - 4
    s1.grow(cap)
    s1.arena[cap - 8:cap] = np.frombuffer(b"\0\0\0\0" + b"4321", np.uint8)
    s, st, val, d = run_minc(torch, s1, idx[:5], 1, cap)
    assert st == [DONE, NAN, DONE, CONVERTED, CONVERTED] and val[4] == 4322


# 9
@pytest.mark.gpu
def test_set_lookup_minc_mget_compact_loop(torch, oracle):
    from tests.test_key_index import Index
    from tests.test_store_mget import Dev as MgetDev, Host, Mget, build_store, expect_frame
    from tests.oracle_lib import synth
    rnd = random.Random(0x100B)
    values, keys = [], []
    for i in range(300):
        kind = i % 4
        if kind == 0:
            values.append(b"%d" % rnd.randrange(-10**12, 10**12))
        elif kind == 1:
            values.append(b"%d" % rnd.randrange(0, 100))
        elif kind == 2:
            values.append(synth(0, 0x100B, i, rnd.randint(3, 60)))     # text, stays PLAIN
        else:
            values.append(synth(1, 0x100B, i, rnd.randint(200, 900)))  # compresses
        keys.append(b"ctr:%d:%s" % (i, bytes(rnd.choice(b"abc") for _ in range(rnd.randint(0, 9)))))
    h = build_store(torch, values, 64, keys)
    assert (h.enc == ENC_LZF).sum() >= 40 and (h.enc == ENC_PLAIN).sum() >= 200
    used = len(h.arena)
    cap = used + 8 * h.n
    d = MgetDev(torch, h)
    arena = torch.from_numpy(np.concatenate([h.arena, np.full(cap - used, FILL, np.uint8),
                                             np.full(ROOM, GUARD, np.uint8)])).cuda()
    x = Index(torch, h.keys, 1024, dev=(d.keys, d.koff, d.klen, d.enc))
    x.insert(0, h.n)
    query = [keys[i] for i in rnd.sample(range(h.n), 200)] + [b"ctr:absent"]
    idx = x.lookup(query)
    want = [x.model_lookup(q) for q in query]
    # the model over the same list
    s = Store.__new__(Store)
    s.n, s.used = h.n, used
    s.arena, s.off, s.size, s.enc = h.arena.copy(), h.off.astype(np.uint64), h.size.astype(np.uint32), h.enc.copy()
    s.time, s.ttl, s.lock = np.full(h.n, NOW, np.int64), np.zeros(h.n, np.int32), np.zeros(h.n, np.int64)
    s.last = np.full(h.n, -1, np.int64)
    status, res, st, val = model_minc(s, want, 5, False, NOW, cap, ttl=False, lock=False)
    assert status == OK and res[4] >= 60 and res[5] >= 20 and res[3] >= 20
    o = Out(torch, len(query), 6)
    d_used = torch.tensor([used], dtype=torch.int64, device="cuda")
    gibson_amd.store_minc(idx, 5, arena[:cap], d_used, d.off, d.size, d.enc, None, None, None, NOW, o.result[:6],
                          o.status[:1], last_access=d.last, entry_status=o.est[:len(query)],
                          entry_value=o.ev[:len(query)], work=o.work[:o.wsize])
    o.check(res, st, val, OK, tag="loop minc")
    assert int(d_used.item()) == s.used == used + 8 * res[4]
    assert (d.off.cpu().numpy().view(np.uint64) == s.off).all() and (d.enc.cpu().numpy() == s.enc).all()
    # MGET over the same list: the frame of the model's items, the NUMBER items included
    s.grow(cap)
    hm = Host(s.arena[:s.used], s.off.astype(np.int64), s.size, s.enc, h.vlen, h.keys)
    valid = [i for i in want if i != PAD]
    assert sum(1 for i in valid if hm.enc[i] == ENC_NUMBER) == res[4]
    exp = expect_frame(oracle, hm, valid, 64 << 20, True)
    r1 = Mget(torch, d, idx, len(exp) + 9, arena=arena[:cap])
    r1.check(torch, exp, [len(valid), 0, 1, 0])
    # compact, then the same MGET from the second arena
    dst = torch.full((cap + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
    dst_used = torch.zeros(1, dtype=torch.int64, device="cuda")
    report = torch.zeros(4, dtype=torch.int64, device="cuda")
    cstatus = torch.full((1,), UNSET, dtype=torch.int32, device="cuda")
    w = gibson_amd.store_compact(arena[:cap], d.off, d.size, d.enc, dst[:cap], dst_used, report, cstatus)
    r2 = Mget(torch, d, idx, len(exp) + 9, arena=dst[:cap])
    r2.check(torch, exp, [len(valid), 0, 1, 0])
    del w
    assert int(cstatus.item()) == OK
    live = int(s.size.astype(np.int64).sum())
    plain_gone = sum(len(values[i]) for i, c in zip(want, st) if c == CONVERTED)
    assert int(dst_used.item()) == live == used - 7 - plain_gone + 8 * res[4]      # the old PLAIN bytes are gone
    usage = torch.zeros(4, dtype=torch.int64, device="cuda")
    w = gibson_amd.store_usage(d.size, d.enc, usage)
    torch.cuda.synchronize()
    del w
    assert usage.cpu().numpy().tolist() == [h.n, live, 0, 0]
    assert (dst[cap:].cpu().numpy() == GUARD).all() and (arena[cap:].cpu().numpy() == GUARD).all()


# 10
@pytest.mark.gpu
def test_set_against_a_locked_key(torch):
    from tests.test_key_index import Index
    from tests.test_store_mget import Dev as MgetDev, build_store
    old = [b"k:forever", b"k:future", b"k:free", b"k:elapsed", b"k:other"]
    new = [b"k:forever", b"k:free", b"k:forever", b"k:future", b"k:elapsed", b"k:new", b"k:new"]
    keys = old + new
    m, nb = len(old), len(new)
    h = build_store(torch, [b"value-%d" % i for i in range(len(keys))], 64, keys)    # the SET of both batches
    d = MgetDev(torch, h)
    time = torch.full((h.n,), NOW - 100, dtype=torch.int64, device="cuda")
    lock = torch.tensor([-1, 500, 0, 100, -1] + [0] * nb, dtype=torch.int64, device="cuda")
    x = Index(torch, h.keys, 64, dev=(d.keys, d.koff, d.klen, d.enc))
    x.insert(0, m)
    occ = x.lookup(new)
    assert occ.cpu().numpy().view(np.uint32).tolist() == [0, 2, 0, 1, 3, PAD, PAD]
    o = Out(torch, nb, 1)
    gibson_amd.store_set_guard(occ, m, d.enc, time, lock, NOW, o.result[:1], refused=o.est[:nb])
    # two batch items on one locked key are both refused; the elapsed lock and the free key let the SET through
    o.check([3], [1, 0, 1, 1, 0, 0, 0], tag="set_guard")
    for k in (0, 2, 3):
        x.m_enc[m + k] = ENC_NULL                        # the refused items are dead
    assert x.insert(m, nb) == (0, [3, 2, 1, 3])          # mapped, replaced, superseded, skipped
    after = x.lookup([b"k:forever", b"k:future", b"k:free", b"k:elapsed", b"k:new", b"k:other"])
    # the lookup still returns the old item of a locked key; an unlocked key is replaced as before
    assert after.cpu().numpy().view(np.uint32).tolist() == [0, 1, m + 1, m + 4, m + 6, 4]
    # an occupant inside the batch range is ignored, locked or not
    lock[m + 1] = -1
    occ = x.lookup(new)
    assert occ.cpu().numpy().view(np.uint32).tolist() == [0, m + 1, 0, 1, m + 4, m + 6, m + 6]
    enc_before = d.enc.cpu().numpy().copy()
    o = Out(torch, nb, 1)
    gibson_amd.store_set_guard(occ, m, d.enc, time, lock, NOW, o.result[:1], refused=o.est[:nb])
    o.check([3], [1, 0, 1, 1, 0, 0, 0], tag="set_guard again")
    assert (d.enc.cpu().numpy() == enc_before).all()     # the refused ones were dead already


# 11
@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 2500])
def test_mdel_equals_count_then_delete_without_locks(torch, mixed, n):
    idx = mixed_list(mixed, n, 0xDE1 + n)
    d_idx = _i32(torch, idx)
    a, b = Dev(torch, mixed, mixed.used), Dev(torch, mixed, mixed.used)
    o = Out(torch, n, 3)
    gibson_amd.store_mdel(d_idx, a.a("enc"), a.a("time"), a.a("ttl"), None, NOW, o.result[:3], entry_status=o.est[:n])
    cnt = torch.full((2,), UNSET, dtype=torch.int64, device="cuda")
    gibson_amd.store_count(d_idx, b.a("enc"), b.a("time"), b.a("ttl"), NOW, cnt)
    gibson_amd.store_delete(d_idx, b.a("enc"))
    s = mixed.copy()
    st, res = model_mdel(s, idx, NOW, lock=False)
    o.check(res, st, tag="mdel")
    a.check(s)
    assert (a.enc.cpu().numpy() == b.enc.cpu().numpy()).all()
    assert cnt.cpu().numpy().tolist() == res[:2] and res[2] == 0
