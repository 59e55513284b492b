"""The device store's renumbering (lzf_gpu_store_renumber, _remap) and the key
index's rebuild (lzf_gpu_key_index_rebuild): the live items copied dense and in
order into a second set of item arrays, their keys packed into a second arena,
against numpy over the arrays read back.  The bar is bit-exact.

Every destination array and arena is a view into a larger tensor whose excess,
in front and behind, holds a guard byte that is checked afterwards; what a call
must not write keeps its fill byte; the source arrays are checked unchanged."""
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

ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL = 0, 1, 2, 0xFF
OK, FULL, ERANGE = 0, 1, 3
PAD = 0xFFFFFFFF
NEW_NAMES = ("lzf_gpu_store_renumber_work_size", "lzf_gpu_store_renumber", "lzf_gpu_store_remap",
             "lzf_gpu_key_index_rebuild")
MEMBERS = (("val_off", np.uint64), ("val_size", np.uint32), ("enc", np.uint8), ("val_len", np.uint32),
           ("key_off", np.uint64), ("key_len", np.uint32), ("item_time", np.int64), ("item_ttl", np.int32),
           ("item_lock", np.int64), ("last_access", np.int64))
REQUIRED = tuple(n for n, _ in MEMBERS[:6])
ALL = tuple(n for n, _ in MEMBERS)
DTYPE = dict(MEMBERS)
WINDOW, LONG = 32768, 256                # the key pack's staging window and its long-key threshold


# ---- CPU ---------------------------------------------------------------------

def test_library_exports_the_renumber_calls():
    L = gibson_amd.lib()
    for n in NEW_NAMES:
        assert hasattr(L, n), n
        assert n in gibson_amd.lzf.EXPORTS
    for n in ("store_renumber_work", "store_renumber", "store_remap", "key_index_rebuild", "StoreItems"):
        assert callable(getattr(gibson_amd, n)), n
    assert gibson_amd.STORE_NO_INDEX == PAD


def test_renumber_calls_reject_bad_arguments_without_device():
    # argument validation happens before any HIP call, so this runs on CPU;
    # only calls that must be refused are made (the pointers are host memory)
    L = gibson_amd.lib()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(4096)
    at = lambda k: ctypes.addressof(buf) + k

    def items(base, drop=(), **put):
        s = gibson_amd.lzf._StoreItems()
        for k, n in enumerate(ALL):
            setattr(s, n, None if n in drop else at(base + 64 * k))
        for n, v in put.items():
            setattr(s, n, v)
        return s

    def call(src, dst, count=1, dst_cap=1, src_keys=at(2048), src_cap=64, dst_keys=at(2112), dst_cap_b=64,
             used=at(3000), remap=at(3100), report=at(3200), status=at(3300), work=at(3400)):
        vp = lambda x: x if isinstance(x, ctypes.c_void_p) else ctypes.c_void_p(x)
        ps = None if src is None else ctypes.byref(src)
        pd = None if dst is None else ctypes.byref(dst)
        return L.lzf_gpu_store_renumber(ps, count, vp(src_keys), src_cap, pd, dst_cap, vp(dst_keys), dst_cap_b,
                                        vp(used), vp(remap), vp(report), vp(status), vp(work), null)

    src, dst = items(0), items(1024)
    assert call(None, dst) == -1 and call(src, None) == -1
    for n in REQUIRED:                               # a required member NULL on either side, or on both
        assert call(items(0, drop=(n,)), dst) == -1, n
        assert call(src, items(1024, drop=(n,))) == -1, n
        assert call(items(0, drop=(n,)), items(1024, drop=(n,))) == -1, n
    for n in ALL[6:]:                                # an optional member on one side only
        assert call(items(0, drop=(n,)), dst) == -1, n
        assert call(src, items(1024, drop=(n,))) == -1, n
    for n in ("item_time", "item_ttl"):              # exactly one of the two, on both sides alike
        assert call(items(0, drop=(n,)), items(1024, drop=(n,))) == -1, n
    for k in ("src_keys", "dst_keys", "used", "report", "status", "work"):
        assert call(src, dst, **{k: null}) == -1, k
    assert call(src, dst, count=0) == -1
    assert call(src, dst, dst_cap=0) == -1
    assert call(src, dst, src_cap=0) == -1
    assert call(src, dst, dst_cap_b=0) == -1
    # src_keys = [2048, 2112): dst_keys one byte into either end of it, and inside
    for d in (2111, 1985, 2048, 2100):
        assert call(src, dst, dst_keys=at(d)) == -1, d
    assert call(src, dst, src_keys=at(0), src_cap=2**64 - 1) == -1     # a range that wraps overlaps all above it
    for n in ALL:                                    # a dst array that is its src array
        assert call(src, items(1024, **{n: getattr(src, n)})) == -1, n

    p = ctypes.c_void_p(at(0))
    assert L.lzf_gpu_store_remap(null, 1, p, 1, null) == -1
    assert L.lzf_gpu_store_remap(p, 1, null, 1, null) == -1
    assert L.lzf_gpu_store_remap(p, 0, p, 1, null) == -1
    assert L.lzf_gpu_store_remap(p, 1, p, 0, null) == -1

    def rebuild(ptrs, slots=16, count=8):
        t, u, k, ko, kl, en, res, st = ptrs
        return L.lzf_gpu_key_index_rebuild(t, slots, u, k, ko, kl, en, count, res, st, null)

    good = [p] * 8
    for k in range(8):
        ptrs = list(good)
        ptrs[k] = null
        assert rebuild(ptrs) == -1, k
    assert rebuild(good, count=0) == -1
    for slots in (0, 8, 17, 24, 2**31 + 1):
        assert rebuild(good, slots=slots) == -1, slots
    assert rebuild([ctypes.c_void_p(at(0) | 4)] + good[1:]) == -1      # a table that is not 8-byte aligned


# recorded from the build: 16 bytes of slack, 8 state words, three u64 per scan tile
WORK_SIZES = {1: 104, 1023: 104, 1024: 104, 1025: 128, 4099: 200, 262145: 6248, 1 << 22: 98384,
              2**32 - 1: 100663376}


def test_renumber_work_size():
    ws = gibson_amd.lib().lzf_gpu_store_renumber_work_size
    prev = 0
    for count in (1, 2, 1023, 1024, 1025, 3000, 300000, 1 << 20, (1 << 31) + 5, 2**32 - 2, 2**32 - 1):
        w = ws(count)
        assert w >= prev and w >= 24 * ((count + 1023) // 1024), count
        assert ws(count + 1 if count < 2**32 - 1 else count) >= w
        prev = w
    assert 24 * (2**32 // 1024) <= ws(2**32 - 1) < 2**32             # 64-bit arithmetic: no wrap
    assert {n: int(ws(n)) for n in WORK_SIZES} == WORK_SIZES


# ---- GPU ---------------------------------------------------------------------

FILL = 0xA5
GUARD = 0x5A
BAND = 64                                # guard bytes in front of and behind every destination


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

    def untouched(self):
        return (self.read().view(np.uint8) == FILL).all()


class Host:
    """a store's item arrays and key arena on the host.  The keys are whatever
    bytes the arena holds at [key_off, key_off + key_len)"""

    def __init__(self, arena, **arrays):
        self.arena = np.ascontiguousarray(arena, np.uint8)
        self.a = {n: np.ascontiguousarray(arrays[n], DTYPE[n]) for n in ALL}
        self.n = len(self.a["enc"])

    def live(self):
        return self.a["enc"] != ENC_NULL

    def key(self, i):
        o, n = int(self.a["key_off"][i]), int(self.a["key_len"][i])
        return bytes(self.arena[o:o + n])


def gather(arena, off, ln):
    """the bytes [off[k], off[k] + ln[k]) of arena, one after another"""
    ln = ln.astype(np.int64)
    starts = np.cumsum(ln) - ln
    pos = np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(starts, ln) + np.repeat(off.astype(np.int64), ln)
    return arena[pos]


def make_store(seed, key_len, dead, share=()):
    """items with the key lengths `key_len`, dead where `dead`; the keys lie in
    the arena in a shuffled order with gaps; share: pairs (i, j), item j naming
    item i's bytes.  Every member holds seeded noise"""
    rs = np.random.RandomState(seed)
    n = len(key_len)
    key_len = np.array(key_len, np.int64)
    order = rs.permutation(n)
    gap = rs.randint(0, 6, n)
    step = key_len[order] + gap[order]
    off = np.empty(n, np.int64)
    off[order] = 3 + np.cumsum(step) - step
    arena = rs.randint(0, 256, int(3 + step.sum() + 9)).astype(np.uint8)
    for i, j in share:
        off[j], key_len[j] = off[i], key_len[i]
    enc = rs.choice(np.array([ENC_PLAIN, ENC_LZF, ENC_NUMBER], np.uint8), n)
    enc[np.asarray(dead, bool)] = ENC_NULL
    return Host(arena, val_off=rs.randint(0, 1 << 40, n), val_size=rs.randint(0, 1 << 20, n), enc=enc,
                val_len=rs.randint(0, 1 << 24, n), key_off=off, key_len=key_len,
                item_time=rs.randint(-(1 << 40), 1 << 40, n), item_ttl=rs.randint(-5, 1 << 20, n),
                item_lock=rs.randint(-1, 1 << 30, n), last_access=rs.randint(0, 1 << 40, n))


def model(h, dst_cap, base, dst_keys_cap, src_keys_cap):
    """-> status, report, and for OK: the dst arrays, remap, the packed keys"""
    live = h.live()
    idx = np.nonzero(live)[0]
    klen = h.a["key_len"].astype(np.int64)
    nlive, kbytes = len(idx), int(klen[live].sum())
    report = [nlive, kbytes, h.n - nlive, int(klen[~live].sum())]
    bad = any(int(o) > src_keys_cap or int(n) > src_keys_cap - int(o)
              for o, n in zip(h.a["key_off"][live], klen[live]))
    if bad:
        return ERANGE, report, None
    if nlive > dst_cap or base + kbytes >= 2**64 or base + kbytes > dst_keys_cap:
        return FULL, report, None
    out = {}
    ends = [min(int(o) + int(s), 2**64 - 1) for o, s in zip(h.a["val_off"][live], h.a["val_size"][live])]
    tail = {"val_off": max(ends) if ends else 0, "key_off": base + kbytes, "enc": ENC_NULL}
    for n in ALL:
        x = np.full(dst_cap, tail.get(n, 0), DTYPE[n])
        x[:nlive] = h.a[n][idx]
        out[n] = x
    out["key_off"][:nlive] = base + np.cumsum(klen[idx]) - klen[idx]
    remap = np.full(h.n, PAD, np.uint32)
    remap[idx] = np.arange(nlive, dtype=np.uint32)
    return OK, report, (out, remap, gather(h.arena, h.a["key_off"][idx], klen[idx]))


class Run:
    """one lzf_gpu_store_renumber call over h on the device; no synchronisation"""

    def __init__(self, torch, h, dst_cap, base=0, dst_keys_cap=None, mis=0, members=ALL, remap=True,
                 src_keys_cap=None):
        self.torch, self.h, self.dst_cap, self.base, self.members = torch, h, dst_cap, base, members
        klive = int(h.a["key_len"].astype(np.int64)[h.live()].sum())
        self.dst_keys_cap = (base % 2**32) + klive + 11 if dst_keys_cap is None else dst_keys_cap
        self.src_keys_cap = len(h.arena) if src_keys_cap is None else src_keys_cap
        self.src = {n: dev(torch, h.a[n]) for n in members}
        self.src_keys = dev(torch, h.arena)
        self.dst = {n: Guarded(torch, dst_cap, DTYPE[n]) for n in members}
        self.dst_keys = Guarded(torch, self.dst_keys_cap, np.uint8, mis)
        self.remap = Guarded(torch, h.n, np.uint32) if remap else None
        self.used = dev(torch, np.array([base, 0x1111], np.uint64))
        self.report = torch.full((5,), -7, dtype=torch.int64, device="cuda")
        self.status = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        self.work = gibson_amd.store_renumber(
            gibson_amd.StoreItems(**self.src), self.src_keys[:self.src_keys_cap],
            {n: g.t for n, g in self.dst.items()}, self.dst_keys.t, self.used[:1], self.report[:4], self.status[:1],
            remap=self.remap.t if remap else None)

    def check(self, expect_status=None):
        """against the model; -> (status, report)"""
        self.torch.cuda.synchronize()
        h = self.h
        status, report, ok = model(h, self.dst_cap, self.base, self.dst_keys_cap, self.src_keys_cap)
        got_status = self.status.cpu().numpy().tolist()
        got_report = self.report.cpu().numpy().tolist()
        used = self.used.cpu().numpy().view(np.uint64).tolist()
        print("renumber count", h.n, "dst_cap", self.dst_cap, "base", self.base, "status", got_status[0], "report",
              got_report[:4], "used", used[0], "expected", status, report)
        if expect_status is not None:
            assert status == expect_status              # the model holds the case the test claims
        assert got_status == [status, -7]
        assert got_report == report + [-7]
        for n in self.members:                          # src is never written
            assert (self.src[n].cpu().numpy().view(DTYPE[n]) == h.a[n]).all(), n
        assert (self.src_keys.cpu().numpy() == h.arena).all()
        if status != OK:                                # a refusal is whole
            assert used == [self.base, 0x1111]
            for n in self.members:
                assert self.dst[n].untouched(), n
            assert self.dst_keys.untouched()
            assert self.remap is None or self.remap.untouched()
            return status, report
        out, remap, packed = ok
        assert used == [self.base + report[1], 0x1111]
        for n in self.members:
            assert (self.dst[n].read() == out[n]).all(), n
        keys = self.dst_keys.read()
        assert (keys[:self.base] == FILL).all() and (keys[self.base + report[1]:] == FILL).all()
        assert (keys[self.base:self.base + report[1]] == packed).all()
        if self.remap is not None:
            assert (self.remap.read() == remap).all()
        return status, report


def dead_patterns(count):
    rs = np.random.RandomState(count)
    z = np.zeros(count, bool)
    pats = {"none": z.copy(), "all": ~z, "alternate": np.arange(count) % 2 == 1, "half": rs.rand(count) < 0.5}
    pats["all but the last"] = ~z
    pats["all but the last"][-1] = False
    pats["only item 0"] = ~z
    pats["only item 0"][0] = False
    if count == 4099:
        pats["one tile"] = (np.arange(count) >= 1024) & (np.arange(count) < 2048)
    return pats


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 5, 1023, 1024, 1025, 4099])
def test_renumber_against_the_model(torch, count):
    rs = np.random.RandomState(0x5EED + count)
    runs = []
    pats = dead_patterns(count)
    assert len(pats) == (7 if count == 4099 else 6)
    for name, dead in pats.items():
        h = make_store(1000 * count + len(runs), rs.randint(8, 41, count), dead)
        live = int(h.live().sum())
        assert live == count - int(dead.sum())
        if live:
            runs.append(Run(torch, h, live, base=5))         # dst_cap == live exactly
        runs.append(Run(torch, h, live + 1 + count % 7, base=0))
    for r in runs:
        assert r.check(OK)[0] == OK


KEY_SHAPES = [0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 40, 255, 256, 257, 4096, 5000, 70001]


@pytest.fixture(scope="module")
def shaped():
    """the key shapes three times over among short keys, shuffled, a third of
    the items dead, two items sharing their source bytes: 2 tiles, one of them
    with more key bytes than a staging window"""
    rs = np.random.RandomState(0x5A9E)
    lens = np.concatenate([np.array(KEY_SHAPES * 3), rs.randint(8, 41, 1100)])
    rs.shuffle(lens)
    dead = rs.rand(len(lens)) < 0.33
    special = [i for i, n in enumerate(lens) if n in (0, 255, 256, 257, 4096, 5000, 70001) or n < 8]
    dead[special] = False
    dead[0] = True
    a, b = [i for i in range(len(lens)) if not dead[i] and lens[i] == 33][:2]
    h = make_store(0x5A9E, lens, dead, share=[(a, b)])
    # from the model alone: what the batch claims to hold
    live, kl, ko = h.live(), h.a["key_len"], h.a["key_off"]
    assert set(KEY_SHAPES) <= set(kl[live].tolist()) and h.n > 1024
    assert kl[live].max() >= LONG and (kl[live] < LONG).any()
    assert any(int(kl[t:t + 1024][live[t:t + 1024]].sum()) > WINDOW for t in range(0, h.n, 1024))
    assert (~live).sum() > 100 and (np.diff(ko.astype(np.int64)[live]) < 0).any()
    assert ko[a] == ko[b] and h.key(a) == h.key(b) and live[a] and live[b]
    ends = np.sort(ko.astype(np.int64) + kl)
    assert (np.sort(ko.astype(np.int64))[1:] > ends[:-1]).any()              # gaps
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 1, 7, 15])
def test_key_shapes_and_alignment(torch, shaped, mis):
    live = int(shaped.live().sum())
    runs = [Run(torch, shaped, live + 3, base=base, mis=mis) for base in (0, 7)]
    for r in runs:
        r.check(OK)


@pytest.mark.gpu
def test_more_than_256_tiles(torch):
    count = 256 * 1024 + 1
    rs = np.random.RandomState(0x256)
    h = make_store(0x256, rs.randint(8, 25, count), rs.rand(count) < 0.1)
    assert (count + 1023) // 1024 > 256 and h.live()[-1]
    Run(torch, h, count, base=3).check(OK)


@pytest.mark.gpu
def test_refusals(torch):
    rs = np.random.RandomState(0x4EF)
    count = 1500
    lens, dead = rs.randint(8, 41, count), rs.rand(count) < 0.3
    h = make_store(0x4EF, lens, dead)
    live = int(h.live().sum())
    need = int(h.a["key_len"].astype(np.int64)[h.live()].sum())
    cases = [
        (Run(torch, h, live - 1), FULL),                                      # items
        (Run(torch, h, live, base=9, dst_keys_cap=9 + need - 1), FULL),       # keys, one byte short
        (Run(torch, h, live, base=9, dst_keys_cap=9 + need), OK),             # exactly the need
        (Run(torch, h, live, base=2**64 - 3, dst_keys_cap=need + 64), FULL),  # the end wraps
    ]
    last_live = int(np.nonzero(h.live())[0][-1])
    first_dead = int(np.nonzero(~h.live())[0][0])
    for who, want in ((last_live, ERANGE), (first_dead, OK)):
        past = make_store(0x4EF, lens, dead)                                  # one byte past src_keys_cap
        past.a["key_off"][who] = len(past.arena) - int(past.a["key_len"][who]) + 1
        cases.append((Run(torch, past, live + 2), want))
        wrap = make_store(0x4EF, lens, dead)                                  # key_off + key_len wraps
        wrap.a["key_off"][who] = 2**64 - 4
        cases.append((Run(torch, wrap, live + 2), want))
        cases.append((Run(torch, wrap, live - 1), ERANGE if want == ERANGE else FULL))
    wants = [w for _, w in cases]
    assert wants.count(FULL) >= 4 and wants.count(ERANGE) >= 3 and wants.count(OK) >= 3
    for r, want in cases:
        assert r.check(want)[0] == want


@pytest.mark.gpu
def test_optional_members(torch):
    rs = np.random.RandomState(0x0B7)
    h = make_store(0x0B7, rs.randint(8, 41, 1300), rs.rand(1300) < 0.4)
    live = int(h.live().sum())
    runs = [Run(torch, h, live + 5, members=REQUIRED + ("item_lock", "last_access")),     # no time / ttl
            Run(torch, h, live + 5, members=REQUIRED + ("item_time", "item_ttl")),        # no lock, no last_access
            Run(torch, h, live + 5, members=REQUIRED),
            Run(torch, h, live + 5, remap=False)]
    for r in runs:
        r.check(OK)


@pytest.mark.gpu
def test_renumber_is_deterministic(torch, shaped):
    live = int(shaped.live().sum())
    a, b = Run(torch, shaped, live + 9, base=7, mis=3), Run(torch, shaped, live + 9, base=7, mis=3)
    torch.cuda.synchronize()
    for n in ALL:
        assert (a.dst[n].buf == b.dst[n].buf).all(), n
    assert (a.dst_keys.buf == b.dst_keys.buf).all() and (a.remap.buf == b.remap.buf).all()
    assert (a.report == b.report).all() and (a.used == b.used).all()


@pytest.mark.gpu
def test_store_remap(torch):
    rs = np.random.RandomState(0x4E4)
    count = 3000
    h = make_store(0x4E4, rs.randint(8, 41, count), rs.rand(count) < 0.5)
    r = Run(torch, h, count)
    _, _, (_, remap, _) = model(h, count, 0, r.dst_keys_cap, r.src_keys_cap)
    lst = np.concatenate([rs.randint(0, count, 5000), [count, count + 1, 2**31, PAD, PAD - 1, 0, 0, count - 1]])
    lst = lst.astype(np.uint32)
    rs.shuffle(lst)
    live = h.live()
    assert (lst >= count).sum() >= 5 and (lst == PAD).any() and len(set(lst.tolist())) < len(lst)
    assert (~live[lst[lst < count]]).any() and live[lst[lst < count]].any()
    g = Guarded(torch, len(lst), np.uint32)
    g.t.copy_(dev(torch, lst))
    gibson_amd.store_remap(g.t, r.remap.t)
    torch.cuda.synchronize()
    exp = np.where(lst < count, remap[np.minimum(lst, count - 1)], PAD).astype(np.uint32)
    assert (g.read() == exp).all()
    r.check(OK)


# ---- the key index's rebuild ---------------------------------------------------

class Kidx:
    """a key index over a Host's keys and enc on the device"""

    def __init__(self, torch, h, slots):
        self.torch, self.h, self.slots = torch, h, slots
        self.keys, self.koff, self.klen = dev(torch, h.arena), dev(torch, h.a["key_off"]), dev(torch, h.a["key_len"])
        self.enc = Guarded(torch, h.n, np.uint8)
        self.enc.t.copy_(dev(torch, h.a["enc"]))
        self.table = Guarded(torch, gibson_amd.key_index_bytes(slots), np.uint8)
        self.table.t.fill_(0x33)                                             # not cleared: the rebuild does that
        self.used = torch.full((2,), 0x7777, dtype=torch.int32, device="cuda")
        self.result = torch.full((5,), -7, dtype=torch.int64, device="cuda")
        self.status = torch.full((2,), -7, dtype=torch.int32, device="cuda")

    def rebuild(self):
        gibson_amd.key_index_rebuild(self.table.t, self.used[:1], self.keys, self.koff, self.klen, self.enc.t,
                                     self.result[:4], self.status[:1])

    def clear_and_insert(self):
        self.table.t.fill_(0xFF)
        self.used[:1] = 0
        gibson_amd.key_index_insert(self.table.t, self.used[:1], self.keys, self.koff, self.klen, self.enc.t, 0,
                                    self.h.n, self.result[:4], self.status[:1])

    def lookup(self, queries):
        torch = self.torch
        ln = np.array([len(q) for q in queries], np.uint32)
        off = 1 + np.cumsum(ln.astype(np.int64)) - ln
        q = dev(torch, np.frombuffer(b"\0" + b"".join(queries) + b"\0" * 8, np.uint8))
        idx = Guarded(torch, len(queries), np.uint32)
        res = torch.zeros(3, dtype=torch.int64, device="cuda")
        gibson_amd.key_index_lookup(self.table.t, self.keys, self.koff, self.klen, self.enc.t, q, dev(torch, off),
                                    dev(torch, ln), idx.t, res)
        torch.cuda.synchronize()
        return idx.read().copy()

    def state(self):
        self.torch.cuda.synchronize()
        assert self.used[1].item() == 0x7777 and self.result[4].item() == -7 and self.status[1].item() == -7
        return (int(self.status[0].item()), self.result[:4].cpu().numpy().tolist(), int(self.used[0].item()),
                self.enc.read().copy())


def model_rebuild(h, slots):
    """the loop of the insert's contract over [0, n) into an empty map, FULL
    judged on the items it does not skip -> status, result, used, enc, map"""
    enc = h.a["enc"].copy()
    takes = [i for i in range(h.n) if enc[i] != ENC_NULL and h.a["key_len"][i]]
    if len(takes) > slots - slots // 4:
        return FULL, [0, 0, 0, 0], 0, enc, {}
    m, superseded = {}, 0
    for i in takes:
        j = m.get(h.key(i))
        if j is not None and enc[j] != ENC_NULL:
            enc[j] = ENC_NULL
            superseded += 1
        m[h.key(i)] = i
    return OK, [len(m), 0, superseded, h.n - len(takes)], len(m), enc, m


def dup_store(seed, n_live, tail):
    """n_live live items, some with duplicate keys and some with empty keys,
    dead ones between them, then a dead tail of `tail` items"""
    rs = np.random.RandomState(seed)
    n = n_live + n_live // 3
    lens = rs.randint(8, 41, n + tail)
    dead = np.zeros(n + tail, bool)
    dead[rs.choice(n, n - n_live, replace=False)] = True
    dead[n:] = True
    lens[n:] = 0
    alive = np.nonzero(~dead)[0]
    lens[rs.choice(alive, 4, replace=False)] = 0
    src = rs.choice(alive, 30, replace=False)
    share = [(int(src[k]), int(src[k + 15])) for k in range(15) if lens[src[k]]]
    return make_store(seed, lens, dead, share=share)


@pytest.mark.gpu
def test_key_index_rebuild_against_the_model_and_the_insert(torch):
    h = dup_store(0x4EB, 900, 700)
    status, result, used, enc, m = model_rebuild(h, 4096)
    live = h.live()
    assert status == OK and result[2] >= 5 and (h.a["key_len"][live] == 0).sum() >= 1 and not live[-700:].any()
    a, b = Kidx(torch, h, 4096), Kidx(torch, h, 4096)
    a.rebuild()
    b.clear_and_insert()
    sa, sb = a.state(), b.state()
    print("rebuild", sa[:3], "insert", sb[:3], "model", status, result, used)
    assert sa[:3] == (status, result, used) and (sa[3] == enc).all()
    assert sb[:3] == sa[:3] and (sb[3] == sa[3]).all()
    queries = [h.key(i) for i in range(h.n)] + [b"absent-%d" % k for k in range(50)] + [b""]
    exp = [m[q] if q in m and enc[m[q]] != ENC_NULL else PAD for q in queries]
    got = a.lookup(queries)
    assert got.tolist() == exp and b.lookup(queries).tolist() == exp
    # a superseded item's key finds the winner; an empty key and a dead item's key find nothing
    assert sum(e != PAD for e in exp) == int((live & (h.a["key_len"] > 0)).sum()) == 896


@pytest.mark.gpu
def test_key_index_rebuild_full_edge(torch):
    slots, bound = 64, 48
    rs = np.random.RandomState(0xF011)

    def store(takes, count):
        lens = rs.randint(8, 41, count)
        dead = np.ones(count, bool)
        dead[rs.choice(count, takes, replace=False)] = False
        return make_store(0xF011 + takes + count, lens, dead)

    over, at, padded = store(bound + 1, 60), store(bound, 60), store(bound, 5000)
    assert model_rebuild(over, slots)[0] == FULL and model_rebuild(at, slots)[0] == OK
    assert model_rebuild(padded, slots)[0] == OK and padded.n > bound        # the insert would refuse this count
    x = Kidx(torch, over, slots)
    x.rebuild()
    status, result, used, enc = x.state()
    assert (status, result, used) == (FULL, [0, 0, 0, 0], 0) and (enc == over.a["enc"]).all()
    assert (x.table.read() == 0xFF).all()                                    # cleared, and it stays so
    assert (x.lookup([over.key(i) for i in range(over.n)]) == PAD).all()
    for h in (at, padded):
        x = Kidx(torch, h, slots)
        x.rebuild()
        mstatus, mresult, mused, menc, m = model_rebuild(h, slots)
        status, result, used, enc = x.state()
        assert (status, result, used) == (OK, mresult, mused) and used == bound and (enc == menc).all()
        got = x.lookup([h.key(i) for i in range(h.n) if h.live()[i]])
        assert got.tolist() == [i for i in range(h.n) if h.live()[i]]


# ---- end to end ------------------------------------------------------------------

class Store:
    """a device store of `cap` item slots: value arena, key arena, the item
    arrays, appended to by set()"""

    def __init__(self, torch, cap, val_room, key_room):
        self.torch, self.cap, self.n = torch, cap, 0
        z = lambda dt: torch.zeros(cap, dtype=dt, device="cuda")
        self.arena = torch.zeros(val_room, dtype=torch.uint8, device="cuda")
        self.used = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.keys = torch.zeros(key_room, dtype=torch.uint8, device="cuda")
        self.keys_used = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.val_off, self.val_size, self.val_len = z(torch.int64), z(torch.int32), z(torch.int32)
        self.key_off, self.key_len = z(torch.int64), z(torch.int32)
        self.enc = torch.full((cap,), ENC_NULL, dtype=torch.uint8, device="cuda")

    def items(self, count):
        return gibson_amd.StoreItems(self.val_off[:count], self.val_size[:count], self.enc[:count],
                                     self.val_len[:count], self.key_off[:count], self.key_len[:count])

    def set(self, keys, values):
        """set_store of the values at items [n, n + len), the keys appended -> first"""
        torch, first, k = self.torch, self.n, len(values)
        ln = np.array([len(v) for v in values], np.uint32)
        off = np.cumsum(ln.astype(np.int64)) - ln
        d_in = dev(torch, np.frombuffer(b"".join(values) + b"\0", np.uint8))
        status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        w = gibson_amd.set_store(d_in, dev(torch, off), dev(torch, ln), 64, int(ln.max()), int(ln.sum()), self.arena,
                                 self.used, self.val_off[first:first + k], self.val_size[first:first + k],
                                 self.enc[first:first + k], status)
        self.val_len[first:first + k] = dev(torch, ln)
        kl = np.array([len(x) for x in keys], np.uint32)
        base = int(self.keys_used.item())
        self.keys[base:base + int(kl.sum())] = dev(torch, np.frombuffer(b"".join(keys), np.uint8))
        self.key_off[first:first + k] = dev(torch, base + np.cumsum(kl.astype(np.int64)) - kl)
        self.key_len[first:first + k] = dev(torch, kl)
        self.keys_used += int(kl.sum())
        torch.cuda.synchronize()
        del w
        assert int(status.item()) == OK
        self.n += k
        return first

    def lookup(self, table, count, queries):
        torch = self.torch
        ln = np.array([len(q) for q in queries], np.uint32)
        q = dev(torch, np.frombuffer(b"".join(queries) + b"\0" * 8, np.uint8))
        idx = torch.zeros(len(queries), dtype=torch.int32, device="cuda")
        res = torch.zeros(3, dtype=torch.int64, device="cuda")
        gibson_amd.key_index_lookup(table, self.keys, self.key_off[:count], self.key_len[:count], self.enc[:count], q,
                                    dev(torch, np.cumsum(ln.astype(np.int64)) - ln), dev(torch, ln), idx, res)
        torch.cuda.synchronize()
        return idx

    def replies(self, count, idx, room, max_len):
        """store_replies (GET) over idx -> the arena's bytes, rep_off, rep_len"""
        torch, n = self.torch, idx.numel()
        rep = torch.zeros(room, dtype=torch.uint8, device="cuda")
        used = torch.zeros(1, dtype=torch.int64, device="cuda")
        off, ln = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        est = torch.zeros(n, dtype=torch.uint8, device="cuda")
        res = torch.zeros(6, dtype=torch.int64, device="cuda")
        w = gibson_amd.store_replies(idx, gibson_amd.REPLY_GET, self.arena, self.val_off[:count], self.val_size[:count],
                                     self.enc[:count], self.val_len[:count], None, None, 0, max_len, rep, used, off,
                                     ln, est, res)
        torch.cuda.synchronize()
        del w
        assert int(res[3].item()) == gibson_amd.REPLY_OK and int(res[5].item()) == 0
        return rep.cpu().numpy()[:int(used.item())].copy(), off.cpu().numpy(), ln.cpu().numpy()


def same_replies(a, b):
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


@pytest.mark.gpu
def test_set_delete_overwrite_renumber_rebuild_compact_set(torch):
    rnd = random.Random(0xE2E17)
    n, cap, slots = 3000, 6000, 16384
    sizes = [rnd.randint(64, 400) for _ in range(n + 1000)]
    for i in rnd.sample(range(n + 1000), 80):
        sizes[i] = rnd.randint(2000, 20480)
    values = [synth(i % 6, 0x5EEDE2E, i, s) for i, s in enumerate(sizes)]
    keys = [b"item:%06d:" % i + bytes(rnd.choice(b"abcdef") for _ in range(rnd.randint(0, 28))) for i in range(n)]
    assert len(set(keys)) == n and 8 <= min(map(len, keys)) and max(map(len, keys)) <= 40
    room = sum(sizes) + 8 * len(sizes) + 64
    old = Store(torch, cap, room, 1 << 18)
    table = torch.full((gibson_amd.key_index_bytes(slots),), 0xFF, dtype=torch.uint8, device="cuda")
    kused = torch.zeros(1, dtype=torch.int32, device="cuda")
    kres, kst = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")

    def insert(st, count, first, k):
        gibson_amd.key_index_insert(table, kused, st.keys, st.key_off[:count], st.key_len[:count], st.enc[:count],
                                    first, k, kres, kst)
        torch.cuda.synchronize()
        assert int(kst.item()) == 0

    old.set(keys, values[:n])
    insert(old, n, 0, n)
    enc0 = old.enc[:n].cpu().numpy()
    assert (enc0 == ENC_LZF).sum() >= 100 and (enc0 == ENC_PLAIN).sum() >= 100
    order = list(range(n))
    rnd.shuffle(order)
    gone, over = order[:1000], order[1000:2000]
    gibson_amd.store_delete(old.lookup(table, n, [keys[i] for i in gone]), old.enc[:n])          # DEL by key
    first = old.set([keys[i] for i in over], values[n:])                                         # overwrite
    count = old.n
    insert(old, count, first, 1000)
    assert int(kres[1].item()) == 1000                                                           # replaced
    queries = keys + [b"item:absent", b"item:"]
    idx_before = old.lookup(table, count, queries)
    before = idx_before.cpu().numpy().view(np.uint32)
    assert (before == PAD).sum() == 1002 and (before[over] >= n).all()
    max_len = max(sizes)
    rep_room = 2 * sum(sizes) + 64 * len(queries)
    a = old.replies(count, idx_before, rep_room, max_len)

    new = Store(torch, cap, room, 1 << 18)
    new.arena = old.arena                                    # value bytes do not move
    remap = torch.zeros(count, dtype=torch.int32, device="cuda")
    report, status = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    w = gibson_amd.store_renumber(old.items(count), old.keys, new.items(cap), new.keys, new.keys_used, report, status,
                                  remap=remap)
    gibson_amd.key_index_rebuild(table, kused, new.keys, new.key_off, new.key_len, new.enc, kres, kst)   # count = dst_cap
    torch.cuda.synchronize()
    del w
    live = int(report[0].item())                             # the one read the host needs: 8 bytes
    assert int(status.item()) == OK and int(kst.item()) == 0 and live == 2000
    assert kres.cpu().numpy().tolist() == [live, 0, 0, cap - live] and int(kused.item()) == live
    idx_after = new.lookup(table, cap, queries)
    after = idx_after.cpu().numpy().view(np.uint32)
    rm = remap.cpu().numpy().view(np.uint32)
    assert (after == np.where(before == PAD, PAD, rm[np.minimum(before, count - 1)])).all()
    assert (after[before != PAD] < live).all()
    translated = idx_before.clone()
    gibson_amd.store_remap(translated, remap)
    torch.cuda.synchronize()
    assert (translated == idx_after).all()
    assert same_replies(new.replies(cap, idx_after, rep_room, max_len), a)

    packed = torch.zeros(room, dtype=torch.uint8, device="cuda")
    pused = torch.zeros(1, dtype=torch.int64, device="cuda")
    w = gibson_amd.store_compact(new.arena, new.val_off, new.val_size, new.enc, packed, pused, report, status)
    torch.cuda.synchronize()
    del w
    assert int(status.item()) == OK and int(report[0].item()) == live and int(report[2].item()) == cap - live
    new.arena, new.used = packed, pused
    assert same_replies(new.replies(cap, idx_after, rep_room, max_len), a)

    new.n = live                                             # a further SET at first = report[0]
    more = [b"late:%d" % i for i in range(40)]
    first = new.set(more, [synth(i % 6, 0x1A7E, i, 100 + 37 * i) for i in range(40)])
    assert first == live
    insert(new, cap, first, 40)
    found = new.lookup(table, cap, more + [keys[over[0]]]).cpu().numpy().view(np.uint32)
    assert found[:40].tolist() == list(range(live, live + 40)) and found[40] == after[over[0]]
    w = gibson_amd.store_usage(new.val_size[:live], new.enc[:live], report)
    torch.cuda.synchronize()
    del w
    assert report.cpu().numpy().tolist()[0] == live and report.cpu().numpy().tolist()[2] == 0
