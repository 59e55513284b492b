"""The device store's lifecycle (lzf_gpu_store_delete, _expire, _usage,
_compact): items nulled by index and by the TTL rule of src/query.c:186-189,
and the semispace compaction of the live items into a second arena, against
numpy over bytes read back.  The bar is bit-exact.

Every arena a test hands over with a cap is allocated larger than the cap and
the excess filled with a guard byte, which is checked afterwards."""
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
NEW_NAMES = ("lzf_gpu_store_delete", "lzf_gpu_store_expire", "lzf_gpu_store_usage",
             "lzf_gpu_store_compact_work_size", "lzf_gpu_store_compact")


# ---- CPU ---------------------------------------------------------------------

def test_library_exports_the_lifecycle_calls():
    L = gibson_amd.lib()
    for n in NEW_NAMES:
        assert hasattr(L, n), n
        assert n in gibson_amd.lzf.EXPORTS
    for n in ("store_delete", "store_expire", "store_usage", "store_compact", "store_compact_work"):
        assert callable(getattr(gibson_amd, n)), n
    assert gibson_amd.STORE_ERANGE == 3


def test_lifecycle_calls_reject_bad_arguments_without_device():
    # argument validation happens before any HIP call, so this runs on CPU;
    # only calls that must be refused are made (the pointers are host memory)
    L = gibson_amd.lib()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(512)
    at = lambda k: ctypes.c_void_p(ctypes.addressof(buf) + k)
    p = at(0)

    def compact(ptrs, count=1, src_cap=64, dst_cap=64):
        src, vo, vs, en, dst, du, rep, sta, wk = ptrs
        return L.lzf_gpu_store_compact(src, src_cap, vo, vs, en, count, dst, dst_cap, du, rep, sta, wk, null)

    good = [at(0), at(256), at(256), at(256), at(128), at(256), at(256), at(256), at(256)]
    for k in range(9):                               # a NULL pointer in each position
        ptrs = list(good)
        ptrs[k] = null
        assert compact(ptrs) == -1, k
    assert compact(good, count=0) == -1
    assert compact(good, dst_cap=0) == -1
    assert compact(good, src_cap=0) == -1
    # src = [64, 128): dst one byte into either end of it
    for d in (127, 1, 64, 100):
        ptrs = list(good)
        ptrs[0], ptrs[4] = at(64), at(d)
        assert compact(ptrs) == -1, d
    # a range that wraps the address space overlaps everything above it
    ptrs = list(good)
    ptrs[0], ptrs[4] = at(0), at(128)
    assert compact(ptrs, src_cap=2**64 - 1) == -1

    assert L.lzf_gpu_store_delete(null, 1, p, 1, null) == -1
    assert L.lzf_gpu_store_delete(p, 1, null, 1, null) == -1
    assert L.lzf_gpu_store_delete(p, 1, p, 0, null) == -1
    for k in range(4):
        ptrs = [p] * 4
        ptrs[k] = null
        assert L.lzf_gpu_store_expire(ptrs[0], ptrs[1], 5, ptrs[2], 1, ptrs[3], null) == -1, k
        assert L.lzf_gpu_store_usage(ptrs[0], ptrs[1], 1, ptrs[2], ptrs[3], null) == -1, k
    assert L.lzf_gpu_store_expire(p, p, 5, p, 0, p, null) == -1
    assert L.lzf_gpu_store_usage(p, p, 0, p, p, null) == -1


def test_compact_work_size():
    ws = gibson_amd.lib().lzf_gpu_store_compact_work_size
    prev = 0
    for count in (1, 2, 1023, 1024, 1025, 3000, 300000, 1 << 20, (1 << 31) + 5, 2**32 - 2, 2**32 - 1):
        w = ws(count)
        assert w >= 16 * count and w >= prev, count      # the live list: two u64 per item
        assert ws(count + 1 if count < 2**32 - 1 else count) >= w
        prev = w
    assert 16 * (2**32 - 1) <= ws(2**32 - 1) < 2**40     # 64-bit arithmetic: no wrap


# ---- GPU ---------------------------------------------------------------------

FILL = 0xA5
GUARD = 0x5A
BASE = 7
ROOM = 4096                              # guard bytes past every cap
PLANTED = [1, 2, 3, 4, 5, 8, 64, 65, 4096, 4097, 16384, 16385, 65536, 65537, 70000, 300003]


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


class Host:
    """a store on the host: the arena's bytes and the three arrays (and the
    values' original lengths, val_len of the frame)"""

    def __init__(self, arena, off, size, enc, vlen=None):
        self.arena = np.ascontiguousarray(arena, np.uint8)
        self.off = np.asarray(off, np.int64).copy()
        self.size = np.asarray(size, np.int64).copy()
        self.enc = np.asarray(enc, np.uint8).copy()
        self.vlen = self.size.copy() if vlen is None else np.asarray(vlen, np.int64).copy()
        self.n = len(self.off)

    def take(self, idx):
        return Host(self.arena, self.off[idx], self.size[idx], self.enc[idx], self.vlen[idx])

    def dead(self, idx):
        h = self.take(np.arange(self.n))
        h.enc[np.asarray(idx, np.int64)] = ENC_NULL
        return h

    def stored(self, i):
        return bytes(self.arena[self.off[i]:self.off[i] + self.size[i]])


def build_store(torch, values, compression, base=BASE, batches=1):
    """lzf_gpu_set_store of ``values`` (in ``batches`` consecutive calls into
    one arena) -> Host"""
    cuts = [len(values) * k // batches for k in range(batches + 1)]
    room = base + sum(len(v) for v in values) + 8 * len(values) + 16
    arena = torch.full((room,), FILL, dtype=torch.uint8, device="cuda")
    used = torch.tensor([base], dtype=torch.int64, device="cuda")
    status = torch.full((batches,), -1, dtype=torch.int32, device="cuda")
    keep, outs = [], []
    for k in range(batches):
        vals = values[cuts[k]:cuts[k + 1]]
        ln = np.array([len(v) for v in vals], np.uint32)
        off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.int64)]).astype(np.int64)
        d_in = _u8(torch, np.frombuffer(b"".join(vals) + b"\0", np.uint8))
        d_off, d_len = _i64(torch, off), _i32(torch, ln)
        vo = torch.full((len(vals),), -1, dtype=torch.int64, device="cuda")
        vs = torch.full((len(vals),), -1, dtype=torch.int32, device="cuda")
        en = torch.full((len(vals),), 0x77, dtype=torch.uint8, device="cuda")
        w = gibson_amd.set_store(d_in, d_off, d_len, compression, int(ln.max()), int(ln.sum()), arena, used, vo, vs,
                                 en, status[k:k + 1])
        keep.append((d_in, d_off, d_len, w))
        outs.append((vo, vs, en))
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()
    return Host(arena.cpu().numpy()[:int(used.item())],
                np.concatenate([o[0].cpu().numpy() for o in outs]),
                np.concatenate([o[1].cpu().numpy().view(np.uint32) for o in outs]),
                np.concatenate([o[2].cpu().numpy() for o in outs]),
                [len(v) for v in values])


def mixed_values():
    """the 3000-value batch of tests/test_store.py"""
    rnd = random.Random(0x5704E)
    count = 3000
    sizes = [rnd.randint(1, 200) for _ in range(count)]
    for i, n in zip(rnd.sample(range(count), len(PLANTED)), PLANTED):
        sizes[i] = n
    return [synth(i % 6, 0x5EED5704, i, n) for i, n in enumerate(sizes)]


@pytest.fixture(scope="module")
def mixed(torch):
    """the 3000-value store at compression 64, base 7, and the dead set of the
    bit-exact test"""
    values = mixed_values()
    h = build_store(torch, values, 64)
    assert (h.enc == ENC_LZF).sum() >= 1000 and (h.enc == ENC_PLAIN).sum() >= 1000
    big = int(np.argmax(h.vlen))
    assert h.vlen[big] == 300003 and 0 < big < h.n - 1
    rnd = random.Random(0xDEAD)
    start = 100 if big > 1500 else 2000
    dead = set(rnd.sample(range(h.n), 700)) | {0, h.n - 1, big - 1, big + 1} | set(range(start, start + 640))
    dead.discard(big)
    eight = int(np.nonzero((h.vlen == 8) & (h.enc == ENC_PLAIN))[0][0])
    dead.discard(eight)
    h.enc[eight] = ENC_NUMBER                # a NUMBER item: live, its 8 stored bytes
    return {"values": values, "host": h, "dead": np.array(sorted(dead)), "big": big}


def expect_report(h):
    live = h.enc != ENC_NULL
    return [int(live.sum()), int(h.size[live].sum()), int((~live).sum()), int(h.size[~live].sum())]


def expect(h, base):
    """what a successful compaction of h from base leaves"""
    live = h.enc != ENC_NULL
    lsz = np.where(live, h.size, 0)
    off = base + np.concatenate([[0], np.cumsum(lsz[:-1])])
    packed = np.frombuffer(b"".join(h.stored(i) for i in np.nonzero(live)[0]), np.uint8)
    report = expect_report(h)
    assert len(packed) == report[1]
    return off, lsz, packed, report


class Run:
    """one lzf_gpu_store_compact call over a copy of h on the device; no
    synchronisation.  src_cap / dst_cap are views of larger guarded tensors"""

    def __init__(self, torch, h, dst_cap, base=BASE, src_cap=None):
        self.h, self.base = h, base
        self.src_cap = len(h.arena) if src_cap is None else src_cap
        self.dst_cap = dst_cap
        src = np.full(max(len(h.arena), self.src_cap) + ROOM, GUARD, np.uint8)
        src[:len(h.arena)] = h.arena
        self.src_np = src
        self.src = _u8(torch, src)
        self.dst = torch.full((dst_cap + ROOM,), FILL, dtype=torch.uint8, device="cuda")
        self.off, self.size, self.enc = _i64(torch, h.off), _i32(torch, h.size), _u8(torch, h.enc)
        self.used = torch.tensor([base], dtype=torch.int64, device="cuda")
        self.report = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        self.status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        wsize = int(gibson_amd.lib().lzf_gpu_store_compact_work_size(h.n))
        self.work = torch.full((wsize + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
        self.wsize = wsize
        gibson_amd.store_compact(self.src[:self.src_cap], self.off, self.size, self.enc, self.dst[:dst_cap], self.used,
                                 self.report, self.status, work=self.work[:wsize])

    def check_common(self, torch, status, report):
        torch.cuda.synchronize()
        assert int(self.status.item()) == status
        assert self.report.cpu().numpy().tolist() == report
        assert (self.src.cpu().numpy() == self.src_np).all()          # the source arena is never written
        assert (self.enc.cpu().numpy() == self.h.enc).all()           # nor enc
        assert (self.work[self.wsize:].cpu().numpy() == GUARD).all()
        return self.dst.cpu().numpy()

    def check_ok(self, torch):
        off, lsz, packed, report = expect(self.h, self.base)
        got = self.check_common(torch, OK, report)
        total = report[1]
        assert int(self.used.item()) == self.base + total
        g_off, g_size = self.off.cpu().numpy(), self.size.cpu().numpy().view(np.uint32).astype(np.int64)
        bad = np.nonzero(g_off != off)[0]
        assert not len(bad), (len(bad), bad[:5], g_off[bad[:5]], off[bad[:5]])
        bad = np.nonzero(g_size != lsz)[0]
        assert not len(bad), (len(bad), bad[:5], g_size[bad[:5]], lsz[bad[:5]])
        assert (np.diff(g_off) >= 0).all()
        bad = np.nonzero(got[self.base:self.base + total] != packed)[0]
        if len(bad):
            i = int(np.searchsorted(off, self.base + bad[0], side="right")) - 1
            raise AssertionError((len(bad), "first wrong byte", int(bad[0]), "item", i, int(self.h.size[i])))
        assert (got[:self.base] == FILL).all() and (got[self.base + total:] == FILL).all()
        return total

    def check_refused(self, torch, status):
        got = self.check_common(torch, status, expect_report(self.h))
        assert (got == FILL).all()                                    # no byte of dst is written
        assert int(self.used.item()) == self.base
        assert (self.off.cpu().numpy() == self.h.off).all()
        assert (self.size.cpu().numpy().view(np.uint32) == self.h.size).all()


def live_bytes(h):
    return int(h.size[h.enc != ENC_NULL].sum())


# 1
@pytest.mark.gpu
def test_compaction_bit_exact(torch, mixed):
    h = mixed["host"].dead(mixed["dead"])
    dead = h.enc == ENC_NULL
    big = mixed["big"]
    assert dead[0] and dead[-1] and dead[big - 1] and dead[big + 1] and not dead[big]
    runs = np.diff(np.nonzero(np.diff(np.concatenate([[0], dead.view(np.uint8), [0]])))[0])[::2]
    assert runs.max() >= 600                                          # longer than the pack kernel's LDS table
    assert (h.enc == ENC_NUMBER).sum() == 1
    r = Run(torch, h, BASE + live_bytes(h) + 100)
    assert r.check_ok(torch) == live_bytes(h) >= 3 * 65536            # several pack tiles


# 7
@pytest.mark.gpu
@pytest.mark.parametrize("pack,tile_kb", [("realign", None), (None, "4"), (None, "1024")])
def test_compaction_pack_forms_bit_exact(torch, mixed, monkeypatch, pack, tile_kb):
    if pack:
        monkeypatch.setenv("LZF_GPU_STORE_PACK", pack)
    if tile_kb:
        monkeypatch.setenv("LZF_GPU_STORE_TILE_KB", tile_kb)
    h = mixed["host"].dead(mixed["dead"])
    Run(torch, h, BASE + live_bytes(h) + 100).check_ok(torch)


# 2
@pytest.mark.gpu
def test_non_monotone_sources(torch, mixed):
    two = build_store(torch, mixed["values"], 64, batches=2)
    perm = np.random.RandomState(0x9E37).permutation(two.n)
    h = two.take(perm)
    assert (np.diff(h.off) < 0).sum() > 1000                          # not increasing in the index
    h = h.dead(np.random.RandomState(5).choice(h.n, 900, replace=False))
    r = Run(torch, h, BASE + live_bytes(h) + 100)
    r.check_ok(torch)
    # per item: the bytes at the new offset are the item's stored bytes
    got, off = r.dst.cpu().numpy(), r.off.cpu().numpy()
    for i in np.nonzero(h.enc != ENC_NULL)[0][::7]:
        assert bytes(got[off[i]:off[i] + h.size[i]]) == h.stored(i), i


def _keys(n, seed):
    rnd = random.Random(seed)
    keys = [bytes(rnd.choice(b"abcdefghij:_0123456789") for _ in range(rnd.randint(1, 40))) for _ in range(n)]
    kl = np.array([len(k) for k in keys], np.uint32)
    return keys, kl, np.concatenate([[0], np.cumsum(kl[:-1], dtype=np.int64)]).astype(np.int64)


def _frame(torch, d_keys, d_koff, d_klen, vals, off, size, enc, vlen, elements, max_val_len, max_response):
    frame = torch.zeros(max_response + 7, dtype=torch.uint8, device="cuda")
    flen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    w = gibson_amd.kv_frame(d_keys, d_koff, d_klen, vals, off, size, enc, vlen, elements, max_val_len, frame,
                            max_response, flen)
    return frame, flen, w


# 3
@pytest.mark.gpu
def test_the_frame_does_not_notice(torch, oracle, mixed):
    n = 400
    h = mixed["host"].take(np.arange(n)).dead(np.arange(3, n, 5))
    live = h.enc != ENC_NULL
    assert ((h.enc == ENC_LZF).sum() >= 64 and (h.enc == ENC_PLAIN).sum() >= 64 and (~live).sum() >= 64)
    keys, kl, koff = _keys(n, 0xF4A3F)
    exp = oracle.kv_frame([(keys[i], int(h.enc[i]), h.stored(i) if live[i] else b"") for i in range(n)],
                          int(live.sum()), 64 << 20, 1 << 20)
    assert exp is not None
    d_keys, d_koff, d_klen = _u8(torch, np.frombuffer(b"".join(keys), np.uint8)), _i64(torch, koff), _i32(torch, kl)
    d_vlen = _i32(torch, h.vlen)
    args = (int(live.sum()), int(h.vlen.max()), len(exp) + 64)
    src, o_off, o_size, o_enc = _u8(torch, h.arena), _i64(torch, h.off), _i32(torch, h.size), _u8(torch, h.enc)
    f0, l0, w0 = _frame(torch, d_keys, d_koff, d_klen, src, o_off, o_size, o_enc, d_vlen, *args)
    r = Run(torch, h, BASE + live_bytes(h) + 100)
    f1, l1, w1 = _frame(torch, d_keys, d_koff, d_klen, r.dst, r.off, r.size, r.enc, d_vlen, *args)
    r.check_ok(torch)
    assert int(l0.item()) == int(l1.item()) == len(exp)
    assert bytes(f0[:len(exp)].cpu().numpy()) == exp
    assert bytes(f1[:len(exp)].cpu().numpy()) == exp


# 4
@pytest.mark.gpu
def test_append_after_compact_without_synchronisation(torch, oracle, mixed):
    n1, n2 = 300, 100
    h = mixed["host"].take(np.arange(n1)).dead(np.arange(0, n1, 3))
    live = h.enc != ENC_NULL
    rnd = random.Random(0xA99E)
    values = [synth(i % 6, 0x5EED5707, i, rnd.choice([rnd.randint(1, 100), rnd.randint(100, 6000)]))
              for i in range(n2)]
    items2 = []
    for v in values:                                                  # gbSingleSet at compression 64
        s = oracle.compress(v, min((len(v) - 4) & 0xFFFFFFFF, len(v) + len(v) // 16 + 8)) if len(v) > 64 else None
        items2.append((ENC_LZF, s) if s else (ENC_PLAIN, v))
    keys, kl, koff = _keys(n1 + n2, 0xF4A40)
    items = [(keys[i], int(h.enc[i]), h.stored(i) if live[i] else b"") for i in range(n1)]
    items += [(keys[n1 + j], e, s) for j, (e, s) in enumerate(items2)]
    elements = int(live.sum()) + n2
    exp = oracle.kv_frame(items, elements, 64 << 20, 1 << 20)
    assert exp is not None
    total = live_bytes(h) + sum(len(s) for _, s in items2)

    # the arrays of both batches side by side: compact rewrites the first n1
    # entries, set_store writes the rest
    off = torch.cat([_i64(torch, h.off), torch.full((n2,), -1, dtype=torch.int64, device="cuda")])
    size = torch.cat([_i32(torch, h.size), torch.full((n2,), -1, dtype=torch.int32, device="cuda")])
    enc = torch.cat([_u8(torch, h.enc), torch.full((n2,), 0x77, dtype=torch.uint8, device="cuda")])
    ln2 = np.array([len(v) for v in values], np.uint32)
    vlen = torch.cat([_i32(torch, h.vlen), _i32(torch, ln2)])
    d_in = _u8(torch, np.frombuffer(b"".join(values) + b"\0", np.uint8))
    d_ioff = _i64(torch, np.concatenate([[0], np.cumsum(ln2[:-1], dtype=np.int64)]))
    d_ilen = _i32(torch, ln2)
    d_keys, d_koff, d_klen = _u8(torch, np.frombuffer(b"".join(keys), np.uint8)), _i64(torch, koff), _i32(torch, kl)
    src = _u8(torch, h.arena)
    cap = BASE + total + 50
    dst = torch.full((cap + ROOM,), FILL, dtype=torch.uint8, device="cuda")
    used = torch.tensor([BASE], dtype=torch.int64, device="cuda")
    report = torch.zeros(4, dtype=torch.int64, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    w1 = gibson_amd.store_compact(src, off[:n1], size[:n1], enc[:n1], dst[:cap], used, report, status[:1])
    w2 = gibson_amd.set_store(d_in, d_ioff, d_ilen, 64, int(ln2.max()), int(ln2.sum()), dst[:cap], used, off[n1:],
                              size[n1:], enc[n1:], status[1:])
    f, fl, w3 = _frame(torch, d_keys, d_koff, d_klen, dst, off, size, enc, vlen, elements,
                       int(max(h.vlen.max(), ln2.max())), len(exp) + 64)
    torch.cuda.synchronize()
    del w1, w2, w3
    assert status.cpu().numpy().tolist() == [0, 0]
    assert int(used.item()) == BASE + total
    assert int(off[n1].item()) == BASE + live_bytes(h)
    assert int(fl.item()) == len(exp)
    assert bytes(f[:len(exp)].cpu().numpy()) == exp
    got = dst.cpu().numpy()
    assert (got[:BASE] == FILL).all() and (got[BASE + total:] == FILL).all()


# 5
@pytest.mark.gpu
def test_refusals(torch, mixed):
    h = mixed["host"].dead(mixed["dead"])
    total = live_bytes(h)
    Run(torch, h, BASE + total).check_ok(torch)                       # exactly enough
    Run(torch, h, BASE + total - 1).check_refused(torch, FULL)        # one byte short
    # base + live bytes wraps 2^64
    r = Run(torch, h, BASE + total + 100, base=-5)
    r.check_refused(torch, FULL)
    # the item stored last in the arena ends one byte past src_cap
    last = int(np.argmax(np.where(h.enc != ENC_NULL, h.off + h.size, -1)))
    assert h.size[last] > 0
    cap = int(h.off[last] + h.size[last]) - 1
    assert cap + 1 <= len(h.arena)
    Run(torch, h, BASE + total + 100, src_cap=cap).check_refused(torch, ERANGE)
    # an offset past the arena altogether, and one whose end wraps
    for bad in (len(h.arena) + 1, -3):
        g = h.take(np.arange(h.n))
        g.off[last] = bad
        Run(torch, g, BASE + total + 100).check_refused(torch, ERANGE)
    # the same item dead: its range is not looked at
    g = h.dead([last])
    Run(torch, g, BASE + total + 100, src_cap=cap).check_ok(torch)


def _random_store(rs, sizes):
    sizes = np.asarray(sizes, np.int64)
    off = np.concatenate([[0], np.cumsum(sizes[:-1])]) + 3
    arena = rs.randint(0, 256, int(sizes.sum()) + 3 + 1).astype(np.uint8)
    return Host(arena, off, sizes, np.zeros(len(sizes), np.uint8))


# 6
@pytest.mark.gpu
def test_edges(torch, mixed):
    m = mixed["host"]
    # all items dead: nothing moves, every offset is the base
    h = m.dead(np.arange(m.n))
    r = Run(torch, h, 64)
    assert r.check_ok(torch) == 0 and int(r.used.item()) == BASE
    assert (r.off.cpu().numpy() == BASE).all() and (r.size.cpu().numpy() == 0).all()
    # no item dead
    assert Run(torch, m, BASE + live_bytes(m) + 1).check_ok(torch) == live_bytes(m)
    rs = np.random.RandomState(0xED6E)
    # one item, live and dead; the live one of size 0
    for size, dead in ((37, False), (37, True), (0, False)):
        h = _random_store(rs, [size])
        Run(torch, h.dead([0]) if dead else h, BASE + 37).check_ok(torch)
    # one past a scan tile, only the last item live
    sizes = rs.randint(0, 300, 1025)
    sizes[-1] = 211
    h = _random_store(rs, sizes).dead(np.arange(1024))
    r = Run(torch, h, BASE + 211)
    assert r.check_ok(torch) == 211
    # live items of size 0 between dead ones, the first and last item among them
    sizes = rs.randint(1, 50, 2101)
    sizes[::2] = 0
    h = _random_store(rs, sizes).dead(np.arange(1, 2101, 4))
    assert (h.size[h.enc != ENC_NULL] == 0).sum() == 1051 and h.size[0] == h.size[-1] == 0
    Run(torch, h, BASE + live_bytes(h) + 5).check_ok(torch)


@pytest.mark.gpu
def test_adjacent_arenas(torch, mixed):
    # src and dst in one allocation, touching but sharing no byte: not an overlap
    h = mixed["host"].take(np.arange(500)).dead(np.arange(0, 500, 2))
    n, total = len(h.arena), live_bytes(h)
    both = torch.full((n + total + ROOM,), FILL, dtype=torch.uint8, device="cuda")
    both[:n] = _u8(torch, h.arena)
    off, size, enc = _i64(torch, h.off), _i32(torch, h.size), _u8(torch, h.enc)
    used = torch.zeros(1, dtype=torch.int64, device="cuda")
    report = torch.zeros(4, dtype=torch.int64, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    w = gibson_amd.store_compact(both[:n], off, size, enc, both[n:n + total], used, report, status)
    torch.cuda.synchronize()
    del w
    e_off, _, packed, e_report = expect(h, 0)
    got = both.cpu().numpy()
    assert int(status.item()) == OK and report.cpu().numpy().tolist() == e_report
    assert (got[:n] == h.arena).all() and (got[n:n + total] == packed).all() and (got[n + total:] == FILL).all()
    assert (off.cpu().numpy() == e_off).all()
    with pytest.raises(RuntimeError, match="EARG"):                   # one byte into src
        gibson_amd.store_compact(both[:n], off, size, enc, both[n - 1:n + total], used, report, status)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_many_tiny_values_every_other_dead(torch):
    # the tiny-value path: thousands of items per pack tile
    rs = np.random.RandomState(11)
    values = [synth(5 if i & 1 else 0, 0x5EED5708, i, int(n)) for i, n in enumerate(rs.randint(1, 4, 20000))]
    h = build_store(torch, values, 24)
    assert (h.enc == ENC_PLAIN).all() and (h.size == h.vlen).all()
    h = h.dead(np.arange(0, 20000, 2))
    r = Run(torch, h, BASE + live_bytes(h) + 9)
    assert r.check_ok(torch) == live_bytes(h)


# 8
@pytest.mark.gpu
def test_delete(torch):
    count = 1000
    rs = np.random.RandomState(0xDE1)
    enc0 = rs.choice([ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL], count + 64).astype(np.uint8)
    idx = np.concatenate([rs.randint(0, count, 300), [8, 9, 10, 11, 9, 9, 16, 17, 19, 0, count - 1, count - 1],
                          [count, count + 3, count + 63, 2**31, 2**32 - 1]]).astype(np.uint32)
    rs.shuffle(idx)
    enc = _u8(torch, enc0)
    gibson_amd.store_delete(_i32(torch, idx), enc[:count])
    torch.cuda.synchronize()
    exp = enc0.copy()
    exp[idx[idx < count]] = ENC_NULL
    assert (enc.cpu().numpy()[:count] == exp[:count]).all()
    assert (enc.cpu().numpy()[count:] == enc0[count:]).all()           # past count: untouched
    assert (exp[:count] != enc0[:count]).sum() > 150


# 9
@pytest.mark.gpu
def test_expire(torch):
    count, now = 5000, 1_700_000_000
    rs = np.random.RandomState(0xE791)
    ttl = rs.choice([-1, 0, 1, 32767, 5, 600], count).astype(np.int32)
    age = rs.randint(-100, 40000, count).astype(np.int64)
    enc0 = rs.choice([ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL], count + 16).astype(np.uint8)
    k = 0
    for t in (-1, 0, 1, 32767):                  # the boundaries, live and already NULL
        for a in (t - 1, t, t + 1, -7):
            for e in (ENC_PLAIN, ENC_NULL):
                ttl[k], age[k], enc0[k] = t, a, e
                k += 1
    ttl[k], age[k], enc0[k] = 2**31 - 1, 2**31 - 1, ENC_LZF            # the largest ttl, reached
    ttl[k + 1], age[k + 1], enc0[k + 1] = 2**31 - 1, 2**31 - 2, ENC_LZF
    time = now - age
    enc = _u8(torch, enc0)
    expired = torch.full((1,), 12345, dtype=torch.int32, device="cuda")
    gibson_amd.store_expire(_i64(torch, time), torch.from_numpy(ttl).cuda(), now, enc[:count], expired)
    torch.cuda.synchronize()
    hit = (enc0[:count] != ENC_NULL) & (ttl > 0) & (now - time >= ttl)            # src/query.c:186-189
    exp = enc0.copy()
    exp[:count][hit] = ENC_NULL
    assert (enc.cpu().numpy() == exp).all()
    assert int(expired.item()) == int(hit.sum()) > 1000
    assert hit[k] and not hit[k + 1]
    # a second sweep finds nothing new
    gibson_amd.store_expire(_i64(torch, time), torch.from_numpy(ttl).cuda(), now, enc[:count], expired)
    torch.cuda.synchronize()
    assert int(expired.item()) == 0 and (enc.cpu().numpy() == exp).all()


# 10
@pytest.mark.gpu
def test_usage(torch, mixed):
    h = mixed["host"]
    size, enc = _i32(torch, h.size), _u8(torch, h.enc)
    report = torch.full((3, 4), -1, dtype=torch.int64, device="cuda")
    w0 = gibson_amd.store_usage(size, enc, report[0])
    gibson_amd.store_delete(_i32(torch, mixed["dead"]), enc)
    w1 = gibson_amd.store_usage(size, enc, report[1])
    torch.cuda.synchronize()
    del w0, w1
    g = h.dead(mixed["dead"])
    assert (enc.cpu().numpy() == g.enc).all()
    assert report[0].cpu().numpy().tolist() == expect(h, 0)[3] == [h.n, int(h.size.sum()), 0, 0]
    assert report[1].cpu().numpy().tolist() == expect(g, 0)[3]
    assert expect(g, 0)[3][3] > 0
    # after a compaction the dead items have size 0
    r = Run(torch, g, BASE + live_bytes(g) + 100)
    w2 = gibson_amd.store_usage(r.size, r.enc, report[2])
    r.check_ok(torch)
    del w2
    e = expect(g, 0)[3]
    assert report[2].cpu().numpy().tolist() == [e[0], e[1], e[2], 0]
