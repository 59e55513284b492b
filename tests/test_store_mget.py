"""The operator layer over the device store: lzf_gpu_store_select_prefix (an
index list in HBM from a key prefix) and the index-list operators
lzf_gpu_store_mget, _count and _mttl, against a Python model of the validity
rule (src/query.c:204-224) and the oracle's reply frame (src/net.c:1256-1342).
The bar is bit-exact.

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

ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL = 0, 1, 2, 0xFF
OK, NOT_FOUND, TOO_BIG, EDECODE = 0, 1, 2, 3
PAD = 0xFFFFFFFF
NEW_NAMES = ("lzf_gpu_store_select_work_size", "lzf_gpu_store_select_prefix", "lzf_gpu_store_mget_work_size",
             "lzf_gpu_store_mget", "lzf_gpu_store_count", "lzf_gpu_store_mttl")


# ---- CPU ---------------------------------------------------------------------

def test_library_exports_the_index_calls():
    L = gibson_amd.lib()
    for n in NEW_NAMES:
        assert hasattr(L, n), n
        assert n in gibson_amd.lzf.EXPORTS
    for n in ("store_select_prefix", "store_select_work", "store_mget", "store_mget_work", "store_count",
              "store_mttl"):
        assert callable(getattr(gibson_amd, n)), n
    assert (gibson_amd.MGET_OK, gibson_amd.MGET_NOT_FOUND, gibson_amd.MGET_TOO_BIG,
            gibson_amd.MGET_EDECODE) == (0, 1, 2, 3)


def test_index_calls_reject_bad_arguments_without_device():
    # argument validation happens before any HIP call, so this runs on CPU;
    # only calls that must be refused are made (the pointers are host memory)
    L = gibson_amd.lib()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(512)
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def select(ptrs, count=1, plen=1, cap=1):
        keys, koff, klen, enc, prefix, sel, result, work = ptrs
        return L.lzf_gpu_store_select_prefix(keys, koff, klen, enc, count, prefix, plen, sel, cap, result, work, null)

    for k in range(8):                               # a NULL pointer in each position
        ptrs = [p] * 8
        ptrs[k] = null
        assert select(ptrs) == -1, k
    assert select([p] * 8, count=0) == -1
    assert select([p] * 8, plen=0) == -1
    assert select([p] * 8, cap=0) == -1

    def mget(ptrs, n=1, count=1, max_val_len=16):
        (idx, keys, koff, klen, store, voff, vsize, enc, vlen, time, ttl, last, frame, flen, result, work) = ptrs
        return L.lzf_gpu_store_mget(idx, n, keys, koff, klen, store, voff, vsize, enc, vlen, count, time, ttl, 5, last,
                                    max_val_len, 1, frame, 64, flen, result, work, null)

    optional = {9, 10, 11}                           # item_time, item_ttl, last_access
    for k in range(16):
        if k in optional:
            continue
        ptrs = [p] * 16
        ptrs[k] = null
        assert mget(ptrs) == -1, k
    for k in (9, 10):                                # exactly one NULL time array
        ptrs = [p] * 16
        ptrs[k] = null
        assert mget(ptrs) == -1, k
    assert mget([p] * 16, n=0) == -1
    assert mget([p] * 16, count=0) == -1
    assert mget([p] * 16, max_val_len=(64 << 20) + 1) == -1

    def count_(ptrs, n=1, count=1):
        idx, enc, time, ttl, last, result = ptrs
        return L.lzf_gpu_store_count(idx, n, enc, count, time, ttl, 5, last, result, null)

    def mttl(ptrs, n=1, count=1):
        idx, enc, time, ttl, last, result = ptrs
        return L.lzf_gpu_store_mttl(idx, n, 9, enc, count, time, ttl, 5, last, result, null)

    for k in (0, 1, 5):
        ptrs = [p] * 6
        ptrs[k] = null
        assert count_(ptrs) == -1 and mttl(ptrs) == -1, k
    for k in (2, 3):                                 # one NULL time array; MTTL needs both
        ptrs = [p] * 6
        ptrs[k] = null
        assert count_(ptrs) == -1 and mttl(ptrs) == -1, k
    assert mttl([p, p, null, null, p, p]) == -1
    for f in (count_, mttl):
        assert f([p] * 6, n=0) == -1
        assert f([p] * 6, count=0) == -1


def test_work_sizes():
    L = gibson_amd.lib()
    sizes = (1, 2, 1023, 1024, 1025, 3000, 262145, 1 << 20, (1 << 31) + 5, 2**32 - 2, 2**32 - 1)
    for ws, per in ((L.lzf_gpu_store_mget_work_size, 58), (L.lzf_gpu_store_select_work_size, 0.125)):
        prev = 0
        for n in sizes:
            w = ws(n)
            assert w >= per * n and w >= prev, n
            prev = w
        assert per * (2**32 - 1) <= ws(2**32 - 1) < 2**40    # 64-bit arithmetic: no wrap


# ---- GPU ---------------------------------------------------------------------

FILL = 0xA5
GUARD = 0x5A
BASE = 7
ROOM = 4096                              # guard bytes past every size
NOW = 1_700_000_000
PLANTED = [4096, 4097, 16385, 70000]
MAXREQ = 1 << 20


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    gibson_amd.lib()
    return t


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _s32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _i64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _u8(torch, a):
    return torch.from_numpy(np.array(a, dtype=np.uint8)).cuda()


def _keys(n, seed, alphabet=b"abcdefghij:_0123456789"):
    rnd = random.Random(seed)
    keys = [bytes(rnd.choice(alphabet) for _ in range(rnd.randint(1, 40))) for _ in range(n)]
    kl = np.array([len(k) for k in keys], np.uint32)
    return keys, kl, np.concatenate([[0], np.cumsum(kl[:-1], dtype=np.int64)]).astype(np.int64)


class Host:
    """a store on the host: the arena's bytes, the per-item arrays and keys"""

    def __init__(self, arena, off, size, enc, vlen, keys):
        self.arena = np.ascontiguousarray(arena, np.uint8)
        self.off = np.asarray(off, np.int64).copy()
        self.size = np.asarray(size, np.int64).copy()
        self.enc = np.asarray(enc, np.uint8).copy()
        self.vlen = np.asarray(vlen, np.int64).copy()
        self.keys = keys
        self.klen = np.array([len(k) for k in keys], np.uint32)
        self.koff = np.concatenate([[0], np.cumsum(self.klen[:-1], dtype=np.int64)]).astype(np.int64)
        self.n = len(self.off)

    def copy(self):
        return Host(self.arena, self.off, self.size, self.enc, self.vlen, self.keys)

    def dead(self, idx):
        h = self.copy()
        h.enc[np.asarray(idx, np.int64)] = ENC_NULL
        return h

    def stored(self, i):
        return bytes(self.arena[self.off[i]:self.off[i] + self.size[i]])


def set_store_args(torch, values):
    ln = np.array([len(v) for v in values], np.uint32)
    off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.int64)]).astype(np.int64)
    return _u8(torch, np.frombuffer(b"".join(values) + b"\0", np.uint8)), _i64(torch, off), _i32(torch, ln), ln


def build_store(torch, values, compression, keys, base=BASE):
    """lzf_gpu_set_store of ``values`` -> Host"""
    room = base + sum(len(v) for v in values) + 8 * len(values) + 16
    arena = torch.full((room,), FILL, dtype=torch.uint8, device="cuda")
    used = torch.tensor([base], dtype=torch.int64, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    d_in, d_off, d_len, ln = set_store_args(torch, values)
    vo = torch.full((len(values),), -1, dtype=torch.int64, device="cuda")
    vs = torch.full((len(values),), -1, dtype=torch.int32, device="cuda")
    en = torch.full((len(values),), 0x77, dtype=torch.uint8, device="cuda")
    w = gibson_amd.set_store(d_in, d_off, d_len, compression, int(ln.max()), int(ln.sum()), arena, used, vo, vs, en,
                             status)
    torch.cuda.synchronize()
    del w
    assert int(status.item()) == 0
    return Host(arena.cpu().numpy()[:int(used.item())], vo.cpu().numpy(), vs.cpu().numpy().view(np.uint32),
                en.cpu().numpy(), [len(v) for v in values], keys)


def main_values():
    rnd = random.Random(0x36E7)
    count = 400
    sizes = [rnd.randint(1, 200) for _ in range(count)]
    for i, n in zip(rnd.sample(range(count), len(PLANTED)), PLANTED):
        sizes[i] = n
    sizes[rnd.choice([i for i in range(count) if sizes[i] < 200])] = 8
    # the planted ones of a kind that compresses
    return [synth(1 if n in PLANTED else i % 6, 0x5EED36E7, i, n) for i, n in enumerate(sizes)]


@pytest.fixture(scope="module")
def main(torch):
    """the 400-value store at compression 64, one 8-byte item a NUMBER, with
    dead items and TTLs of every kind"""
    values = main_values()
    keys, _, _ = _keys(len(values), 0x36E7)
    h = build_store(torch, values, 64, keys)
    assert (h.enc == ENC_LZF).sum() >= 64 and (h.enc == ENC_PLAIN).sum() >= 64
    assert set(PLANTED) <= set(h.vlen[h.enc == ENC_LZF].tolist())
    eight = int(np.nonzero((h.vlen == 8) & (h.enc == ENC_PLAIN))[0][0])
    h.enc[eight] = ENC_NUMBER
    rs = np.random.RandomState(0x36E7)
    dead = rs.choice(h.n, 90, replace=False)
    dead = dead[dead != eight]
    ttl = rs.choice([-1, 0, 5, 600, 32767], h.n).astype(np.int32)
    ttl[eight] = 0
    age = rs.randint(0, 1200, h.n).astype(np.int64)
    return {"values": values, "host": h.dead(dead), "fresh": h, "dead": dead, "eight": eight, "ttl": ttl,
            "time": NOW - age}


def model(idx, enc, count, time, ttl, now):
    """the validity rule over a list, every entry judged on enc as it is before
    the call: (valid entries in list order, expired entries, skipped)"""
    valid, expired, skipped = [], [], 0
    for i in idx:
        i = int(i)
        if i >= count or enc[i] == ENC_NULL:
            skipped += 1
        elif ttl is not None and ttl[i] > 0 and now - int(time[i]) >= ttl[i]:
            expired.append(i)
        else:
            valid.append(i)
    return valid, expired, skipped


def expect_frame(oracle, h, valid, max_response, header):
    items = [(h.keys[i], int(h.enc[i]), h.stored(i)) for i in valid]
    return oracle.kv_frame(items, len(valid), max_response, MAXREQ, reply_header=header)


class Dev:
    """the store's arrays on the device"""

    def __init__(self, torch, h, time=None, ttl=None, key_shift=0):
        self.h = h
        self.keys = _u8(torch, np.frombuffer(b"\0" * key_shift + b"".join(h.keys) + b"\0", np.uint8))
        self.koff, self.klen = _i64(torch, h.koff + key_shift), _i32(torch, h.klen)
        self.arena = _u8(torch, np.concatenate([h.arena, np.full(ROOM, GUARD, np.uint8)]))
        self.off, self.size, self.enc = _i64(torch, h.off), _i32(torch, h.size), _u8(torch, h.enc)
        self.vlen = _i32(torch, h.vlen)
        self.time = None if time is None else _i64(torch, time)
        self.ttl = None if ttl is None else _s32(torch, ttl)
        self.last = torch.full((h.n,), -1, dtype=torch.int64, device="cuda")


class Mget:
    """one lzf_gpu_store_mget call; no synchronisation"""

    def __init__(self, torch, d, idx, max_response, header=True, now=NOW, arena=None, off=None, size=None):
        self.d, self.header, self.max_response = d, header, max_response
        self.hdr = 7 if header else 0
        self.idx = idx if hasattr(idx, "numel") else _i32(torch, np.asarray(idx, np.uint32))
        self.frame = torch.full((self.hdr + max_response + ROOM,), FILL, dtype=torch.uint8, device="cuda")
        self.flen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        self.result = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        self.wsize = int(gibson_amd.lib().lzf_gpu_store_mget_work_size(int(self.idx.numel())))
        self.work = torch.full((self.wsize + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
        gibson_amd.store_mget(self.idx, d.keys, d.koff, d.klen, d.arena if arena is None else arena,
                              d.off if off is None else off, d.size if size is None else size, d.enc, d.vlen,
                              d.time, d.ttl, now, int(d.h.vlen.max()), self.frame[:self.hdr + max_response],
                              max_response, self.flen, self.result, last_access=d.last, work=self.work[:self.wsize],
                              reply_header=header)

    def check(self, torch, exp, result):
        """exp: the frame, or None where none is written"""
        torch.cuda.synchronize()
        got = self.frame.cpu().numpy()
        print("mget result", self.result.cpu().numpy().tolist(), "frame_len", int(self.flen.item()),
              "expected", result, None if exp is None else len(exp))
        assert self.result.cpu().numpy().tolist() == list(result)
        assert (self.work[self.wsize:].cpu().numpy() == GUARD).all()
        if exp is None:
            assert int(self.flen.item()) == 0
            assert (got == FILL).all()                                # no byte of the frame is written
            return
        assert int(self.flen.item()) == len(exp)
        bad = np.nonzero(got[:len(exp)] != np.frombuffer(exp, np.uint8))[0]
        assert not len(bad), (len(bad), "first wrong byte", int(bad[0]))
        assert (got[len(exp):] == FILL).all()


def check_side_effects(d, enc_before, valid, expired, last_before=None, now=NOW):
    """enc is nulled exactly at the expired entries, last_access is now
    exactly at the valid ones"""
    exp_enc = np.asarray(enc_before).copy()
    exp_enc[np.asarray(expired, np.int64)] = ENC_NULL
    assert (d.enc.cpu().numpy() == exp_enc).all()
    exp_last = np.full(d.h.n, -1, np.int64) if last_before is None else np.asarray(last_before).copy()
    exp_last[np.asarray(valid, np.int64)] = now
    assert (d.last.cpu().numpy() == exp_last).all()


def mixed_list(m, n=150, seed=0x715):
    """a shuffled list with live, dead, expired and out-of-range entries and
    duplicates of a valid and of an expired one"""
    h = m["host"]
    rs = np.random.RandomState(seed)
    idx = rs.choice(np.delete(np.arange(h.n), m["eight"]), n - 6, replace=False).astype(np.uint32)
    valid, expired, _ = model(idx, h.enc, h.n, m["time"], m["ttl"], NOW)
    assert len(valid) >= 40 and len(expired) >= 15 and (h.enc[idx] == ENC_NULL).sum() >= 15
    idx = np.concatenate([idx, [h.n, PAD, h.n + 5, valid[3], expired[2], m["eight"]]]).astype(np.uint32)
    rs.shuffle(idx)
    return idx


# 1
@pytest.mark.gpu
@pytest.mark.parametrize("header", [True, False])
def test_mget_bit_exact(torch, oracle, main, header):
    h = main["host"]
    idx = mixed_list(main)
    valid, expired, skipped = model(idx, h.enc, h.n, main["time"], main["ttl"], NOW)
    assert len(valid) + len(expired) + skipped == 150 and skipped >= 18
    assert len(set(valid)) == len(valid) - 1 and len(set(expired)) == len(expired) - 1
    assert set(h.enc[valid].tolist()) == {ENC_PLAIN, ENC_LZF, ENC_NUMBER}
    exp = expect_frame(oracle, h, valid, 64 << 20, header)
    d = Dev(torch, h, main["time"], main["ttl"])
    r = Mget(torch, d, idx, len(exp) + 100, header)
    r.check(torch, exp, [len(valid), len(expired), skipped, OK])
    check_side_effects(d, h.enc, valid, expired)
    assert (d.arena.cpu().numpy()[len(h.arena):] == GUARD).all()


# 2
@pytest.mark.gpu
def test_expiry_edges(torch, oracle, main):
    h = main["fresh"].copy()
    k = 0
    ttl = np.zeros(h.n, np.int32)
    age = np.zeros(h.n, np.int64)
    for t in (-1, 0, 1, 5, 32767, 2**31 - 1):
        for a in (t - 1, t, t + 1, 0, -7):
            ttl[k], age[k] = t, a
            k += 1
    idx = np.arange(k + 10, dtype=np.uint32)
    time = NOW - age
    valid, expired, skipped = model(idx, h.enc, h.n, time, ttl, NOW)
    # by hand: positive ttl and age >= ttl
    assert expired == [i for i in range(k) if ttl[i] > 0 and age[i] >= ttl[i]] and len(expired) == 8 and not skipped
    d = Dev(torch, h, time, ttl)
    exp = expect_frame(oracle, h, valid, 64 << 20, True)
    Mget(torch, d, idx, len(exp), True).check(torch, exp, [len(valid), len(expired), 0, OK])
    check_side_effects(d, h.enc, valid, expired)
    # both time arrays NULL: nothing expires
    d = Dev(torch, h)
    exp = expect_frame(oracle, h, list(idx), 64 << 20, True)
    Mget(torch, d, idx, len(exp), True).check(torch, exp, [len(idx), 0, 0, OK])
    check_side_effects(d, h.enc, idx, [])


# 3
@pytest.mark.gpu
def test_statuses(torch, oracle, main):
    h = main["host"]
    time, ttl = main["time"], main["ttl"]
    # every entry dead, expired or out of range
    every = np.arange(h.n, dtype=np.uint32)
    _, expired, _ = model(every, h.enc, h.n, time, ttl, NOW)
    idx = np.concatenate([main["dead"][:20], expired[:20], [h.n, PAD]]).astype(np.uint32)
    d = Dev(torch, h, time, ttl)
    Mget(torch, d, idx, 1 << 16).check(torch, None, [0, 20, 22, NOT_FOUND])
    check_side_effects(d, h.enc, [], expired[:20])
    # the payload fits exactly; one byte less does not
    idx = mixed_list(main, seed=0x716)
    valid, expired, skipped = model(idx, h.enc, h.n, time, ttl, NOW)
    exp = expect_frame(oracle, h, valid, 64 << 20, False)
    d = Dev(torch, h, time, ttl)
    Mget(torch, d, idx, len(exp), False).check(torch, exp, [len(valid), len(expired), skipped, OK])
    d = Dev(torch, h, time, ttl)
    assert expect_frame(oracle, h, valid, len(exp) - 1, False) is None
    Mget(torch, d, idx, len(exp) - 1, False).check(torch, None, [len(valid), len(expired), skipped, TOO_BIG])
    check_side_effects(d, h.enc, valid, expired)                      # done whatever the status
    # one LZF stream corrupted on the device
    lzf = [i for i in valid if h.enc[i] == ENC_LZF and h.size[i] >= 8]
    bad = lzf[len(lzf) // 2]
    assert oracle.decompress(b"\xff" * int(h.size[bad]), int(h.vlen[bad]))[0] is None
    d = Dev(torch, h, time, ttl)
    d.arena[int(h.off[bad]):int(h.off[bad] + h.size[bad])] = 0xFF
    r = Mget(torch, d, idx, len(exp) + 64, False)
    torch.cuda.synchronize()
    assert r.result.cpu().numpy().tolist() == [len(valid), len(expired), skipped, EDECODE]
    assert int(r.flen.item()) == 0
    assert (r.frame.cpu().numpy()[len(exp):] == FILL).all()
    assert (r.work[r.wsize:].cpu().numpy() == GUARD).all()
    check_side_effects(d, h.enc, valid, expired)


# 4
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025])
def test_list_sizes_around_a_tile(torch, oracle, main, n):
    h = main["host"]
    rs = np.random.RandomState(n)
    small = np.nonzero(h.vlen <= 16385)[0]
    idx = rs.choice(small, n).astype(np.uint32)                       # with repeats
    if n == 1:
        idx[0] = int(np.nonzero(h.enc == ENC_LZF)[0][0])
    valid, expired, skipped = model(idx, h.enc, h.n, None, None, NOW)
    exp = expect_frame(oracle, h, valid, 64 << 20, True)
    d = Dev(torch, h)
    Mget(torch, d, idx, len(exp) + 9).check(torch, exp, [len(valid), 0, skipped, OK])


@pytest.mark.gpu
def test_list_past_the_block_sum_chunk(torch, oracle):
    # 256 tiles of 1024 entries and one more: the scan of the tile sums takes a second piece
    rs = np.random.RandomState(0xB16)
    count, n = 5000, 262145
    values = [bytes(rs.randint(0, 256, int(s)).astype(np.uint8)) for s in rs.randint(1, 9, count)]
    keys, _, _ = _keys(count, 0xB16)
    h = build_store(torch, values, 64, keys)
    assert (h.enc == ENC_PLAIN).all()
    h = h.dead(rs.choice(count, 500, replace=False))
    idx = rs.randint(0, count + 50, n).astype(np.uint32)
    valid, expired, skipped = model(idx, h.enc, h.n, None, None, NOW)
    assert skipped > 20000
    exp = expect_frame(oracle, h, valid, 64 << 20, True)
    d = Dev(torch, h)
    Mget(torch, d, idx, len(exp) + 9).check(torch, exp, [len(valid), 0, skipped, OK])


# 5
@pytest.mark.gpu
def test_whole_store_equals_kv_frame(torch, main):
    h = main["host"]
    live = int((h.enc != ENC_NULL).sum())
    d = Dev(torch, h)
    cap = int(h.vlen[h.enc != ENC_NULL].sum() + 60 * h.n)
    frame = torch.full((cap + 7,), FILL, dtype=torch.uint8, device="cuda")
    flen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    w = gibson_amd.kv_frame(d.keys, d.koff, d.klen, d.arena, d.off, d.size, d.enc, d.vlen, live, int(h.vlen.max()),
                            frame, cap, flen)
    r = Mget(torch, d, np.arange(h.n, dtype=np.uint32), cap)
    torch.cuda.synchronize()
    del w
    assert int(flen.item()) == int(r.flen.item()) > 7 + 4 + 9 * live
    assert (frame.cpu().numpy() == r.frame.cpu().numpy()[:cap + 7]).all()
    assert r.result.cpu().numpy().tolist() == [live, 0, h.n - live, OK]


# 6
@pytest.mark.gpu
def test_chain_without_synchronisation(torch, oracle, main):
    """set_store -> expire -> mget -> delete -> mget -> compact -> mget, one
    synchronise at the end"""
    f, values = main["fresh"], main["values"]                         # what set_store leaves, known from the fixture
    time, ttl = main["time"], main["ttl"]
    n = f.n
    h0 = f.copy()
    h0.enc[main["eight"]] = ENC_PLAIN                                 # set_store stores it PLAIN
    swept = [i for i in range(n) if ttl[i] > 0 and NOW - time[i] >= ttl[i]]
    h1 = h0.dead(swept)                                               # after store_expire at NOW
    later = NOW + 700                                                 # mget 1 finds more of them expired
    idx1 = np.random.RandomState(1).permutation(n)[:200].astype(np.uint32)
    v1, e1, s1 = model(idx1, h1.enc, n, time, ttl, later)
    assert e1 and s1
    h2 = h1.dead(e1)
    gone = np.array(v1[::3], np.uint32)                               # DEL
    h3 = h2.dead(gone)
    idx2 = np.concatenate([idx1[::2], [PAD]]).astype(np.uint32)
    v2, e2, s2 = model(idx2, h3.enc, n, time, ttl, later)
    assert not e2 and s2 > len(gone) // 2
    idx3 = np.arange(n, dtype=np.uint32)[::-1].copy()
    v3, e3, s3 = model(idx3, h3.enc, n, time, ttl, later)
    h4 = h3.dead(e3)
    exps = [expect_frame(oracle, h0, v, 64 << 20, True) for v in (v1, v2, v3)]

    d = Dev(torch, h0, time, ttl)
    d_in, d_off, d_len, ln = set_store_args(torch, values)
    room = len(f.arena) + 64
    arena = torch.full((room,), FILL, dtype=torch.uint8, device="cuda")
    arena2 = torch.full((room,), FILL, dtype=torch.uint8, device="cuda")
    used = torch.tensor([BASE], dtype=torch.int64, device="cuda")
    used2 = torch.tensor([0], dtype=torch.int64, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    off = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    size = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d.enc = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    expired = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    report = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    w = [gibson_amd.set_store(d_in, d_off, d_len, 64, int(ln.max()), int(ln.sum()), arena, used, off, size, d.enc,
                              status[:1])]
    gibson_amd.store_expire(d.time, d.ttl, NOW, d.enc, expired)
    r1 = Mget(torch, d, idx1, len(exps[0]) + 5, now=later, arena=arena, off=off, size=size)
    gibson_amd.store_delete(_i32(torch, gone), d.enc)
    r2 = Mget(torch, d, idx2, len(exps[1]) + 5, now=later, arena=arena, off=off, size=size)
    w.append(gibson_amd.store_compact(arena, off, size, d.enc, arena2, used2, report, status[1:]))
    r3 = Mget(torch, d, idx3, len(exps[2]) + 5, now=later, arena=arena2, off=off, size=size)
    torch.cuda.synchronize()
    del w
    assert status.cpu().numpy().tolist() == [0, 0] and int(expired.item()) == len(swept)
    r1.check(torch, exps[0], [len(v1), len(e1), s1, OK])
    r2.check(torch, exps[1], [len(v2), 0, s2, OK])
    r3.check(torch, exps[2], [len(v3), len(e3), s3, OK])
    assert (d.enc.cpu().numpy() == h4.enc).all()
    last = np.full(n, -1, np.int64)
    last[np.array(v1 + v2 + v3, np.int64)] = later
    assert (d.last.cpu().numpy() == last).all()


# 7
def select_keys(count, seed):
    keys, kl, koff = _keys(count, seed, alphabet=b"ab:")
    return keys


def py_select(keys, enc, prefix):
    return [i for i, k in enumerate(keys) if enc[i] != ENC_NULL and k.startswith(prefix)]


class Select:
    def __init__(self, torch, keys, enc, prefix, cap, key_shift=1):
        kl = np.array([len(k) for k in keys], np.uint32)
        koff = np.concatenate([[0], np.cumsum(kl[:-1], dtype=np.int64)]).astype(np.int64) + key_shift
        self.cap = cap
        self.keys = _u8(torch, np.frombuffer(b"\xee" * key_shift + b"".join(keys) + b"\0", np.uint8))
        self.koff, self.klen, self.enc = _i64(torch, koff), _i32(torch, kl), _u8(torch, enc)
        self.prefix = _u8(torch, np.frombuffer(prefix, np.uint8))
        self.sel = torch.full((cap + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.result = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        self.wsize = int(gibson_amd.lib().lzf_gpu_store_select_work_size(len(keys)))
        self.work = torch.full((self.wsize + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
        gibson_amd.store_select_prefix(self.keys, self.koff, self.klen, self.enc, self.prefix, self.sel[:cap],
                                       self.result, work=self.work[:self.wsize])

    def check(self, torch, exp):
        torch.cuda.synchronize()
        sel = self.sel.cpu().numpy().view(np.uint32)
        res = self.result.cpu().numpy().view(np.uint32).tolist()
        k = min(len(exp), self.cap)
        assert res == [k, len(exp)]
        assert sel[:k].tolist() == exp[:k]
        assert (sel[k:self.cap] == PAD).all()
        assert (sel[self.cap:] == 0x5A5A5A5A).all()
        assert (self.work[self.wsize:].cpu().numpy() == GUARD).all()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 1025, 70000])
def test_select(torch, count):
    keys = select_keys(count, 0x5E1 + count)
    rs = np.random.RandomState(count)
    enc = rs.choice([ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL], count).astype(np.uint8)
    if count == 1:
        enc[0] = ENC_LZF
    long_key = max(keys, key=len)
    whole = keys[count // 2]
    # of length 1 and 3, a whole key, the longest key, longer than every key, of 5 and 8 (dwords and a tail)
    prefixes = [keys[0][:1], b"ab:", b"a:b", whole, long_key, long_key + b"a", b"a" * 41, b"abab:", b"ab:ab:ab"]
    for prefix in prefixes:
        exp = py_select(keys, enc, prefix)
        for shift in (1, 2) if prefix in (whole, b"a:b") else (1,):
            Select(torch, keys, enc, prefix, len(exp) + 7, key_shift=shift).check(torch, exp)   # the tail is padding
        if len(exp) > 1:
            Select(torch, keys, enc, prefix, len(exp) // 2).check(torch, exp)   # the first cap, in index order
            Select(torch, keys, enc, prefix, len(exp)).check(torch, exp)
    if count > 1:
        assert len(py_select(keys, enc, b"a")) > count // 8 and len(py_select(keys, enc, b"ab:")) > count // 64
    # a dead item whose key matches is not selected, an expired one would be (no time arrays here)
    enc[:] = ENC_NULL
    Select(torch, keys, enc, keys[0][:1], 5).check(torch, [])


@pytest.mark.gpu
def test_select_past_the_carry_chunk(torch):
    # 2048 tiles of 1024 items and one more: the scan of the tile counts takes a second piece
    count = 2048 * 1024 + 1
    rs = np.random.RandomState(0xCA44)
    kl = rs.randint(1, 9, count).astype(np.uint32)
    koff = np.concatenate([[0], np.cumsum(kl[:-1], dtype=np.int64)]).astype(np.int64) + 3
    keys = np.concatenate([np.zeros(3, np.uint8), np.frombuffer(b"ab:", np.uint8)[rs.randint(0, 3, int(kl.sum()))],
                           np.zeros(8, np.uint8)])
    enc = rs.choice([ENC_PLAIN, ENC_LZF, ENC_NULL], count).astype(np.uint8)
    keys[koff[-1]:koff[-1] + 2] = np.frombuffer(b"b:", np.uint8)      # the item alone in the last tile matches
    kl[-1], enc[-1] = max(kl[-1], 2), ENC_PLAIN
    exp = np.nonzero((enc != ENC_NULL) & (kl >= 2) & (keys[koff] == ord("b")) & (keys[koff + 1] == ord(":")))[0]
    assert exp[-1] == count - 1 and len(exp) > count // 20
    cap = len(exp) + 5
    sel = torch.full((cap + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    res = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    w = gibson_amd.store_select_prefix(_u8(torch, keys), _i64(torch, koff), _i32(torch, kl), _u8(torch, enc),
                                       _u8(torch, np.frombuffer(b"b:", np.uint8)), sel[:cap], res)
    torch.cuda.synchronize()
    del w
    got = sel.cpu().numpy().view(np.uint32)
    assert res.cpu().numpy().tolist() == [len(exp), len(exp)]
    assert (got[:len(exp)] == exp).all() and (got[len(exp):cap] == PAD).all() and (got[cap:] == 0x5A5A5A5A).all()


@pytest.mark.gpu
def test_select_of_a_sparse_store_past_one_piece_of_the_carry_scan(torch):
    # 2 048 tiles of 1 024 items are one piece of the scan over the tile counts; the carry between
    # pieces shows only past that.  A store of dead items, with live ones at both ends and around the
    # seam; a dead item's key matches the prefix too
    seam = 2048 * 1024
    count = seam + 1025
    rnd = random.Random(0x5E1EC7)
    fixed = [0, 1, 1023, 1024, seam - 1, seam, seam + 1, count - 1]
    live = set(fixed) | set(rnd.sample(range(2, seam - 1), 150)) | set(rnd.sample(range(seam + 2, count - 1), 150))
    live = sorted(live)
    keys = np.tile(np.frombuffer(b"ab:z", np.uint8), count)
    enc = np.full(count, ENC_NULL, np.uint8)
    exp = []
    for i in live:
        enc[i] = rnd.choice([ENC_PLAIN, ENC_LZF, ENC_NUMBER])
        if i in fixed or rnd.random() < 2 / 3:
            exp.append(i)
        else:
            keys[4 * i:4 * i + 4] = np.frombuffer(b"a:bz", np.uint8)
    assert len(live) > 300 and len(exp) < len(live) and sum(1 for i in exp if i >= seam) > 50
    d_keys = _u8(torch, np.concatenate([np.zeros(3, np.uint8), keys, np.zeros(8, np.uint8)]))
    d_koff = _i64(torch, np.arange(count, dtype=np.int64) * 4 + 3)
    d_klen, d_enc = _i32(torch, np.full(count, 4, np.uint32)), _u8(torch, enc)
    d_prefix = _u8(torch, np.frombuffer(b"ab:", np.uint8))
    wsize = int(gibson_amd.lib().lzf_gpu_store_select_work_size(count))
    for cap in (len(exp) + 9, len(exp) // 2):
        sel = torch.full((cap + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        res = torch.full((2,), -1, dtype=torch.int32, device="cuda")
        work = torch.full((wsize + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
        gibson_amd.store_select_prefix(d_keys, d_koff, d_klen, d_enc, d_prefix, sel[:cap], res, work=work[:wsize])
        torch.cuda.synchronize()
        got = sel.cpu().numpy().view(np.uint32)
        k = min(len(exp), cap)
        assert res.cpu().numpy().tolist() == [k, len(exp)]
        assert got[:k].tolist() == exp[:k]
        assert (got[k:cap] == PAD).all() and (got[cap:] == 0x5A5A5A5A).all()
        assert (work[wsize:].cpu().numpy() == GUARD).all()


# 8
def select_list(torch, d, prefix, cap):
    sel = torch.full((cap,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    res = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    w = gibson_amd.store_select_prefix(d.keys, d.koff, d.klen, d.enc, _u8(torch, np.frombuffer(prefix, np.uint8)),
                                       sel, res)
    return sel, res, w


@pytest.fixture(scope="module")
def chained(main):
    """the main store under colliding keys, and a prefix with valid, dead and
    expired matches"""
    h = main["host"].copy()
    h = Host(h.arena, h.off, h.size, h.enc, h.vlen, select_keys(h.n, 0xC4A1))
    prefix = b"a"
    match_all = [i for i, k in enumerate(h.keys) if k.startswith(prefix)]
    match = py_select(h.keys, h.enc, prefix)
    valid, expired, skipped = model(match, h.enc, h.n, main["time"], main["ttl"], NOW)
    assert len(valid) >= 20 and len(expired) >= 10 and not skipped and len(match_all) - len(match) >= 10
    return {"host": h, "prefix": prefix, "match": match, "valid": valid, "expired": expired}


@pytest.mark.gpu
def test_select_count_and_mdel(torch, main, chained):
    h, match, valid, expired = chained["host"], chained["match"], chained["valid"], chained["expired"]
    d = Dev(torch, h, main["time"], main["ttl"], key_shift=3)
    sel, res, w = select_list(torch, d, chained["prefix"], h.n)
    result = torch.full((2, 2), -1, dtype=torch.int64, device="cuda")
    gibson_amd.store_count(sel, d.enc, d.time, d.ttl, NOW, result[0], last_access=d.last)
    torch.cuda.synchronize()
    assert res.cpu().numpy().tolist() == [len(match), len(match)]
    assert result[0].cpu().numpy().tolist() == [len(valid), len(expired)]      # the model's COUNT
    check_side_effects(d, h.enc, valid, expired)
    # a second COUNT finds the same valid items and nothing left to expire
    gibson_amd.store_count(sel, d.enc, None, None, NOW, result[1])
    # MDEL: count, then delete over the same list
    d = Dev(torch, h, main["time"], main["ttl"], key_shift=3)
    gibson_amd.store_count(sel, d.enc, d.time, d.ttl, NOW, result[0], last_access=d.last)
    gibson_amd.store_delete(sel, d.enc)
    torch.cuda.synchronize()
    del w
    assert result[1].cpu().numpy().tolist() == [len(valid), 0]
    assert int(result[0, 0].item()) == len(valid)                     # the reply of gbQueryMultiDelHandler
    assert (d.enc.cpu().numpy() == h.dead(match).enc).all()           # exactly the model's MDEL store
    # COUNT of nothing is 0, an ordinary result
    gibson_amd.store_count(_i32(torch, np.array([h.n, PAD], np.uint32)), d.enc, d.time, d.ttl, NOW, result[0])
    torch.cuda.synchronize()
    assert result[0].cpu().numpy().tolist() == [0, 0]


@pytest.mark.gpu
def test_select_mttl(torch, main, chained):
    h, valid, expired = chained["host"], chained["valid"], chained["expired"]
    d = Dev(torch, h, main["time"], main["ttl"])
    sel, res, w = select_list(torch, d, chained["prefix"], h.n + 9)
    result = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    gibson_amd.store_mttl(sel, 4321, d.enc, d.time, d.ttl, NOW + 3, result, last_access=d.last)
    torch.cuda.synchronize()
    del w
    v2, e2, _ = model(chained["match"], h.enc, h.n, main["time"], main["ttl"], NOW + 3)
    assert result.cpu().numpy().tolist() == [len(v2), len(e2)]
    check_side_effects(d, h.enc, v2, e2, now=NOW + 3)
    time, ttl = main["time"].copy(), main["ttl"].copy()
    time[np.array(v2)] = NOW + 3
    ttl[np.array(v2)] = 4321
    assert (d.time.cpu().numpy() == time).all() and (d.ttl.cpu().numpy() == ttl).all()


@pytest.mark.gpu
def test_select_mget(torch, oracle, main, chained):
    h, valid, expired = chained["host"], chained["valid"], chained["expired"]
    exp = expect_frame(oracle, h, valid, 64 << 20, True)
    d = Dev(torch, h, main["time"], main["ttl"], key_shift=1)
    sel, res, w = select_list(torch, d, chained["prefix"], len(chained["match"]) + 33)
    r = Mget(torch, d, sel, len(exp) + 1)                             # the list never leaves the device
    r.check(torch, exp, [len(valid), len(expired), 33, OK])
    del w
    check_side_effects(d, h.enc, valid, expired)
