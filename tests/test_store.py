"""The device SET path (lzf_gpu_set_store): gbSingleSet's store decision and
the dense packing of a batch into a store arena in HBM, against the oracle's
streams and plain Python; the STATS fold (lzf_host_store_stats) against the
recurrence of src/query.c:400-405.  The bar is bit-exact."""
import ctypes
import random
import struct

import numpy as np
import pytest

from tests.oracle_lib import synth

try:                                    # before liblzf_hip.so loads: one HIP runtime in the process
    import torch as _torch  # noqa: F401
except ImportError:
    _torch = None

import gibson_amd

ENC_PLAIN, ENC_LZF, ENC_NULL = 0, 1, 0xFF
NEW_NAMES = ("lzf_gpu_set_store_work_size", "lzf_gpu_set_store", "lzf_host_store_stats")


def needcompr(n):
    """out_len of src/query.c:384-391 as gb_needcompr states it"""
    return min((n - 4) & 0xFFFFFFFF, n + n // 16 + 8)


def expect_items(oracle, values, compression, max_in_len=None):
    """[(enc, stored bytes, why)]: why is "lzf", "failed" (compressed, no
    stream), "small" (at or below the threshold) or "bound" (past max_in_len)"""
    out = []
    for v in values:
        n = len(v)
        if max_in_len is not None and n > max_in_len:
            out.append((ENC_PLAIN, v, "bound"))
        elif n > compression:
            s = oracle.compress(v, needcompr(n))
            out.append((ENC_LZF, s, "lzf") if s else (ENC_PLAIN, v, "failed"))
        else:
            out.append((ENC_PLAIN, v, "small"))
    return out


# ---- CPU ---------------------------------------------------------------------

def test_library_exports_the_store_calls():
    L = gibson_amd.lib()
    for n in NEW_NAMES:
        assert hasattr(L, n), n
        assert n in gibson_amd.lzf.EXPORTS
    for n in ("set_store_work", "set_store", "store_stats"):
        assert callable(getattr(gibson_amd, n)), n
    assert (gibson_amd.STORE_OK, gibson_amd.STORE_FULL, gibson_amd.STORE_EWORK) == (0, 1, 2)


def test_set_store_rejects_bad_arguments_without_device():
    # argument validation happens before any HIP call, so this runs on CPU
    L = gibson_amd.lib()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(ptrs, count=1, max_in_len=16, store_cap=64):
        i, io, il, st, su, vo, vs, en, sta, wk = ptrs
        return L.lzf_gpu_set_store(i, io, il, count, max_in_len, 64, 0, st, store_cap, su, vo, vs, en, sta, wk, null)

    for k in range(10):                              # a NULL pointer in each position
        ptrs = [p] * 10
        ptrs[k] = null
        assert call(ptrs) == -1, k
    assert call([p] * 10, count=0) == -1
    assert call([p] * 10, max_in_len=(64 << 20) + 1) == -1
    assert call([p] * 10, store_cap=0) == -1


def test_set_store_work_size():
    ws = gibson_amd.lib().lzf_gpu_set_store_work_size
    for count, nbytes in [(1, 0), (1, 1), (3000, 838958), (300000, 6 << 20), (1 << 20, 4 << 30)]:
        assert ws(count, nbytes) >= nbytes + 8 * count
        assert ws(count + 1, nbytes) >= ws(count, nbytes)          # monotone in both
        assert ws(count + 5000, nbytes) > ws(count, nbytes)
        assert ws(count, nbytes + 1) >= ws(count, nbytes)
        assert ws(count, nbytes + 4096) > ws(count, nbytes)
    top = ws(2**32 - 1, 2**40)                                     # 64-bit arithmetic: no wrap
    assert 2**40 + 8 * (2**32 - 1) <= top < 2**64 - 1
    assert top >= ws(2**32 - 2, 2**40) and top >= ws(2**32 - 1, 2**40 - 1)


def _py_stats(enc, size, vlen, avg=0.0, n=0):
    # src/query.c:400-405
    for e, c, v in zip(enc, size, vlen):
        if e != ENC_LZF:
            continue
        rate = 100.0 - (c * 100.0) / v
        avg = rate if avg == 0 else (avg + rate) / 2.0
        n += 1
    return avg, n


def test_store_stats_matches_the_recurrence():
    bits = lambda x: struct.pack("<d", x)
    # the first LZF value sets the mean; later ones average; a stream longer
    # than its value (1 B stored as 2) gives a negative rate; PLAIN and NULL
    # entries are skipped
    enc = [ENC_PLAIN, ENC_LZF, ENC_NULL, ENC_LZF, ENC_LZF, ENC_PLAIN, ENC_LZF, ENC_LZF]
    size = [10, 1500, 0, 2, 333, 7, 4000, 3]
    vlen = [10, 4096, 55, 1, 1000, 7, 4097, 2]
    got = gibson_amd.store_stats(np.array(enc, np.uint8), np.array(size, np.uint32), np.array(vlen, np.uint32))
    exp = _py_stats(enc, size, vlen)
    assert bits(got[0]) == bits(exp[0]) and got[1] == exp[1] == 5
    first = gibson_amd.store_stats(np.array(enc[:2], np.uint8), np.array(size[:2], np.uint32),
                                   np.array(vlen[:2], np.uint32))
    assert bits(first[0]) == bits(100.0 - (1500 * 100.0) / 4096) and first[1] == 1
    neg = gibson_amd.store_stats(np.array([ENC_LZF], np.uint8), np.array([2], np.uint32), np.array([1], np.uint32))
    assert neg == (-100.0, 1)
    # nothing stored LZF: untouched
    assert gibson_amd.store_stats(np.array([ENC_PLAIN, ENC_NULL], np.uint8), np.array([3, 0], np.uint32),
                                  np.array([3, 9], np.uint32), 12.5, 4) == (12.5, 4)
    # a start from a non-zero mean, over many pseudo-random entries
    rnd = random.Random(0x57A75)
    enc = [rnd.choice([ENC_PLAIN, ENC_LZF, ENC_LZF, ENC_NULL]) for _ in range(5000)]
    vlen = [rnd.randint(1, 70000) for _ in range(5000)]
    size = [rnd.randint(1, v + v // 32 + 1) for v in vlen]
    got = gibson_amd.store_stats(np.array(enc, np.uint8), np.array(size, np.uint32), np.array(vlen, np.uint32),
                                 37.25, 11)
    exp = _py_stats(enc, size, vlen, 37.25, 11)
    assert bits(got[0]) == bits(exp[0]) and got[1] == exp[1]
    L = gibson_amd.lib()
    assert L.lzf_host_store_stats(None, None, None, 1, None, None) == -1


# ---- GPU ---------------------------------------------------------------------

FILL = 0xA5
GUARD = 0x5A
BASE = 7


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    gibson_amd.lib()
    return t


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


class Batch:
    """a batch in HBM: the input arena packed with no alignment, so every
    source offset mod 16 occurs"""

    def __init__(self, torch, values):
        self.n = len(values)
        self.len = np.array([len(v) for v in values], np.uint32)
        self.off = np.concatenate([[0], np.cumsum(self.len[:-1], dtype=np.int64)]).astype(np.int64)
        self.nbytes = int(self.len.sum())
        arena = np.frombuffer(b"".join(values) + b"\0", np.uint8).copy()
        self.d_in = torch.from_numpy(arena).cuda()
        self.d_off = torch.from_numpy(self.off).cuda()
        self.d_len = _i32(torch, self.len)
        self.d_voff = torch.full((self.n,), -1, dtype=torch.int64, device="cuda")
        self.d_vsize = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.d_enc = torch.full((self.n,), 0x77, dtype=torch.uint8, device="cuda")

    def results(self):
        return (self.d_enc.cpu().numpy(), self.d_vsize.cpu().numpy().view(np.uint32).astype(np.int64),
                self.d_voff.cpu().numpy())


class Store:
    def __init__(self, torch, room, base=BASE):
        self.t = torch.full((room,), FILL, dtype=torch.uint8, device="cuda")
        self.used = torch.tensor([base], dtype=torch.int64, device="cuda")
        self.status = torch.full((1,), -1, dtype=torch.int32, device="cuda")


def set_store(torch, b, st, compression, max_in_len=None, cap=None, in_bytes=None, guard=0):
    """one lzf_gpu_set_store call; no synchronisation.  -> (work, size of work)"""
    in_bytes = b.nbytes if in_bytes is None else in_bytes
    wsize = int(gibson_amd.lib().lzf_gpu_set_store_work_size(b.n, in_bytes))
    buf = torch.full((wsize + guard,), GUARD, dtype=torch.uint8, device="cuda")
    gibson_amd.set_store(b.d_in, b.d_off, b.d_len, compression, int(b.len.max()) if max_in_len is None else max_in_len,
                         in_bytes, st.t if cap is None else st.t[:cap], st.used, b.d_voff, b.d_vsize, b.d_enc,
                         st.status, work=buf[:wsize])
    b.work = buf                             # alive until the caller has synchronised
    return buf, wsize


def check_stored(b, st, exp, base):
    """every per-value property of a successful batch, in numpy"""
    enc, vsize, voff = b.results()
    e_enc = np.array([e for e, _, _ in exp], np.uint8)
    e_size = np.array([len(s) for _, s, _ in exp], np.int64)
    e_off = base + np.concatenate([[0], np.cumsum(e_size[:-1])])
    total = int(e_size.sum())
    assert int(st.status.item()) == 0
    assert int(st.used.item()) == base + total
    bad = np.nonzero(enc != e_enc)[0]
    assert not len(bad), (len(bad), bad[:5], enc[bad[:5]], e_enc[bad[:5]])
    bad = np.nonzero(vsize != e_size)[0]
    assert not len(bad), (len(bad), bad[:5], vsize[bad[:5]], e_size[bad[:5]])
    bad = np.nonzero(voff != e_off)[0]
    assert not len(bad), (len(bad), bad[:5], voff[bad[:5]], e_off[bad[:5]])
    got = st.t.cpu().numpy()
    packed = np.frombuffer(b"".join(s for _, s, _ in exp), np.uint8)
    bad = np.nonzero(got[base:base + total] != packed)[0]
    if len(bad):
        i = int(np.searchsorted(e_off, base + bad[0], side="right")) - 1
        raise AssertionError((len(bad), "first wrong byte", int(bad[0]), "value", i, int(b.len[i]), exp[i][2]))
    assert (got[:base] == FILL).all() and (got[base + total:] == FILL).all()
    return total


PLANTED = [1, 2, 3, 4, 5, 8, 64, 65, 4096, 4097, 16384, 16385, 65536, 65537, 70000, 300003]


@pytest.fixture(scope="module")
def mixed_case(oracle):
    """the 3000-value batch and the oracle's decisions at both thresholds"""
    rnd = random.Random(0x5704E)
    count = 3000
    sizes = [rnd.randint(1, 200) for _ in range(count)]
    for i, n in zip(rnd.sample(range(count), len(PLANTED)), PLANTED):
        sizes[i] = n
    values = [synth(i % 6, 0x5EED5704, i, n) for i, n in enumerate(sizes)]
    exp = {c: expect_items(oracle, values, c) for c in (0, 64)}
    for c in (0, 64):
        why = [w for _, _, w in exp[c]]
        assert why.count("lzf") >= 1000 and why.count("failed") >= 500
    longer = sum(1 for (e, s, _), v in zip(exp[0], values) if e == ENC_LZF and len(s) > len(v))
    assert longer >= 1                       # 1-3 byte values: the stream is longer than the value
    # the batch as the oracle decides it: LZF, PLAIN by failed compression,
    # PLAIN at or below the threshold, packed bytes (of 838958 input bytes)
    assert sum(sizes) == 838958 and longer == 46
    for c, table in ((0, (1605, 1395, 0, 522398)), (64, (1410, 616, 974, 524729))):
        why = [w for _, _, w in exp[c]]
        assert (why.count("lzf"), why.count("failed"), why.count("small"),
                sum(len(s) for _, s, _ in exp[c])) == table
    return {"values": values, "sizes": sizes, "exp": exp}


@pytest.mark.gpu
@pytest.mark.parametrize("compression", [0, 64])
def test_mixed_batch_bit_exact(torch, mixed_case, compression):
    exp = mixed_case["exp"][compression]
    total = sum(len(s) for _, s, _ in exp)
    b = Batch(torch, mixed_case["values"])
    st = Store(torch, BASE + total + 100)    # base 7: the store is misaligned against every tile
    set_store(torch, b, st, compression)
    torch.cuda.synchronize()
    assert check_stored(b, st, exp, BASE) == total


@pytest.mark.gpu
@pytest.mark.parametrize("pack,tile_kb", [("realign", None), (None, "4"), (None, "1024")])
def test_pack_forms_bit_exact(torch, mixed_case, monkeypatch, pack, tile_kb):
    # the pack kernel's diagnostic forms (realigned loads, the smallest and the
    # largest tile) store the same bytes
    if pack:
        monkeypatch.setenv("LZF_GPU_STORE_PACK", pack)
    if tile_kb:
        monkeypatch.setenv("LZF_GPU_STORE_TILE_KB", tile_kb)
    exp = mixed_case["exp"][64]
    b = Batch(torch, mixed_case["values"])
    st = Store(torch, BASE + sum(len(s) for _, s, _ in exp) + 100)
    set_store(torch, b, st, 64)
    torch.cuda.synchronize()
    check_stored(b, st, exp, BASE)


@pytest.mark.gpu
@pytest.mark.parametrize("bound", [4096, 65536])
def test_routed_generations_bit_exact(torch, oracle, mixed_case, monkeypatch, bound):
    # with the batch-size threshold lifted the compress step takes the lane
    # (<= 16 KiB) and the table (<= 64 KiB) generations, which see the values at
    # or below the threshold as 0-length values
    monkeypatch.setenv("LZF_GPU_LANE_MIN", "0")
    monkeypatch.delenv("LZF_GPU_KERNEL", raising=False)
    keep = [i for i, n in enumerate(mixed_case["sizes"]) if n <= bound]
    values = [mixed_case["values"][i] for i in keep]
    exp = [mixed_case["exp"][64][i] for i in keep]
    assert max(len(v) for v in values) == bound
    b = Batch(torch, values)
    st = Store(torch, BASE + sum(len(s) for _, s, _ in exp) + 100)
    set_store(torch, b, st, 64)
    torch.cuda.synchronize()
    check_stored(b, st, exp, BASE)


@pytest.fixture(scope="module")
def tiny_case(oracle):
    count = 300000
    rs = np.random.RandomState(7)
    sizes = rs.randint(1, 41, count)
    zero = np.concatenate([rs.choice(count, 25, replace=False), np.arange(123456, 123456 + 25)])
    sizes[zero] = 0                          # 50 zero-length values, 25 of them one run
    sizes = [int(n) for n in sizes]
    values = [synth(5 if i & 1 else 0, 0x5EED5705, i, n) for i, n in enumerate(sizes)]
    exp = expect_items(oracle, values, 24)
    why = [w for _, _, w in exp]
    assert min(why.count("lzf"), why.count("failed"), why.count("small")) >= 10000
    return values, exp


@pytest.mark.gpu
def test_many_tiny_values(torch, tiny_case):
    # 293 scan tiles (the carry scan loops twice), runs of values below a
    # granule, zero-size values whose offsets tie
    values, exp = tiny_case
    total = sum(len(s) for _, s, _ in exp)
    b = Batch(torch, values)
    st = Store(torch, BASE + total + 100)
    set_store(torch, b, st, 24)
    torch.cuda.synchronize()
    check_stored(b, st, exp, BASE)


@pytest.mark.gpu
def test_append_without_synchronisation(torch, mixed_case):
    values, exp = mixed_case["values"], mixed_case["exp"][0]
    half = len(values) // 2
    first = sum(len(s) for _, s, _ in exp[:half])
    total = sum(len(s) for _, s, _ in exp)
    b1, b2 = Batch(torch, values[:half]), Batch(torch, values[half:])
    st = Store(torch, BASE + total + 100)
    status2 = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    w1 = set_store(torch, b1, st, 0)
    w2 = gibson_amd.set_store(b2.d_in, b2.d_off, b2.d_len, 0, int(b2.len.max()), b2.nbytes, st.t, st.used, b2.d_voff,
                         b2.d_vsize, b2.d_enc, status2)
    torch.cuda.synchronize()
    del w1, w2
    assert int(st.status.item()) == 0 and int(status2.item()) == 0
    assert int(st.used.item()) == BASE + total
    assert int(b2.d_voff[0].item()) == BASE + first
    got = st.t.cpu().numpy()
    assert bytes(got[BASE:BASE + total]) == b"".join(s for _, s, _ in exp)
    assert (got[:BASE] == FILL).all() and (got[BASE + total:] == FILL).all()
    for b, e, at in ((b1, exp[:half], BASE), (b2, exp[half:], BASE + first)):
        enc, vsize, voff = b.results()
        assert (enc == np.array([x for x, _, _ in e], np.uint8)).all()
        sz = np.array([len(s) for _, s, _ in e], np.int64)
        assert (vsize == sz).all() and (voff == at + np.concatenate([[0], np.cumsum(sz[:-1])])).all()


def check_refused(b, st, status):
    assert int(st.status.item()) == status
    assert int(st.used.item()) == BASE
    assert (st.t.cpu().numpy() == FILL).all()
    enc, vsize, _ = b.results()
    assert (enc == ENC_NULL).all() and (vsize == 0).all()


@pytest.mark.gpu
def test_refusal(torch, mixed_case):
    values, exp = mixed_case["values"], mixed_case["exp"][0]
    total = sum(len(s) for _, s, _ in exp)
    b = Batch(torch, values)
    st = Store(torch, BASE + total + 100)
    set_store(torch, b, st, 0, cap=BASE + total)             # exactly full: taken
    torch.cuda.synchronize()
    check_stored(b, st, exp, BASE)
    b = Batch(torch, values)
    st = Store(torch, BASE + total + 100)
    set_store(torch, b, st, 0, cap=BASE + total - 1)         # one byte short: LZF_STORE_FULL
    torch.cuda.synchronize()
    check_refused(b, st, 1)
    b = Batch(torch, values)
    st = Store(torch, BASE + total + 100)
    buf, wsize = set_store(torch, b, st, 0, in_bytes=b.nbytes // 2, guard=1 << 16)   # LZF_STORE_EWORK
    torch.cuda.synchronize()
    check_refused(b, st, 2)
    assert (buf[wsize:].cpu().numpy() == GUARD).all()


@pytest.mark.gpu
def test_understated_bound(torch, oracle, mixed_case):
    # max_in_len 4096 with the 70000 B and 300003 B values present: both stored
    # PLAIN with their own bytes, every other value as before
    keep = [i for i, n in enumerate(mixed_case["sizes"]) if n <= 4096 or n in (70000, 300003)]
    values = [mixed_case["values"][i] for i in keep]
    exp = expect_items(oracle, values, 0, max_in_len=4096)
    big = [k for k, (_, _, w) in enumerate(exp) if w == "bound"]
    assert sorted(len(values[k]) for k in big) == [70000, 300003]
    assert [exp[k] for k in range(len(exp)) if k not in big] == \
           [mixed_case["exp"][0][i] for k, i in enumerate(keep) if k not in big]
    b = Batch(torch, values)
    st = Store(torch, BASE + sum(len(s) for _, s, _ in exp) + 100)
    set_store(torch, b, st, 0, max_in_len=4096)
    torch.cuda.synchronize()
    check_stored(b, st, exp, BASE)


@pytest.mark.gpu
def test_round_trip_through_the_frame(torch, oracle):
    rnd = random.Random(0xF4A3E)
    sizes = [rnd.choice([rnd.randint(1, 300), rnd.randint(300, 20000)]) for _ in range(500)]
    values = [synth(i % 6, 0x5EED5706, i, n) for i, n in enumerate(sizes)]
    keys = [bytes(rnd.choice(b"abcdefghij:_0123456789") for _ in range(rnd.randint(1, 40))) for _ in sizes]
    exp = expect_items(oracle, values, 64)
    encs = [e for e, _, _ in exp]
    assert encs.count(ENC_LZF) > 100 and encs.count(ENC_PLAIN) > 100
    frame_exp = oracle.kv_frame([(k, e, s) for k, (e, s, _) in zip(keys, exp)], 500, 64 << 20, 1 << 20)
    assert frame_exp is not None
    b = Batch(torch, values)
    st = Store(torch, sum(len(s) for _, s, _ in exp) + 100, base=0)
    set_store(torch, b, st, 64)
    # the output arrays unchanged into the frame, in_len as val_len
    kl = np.array([len(k) for k in keys], np.uint32)
    d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda()
    d_koff = torch.from_numpy(np.concatenate([[0], np.cumsum(kl[:-1], dtype=np.int64)]).astype(np.int64)).cuda()
    max_response = len(frame_exp) + 64
    frame = torch.zeros(max_response + 7, dtype=torch.uint8, device="cuda")
    flen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    gibson_amd.kv_frame(d_keys, d_koff, _i32(torch, kl), st.t, b.d_voff, b.d_vsize, b.d_enc, b.d_len, 500,
                        max(sizes), frame, max_response, flen)
    torch.cuda.synchronize()
    assert int(st.status.item()) == 0
    assert bytes(frame[:int(flen.item())].cpu().numpy()) == frame_exp


@pytest.mark.gpu
def test_single_one_byte_value(torch, oracle):
    exp = expect_items(oracle, [b"x"], 0)
    assert exp == [(ENC_LZF, b"\x00\x78", "lzf")]            # the wrapped vlen - 4: no limit, as the reference
    b = Batch(torch, [b"x"])
    st = Store(torch, 64, base=0)
    set_store(torch, b, st, 0)
    torch.cuda.synchronize()
    check_stored(b, st, exp, 0)
    assert bytes(st.t[:2].cpu().numpy()) == b"\x00\x78"
    assert int(b.d_enc[0].item()) == ENC_LZF and int(b.d_vsize[0].item()) == 2


@pytest.mark.gpu
def test_store_stats_equal_gb_set_batch(torch, mixed_case):
    from gibson_amd import gb
    values = mixed_case["values"]
    stats = gb.Stats()
    gb.set_batch(values, 64, stats)
    b = Batch(torch, values)
    st = Store(torch, BASE + sum(len(s) for _, s, _ in mixed_case["exp"][64]) + 100)
    set_store(torch, b, st, 64)
    torch.cuda.synchronize()
    avg, n = gibson_amd.store_stats(b.d_enc, b.d_vsize, b.d_len)
    assert n == stats.ncompressed and n >= 1000
    assert struct.pack("<d", avg) == struct.pack("<d", stats.compravg)
