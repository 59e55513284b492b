"""Size-class routing of mixed-size batches: the class rule, the stable
partition (host twin on CPU, the kernels on the GPU), and the mixed compress /
decompress calls -- device pointers, host memory, and the gb_* opt-in --
against the oracle and the uniform calls.  The bar is bit-exact: identical
streams, lengths and errno, per index."""
import ctypes
import errno
import random

import numpy as np
import pytest

from tests.oracle_lib import synth

import gibson_amd
from gibson_amd import KIND_COMPRESS, KIND_DECOMPRESS, NCLASS

EDGES = {KIND_COMPRESS: [4096, 8192, 16384, 65536], KIND_DECOMPRESS: [4096, 16384]}
NEW_NAMES = ("lzf_gpu_size_class", "lzf_gpu_size_partition_work_size", "lzf_gpu_size_partition",
             "lzf_host_size_partition", "lzf_gpu_mixed_work_size", "lzf_gpu_compress_mixed",
             "lzf_gpu_decompress_mixed", "lzf_gpu_mixed_last_plan", "lzf_host_compress_mixed",
             "lzf_host_decompress_mixed")


def np_classes(lens, bound, kind):
    c = np.searchsorted(np.array(EDGES[kind], np.uint64), lens.astype(np.uint64), side="left")
    return np.where(lens > bound, NCLASS, c)


def np_partition(lens, bound, kind):
    cls = np_classes(lens, bound, kind)
    perm = np.argsort(cls, kind="stable").astype(np.uint32)
    cc = np.bincount(cls, minlength=NCLASS + 1).astype(np.uint32)
    cm = np.array([int(lens[cls == c].max()) if cc[c] else 0 for c in range(NCLASS + 1)], np.uint32)
    return perm, cc, cm


def length_patterns(count, kind, seed):
    """(name, lengths, bound): random over all classes, sorted both ways (whole
    tiles of one class, empty tiles of the others), one class, all refused."""
    rnd = np.random.RandomState(seed)
    top = 200000
    # log-uniform, so every class gets values, with the edges themselves mixed in
    ln = np.exp(rnd.uniform(0, np.log(top), count)).astype(np.uint32)
    edge = np.array([0, 1] + [e + d for e in EDGES[kind] for d in (0, 1)], np.uint32)
    pick = rnd.rand(count) < 0.05
    ln[pick] = edge[rnd.randint(0, len(edge), int(pick.sum()))]
    bound = 150000                                   # some random values are refused
    yield "random", ln, bound
    yield "ascending", np.sort(ln), bound
    yield "descending", np.sort(ln)[::-1].copy(), bound
    yield "one-class", rnd.randint(4097, 8193, count).astype(np.uint32), bound
    yield "all-refused", rnd.randint(11, 5000, count).astype(np.uint32), 10


# ---- CPU ---------------------------------------------------------------------

def test_library_exports_the_mixed_calls():
    L = gibson_amd.lib()
    for n in NEW_NAMES:
        assert hasattr(L, n), n
        assert n in gibson_amd.lzf.EXPORTS
    for n in ("size_class", "size_partition", "host_size_partition", "compress_mixed", "decompress_mixed",
              "host_compress_mixed", "host_decompress_mixed", "mixed_last_plan"):
        assert callable(getattr(gibson_amd, n)), n


def test_size_class_edges():
    at = [0, 1, 4096, 4097, 8192, 8193, 16384, 16385, 65536, 65537, 64 << 20]
    assert [gibson_amd.size_class(n, KIND_COMPRESS) for n in at] == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert [gibson_amd.size_class(n, KIND_DECOMPRESS) for n in at] == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    assert gibson_amd.lib().lzf_gpu_size_class(1, 2) == -1


@pytest.mark.parametrize("kind", [KIND_COMPRESS, KIND_DECOMPRESS])
@pytest.mark.parametrize("count", [1, 64, 65, 2049, 70001])
def test_host_size_partition_matches_numpy(count, kind):
    for name, ln, bound in length_patterns(count, kind, 1000 + count):
        perm, cc, cm = gibson_amd.host_size_partition(ln, bound, kind)
        eperm, ecc, ecm = np_partition(ln, bound, kind)
        assert np.array_equal(cc, ecc), (name, cc, ecc)
        assert np.array_equal(cm, ecm), (name, cm, ecm)
        assert np.array_equal(perm, eperm), name
        if name == "one-class":
            assert int((cc > 0).sum()) == 1
        if name == "all-refused":
            assert cc[NCLASS] == count and np.array_equal(perm, np.arange(count))


def test_mixed_calls_reject_bad_arguments_without_device():
    # argument validation happens before any HIP call, so this runs on CPU
    L = gibson_amd.lib()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.lzf_gpu_compress_mixed(null, p, p, p, p, p, p, 1, 16, p, null) == -1
    assert L.lzf_gpu_compress_mixed(p, p, p, p, p, p, null, 1, 16, p, null) == -1
    assert L.lzf_gpu_compress_mixed(p, p, p, p, p, p, p, 0, 16, p, null) == -1
    assert L.lzf_gpu_compress_mixed(p, p, p, p, p, p, p, 1, 16, null, null) == -1
    assert L.lzf_gpu_compress_mixed(p, p, p, p, p, p, p, 1, (64 << 20) + 1, p, null) == -1
    assert L.lzf_gpu_decompress_mixed(p, p, p, p, p, p, p, null, 1, 16, p, null) == -1
    assert L.lzf_gpu_decompress_mixed(p, p, p, p, p, p, p, p, 0, 16, p, null) == -1
    assert L.lzf_gpu_decompress_mixed(p, p, p, p, p, p, p, p, 1, 16, null, null) == -1
    assert L.lzf_gpu_size_partition(p, 0, 16, 0, p, p, p, p, null) == -1
    assert L.lzf_gpu_size_partition(p, 1, 16, 0, p, p, p, null, null) == -1
    assert L.lzf_gpu_size_partition(p, 1, 16, 7, p, p, p, p, null) == -1
    assert L.lzf_host_size_partition(null, 1, 16, 0, p, p, p) == -1
    assert L.lzf_host_size_partition(p, 0, 16, 0, p, p, p) == -1
    assert L.lzf_host_compress_mixed(null, p, p, p, p, p, p, 1) == -1
    assert L.lzf_host_decompress_mixed(p, p, p, p, p, p, p, null, 1) == -1
    assert L.lzf_host_decompress_mixed(p, p, p, p, p, p, p, p, 0) == -1
    assert L.lzf_gpu_size_partition_work_size(1) > 0 and L.lzf_gpu_mixed_work_size(1) > 0


# ---- GPU ---------------------------------------------------------------------

FILL = 0xA5


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    gibson_amd.lib()
    return t


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 64, 65, 2048, 2049, 4113, 70001, 1200001])
def test_device_partition_equals_host(torch, count):
    # 1 200 001 lengths are 586 tiles: 3516 table entries, past one workgroup's
    # 1024-entry piece of the scan
    for kind in (KIND_COMPRESS, KIND_DECOMPRESS):
        for name, ln, bound in length_patterns(count, kind, 7 + count):
            eperm, ecc, ecm = gibson_amd.host_size_partition(ln, bound, kind)
            perm, cc, cm = gibson_amd.size_partition(_i32(torch, ln), bound, kind)
            torch.cuda.synchronize()
            cc, cm = cc.cpu().numpy().view(np.uint32), cm.cpu().numpy().view(np.uint32)
            assert np.array_equal(cc, ecc), (name, kind, cc, ecc)
            assert np.array_equal(cm, ecm), (name, kind, cm, ecm)
            assert np.array_equal(perm.cpu().numpy().view(np.uint32), eperm), (name, kind)


def _layout(sizes, align=16):
    off = np.zeros(len(sizes), np.int64)
    pos = 0
    for i, n in enumerate(sizes):
        off[i] = pos
        pos += (max(int(n), 1) + align - 1) // align * align
    return off, max(pos, 16)


def run_compress_mixed(torch, values, caps, max_in_len):
    """-> ([stream or None], out arena, out_off, out_len) through lzf_gpu_compress_mixed"""
    from tests.gpu_batch import _pack
    arena, in_off = _pack(values)
    out_off, out_size = _layout(caps)
    d_out = torch.full((out_size,), FILL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((len(values),), -1, dtype=torch.int32, device="cuda")
    work = gibson_amd.compress_mixed(torch.from_numpy(arena).cuda(), torch.from_numpy(in_off).cuda(),
                                     _i32(torch, [len(v) for v in values]), d_out, torch.from_numpy(out_off).cuda(),
                                     _i32(torch, caps), d_len, max_in_len)
    torch.cuda.synchronize()
    del work
    out, lens = d_out.cpu().numpy(), d_len.cpu().numpy().astype(np.int64)
    return [bytes(out[o:o + l]) if l > 0 else None for o, l in zip(out_off, lens)], out, out_off, lens


def run_decompress_mixed(torch, streams, caps, max_out_cap):
    """-> ([(bytes or None, errno)], out arena, out_off) through lzf_gpu_decompress_mixed"""
    from tests.gpu_batch import _pack
    arena, in_off = _pack(streams)
    out_off, out_size = _layout(caps)
    d_out = torch.full((out_size,), FILL, dtype=torch.uint8, device="cuda")
    d_len = torch.full((len(streams),), -1, dtype=torch.int32, device="cuda")
    d_err = torch.full((len(streams),), -1, dtype=torch.int32, device="cuda")
    work = gibson_amd.decompress_mixed(torch.from_numpy(arena).cuda(), torch.from_numpy(in_off).cuda(),
                                       _i32(torch, [len(s) for s in streams]), d_out,
                                       torch.from_numpy(out_off).cuda(), _i32(torch, caps), d_len, d_err, max_out_cap)
    torch.cuda.synchronize()
    del work
    out, lens, errs = d_out.cpu().numpy(), d_len.cpu().numpy().astype(np.int64), d_err.cpu().numpy()
    return [(bytes(out[o:o + l]) if l > 0 else None, int(e)) for o, l, e in zip(out_off, lens, errs)], out, out_off


MAX_IN = 300003
SPECIAL = [4096, 4097, 8192, 8193, 16384, 16385, 65536, 65537, 70000, MAX_IN, 0, 1, 2]
REFUSED = [MAX_IN + 1, 310000, 400000]


@pytest.fixture(scope="module")
def compress_case(oracle):
    """The 4113-value batch of the compress tests and the oracle's streams,
    made once: mostly 1-200 B, every class edge, two large values, the empty
    and tiny ones, three past the stated max_in_len."""
    rnd = random.Random(0x4113)
    count = 4113
    sizes = [rnd.randint(1, 200) for _ in range(count)]
    where = rnd.sample(range(count), len(SPECIAL) + len(REFUSED))
    for i, n in zip(where, SPECIAL + REFUSED):
        sizes[i] = n
    special = set(where)
    values = [synth(i % 6, 0x5EED4113, i, n) for i, n in enumerate(sizes)]
    caps = []
    for i, n in enumerate(sizes):
        roomy = n + n // 16 + 64
        if i in special:                  # decided, so every edge value yields a stream to compare
            caps.append(roomy if i % 2 else max(n - 4, 0))
        else:
            caps.append(rnd.choice([max(n - 4, 0), roomy, 0, rnd.randint(1, n)]))
    refused = [i for i in range(count) if sizes[i] > MAX_IN]
    assert len(refused) == 3
    expect = [None if (i in refused or not n or not c) else oracle.compress(v, c)
              for i, (v, n, c) in enumerate(zip(values, sizes, caps))]
    assert sum(e is None for e in expect) > 100 and sum(e is not None for e in expect) > 1000
    return {"values": values, "sizes": sizes, "caps": caps, "refused": refused, "expect": expect}


@pytest.fixture(scope="module")
def uniform_streams(torch, compress_case):
    """the uniform call's streams for the values the bound admits"""
    import os
    from tests.gpu_batch import gpu_compress
    c = compress_case
    keep = [i for i in range(len(c["values"])) if i not in c["refused"]]
    prev = os.environ.get("LZF_GPU_LANE_MIN")
    os.environ["LZF_GPU_LANE_MIN"] = "0"
    try:
        res = gpu_compress([c["values"][i] for i in keep], [c["caps"][i] for i in keep])
    finally:
        if prev is None:
            del os.environ["LZF_GPU_LANE_MIN"]
        else:
            os.environ["LZF_GPU_LANE_MIN"] = prev
    return dict(zip(keep, res))


@pytest.mark.gpu
@pytest.mark.parametrize("lane_min", ["0", None])
def test_compress_mixed_bit_exact(torch, compress_case, uniform_streams, monkeypatch, lane_min):
    c = compress_case
    if lane_min is None:
        monkeypatch.delenv("LZF_GPU_LANE_MIN", raising=False)
    else:
        monkeypatch.setenv("LZF_GPU_LANE_MIN", lane_min)
    monkeypatch.delenv("LZF_GPU_KERNEL", raising=False)
    res, out, out_off, lens = run_compress_mixed(torch, c["values"], c["caps"], MAX_IN)
    plan = gibson_amd.mixed_last_plan()
    _, ecc, ecm = np_partition(np.array(c["sizes"], np.uint32), MAX_IN, KIND_COMPRESS)
    assert plan["class_count"] == ecc.tolist() and plan["class_max"] == ecm.tolist()
    assert plan["batches"] == 5
    # lane, lane, lane, table, window64 with the threshold lifted; at the
    # product thresholds these counts are all below the crossover: window64
    assert plan["route"] == ([1, 1, 1, 2, 3, 0] if lane_min == "0" else [3, 3, 3, 3, 3, 0]), plan
    assert "mixed=5" in gibson_amd.kernel_info()
    bad = [i for i, (r, e) in enumerate(zip(res, c["expect"])) if r != e]
    assert not bad, (len(bad), [(i, c["sizes"][i], c["caps"][i]) for i in bad[:5]])
    bad = [i for i, u in uniform_streams.items() if res[i] != u]
    assert not bad, (len(bad), bad[:5])
    for i in c["refused"]:                       # out_len 0, the slot untouched
        assert lens[i] == 0
        assert (out[out_off[i]:out_off[i] + c["caps"][i]] == FILL).all(), i
    # the successes back through decompress_mixed
    ok = [i for i, r in enumerate(res) if r is not None]
    dec, _, _ = run_decompress_mixed(torch, [res[i] for i in ok], [c["sizes"][i] for i in ok], MAX_IN)
    bad = [i for i, d in zip(ok, dec) if d != (c["values"][i], 0)]
    assert not bad, (len(bad), bad[:5])


@pytest.mark.gpu
def test_decompress_mixed_against_oracle_decoder(torch, golden, oracle):
    from tests.test_oracle import decoder_cases
    rnd = random.Random(0xDEC0)
    streams, caps = [], []
    for c, s in decoder_cases(golden, oracle):      # valid, tight, truncated, corrupted, random
        streams.append(s)
        caps.append(c["out_len"])
    for k in range(1500):                           # small slots: exact, roomy, too small (E2BIG)
        n = rnd.randint(1, 300)
        v = synth(k % 6, 0x5EEDDEC0, k, n)
        streams.append(oracle.compress(v, n + n // 16 + 64))
        caps.append(rnd.choice([n, n, rnd.randint(n, 300), rnd.randint(1, n)]))
    for k, n in enumerate([4096, 4097, 16384, 16385, 70000, 300003]):
        v = synth(k % 6, 0x5EEDDEC1, k, n)
        streams.append(oracle.compress(v, n + n // 16 + 64))
        caps.append(n)
    streams.append(b"")                             # 0-length stream: its phantom control byte is read
    caps.append(64)
    max_cap = 300003
    past = [len(streams), len(streams) + 1]         # slots past the stated max_out_cap
    for k in range(2):
        v = synth(1, 0x5EEDDEC2, k, 500)
        streams.append(oracle.compress(v, 600))
        caps.append(max_cap + 1 + 5000 * k)
    order = list(range(len(streams)))
    rnd.shuffle(order)
    streams, caps = [streams[i] for i in order], [caps[i] for i in order]
    past = [order.index(i) for i in past]
    expect = [(None, errno.EINVAL) if i in past else oracle.decompress(s, c)
              for i, (s, c) in enumerate(zip(streams, caps))]
    errs = {e for _, e in expect}
    assert {0, errno.E2BIG, errno.EINVAL} <= errs
    res, out, out_off = run_decompress_mixed(torch, streams, caps, max_cap)
    bad = [(i, caps[i], expect[i][1], res[i][1]) for i in range(len(res)) if res[i] != expect[i]]
    assert not bad, (len(bad), bad[:5])
    for i in past:
        assert (out[out_off[i]:out_off[i] + caps[i]] == FILL).all(), i
    plan = gibson_amd.mixed_last_plan()
    _, ecc, ecm = np_partition(np.array(caps, np.uint32), max_cap, KIND_DECOMPRESS)
    assert plan["class_count"] == ecc.tolist() and plan["class_max"] == ecm.tolist()
    assert plan["route"] == [1, 2, 3, 0, 0, 0] and plan["batches"] == 3, plan   # tokpar, tokpar-far, pipe


@pytest.mark.gpu
def test_degenerate_plans(torch, oracle, monkeypatch):
    monkeypatch.setenv("LZF_GPU_LANE_MIN", "0")

    def check(sizes, classes):
        values = [synth(i % 6, 0x5EED0DE6, i, n) for i, n in enumerate(sizes)]
        caps = [n + n // 16 + 64 for n in sizes]
        res, _, _, _ = run_compress_mixed(torch, values, caps, max(sizes))
        assert res == [oracle.compress(v, c) for v, c in zip(values, caps)]
        plan = gibson_amd.mixed_last_plan()
        assert [k for k in range(NCLASS + 1) if plan["class_count"][k]] == classes, plan
        assert [k for k in range(NCLASS + 1) if plan["route"][k]] == classes, plan
        assert plan["batches"] == len(classes)
        assert f"mixed={len(classes)}" in gibson_amd.kernel_info().split()
        dec, _, _ = run_decompress_mixed(torch, res, sizes, max(sizes))
        assert dec == [(v, 0) for v in values]
        assert gibson_amd.mixed_last_plan()["batches"] == 1

    check([777], [0])                                         # count = 1
    check([5000 + 13 * i for i in range(200)], [1])           # one class of many values
    check([70000, 65537, 123457], [4])                        # only values past 64 KiB


@pytest.fixture
def registered():
    held = []

    def reg(a):
        gibson_amd.host_register(a)
        held.append(a)
        return a
    yield reg
    for a in held:
        gibson_amd.host_unregister(a)


def _aligned(nbytes):
    raw = np.zeros(nbytes + 8192, np.uint8)
    k = (-raw.ctypes.data) % 4096
    return raw[k:k + nbytes]


@pytest.fixture(scope="module")
def host_case(oracle):
    rnd = random.Random(600)
    sizes = [int(np.exp(rnd.uniform(0, np.log(200 * 1024)))) for _ in range(600)]
    sizes[:4] = [1, 200 * 1024, 65536, 65537]
    values = [synth(i % 6, 0x5EED0600, i, n) for i, n in enumerate(sizes)]
    caps = [max(n - 4, 0) if i % 3 else n + n // 16 + 64 for i, n in enumerate(sizes)]
    expect = [oracle.compress(v, c) if c else None for v, c in zip(values, caps)]
    return sizes, values, caps, expect


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["staged", "registered"])
def test_host_mixed_calls(torch, host_case, registered, path):
    sizes, values, caps, expect = host_case
    arena_of = (lambda n: registered(_aligned(n))) if path == "registered" else (lambda n: np.zeros(n, np.uint8))
    ln = np.array(sizes, np.uint32)
    in_off = np.concatenate([[0], np.cumsum(ln[:-1], dtype=np.uint64)]).astype(np.uint64)
    arena = arena_of(int(ln.sum()) + 16)
    for o, v in zip(in_off, values):
        arena[int(o):int(o) + len(v)] = np.frombuffer(v, np.uint8)
    cap = np.array(caps, np.uint32)
    out_off, out_size = _layout(caps)
    out_off = out_off.astype(np.uint64)
    out = arena_of(out_size)
    olen = np.full(len(sizes), 0xFFFFFFFF, np.uint32)
    gibson_amd.host_compress_mixed(arena, in_off, ln, out, out_off, cap, olen)
    got = [bytes(out[int(o):int(o) + int(l)]) if l else None for o, l in zip(out_off, olen)]
    bad = [i for i in range(len(sizes)) if got[i] != expect[i]]
    assert not bad, (len(bad), [(i, sizes[i], caps[i]) for i in bad[:5]])
    ok = np.nonzero(olen)[0]
    assert len(ok) > 300
    # decode the successes; every fourth slot one byte short: E2BIG
    dcap = np.array([sizes[i] - (1 if k % 4 == 3 else 0) for k, i in enumerate(ok)], np.uint32)
    d_off, d_size = _layout(dcap)
    dec = arena_of(d_size)
    dl = np.full(len(ok), 0xFFFFFFFF, np.uint32)
    er = np.full(len(ok), -1, np.int32)
    gibson_amd.host_decompress_mixed(out, out_off[ok], olen[ok], dec, d_off.astype(np.uint64), dcap, dl, er)
    for k, i in enumerate(ok):
        exp = (values[i], 0) if dcap[k] == sizes[i] else (None, errno.E2BIG)
        assert (bytes(dec[int(d_off[k]):int(d_off[k]) + int(dl[k])]) if dl[k] else None, int(er[k])) == exp, i


@pytest.mark.gpu
def test_gb_calls_with_mixed_switch(torch, host_case, monkeypatch):
    # LZF_GPU_MIXED is read per call: same decisions, streams, stats and frame
    from gibson_amd import gb
    sizes, values, _, _ = host_case
    values = values[:200]
    runs = {}
    for mode in (None, "1"):
        if mode is None:
            monkeypatch.delenv("LZF_GPU_MIXED", raising=False)
        else:
            monkeypatch.setenv("LZF_GPU_MIXED", mode)
        stats = gb.Stats()
        stored = gb.set_batch(values, 100, stats)
        items = [(b"key%05d" % i, enc, data) for i, (enc, data, _) in enumerate(stored)]
        orig = [o for _, _, o in stored]
        total = sum(sizes[:200]) + 64 * 200
        frame = gb.mget_payload(items, len(items), 1 << 20, total, orig_lens=orig)
        frame_sized = gb.mget_payload(items, len(items), 1 << 20, total)      # sizes from the pre-pass
        runs[mode] = (stored, stats.compravg, stats.ncompressed, frame, frame_sized)
    assert runs[None][3] is not None and runs[None][3] == runs[None][4]
    assert any(enc == gb.ENC_LZF for enc, _, _ in runs[None][0]) and runs[None][2] > 50
    assert runs["1"] == runs[None]
