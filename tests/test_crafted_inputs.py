"""The compressors on inputs crafted one parse rule at a time (tests/
lzf_inputs.py): a match at distance exactly 8192 and 8193, a slot collision in
front of a true match, a trigram at each position a match inserts or skips,
same-slot chains several skipped links deep, lengths around every emission
edge, caps that run out at each of the reference's three checks, and -- for
the stream cand kernel -- neighbouring values of one workgroup's stream that
share their slots, and values that straddle the stream's 65536 wrap.

On the CPU every case's claim (a predicate that follows from its construction)
is checked on the oracle's result, the oracle against a Python restatement of
src/lzf_c.c and, where built, the compiled reference.  The model runs on every
case of at most 16 KiB and on one case per family above that (it is the cost).
On the GPU the expected result is the oracle's, bit for bit, on every
generation of tests/test_gpu_parity.py."""
import collections
import contextlib
import re

import pytest

from tests import lzf_inputs, oracle_lib
from tests.lzf_inputs import family, roomy, tight

try:                                    # before liblzf_hip.so loads: one HIP runtime in the process
    import torch as _torch  # noqa: F401
except ImportError:
    _torch = None

try:                                    # the generation tables: imported, not copied
    from tests.test_gpu_parity import DIAG, GEN_ENV, GENERATIONS, _diag
except pytest.skip.Exception:           # no torch: the GPU tests below have nothing to run on
    DIAG, GEN_ENV, GENERATIONS, _diag = set(), {}, [], None

CPU_G = 256                             # workgroups of the stream layers on the CPU (the MI355X's CUs)
_EXPECT = {}


def expected(oracle, c):
    """the oracle's result of a case, computed once per distinct (value, cap)"""
    key = (c.value, c.cap)
    if key not in _EXPECT:
        _EXPECT[key] = oracle.compress(c.value, c.cap)
    return _EXPECT[key]


# ---- the batches ----------------------------------------------------------------

CLASSES = (4096, 8192, 16384, 65536, 1 << 30)       # routing classes, by the largest value present


def small_cases():
    return [c for c in lzf_inputs.base_cases() if len(c.value) <= 300]


def class_batch(nmax):
    """The crafted cases whose size selects the class, each at the roomy and at
    the tight cap, a small case between every two so that waves are mixed
    (the <= 4096 class holds the small ones anyway; past 64 KiB eight of them)."""
    lo = ([0] + list(CLASSES))[CLASSES.index(nmax)]
    big = [c for c in lzf_inputs.base_cases() if lo < len(c.value) <= nmax]
    main = [c._replace(cap=cap(len(c.value))) for c in big for cap in (roomy, tight)]
    small = small_cases() if lo else []
    if nmax > 65536:
        small = small[::len(small) // 8][:8]
    small = [c._replace(cap=(roomy, tight)[i % 2](len(c.value))) for i, c in enumerate(small)]
    res = []
    for i in range(max(len(main), len(small))):
        res += main[i:i + 1] + small[i:i + 1]
    return res


def stream_batch(kind, G):
    if kind == "neighbour":
        layers = lzf_inputs.neighbour_layers(G)
    elif kind == "wrap16k":
        layers = lzf_inputs.wrap_layers(G, 16384, 5, (8000, 8192))
    else:
        assert kind == "wrap4k"
        layers = lzf_inputs.wrap_layers(G, 4096, 17, (3900, 4060))
    return layers


STREAM_KINDS = ("neighbour", "wrap16k", "wrap4k")


# ---- CPU ------------------------------------------------------------------------

def test_slot_and_colliders():
    assert lzf_inputs.slot(0, 0, 0) == 0 and lzf_inputs.slot(1, 2, 3) == (0x0102 - 5 * 0x0203) & 0xFFFF
    cs = lzf_inputs.colliders((200, 201, 202))
    assert len(cs) == 36 and (129, 187, 148) in cs
    assert {lzf_inputs.slot(*c) for c in cs} == {lzf_inputs.slot(200, 201, 202)}
    assert all(min(c) >= 128 for c in cs) and (200, 201, 202) not in cs
    data = bytes(range(7, 60))
    assert lzf_inputs.slots_of(data).tolist() == [lzf_inputs.slot(*data[i:i + 3]) for i in range(len(data) - 2)]


def test_tokens_and_model_on_known_streams(oracle):
    T = lzf_inputs.Tok
    assert lzf_inputs.tokens(b"\x00a") == [T("lit", 0, 1, 0)]
    assert lzf_inputs.tokens(b"\x01ab\x20\x01\xe0\x00\xff") == [T("lit", 0, 2, 0), T("ref", 2, 3, 2), T("ref", 5, 9, 256)]
    assert lzf_inputs.tokens(b"\xff\xff\xff") == [T("ref", 0, 264, 8192)]
    for v, cap in ((b"", 10), (b"x", 0), (b"x", 3), (b"ab", 5), (b"a" * 5, 1), (b"a" * 300, 296), (b"ab" * 4000, 8000)):
        assert lzf_inputs.model_compress(v, cap) == oracle.compress(v, cap), (len(v), cap)
    # the 16 unrolled compares carry no bound: 19 equal bytes at the end are one reference (:181-206)
    v = b"q" + bytes(range(100, 119)) + b"zz" + bytes(range(100, 119))
    assert lzf_inputs.tokens(oracle.compress(v, 100))[-1] == T("ref", 22, 19, 21)


def test_every_claim_holds_on_the_oracle(oracle):
    ref = oracle_lib.reference()                       # None when oracle/_ref is not built
    cases = lzf_inputs.all_cases()
    for c in cases:
        r = expected(oracle, c)
        assert c.claim(r), (c.label, c.note, len(c.value), c.cap)
        if ref is not None:
            assert ref.compress(c.value, c.cap) == r, (c.label, c.note)
        if r is not None:
            assert oracle.decompress(r, len(c.value)) == (c.value, 0), (c.label, c.note)
    count = collections.Counter(c.label for c in cases)
    for label, n in lzf_inputs.MIN_COUNT.items():
        assert count[label] >= n, (label, dict(count))
    assert set(count) == set(lzf_inputs.MIN_COUNT), sorted(set(count) ^ set(lzf_inputs.MIN_COUNT))
    # the three sizes of the large cases, and what goes past 64 KiB
    for fam in ("dist", "collide", "skip", "chain", "len", "end", "window", "lit"):
        sizes = [len(c.value) for c in cases if family(c.label) == fam]
        assert min(sizes) <= 4096 and any(8192 < n <= 16384 for n in sizes) and any(16384 < n <= 65536 for n in sizes), fam
    assert sorted({c.label for c in cases if len(c.value) > 65536}) == ["alias64k", "dist:large", "run"]


def test_chain_agreements_cover_the_combine_rule():
    pairs = [(a, b) for ag in lzf_inputs.CHAINS for a, b in zip(ag, ag[1:])]
    assert any(a < b for a, b in pairs) and any(a > b for a, b in pairs) and any(a == b for a, b in pairs)
    assert {x for ag in lzf_inputs.CHAINS for x in ag} >= {3, 4, 5, 6, 7, 8, 9, 16, 17}
    assert {a for a, b in pairs if a == b} >= {8, 9, 16, 17}
    assert {len(ag) for ag in lzf_inputs.CHAINS} >= {1, 2, 3, 4, 5, 8}


def test_model_equals_oracle(oracle):
    seen = set()
    for c in lzf_inputs.all_cases():
        if len(c.value) > 16384:
            if family(c.label) in seen:
                continue
            seen.add(family(c.label))
        got, why = lzf_inputs.model_compress(c.value, c.cap, why=True)
        assert got == expected(oracle, c), (c.label, c.note, c.cap)
        if family(c.label) == "cap":                   # the refusal kind the label names
            assert c.label == "cap:" + why
    assert {"dist", "alias64k", "run", "chain", "skip"} <= seen


def test_cap_cases_cover_every_refusal(oracle):
    cs = lzf_inputs.cap_cases()
    assert 900 <= len(cs) <= 2400 and max(len(c.value) for c in cs) <= 300
    by_value = collections.defaultdict(list)
    for c in cs:
        by_value[c.value].append(c)
    assert 38 <= len(by_value) <= 40
    full, late = 0, {}
    for v, group in by_value.items():
        r = len(oracle.compress(v, roomy(len(v))))
        caps = {c.cap for c in group}
        assert set(range(1, 9)) | set(range(max(1, r - 6), r + 3)) <= caps
        full += caps == set(range(1, r + 3))
        assert all(c.label != "cap:fits" for c in group if c.cap < r)
        # :176 and :276 refuse some outputs that would have fitted: a cap of at least r that still gives 0
        late[v] = {c.label for c in group if c.cap >= r and c.label != "cap:fits"}
    assert full >= 6
    assert {k for kinds in late.values() for k in kinds} == {"cap:match", "cap:tail"}, late.values()


def test_class_batches_are_small():
    seen = set()
    for nmax in CLASSES:
        b = class_batch(nmax)
        nbytes = sum(len(c.value) for c in b)
        lo = ([0] + list(CLASSES))[CLASSES.index(nmax)]
        assert lo < max(len(c.value) for c in b) <= nmax
        if nmax > 65536:
            assert len(b) <= 24 and nbytes <= 2 << 20
        else:
            assert 200 <= len(b) <= 2000 and nbytes <= 16 << 20
        assert {c.cap for c in b if len(c.value) > 300} >= {tight(len(c.value)) for c in b if len(c.value) > 300}
        seen |= {c.label for c in b}
    assert seen == {c.label for c in lzf_inputs.base_cases()}


@pytest.mark.parametrize("kind", STREAM_KINDS)
def test_stream_layers(oracle, kind):
    layers = stream_batch(kind, CPU_G)
    assert all(len(layer) == CPU_G for layer in layers)
    flat = [c for layer in layers for c in layer]
    assert sum(len(c.value) for c in flat) <= 24 << 20
    distinct = {(c.value, c.cap): c for c in flat}
    assert len(distinct) <= 100                        # the oracle runs once per distinct (value, cap)
    for c in distinct.values():
        r = expected(oracle, c)
        assert c.claim(r), (c.label, c.note)
        if len(c.value) <= 4096 or c.label == "wrap":
            assert lzf_inputs.model_compress(c.value, c.cap) == r, (c.label, c.note)
    if kind == "neighbour":
        assert {len(c.value) for c in flat} == set(lzf_inputs.NEIGHBOUR_N)
        for j in range(CPU_G):
            a, b, c = (layer[j] for layer in layers)
            assert a.value == b.value and c.value[1:] == b.value[:-1] and c.value != b.value
            assert 64 * lzf_inputs.stream_windows(len(a.value)) <= 8192
        for c in flat:                                     # text with matches, not noise
            assert len(c.value) < 960 or c.cap < len(c.value) or len(expected(oracle, c)) < len(c.value) * 7 // 10
    else:
        n = 16384 if kind == "wrap16k" else 4096
        assert len(layers) == 1 + (5 if n == 16384 else 17)
        assert all(len(c.value) == n for layer in layers[1:] for c in layer)
        inside = lzf_inputs.boundary_inside(layers)        # the 65536 boundary inside a value, pairs round it
        assert len(inside) >= CPU_G // 2 and all(layers[k][j].label.startswith("wrap") and k > 0 for j, k in inside)
        far = {"wrap16k": 8000, "wrap4k": 3900}[kind]
        for c in {c.value: c for c in flat if c.label == "wrap"}.values():
            d = [t.dist for t in lzf_inputs.tokens(expected(oracle, c)) if t.kind == "ref" and t.length == 8]
            assert any(x >= far for x in d) and any(x <= 200 for x in d) and len(d) >= 10, (kind, sorted(d))


# ---- GPU ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    import gibson_amd
    gibson_amd.lib()
    return t


@contextlib.contextmanager
def generation(monkeypatch, gen):
    """the environment (and library) of one generation of tests/test_gpu_parity.py"""
    for k in ("LZF_GPU_KERNEL", "LZF_GPU_CAND", "LZF_GPU_TCAND"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LZF_GPU_LANE_MIN", "0")         # the batches are small: ask for the routed kernels
    for k, v in GEN_ENV[gen].items():
        monkeypatch.setenv(k, v)
    if gen in DIAG:
        with _diag():
            yield
    else:
        yield


def mismatches(cases, got, exp):
    """(label, note, n, cap, oracle's length, the GPU's) of the values that differ"""
    return [(c.label, c.note, len(c.value), c.cap, len(e) if e else 0, len(g) if g else 0)
            for c, g, e in zip(cases, got, exp) if g != e]


def report(what, cases, got, exp):
    bad = mismatches(cases, got, exp)
    labels = dict(collections.Counter(b[0] for b in bad))
    assert not bad, f"{what}: {len(bad)} of {len(cases)} differ, by label {labels}; first {bad[:5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("nmax", CLASSES, ids=[str(n) if n <= 65536 else "past64k" for n in CLASSES])
@pytest.mark.parametrize("gen", GENERATIONS)
def test_class_batch_on_every_generation(torch, oracle, monkeypatch, gen, nmax):
    from tests.gpu_batch import gpu_compress
    if gen == "serial" and nmax > 65536:
        pytest.skip("the serial kernel is limited to 64 KiB")
    cases = class_batch(nmax)
    exp = [expected(oracle, c) for c in cases]
    with generation(monkeypatch, gen):
        for align in (16, 3):
            got = gpu_compress([c.value for c in cases], [c.cap for c in cases], align=align)
            report(f"{gen}, class {nmax}, align {align}", cases, got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("gen", ["default", "lane", "table", "window"])
def test_cap_batch_writes_nothing_past_a_cap(torch, oracle, monkeypatch, gen):
    from tests.test_bounds import _guards_intact, _run_compress
    cases = list(lzf_inputs.cap_cases())
    exp = [expected(oracle, c) for c in cases]
    kinds = collections.Counter(c.label for c in cases)
    assert all(kinds["cap:" + k] >= 20 for k in lzf_inputs.CAP_KINDS), dict(kinds)
    with generation(monkeypatch, gen):
        out, offs, olen = _run_compress([c.value for c in cases], [c.cap for c in cases],
                                        max(len(c.value) for c in cases))
    got = [bytes(out[o:o + n]) if n else None for o, n in zip(offs, olen)]
    report(f"{gen}, caps", cases, got, exp)
    assert _guards_intact(out, offs, [c.cap for c in cases])


def lane_route_ran(info, count, max_len):
    """kernel_info() of a lane launch: the stream cand kernel, the batch at or
    above the class's threshold (below it the batch goes to window64), the
    LDS order check held (else window64 too), one scratch chunk (a workgroup's
    stream is cut at a chunk's end)"""
    m = re.search(r"below (\d+) values of <= 4 KiB / (\d+) of <= 8 KiB / (\d+) of <= 16 KiB", info)
    least = int(m.group(1 if max_len <= 4096 else 2 if max_len <= 8192 else 3)) if m else None
    return ("compress=lane(cand_stream+parse_lane" in info and least is not None and count >= least
            and "lds_order=held" in info and "scratch_chunks=1" in info.split())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", STREAM_KINDS)
@pytest.mark.parametrize("gen", ["default", "lane", "table-stream"])
def test_stream_batches(torch, oracle, monkeypatch, gen, kind):
    import gibson_amd
    from tests.gpu_batch import gpu_compress
    G = torch.cuda.get_device_properties(0).multi_processor_count
    layers = stream_batch(kind, G)
    cases = [c for layer in layers for c in layer]
    assert sum(len(c.value) for c in cases) <= 24 << 20 and len(cases) >= 3 * G
    exp = [expected(oracle, c) for c in cases]
    max_len = max(len(c.value) for c in cases)
    with generation(monkeypatch, gen):
        got = gpu_compress([c.value for c in cases], [c.cap for c in cases])
        info = gibson_amd.kernel_info()
    if gen == "table-stream":                          # the record form of the same kernel, one chunk
        assert "compress=table(cand_table+parse_rec" in info and "scratch_chunks=1" in info.split(), info
    else:
        assert lane_route_ran(info, len(cases), max_len), info
    report(f"{gen}, {kind}, {G} workgroups", cases, got, exp)


@pytest.mark.gpu
def test_mixed_batch(torch, oracle, monkeypatch):
    import gibson_amd
    from tests.test_mixed import run_compress_mixed
    cases = [c for nmax in CLASSES for c in class_batch(nmax)]
    exp = [expected(oracle, c) for c in cases]
    with generation(monkeypatch, "default"):
        got, _, _, _ = run_compress_mixed(torch, [c.value for c in cases], [c.cap for c in cases],
                                          max(len(c.value) for c in cases))
        plan = gibson_amd.mixed_last_plan()
    assert plan["batches"] == 5 and plan["route"] == [1, 1, 1, 2, 3, 0], plan     # lane, lane, lane, table, window64
    report("compress_mixed", cases, got, exp)


@pytest.mark.gpu
def test_set_store_batch(torch, oracle, monkeypatch):
    from tests.test_store import BASE, Batch, Store, check_stored, expect_items, set_store
    cases = [c for c in lzf_inputs.base_cases() if len(c.value) <= 700][:300]
    values = [c.value for c in cases]
    compression = sorted(len(v) for v in values)[len(values) // 2]      # about half go to LZF
    exp = expect_items(oracle, values, compression)
    why = collections.Counter(w for _, _, w in exp)
    assert len(values) >= 250 and why["small"] >= 100 and why["lzf"] + why["failed"] >= 100 and why["lzf"] >= 50, dict(why)
    total = sum(len(s) for _, s, _ in exp)
    with generation(monkeypatch, "default"):
        b = Batch(torch, values)
        st = Store(torch, BASE + total + 100)
        set_store(torch, b, st, compression)
        torch.cuda.synchronize()
    try:
        assert check_stored(b, st, exp, BASE) == total
    except AssertionError as e:
        enc, vsize, _ = b.results()
        bad = [(c.label, c.note) for c, (ee, s, _), g, z in zip(cases, exp, enc, vsize) if g != ee or z != len(s)]
        raise AssertionError(f"{e}; cases that differ in enc or size: {bad[:5]}") from e


@pytest.mark.gpu
@pytest.mark.parametrize("nmax", [4096, 16384, 65536])      # tokpar, the FAR route, the pipe
def test_round_trip_of_the_oracles_streams(torch, oracle, nmax):
    from tests.gpu_batch import gpu_decompress
    cases = [c for c in class_batch(nmax) if expected(oracle, c) is not None]
    assert len(cases) >= 100 and max(len(c.value) for c in cases) > nmax // 2
    got = gpu_decompress([expected(oracle, c) for c in cases], [len(c.value) for c in cases])
    bad = [(c.label, c.note, len(c.value), e) for c, (v, e) in zip(cases, got) if (v, e) != (c.value, 0)]
    assert not bad, f"{len(bad)} of {len(cases)} differ; first {bad[:5]}"
