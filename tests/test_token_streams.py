"""The decoders on streams crafted from the LZF token grammar
(tests/lzf_tokens.py): one fault planted at a chosen token -- a cap that ends
inside it, a cut stream, a distance past the output start, two different
errors in one round -- on every decoder route, in the decoded-size pre-pass
and the decode-in-place of lzf_gpu_kv_frame and lzf_gpu_store_mget.  The expected result is the oracle's, bit for bit.  On the
CPU the builder and the oracle are first checked against a Python restatement
of src/lzf_d.c and, where built, the compiled reference."""
import functools
import random
import struct

import numpy as np
import pytest

from tests import lzf_tokens, oracle_lib
from tests.lzf_tokens import E2BIG, EINVAL, ROUTES, route_cases

try:                                    # before liblzf_hip.so loads: one HIP runtime in the process
    import torch as _torch  # noqa: F401
except ImportError:
    _torch = None

ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL = 0, 1, 2, 0xFF
SIZES = (40, 250, 1000, 4096, 9000, 16384, 20000)
_EXPECT = {}


def expected(oracle, route):
    """the oracle's (bytes or None, errno) per case of a route's batch, computed once"""
    if route not in _EXPECT:
        _EXPECT[route] = [oracle.decompress(s, c) for s, c, _ in route_cases(route)]
    return _EXPECT[route]


# ---- CPU ---------------------------------------------------------------------

def test_token_encoders():
    assert lzf_tokens.lit(b"a") == b"\x00a" and lzf_tokens.lit(b"x" * 32)[0] == 31
    assert lzf_tokens.ref(3, 1) == b"\x20\x00"
    assert lzf_tokens.ref(8, 8192) == b"\xdf\xff"                  # the longest 2-byte form
    assert lzf_tokens.ref(9, 1) == b"\xe0\x00\x00"                 # the shortest 3-byte form
    assert lzf_tokens.ref(264, 4097) == b"\xf0\xff\x00"
    rnd = random.Random(1)
    for mode in ("mix", "lit1", "ref"):
        tokens, out_len = lzf_tokens.build(rnd, 20000, mode)
        assert out_len == 20000 and tokens[0].kind == "lit"
        pos = opos = 0
        for t in tokens:
            assert (t.ioff, t.Ot) == (pos, opos)
            pos, opos = pos + len(t.data), opos + t.olen
        per_round = [b - a + 1 for a, b in lzf_tokens.rounds(tokens)[:-1]]
        if mode == "lit1":
            assert set(per_round) == {64}                          # 64 two-byte tokens per round
        if mode == "ref":                                          # past 8 KiB of output in one round
            assert max(tokens[b].Ot + tokens[b].olen - tokens[a].Ot for a, b in lzf_tokens.rounds(tokens)) > 8192


@functools.lru_cache(maxsize=None)
def _cpu_cases():
    """about 2000 cases over SIZES and the three modes: (size, mode, stream, cap, label)"""
    rnd = random.Random(0x70CE)
    res, i = [], 0
    while len(res) < 2000:
        size, mode = SIZES[i % len(SIZES)], ("mix", "lit1", "ref")[(i // len(SIZES)) % 3]
        i += 1
        tokens, out_len = lzf_tokens.build(rnd, size, mode)
        res += [(size, mode) + c for c in lzf_tokens.cases(rnd, tokens, out_len)]
    return tuple(res)


def test_model_equals_oracle(oracle):
    seen = {}
    for size, mode, s, cap, label in _cpu_cases():
        exp = oracle.decompress(s, cap)
        assert lzf_tokens.model_decompress(s, cap) == exp, (size, mode, label, cap, len(s))
        seen[(size, exp[1])] = seen.get((size, exp[1]), 0) + 1
    for size in SIZES:
        for e in (0, E2BIG, EINVAL):
            assert seen.get((size, e), 0) >= 20, (size, e, seen)
    # the phantom control byte of a 0-length stream (the harness keeps 0xFF there)
    for cap in (1, 64):
        assert lzf_tokens.model_decompress(b"", cap) == oracle.decompress(b"", cap) == (None, EINVAL)


def test_model_equals_compiled_reference():
    ref = oracle_lib.reference()
    if ref is None:
        pytest.skip("oracle/_ref is not built")
    for size, mode, s, cap, label in _cpu_cases():
        assert lzf_tokens.model_decompress(s, cap) == ref.decompress(s, cap), (size, mode, label, cap, len(s))


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_batches_hold_every_class(oracle, route):
    # the batches of the GPU tests below, judged from the oracle's results alone
    cs = route_cases(route)
    assert 300 <= len(cs) <= 600
    lzf_tokens.check_classes(expected(oracle, route), [label for _, _, label in cs])
    _, _, lo, hi = ROUTES[route]
    assert lo <= max(c for _, c, _ in cs) <= hi and min(c for _, c, _ in cs) >= 1
    assert len({len(s) for s, _, _ in cs}) > 20


# ---- GPU ---------------------------------------------------------------------

FILL = 0xA5
ROOM = 4096


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    import gibson_amd
    gibson_amd.lib()
    return t


def _mismatches(cs, got, exp):
    return [(label, len(s), cap, e, (len(g[0]) if g[0] else 0, g[1]))
            for (s, cap, label), g, e in zip(cs, got, ((len(x[0]) if x[0] else 0, x[1]) for x in exp))
            if (len(g[0]) if g[0] else 0, g[1]) != e]


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_route_matches_oracle(torch, oracle, route):
    from tests.gpu_batch import gpu_decompress
    cs, exp = route_cases(route), expected(oracle, route)
    lzf_tokens.check_classes(exp, [label for _, _, label in cs])
    _, _, lo, hi = ROUTES[route]
    streams, caps = [s for s, _, _ in cs], [c for _, c, _ in cs]
    assert lo <= max(caps) <= hi                       # lzf_launch_decompress routes by the largest cap
    for align in (16, 3):
        got = gpu_decompress(streams, caps, align=align)
        bad = _mismatches(cs, got, exp)
        assert not bad, f"{route} align {align}: {len(bad)} of {len(cs)} differ (label, in_len, cap, oracle, gpu): {bad[:5]}"
        assert got == exp, f"{route} align {align}: bytes differ"


@pytest.mark.gpu
@pytest.mark.parametrize("route", list(ROUTES))
def test_decoded_size_on_crafted_streams(torch, oracle, route):
    import gibson_amd
    from tests.gpu_batch import _pack
    cs, exp = route_cases(route), expected(oracle, route)
    arena, offs = _pack([s for s, _, _ in cs])
    d_in = torch.from_numpy(arena).cuda()
    lens = np.array([len(s) for s, _, _ in cs], np.int32)
    caps = np.array([c for _, c, _ in cs])
    bad = []
    for limit in sorted(set(caps.tolist())):           # one call per out_limit
        sel = np.nonzero(caps == limit)[0]
        size = torch.full((len(sel),), -1, dtype=torch.int32, device="cuda")
        err = torch.full((len(sel),), -1, dtype=torch.int32, device="cuda")
        gibson_amd.decoded_size_batch(d_in, torch.from_numpy(offs[sel]).cuda(), torch.from_numpy(lens[sel]).cuda(),
                                      size, err, limit)
        torch.cuda.synchronize()
        for i, z, e in zip(sel, size.cpu().tolist(), err.cpu().tolist()):
            want = (len(exp[i][0]) if exp[i][0] else 0, exp[i][1])
            if (z, e) != want:
                bad.append((cs[i][2], len(cs[i][0]), limit, want, (z, e)))
    assert not bad, f"{route}: {len(bad)} differ (label, in_len, limit, oracle, gpu): {bad[:5]}"


# ---- decode in place: lzf_gpu_kv_frame and lzf_gpu_store_mget ----------------

def _frame_items():
    """about 60 items, keys of 1-40 bytes: crafted valid streams of all three
    modes and of every decoder class, between PLAIN, NUMBER and NULL items"""
    rnd = random.Random(0xF4A3)
    sizes = [1, 3, 40, 250, 1000, 4095, 4096, 4097, 9000, 16384, 16385, 20000]
    rnd.shuffle(sizes)
    lzf = [(sizes[i % len(sizes)], ("mix", "lit1", "ref")[i % 3]) for i in range(40)]
    items, lens = [], []
    for i in range(62):
        k = bytes(rnd.choice(b"abcdefghij:_0123456789") for _ in range(rnd.randint(1, 40)))
        r = i % 5
        if r == 1 and i % 10 == 1:
            items.append((k, ENC_NULL, b"")); lens.append(0)
        elif r == 1:
            items.append((k, ENC_NUMBER, struct.pack("<q", rnd.randint(-2**40, 2**40)))); lens.append(8)
        elif r == 3:
            v = rnd.randbytes(rnd.randint(1, 300))
            items.append((k, ENC_PLAIN, v)); lens.append(len(v))
        else:
            n, mode = lzf.pop()
            tokens, out_len = lzf_tokens.build(rnd, n, mode)
            items.append((k, ENC_LZF, b"".join(t.data for t in tokens))); lens.append(out_len)
    return items, lens


def _failing_items(oracle):
    """(stream, val_len, errno): a stream that does not decode to its val_len,
    one per outcome class -- decodes, but one byte short; E2BIG; EINVAL"""
    rnd = random.Random(0xBAD)
    tokens, out_len = lzf_tokens.build(rnd, 5000, "mix")
    res = {}
    for s, cap, label in lzf_tokens.cases(rnd, tokens, out_len):
        e = oracle.decompress(s, cap)[1]
        if label in ("ok+1", "cap-in-ref", "back") and e not in res:
            res[e] = (s, cap, e)
    assert sorted(res) == [0, E2BIG, EINVAL]
    return [res[e] for e in (0, E2BIG, EINVAL)]


def _kv_frame(torch, items, lens, elements, max_response, header):
    """lzf_gpu_kv_frame into a frame with ROOM canary bytes behind it -> (frame_len, frame bytes, canaries)"""
    import gibson_amd
    keys = b"".join(k for k, _, _ in items)
    vals = b"".join(v for _, _, v in items) + b"\0"
    T = lambda a, dt: torch.from_numpy(np.array(a, dt)).cuda()
    ko = np.cumsum([0] + [len(k) for k, _, _ in items[:-1]])
    vo = np.cumsum([0] + [len(v) for _, _, v in items[:-1]])
    hdr = 7 if header else 0
    frame = torch.full((hdr + max_response + ROOM,), FILL, dtype=torch.uint8, device="cuda")
    flen = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    w = gibson_amd.kv_frame(T(np.frombuffer(keys, np.uint8), np.uint8), T(ko, np.int64),
                            T([len(k) for k, _, _ in items], np.int32),
                            T(np.frombuffer(vals, np.uint8), np.uint8), T(vo, np.int64),
                            T([len(v) for _, _, v in items], np.int32), T([e for _, e, _ in items], np.uint8),
                            T(lens, np.int32), elements, max(lens), frame, max_response, flen, reply_header=header)
    torch.cuda.synchronize()
    del w
    got = frame.cpu().numpy()
    return int(flen.item()), got[:hdr + max_response], got[hdr + max_response:]


@pytest.mark.gpu
@pytest.mark.parametrize("header", [True, False])
def test_kv_frame_decodes_crafted_streams_in_place(torch, oracle, header):
    items, lens = _frame_items()
    assert sum(e == ENC_LZF for _, e, _ in items) >= 30 and {e for _, e, _ in items} == {0, 1, 2, 0xFF}
    for (_, e, s), n in zip(items, lens):               # valid: every stream decodes to its val_len
        assert e != ENC_LZF or len(oracle.decompress(s, n)[0]) == n
    elements = sum(1 for _, e, _ in items if e != ENC_NULL)
    exp = oracle.kv_frame(items, elements, 64 << 20, 1 << 20, reply_header=header)
    hdr = 7 if header else 0
    for room in (0, 100):                               # the payload fits exactly; with room to spare
        n, frame, canary = _kv_frame(torch, items, lens, elements, len(exp) - hdr + room, header)
        assert n == len(exp) and bytes(frame[:n]) == exp
        assert (frame[n:] == FILL).all() and (canary == FILL).all()
    at = [i for i, (_, e, _) in enumerate(items) if e == ENC_LZF]
    for j, (s, cap, e) in enumerate(_failing_items(oracle)):
        i = at[(7 * j + 3) % len(at)]
        bad_items, bad_lens = list(items), list(lens)
        bad_items[i], bad_lens[i] = (items[i][0], ENC_LZF, s), cap
        n, frame, canary = _kv_frame(torch, bad_items, bad_lens, elements, len(exp) + 20000, header)
        assert n == 0, (e, n)
        assert (canary == FILL).all(), e


@pytest.mark.gpu
@pytest.mark.parametrize("header", [True, False])
def test_store_mget_decodes_crafted_streams_in_place(torch, oracle, header):
    from tests.test_store_mget import EDECODE, GUARD, OK, Dev, Host, Mget, expect_frame
    items, lens = _frame_items()

    def host(items, lens):
        size = [len(v) for _, _, v in items]
        off = np.concatenate([[0], np.cumsum(size[:-1])])
        return Host(np.frombuffer(b"".join(v for _, _, v in items), np.uint8), off, size, [e for _, e, _ in items],
                    lens, [k for k, _, _ in items])

    h = host(items, lens)
    idx = np.arange(h.n, dtype=np.uint32)               # the identity list
    valid = [i for i in range(h.n) if h.enc[i] != ENC_NULL]
    exp = expect_frame(oracle, h, valid, 64 << 20, header)
    assert exp == oracle.kv_frame(items, len(valid), 64 << 20, 1 << 20, reply_header=header)
    hdr = 7 if header else 0
    for room in (0, 100):
        d = Dev(torch, h)
        # Mget.check: the frame, then FILL to the end of the ROOM canary bytes
        Mget(torch, d, idx, len(exp) - hdr + room, header).check(torch, exp, [len(valid), 0, h.n - len(valid), OK])
        assert (d.arena.cpu().numpy()[len(h.arena):] == GUARD).all()
    at = [i for i in range(h.n) if h.enc[i] == ENC_LZF]
    for j, (s, cap, e) in enumerate(_failing_items(oracle)):
        i = at[(7 * j + 3) % len(at)]
        bad_items, bad_lens = list(items), list(lens)
        bad_items[i], bad_lens[i] = (items[i][0], ENC_LZF, s), cap
        d = Dev(torch, host(bad_items, bad_lens))
        max_response = len(exp) + 20000
        r = Mget(torch, d, idx, max_response, header)
        torch.cuda.synchronize()
        assert r.result.cpu().numpy().tolist() == [len(valid), 0, h.n - len(valid), EDECODE], e
        assert int(r.flen.item()) == 0, e
        assert (r.frame.cpu().numpy()[hdr + max_response:] == FILL).all(), e
        assert (r.work[r.wsize:].cpu().numpy() == GUARD).all(), e
