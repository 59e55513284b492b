"""Nothing is written outside a value's output range (needs a GPU).

Every value's output region out[out_off, out_off + out_cap) is followed by a
guard gap, and the first one preceded by one; the arena starts as a canary
pattern.  After compress (server caps, tight caps, failing caps) and decompress (valid, E2BIG, EINVAL
streams) every guard byte is unchanged.  A batch whose stated max length is
below a value's length (a caller contract violation) refuses that value --
out_len 0 (and EINVAL on decompress) -- and leaves its region untouched
(include/lzf_gpu.h)."""
import random

import numpy as np
import pytest

from tests.oracle_lib import synth

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def _lane_for_any_batch(monkeypatch):
    monkeypatch.setenv("LZF_GPU_LANE_MIN", "0")


def _layout(caps):
    offs, pos = [], GUARD                # a band before the first region too: an underrun of region 0
    for c in caps:
        offs.append(pos)
        pos += c + GUARD
    return np.array(offs, np.int64), pos


def _run_compress(vals, caps, max_len):
    import gibson_amd
    dev = "cuda"
    in_offs, pos = [], 0
    for v in vals:
        in_offs.append(pos)
        pos += len(v) + 7
    arena = np.zeros(pos + 16, np.uint8)
    for o, v in zip(in_offs, vals):
        arena[o:o + len(v)] = np.frombuffer(v, np.uint8)
    out_off, size = _layout(caps)
    out = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    olen = torch.full((len(vals),), 0x7777, dtype=torch.int32, device=dev)
    gibson_amd.compress_batch(torch.from_numpy(arena).to(dev), torch.tensor(in_offs, device=dev),
                              torch.tensor([len(v) for v in vals], dtype=torch.int32, device=dev), out,
                              torch.from_numpy(out_off).to(dev), torch.tensor(caps, dtype=torch.int32, device=dev),
                              olen, max_len)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_off, olen.cpu().numpy()


def _guards_intact(out, offs, caps):
    if offs[0] != GUARD or not (out[:GUARD] == CANARY).all():
        return False
    for o, c in zip(offs, caps):
        g = out[o + c:o + c + GUARD]
        if not (g == CANARY).all():
            return False
    return True


@pytest.mark.parametrize("nmax", [4096, 16384, 65536])
def test_compress_writes_nothing_past_out_cap(oracle, nmax):
    rnd = random.Random(nmax)
    vals, caps = [], []
    for i in range(400):
        n = rnd.randint(1, nmax)
        v = synth(rnd.randrange(6), 0x5EED0B00, i, n)
        full = oracle.compress(v, n + n // 16 + 64)
        F = len(full) if full else n
        caps.append(max(1, rnd.choice([n - 4, F - 1, F, F + 1, rnd.randint(1, n + 8), F // 2])))
        vals.append(v)
    out, offs, olen = _run_compress(vals, caps, nmax)
    assert _guards_intact(out, offs, caps)
    for v, c, o, ln in zip(vals, caps, offs, olen):
        exp = oracle.compress(v, c)
        assert (bytes(out[o:o + ln]) if ln else None) == exp


@pytest.mark.parametrize("nmax", [4096, 16384, 65536])
def test_free_literal_runs_at_tight_caps(oracle, nmax):
    # whole waves of random and mixed-entropy values, so the parses'
    # free-literal path (profiles/r03/INDEX.md: at least 8 lanes of a wave at a
    # literal with no candidate) runs, and caps that run out inside such runs
    rnd = random.Random(100 + nmax)
    vals, caps = [], []
    for i in range(320):
        n = rnd.choice([nmax, rnd.randint(nmax // 2, nmax)])
        kind = 4 if i % 3 else 3                       # random bytes, mixed entropy
        v = synth(kind, 0x5EED0B30, i, n)
        full = oracle.compress(v, n + n // 16 + 64)
        F = len(full) if full else n
        caps.append(max(1, rnd.choice([n - 4, F - 1, F, F + 33, rnd.randint(1, n), n // 3])))
        vals.append(v)
    out, offs, olen = _run_compress(vals, caps, nmax)
    assert _guards_intact(out, offs, caps)
    for v, c, o, ln in zip(vals, caps, offs, olen):
        assert (bytes(out[o:o + ln]) if ln else None) == oracle.compress(v, c)


def test_compress_refuses_value_past_stated_max_len(oracle):
    rnd = random.Random(3)
    vals = [synth(rnd.randrange(4), 0x5EED0B10, i, rnd.choice([900, 5000, 9000, 30000])) for i in range(200)]
    caps = [len(v) - 4 for v in vals]
    stated = 6000                       # below the 9000 / 30000 values
    out, offs, olen = _run_compress(vals, caps, stated)
    for v, c, o, ln in zip(vals, caps, offs, olen):
        if len(v) > stated:
            assert ln == 0
            assert (out[o:o + c + GUARD] == CANARY).all()
        else:
            assert (bytes(out[o:o + ln]) if ln else None) == oracle.compress(v, c)


def _run_decompress(streams, caps, max_cap):
    import gibson_amd
    dev = "cuda"
    in_offs, pos = [], 0
    for s in streams:
        in_offs.append(pos)
        pos += max(len(s), 1) + 5
    arena = np.full(pos + 16, 0xFF, np.uint8)
    for o, s in zip(in_offs, streams):
        arena[o:o + len(s)] = np.frombuffer(s, np.uint8)
    out_off, size = _layout(caps)
    out = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    olen = torch.full((len(streams),), 0x7777, dtype=torch.int32, device=dev)
    err = torch.full((len(streams),), -1, dtype=torch.int32, device=dev)
    gibson_amd.decompress_batch(torch.from_numpy(arena).to(dev), torch.tensor(in_offs, device=dev),
                                torch.tensor([len(s) for s in streams], dtype=torch.int32, device=dev), out,
                                torch.from_numpy(out_off).to(dev), torch.tensor(caps, dtype=torch.int32, device=dev),
                                olen, err, max_cap)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out_off, olen.cpu().numpy(), err.cpu().numpy()


def test_decompress_writes_nothing_past_out_cap(oracle):
    rnd = random.Random(17)
    streams, caps = [], []
    for i in range(500):
        n = rnd.randint(1, 20000)
        v = synth(rnd.randrange(6), 0x5EED0B20, i, n)
        s = oracle.compress(v, n + n // 16 + 64)
        kind = rnd.randrange(4)
        if kind == 1:
            s = s[:rnd.randrange(1, len(s))]                     # EINVAL (truncated)
        elif kind == 2:
            b = bytearray(s)
            b[rnd.randrange(len(b))] = rnd.randrange(256)       # corrupted
            s = bytes(b)
        cap = n if kind != 3 else rnd.randint(1, max(1, n - 1))  # E2BIG
        streams.append(s)
        caps.append(cap)
    out, offs, olen, err = _run_decompress(streams, caps, 20000)
    assert _guards_intact(out, offs, caps)
    for s, c, o, ln, e in zip(streams, caps, offs, olen, err):
        exp, ee = oracle.decompress(s, c)
        assert (bytes(out[o:o + ln]) if ln else None, int(e)) == (exp, ee)


def test_decompress_refuses_cap_past_stated_max(oracle):
    import errno
    vals = [synth(0, 0x5EED0B30, i, 3000 + 1000 * (i % 8)) for i in range(64)]
    streams = [oracle.compress(v, len(v) + 64) for v in vals]
    caps = [len(v) for v in vals]
    stated = 6500
    out, offs, olen, err = _run_decompress(streams, caps, stated)
    for v, c, o, ln, e in zip(vals, caps, offs, olen, err):
        if c > stated:
            assert ln == 0 and e == errno.EINVAL
            assert (out[o:o + c + GUARD] == CANARY).all()
        else:
            assert bytes(out[o:o + ln]) == v and e == 0


# ---- the decoder's routes, one by one ---------------------------------------

# the batch's stated max_out_cap -> the route lzf_launch_decompress takes and
# the crafted batch (tests/lzf_tokens.py) whose cases fit under it
DECODE_ROUTES = {256: "w256", 1024: "w1024", 4096: "w4096", 9000: "far", 16384: "far", 20000: "pipe"}


def _period1_run(rnd, max_cap):
    """a literal and 264-byte references at distance 1 behind it (one byte
    repeated: the CD_PERIOD shortcut), with caps that end inside the run"""
    from tests.lzf_tokens import lit, ref
    k = max(1, min(40, (max_cap - 4) // 264))
    s = lit(rnd.randbytes(rnd.randint(1, 4))) + ref(264, 1) * k
    top = min(max_cap, 4 + 264 * k)
    return [(s, c) for c in (top, top - 1, rnd.randint(5, top), rnd.randint(5, top), 5 + 264 * rnd.randrange(k))]


@pytest.mark.parametrize("max_cap", sorted(DECODE_ROUTES))
def test_decompress_guards_by_route(oracle, max_cap):
    from tests.lzf_tokens import route_cases
    rnd = random.Random(0xB0 + max_cap)
    streams, caps = [], []
    for i in range(160):                                         # compressor streams, as above
        n = rnd.choice([max_cap, rnd.randint(1, max_cap)])
        v = synth(rnd.randrange(6), 0x5EED0B40, i, n)
        s = oracle.compress(v, n + n // 16 + 64)
        kind = rnd.randrange(4)
        if kind == 1:
            s = s[:rnd.randrange(1, len(s))]                     # EINVAL (truncated)
        elif kind == 2:
            b = bytearray(s)
            b[rnd.randrange(len(b))] = rnd.randrange(256)       # corrupted
            s = bytes(b)
        streams.append(s)
        caps.append(n if kind != 3 else rnd.randint(1, max(1, n - 1)))   # E2BIG
    crafted = [(s, c, label) for s, c, label in route_cases(DECODE_ROUTES[max_cap]) if c <= max_cap]
    labels = {label for _, _, label in crafted}
    assert len(crafted) >= 200 and {"cap-in-lit", "cap-in-ref", "back", "cut+cap", "two-errors"} <= labels
    for s, c, _ in crafted:
        streams.append(s)
        caps.append(c)
    for _ in range(4):
        for s, c in _period1_run(rnd, max_cap):
            streams.append(s)
            caps.append(c)
    assert max(caps) == max_cap
    order = list(range(len(streams)))
    rnd.shuffle(order)
    # region 0, behind the leading guard: a back-reference to one byte before the output start
    first = 160 + next(i for i, (_, c, label) in enumerate(crafted) if label == "back" and c > max_cap // 2)
    order.remove(first)
    order.insert(0, first)
    streams, caps = [streams[i] for i in order], [caps[i] for i in order]
    expect = [oracle.decompress(s, c) for s, c in zip(streams, caps)]
    assert {e for _, e in expect} == {0, 7, 22}
    out, offs, olen, err = _run_decompress(streams, caps, max_cap)
    assert _guards_intact(out, offs, caps)
    bad = [(i, len(s), c, exp[1], int(ln), int(e)) for i, (s, c, o, ln, e, exp)
           in enumerate(zip(streams, caps, offs, olen, err, expect))
           if (bytes(out[o:o + ln]) if ln else None, int(e)) != exp]
    assert not bad, (len(bad), bad[:5])


# ---- the compressor's other routes ------------------------------------------

def _cap_choices(oracle, rnd, v):
    n = len(v)
    full = oracle.compress(v, n + n // 16 + 64)
    F = len(full) if full else n
    return max(1, rnd.choice([n - 4, F - 1, F, F + 1, rnd.randint(1, n + 8), F // 2]))


def test_compress_guards_on_window64_by_default(oracle, monkeypatch):
    # the product thresholds (LZF_GPU_LANE_MIN unset): a batch this small goes to window64
    import re
    import gibson_amd
    monkeypatch.delenv("LZF_GPU_LANE_MIN", raising=False)
    monkeypatch.delenv("LZF_GPU_KERNEL", raising=False)
    rnd = random.Random(64)
    vals = [synth(rnd.randrange(6), 0x5EED0B50, i, rnd.choice([4096, rnd.randint(1, 4096), rnd.randint(1, 200)]))
            for i in range(200)]
    caps = [_cap_choices(oracle, rnd, v) for v in vals]
    out, offs, olen = _run_compress(vals, caps, 4096)
    m = re.search(r"window64 past 64 KiB or below (\d+) values of <= 4 KiB", gibson_amd.kernel_info())
    assert m and int(m.group(1)) > len(vals), gibson_amd.kernel_info()
    assert _guards_intact(out, offs, caps)
    for v, c, o, ln in zip(vals, caps, offs, olen):
        assert (bytes(out[o:o + ln]) if ln else None) == oracle.compress(v, c)


def test_compress_guards_past_64k(oracle):
    # a value past 64 KiB takes the whole batch to window64 with 64-bit bucket heads
    import gibson_amd
    rnd = random.Random(65537)
    sizes = [65537, 70000, 65536, 1, 100, 4096] + [rnd.randint(1, 70000) for _ in range(34)]
    rnd.shuffle(sizes)
    vals = [synth(rnd.randrange(6), 0x5EED0B60, i, n) for i, n in enumerate(sizes)]
    caps = [_cap_choices(oracle, rnd, v) for v in vals]
    out, offs, olen = _run_compress(vals, caps, 70000)
    assert "window64 past 64 KiB" in gibson_amd.kernel_info()
    assert _guards_intact(out, offs, caps)
    for v, c, o, ln in zip(vals, caps, offs, olen):
        assert (bytes(out[o:o + ln]) if ln else None) == oracle.compress(v, c)
