"""Streams built from the LZF token grammar itself (src/lzf_d.c:64-148), not by
a compressor: a Python restatement of the reference decoder, token encoders, a
seeded stream builder and a planter of single faults at chosen tokens.  Pure
Python; the expected result of a case is always the oracle's, never this
module's (the model is a third opinion, compared on the CPU only)."""
import collections
import errno
import functools
import random

E2BIG, EINVAL = errno.E2BIG, errno.EINVAL
ROUND = 128                     # input bytes of one decoder round (CD_ROUND)
LABELS = ("ok", "ok+1", "cap-1", "cap-in-lit", "cap-in-ref", "cut-ctrl", "cut-len", "cut-lit", "cut+cap",
          "back", "back+cap", "two-errors")

Token = collections.namedtuple("Token", "data ioff Ot olen kind")     # kind: "lit" or "ref"


def model_decompress(stream, out_len, phantom=0xFF):
    """lzf_decompress (src/lzf_d.c:64-148) -> (bytes or None, errno).  The
    do-while reads one control byte even when in_len is 0: ``phantom`` is the
    byte the callers here keep behind every stream."""
    data = bytes(stream) + bytes([phantom])
    in_end = len(stream)
    out = bytearray()
    ip = 0
    while True:                                         # do
        ctrl = data[ip]
        ip += 1
        if ctrl < (1 << 5):                             # literal run
            ctrl += 1
            if len(out) + ctrl > out_len:               # :72
                return None, E2BIG
            if ip + ctrl > in_end:                      # :79
                return None, EINVAL
            out += data[ip:ip + ctrl]
            ip += ctrl
        else:                                           # back reference
            ln = ctrl >> 5
            ref = len(out) - ((ctrl & 0x1f) << 8) - 1
            if ip >= in_end:                            # :101
                return None, EINVAL
            if ln == 7:
                ln += data[ip]
                ip += 1
                if ip >= in_end:                        # :111
                    return None, EINVAL
            ref -= data[ip]
            ip += 1
            if len(out) + ln + 2 > out_len:             # :121
                return None, E2BIG
            if ref < 0:                                 # :127
                return None, EINVAL
            # :137-142 copies byte by byte, so an overlapping source repeats
            # with period d: the same bytes, whole periods at a time
            n, d = ln + 2, len(out) - ref
            if d >= n:
                out += out[ref:ref + n]
            else:
                out += (bytes(out[ref:]) * (n // d + 1))[:n]
        if not ip < in_end:                             # while (ip < in_end)
            break
    return bytes(out), 0


def lit(payload):
    assert 1 <= len(payload) <= 32
    return bytes([len(payload) - 1]) + bytes(payload)


def ref(length, back):
    assert 3 <= length <= 264 and 1 <= back <= 8192
    l, b = length - 2, back - 1
    if l < 7:
        return bytes([(l << 5) | (b >> 8), b & 255])
    return bytes([(7 << 5) | (b >> 8), l - 7, b & 255])


def _back(rnd, Ot):
    d = rnd.choice((1, 2, Ot, min(Ot, 8192), 4095, 4096, 4097, rnd.randint(1, 8192)))
    return min(d, Ot, 8192)


def build(rnd, target_out, mode):
    """-> (tokens, out_len) with out_len == target_out: a valid stream."""
    assert mode in ("mix", "lit1", "ref") and target_out >= 1
    tokens, ioff, Ot = [], 0, 0
    while Ot < target_out:
        left = target_out - Ot
        if mode == "mix":
            want_ref = rnd.random() < 0.5
            n = rnd.choice((3, 8, 9, 10, 264, rnd.randint(3, 264))) if want_ref else rnd.randint(1, 32)
        elif mode == "lit1":                            # two-byte tokens only
            want_ref = rnd.random() < 0.1
            n = rnd.randint(3, 8) if want_ref else 1
        else:
            want_ref = rnd.random() < 0.95
            n = (264 if rnd.random() < 0.95 else rnd.randint(9, 264)) if want_ref else rnd.randint(1, 4)
        n = min(n, left)
        if want_ref and Ot > 0 and n >= 3:
            if mode == "lit1":
                n = min(n, 8)
            data, kind = ref(n, _back(rnd, Ot)), "ref"
        else:
            n = min(n, 32)
            data, kind = lit(rnd.randbytes(n)), "lit"
        tokens.append(Token(data, ioff, Ot, n, kind))
        ioff += len(data)
        Ot += n
    return tokens, Ot


def rounds(tokens):
    """[(first, last)] token indices of the decoder's rounds: a round takes the
    tokens that start within ROUND input bytes of its base, the next begins
    behind its last token."""
    res, first = [], 0
    while first < len(tokens):
        base, last = tokens[first].ioff, first
        while last + 1 < len(tokens) and tokens[last + 1].ioff - base < ROUND:
            last += 1
        res.append((first, last))
        first = last + 1
    return res


def _near(tokens, k, pred, reach=48):
    for d in range(reach):
        for j in (k + d, k - d):
            if 0 <= j < len(tokens) and pred(j):
                return j
    return None


def _faults(rnd, tokens, out_len, k, stream):
    """the single-token faults token k's kind allows"""
    t = tokens[k]
    capj = max(1, t.Ot + rnd.randrange(t.olen))          # a cap that ends inside token k
    if t.kind == "lit":
        yield stream, capj, "cap-in-lit"
        yield stream[:t.ioff + 1], out_len, "cut-ctrl"
        if t.olen >= 2:
            cut = stream[:t.ioff + 1 + rnd.randint(1, t.olen - 1)]
            yield cut, out_len, "cut-lit"
            yield cut, capj, "cut+cap"                   # E2BIG: :72 precedes :79
        else:
            yield stream[:t.ioff + 1], capj, "cut+cap"
    else:
        yield stream, capj, "cap-in-ref"
        yield stream[:t.ioff + 1], out_len, "cut-ctrl"
        if len(t.data) == 3:
            yield stream[:t.ioff + 2], out_len, "cut-len"
        yield stream[:t.ioff + rnd.randint(1, len(t.data) - 1)], capj, "cut+cap"   # EINVAL: :101/:111 precede :121
        if t.Ot < 8192:
            bad = stream[:t.ioff] + ref(t.olen, t.Ot + 1) + stream[t.ioff + len(t.data):]
            yield bad, out_len, "back"
            yield bad, t.Ot + 1, "back+cap"              # E2BIG: :121 precedes :127


def _two_errors(rnd, tokens, rnds, k, stream):
    """tokens k and k + 1 of one round both fail, with different errno"""
    last_of = {}
    for a, b in rnds:
        for j in range(a, b + 1):
            last_of[j] = b
    nxt = lambda j: j + 1 <= last_of[j]
    # EINVAL (distance past the output start) then E2BIG (the cap ends in k + 1)
    j = _near(tokens, k, lambda j: nxt(j) and tokens[j].kind == "ref" and tokens[j].Ot < 8192)
    if j is not None:
        t, u = tokens[j], tokens[j + 1]
        bad = stream[:t.ioff] + ref(t.olen, t.Ot + 1) + stream[t.ioff + len(t.data):]
        yield bad, u.Ot + rnd.randrange(u.olen), "two-errors"
    # E2BIG (the cap ends in k) then EINVAL
    j = _near(tokens, k, lambda j: nxt(j) and tokens[j + 1].kind == "ref" and tokens[j + 1].Ot < 8192)
    if j is not None:
        t, u = tokens[j], tokens[j + 1]
        bad = stream[:u.ioff] + ref(u.olen, u.Ot + 1) + stream[u.ioff + len(u.data):]
        yield bad, max(1, t.Ot + rnd.randrange(t.olen)), "two-errors"


POSITIONS = ("first", "middle", "tail", "round-first", "round-last")


def cases(rnd, tokens, out_len, positions=POSITIONS):
    """(stream, cap, label): the valid stream at three caps, then the stream
    that ends before a token (valid too) and one fault per case at a token of
    the first round, of a middle round far from both ends (streams of 600
    bytes and more), of the last 160 input bytes, and at the first and the
    last token of a round (``positions``: which of these)."""
    stream = b"".join(t.data for t in tokens)
    in_len = len(stream)
    yield stream, out_len, "ok"
    yield stream, out_len + 1, "ok+1"
    if out_len > 1:
        yield stream, out_len - 1, "cap-1"
    rnds = rounds(tokens)
    picks = []                                           # (token, exactly this one)
    for p in positions:
        if p == "first":
            picks.append((rnd.randint(*rnds[0]), False))
        elif p == "middle":
            mid = [i for i, t in enumerate(tokens) if 160 <= t.ioff <= in_len - 340]
            if mid:
                picks.append((rnd.choice(mid), False))
        elif p == "tail":
            picks.append((rnd.choice([i for i, t in enumerate(tokens) if t.ioff >= in_len - 160]), False))
        elif p == "round-first":
            picks.append((rnd.choice(rnds)[0], True))
        else:
            assert p == "round-last"
            picks.append((rnd.choice(rnds)[1], True))
    for k, exact in picks:
        if exact:
            ks = [k]
        else:                                            # a literal and a reference near k
            ks = {_near(tokens, k, lambda j: tokens[j].kind == "lit"), _near(tokens, k, lambda j: tokens[j].kind == "ref")}
            ks = sorted(j for j in ks if j is not None)
        if k:                                            # the stream up to token k is a valid stream
            yield stream[:tokens[k].ioff], tokens[k].Ot, "ok"
            yield stream[:tokens[k].ioff], tokens[k].Ot + 1, "ok+1"
        for j in ks:
            yield from _faults(rnd, tokens, out_len, j, stream)
        yield from _two_errors(rnd, tokens, rnds, k, stream)


# ---- the batches of the decoder-route tests ---------------------------------

# route -> (targets, small targets mixed in, lowest and highest cap that
# selects the route as a batch's largest cap): lzf_launch_decompress picks the
# tokpar64 window by the largest cap up to 4 KiB, FAR up to 16 KiB, the pipe
# past that
ROUTES = {
    "w256": ((250, 255, 256), (40,), 129, 256),
    "w512": ((500, 511, 512), (40, 250), 257, 512),
    "w1024": ((1000, 1023, 1024), (40, 250), 513, 1024),
    "w2048": ((2000, 2047, 2048), (40, 1000), 1025, 2048),
    "w4096": ((2049, 4095, 4096), (40, 1000), 2049, 4096),
    "far": ((4097, 9000, 16384), (40, 250, 4096), 4097, 16384),
    "pipe16385": ((16384, 16385), (40, 4096), 16385, 16385),
    "pipe": ((16386, 20000), (40, 4096, 9000), 16386, 20000),
}
MODES = ("mix", "lit1", "ref")


@functools.lru_cache(maxsize=None)
def route_cases(route, want=450, limit=600):
    """The crafted batch of one decoder route: [(stream, cap, label)], between
    ``want`` and ``limit`` cases: every (target, mode) pair in turn, every
    fourth stream a small one, two fault positions per stream, every cap
    inside the route's range."""
    targets, small, _, top = ROUTES[route]
    rnd = random.Random("route-" + route)
    main = [(t, m) for m in MODES for t in targets]
    res, i, nm, ns = [], 0, 0, 0
    while len(res) < want:
        if i % 4 == 3:
            target, mode = small[ns % len(small)], MODES[(ns // len(small)) % 3]
            ns += 1
        else:
            target, mode = main[nm % len(main)]
            nm += 1
        tokens, out_len = build(rnd, target, mode)
        pos = (POSITIONS[(2 * i) % 5], POSITIONS[(2 * i + 1) % 5])
        res += [c for c in cases(rnd, tokens, out_len, pos) if c[1] <= top]
        i += 1
    return tuple(res[:limit])


def check_classes(expected, labels, min_class=30, min_label=5):
    """every outcome class and every fault label is present: from the oracle's
    results ``expected`` [(bytes or None, errno)] alone"""
    by_errno = collections.Counter(e for _, e in expected)
    for e in (0, E2BIG, EINVAL):
        assert by_errno[e] >= min_class, (e, dict(by_errno))
    assert set(by_errno) == {0, E2BIG, EINVAL}, dict(by_errno)
    by_label = collections.Counter(labels)
    for name in LABELS:
        assert by_label[name] >= min_label, (name, dict(by_label))
