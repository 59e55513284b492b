"""Inputs built for the compressors, one parse rule of src/lzf_c.c at a time
(HLOG 16, VERY_FAST 1, the table treated as cleared): a Python restatement of
lzf_compress, a token splitter, a builder of values whose fillers provably
keep off chosen table slots, and the case families of tests/
test_crafted_inputs.py.  The expected result of a case is always the oracle's,
never this module's: the model is a third opinion (compared on the CPU only)
and the source of the claims -- predicates over the oracle's result that
follow from a case's construction.

The rules, by the reference's lines:
  R1 slot        :47-57, 147-149  one entry per slot, the latest position wins
  R2 inserted    :232-247         a match inserts its start and its last two
  R3 acceptance  :155-165         distance <= 8192, ip + 4 < in_end, ref > in_data
  R4 length      :169-209         maxlen = min(in_end - ip - 2, 264), 16 unrolled
  R5 emission    :173-174, 268-272, 290-291
  R6 space       :176, 263, 276
"""
import collections
import functools
import random

import numpy as np

MAX_LIT, MAX_OFF, MAX_REF = 1 << 5, 1 << 13, (1 << 8) + (1 << 3)

Tok = collections.namedtuple("Tok", "kind pos length dist")          # kind: "lit" or "ref"; pos: in the value
Case = collections.namedtuple("Case", "value cap label claim note")  # claim(oracle's result: bytes or None) -> bool


def family(label):
    return label.split(":")[0]


def roomy(n):
    return n + n // 16 + 64


def tight(n):
    return max(1, n - 4)


# ---- R1 -----------------------------------------------------------------------

def slot(b0, b1, b2):
    """IDX(hval) of src/lzf_c.c:53 (VERY_FAST, HLOG 16) for the three bytes at ip"""
    return (((b0 << 8) | b1) - 5 * ((b1 << 8) | b2)) & 0xFFFF


def slots_of(data):
    """the slot of every trigram of data, as an array (len(data) - 2 entries)"""
    a = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    if len(a) < 3:
        return np.zeros(0, np.int64)
    return (((a[:-2] << 8) | a[1:-1]) - 5 * ((a[1:-1] << 8) | a[2:])) & 0xFFFF


def colliders(tri, lo=128, hi=256):
    """the other trigrams of bytes lo..hi-1 with tri's slot"""
    s, res = slot(*tri), []
    for b1 in range(lo, hi):
        for b2 in range(lo, hi):
            t = (s + 5 * ((b1 << 8) | b2)) & 0xFFFF                  # (b0 << 8 | b1) must be this
            if t & 0xFF == b1 and lo <= t >> 8 < hi and (t >> 8, b1, b2) != tuple(tri):
                res.append((t >> 8, b1, b2))
    return sorted(res)


# ---- the model ------------------------------------------------------------------

def model_compress(data, out_len, why=False):
    """lzf_compress (src/lzf_c.c:98-294) -> the stream or None; with ``why``
    -> (stream or None, "fits" | "match" | "literal" | "tail" | "empty"): the
    check that refused (:176, :263, :276)."""
    done = (lambda r, k: (r, k)) if why else (lambda r, k: r)
    n = len(data)
    if not n or not out_len:                                # :131
        return done(None, "empty")
    htab = {}                                               # cleared: no entry
    out = bytearray(out_len + 8)
    op, lit, ip = 1, 0, 0                                   # :142 start run
    while ip < n - 2:                                       # :145
        s = slot(data[ip], data[ip + 1], data[ip + 2])      # :147-148
        ref = htab.get(s, -1)
        htab[s] = ip                                        # :149
        if (ref >= 0 and ip - ref - 1 < MAX_OFF             # :155
                and ip + 4 < n                              # :156
                and ref > 0                                 # :157
                and data[ref] == data[ip] and data[ref + 1] == data[ip + 1] and data[ref + 2] == data[ip + 2]):
            off = ip - ref - 1
            ln = 2
            maxlen = min(n - ip - ln, MAX_REF)              # :170-171
            out[op - lit - 1] = (lit - 1) & 0xFF            # :173 stop run
            if not lit:                                     # :174 undo run if length is zero
                op -= 1
            if op + 3 + 1 >= out_len:                       # :176
                return done(None, "match")
            while True:                                     # :179
                if maxlen > 16:                             # :181-202, no bound on len inside
                    diff = False
                    for _ in range(16):
                        ln += 1
                        if data[ref + ln] != data[ip + ln]:
                            diff = True
                            break
                    if diff:
                        break
                while True:                                 # :204-206 do len++ while (...)
                    ln += 1
                    if not (ln < maxlen and data[ref + ln] == data[ip + ln]):
                        break
                break
            ln -= 2                                         # :211
            ip += 1
            if ln < 7:                                      # :214-224
                out[op] = (off >> 8) + (ln << 5)
                op += 1
            else:
                out[op] = (off >> 8) + (7 << 5)
                out[op + 1] = ln - 7
                op += 2
            out[op] = off & 0xFF
            op += 1
            lit = 0                                         # :225 start run
            op += 1
            ip += ln + 1                                    # :227
            if ip >= n - 2:                                 # :229
                break
            ip -= 2                                         # :233-247: the last two positions
            for _ in range(2):
                htab[slot(data[ip], data[ip + 1], data[ip + 2])] = ip
                ip += 1
        else:
            if op >= out_len:                               # :263
                return done(None, "literal")
            lit += 1                                        # :266
            out[op] = data[ip]
            op += 1
            ip += 1
            if lit == MAX_LIT:                              # :268-272
                out[op - lit - 1] = lit - 1
                lit = 0
                op += 1
    if op + 3 > out_len:                                    # :276
        return done(None, "tail")
    while ip < n:                                           # :279-288
        lit += 1
        out[op] = data[ip]
        op += 1
        ip += 1
        if lit == MAX_LIT:
            out[op - lit - 1] = lit - 1
            lit = 0
            op += 1
    out[op - lit - 1] = (lit - 1) & 0xFF                    # :290
    if not lit:                                             # :291
        op -= 1
    return done(bytes(out[:op]), "fits")


def tokens(stream):
    """a valid stream as [Tok(kind, position in the value, length, distance)]"""
    res, ip, pos = [], 0, 0
    while ip < len(stream):
        c = stream[ip]
        ip += 1
        if c < MAX_LIT:
            res.append(Tok("lit", pos, c + 1, 0))
            ip += c + 1
            pos += c + 1
        else:
            ln = c >> 5
            if ln == 7:
                ln += stream[ip]
                ip += 1
            res.append(Tok("ref", pos, ln + 2, (((c & 0x1F) << 8) | stream[ip]) + 1))
            ip += 1
            pos += ln + 2
    assert ip == len(stream)
    return res


# ---- claims ---------------------------------------------------------------------

def has_ref(pos, length, dist):
    want = Tok("ref", pos, length, dist)
    return lambda r: r is not None and want in tokens(r)


def literal_span(pos, n):
    """every position of [pos, pos + n) is a literal"""
    def claim(r):
        if r is None:
            return False
        left = set(range(pos, pos + n))
        for t in tokens(r):
            if t.kind == "lit":
                left -= set(range(max(pos, t.pos), min(pos + n, t.pos + t.length)))
        return not left
    return claim


def all_of(*claims):
    return lambda r: all(c(r) for c in claims)


def same_tokens(stream):
    """the token list of ``stream`` (the model's); None: the result is 0"""
    if stream is None:
        return lambda r: r is None
    want = tokens(stream)
    return lambda r: r is not None and tokens(r) == want


def anything(r):
    return True


# ---- the builder ----------------------------------------------------------------

class Build:
    """A value made of pieces (markers, from one half of the byte range) and
    fillers (random bytes of the other half).  A filler keeps every trigram it
    forms -- its own and those with its neighbours -- off the slots reserved so
    far; and the three positions in front of the piece that follows get slots
    no earlier position of the value has, so they are literals and the piece's
    first position is visited (R2).  Fillers of at most SMALL bytes go further:
    none of their slots occurs earlier in the value, so a value made of such
    fillers has no match but the constructed ones."""
    SMALL = 2048

    def __init__(self, seed, half=0):
        self.rnd = random.Random(seed)
        self.lo, self.hi = 128 * half, 128 * (1 - half)
        self.b = bytearray()
        self.avoid = np.zeros(65536, bool)
        self.used = np.zeros(65536, bool)

    def __len__(self):
        return len(self.b)

    def reserve(self, data):
        self.avoid[slots_of(data)] = True

    def marker(self, n, period=None):
        """n bytes of the markers' half whose trigrams have slots of their own:
        different from one another, from every reserved one and from every one
        used so far; with ``period`` the bytes repeat with exactly that period"""
        for _ in range(20000):
            if period:
                m = (bytes(self.hi + self.rnd.randrange(128) for _ in range(period)) * (n // period + 1))[:n]
            else:
                m = bytes(self.hi + self.rnd.randrange(128) for _ in range(n))
            tris = {m[i:i + 3] for i in range(len(m) - 2)}
            if period and len(tris) != min(period, len(m) - 2):
                continue
            ss = [slot(*t) for t in tris]
            if len(set(ss)) == len(ss) and not (self.avoid[ss].any() or self.used[ss].any()):
                self.reserve(m)
                return m
        raise AssertionError("no marker")

    def other(self, byte):
        """a byte of the markers' half that is not ``byte``"""
        while True:
            c = self.hi + self.rnd.randrange(128)
            if c != byte:
                return c

    def put(self, data):
        pos = len(self.b)
        self.b += data
        self.used[slots_of(self.b[max(0, pos - 2):])] = True
        return pos

    def _draw(self, not_this=None):
        while True:
            c = self.lo + self.rnd.randrange(128)
            if c != not_this:
                return c

    def fill(self, n, nxt=b"", not_first=None):
        """n filler bytes in front of the piece ``nxt`` (not appended here)"""
        assert n >= 0
        pos = len(self.b)
        if n == 0:
            return pos
        ctx = bytes(self.b[-2:])
        nxt = bytes(nxt[:2])
        if n <= self.SMALL:
            forb = self.avoid | self.used
            f = bytearray()
            for i in range(n):
                for _ in range(4000):
                    c = self._draw(not_first if i == 0 else None)
                    seq = (ctx + bytes(f))[-2:] + bytes([c])
                    tris = [seq] if len(seq) == 3 else []
                    if i == n - 1:                            # the trigrams with the next piece
                        tail = seq[-2:] + nxt
                        tris += [tail[k:k + 3] for k in range(len(tail) - 2)]
                    ss = [slot(*t) for t in tris]
                    if len(set(ss)) == len(ss) and not forb[ss].any():
                        break
                else:
                    raise AssertionError("no filler byte")
                f.append(c)
                if len(seq) == 3:
                    forb[ss[0]] = True
            self.put(bytes(f))
            return pos
        raw = (np.frombuffer(self.rnd.randbytes(n), np.uint8) & 0x7F) | self.lo
        raw = raw.copy()
        if not_first is not None and raw[0] == not_first:
            raw[0] = self._draw(not_first)
        nc = len(ctx)
        for _ in range(10000):
            s = slots_of(ctx + raw.tobytes() + nxt)          # trigram k starts at byte k - nc of raw
            bad = set(np.nonzero(self.avoid[s])[0].tolist())
            if len(nxt) == 2:                                # the three positions in front of the piece
                seen = self.used.copy()
                seen[s[:-3]] = True
                last = s[-3:].tolist()
                if seen[last].any() or len(set(last)) != 3:
                    bad.add(len(s) - 3)
            if not bad:
                break
            for k in bad:
                for j in (k - nc, k - nc + 1, k - nc + 2):
                    if 0 <= j < n:
                        raw[j] = self._draw(not_first if j == 0 else None)
        else:
            raise AssertionError("no filler")
        self.put(raw.tobytes())
        return pos

    def case(self, label, claim, note, cap=None):
        v = bytes(self.b)
        return Case(v, roomy(len(v)) if cap is None else cap, label, claim, note)


def _tail(rnd):
    return rnd.randint(24, 40)        # past the copy: maxlen > 16, so the unrolled compares run (R4)


# ---- families -------------------------------------------------------------------

SIZE_LEADS = (9000, 30000)            # leads that lift a small construction into the 16 KiB and 64 KiB classes


def dist_case(d, lead=1, total=None):
    """an 8-byte marker at ``lead`` and again d further on (R3: off < MAX_OFF);
    with ``total`` the second one lies near the end of a value that long.  For
    d < 8 the two overlap: 8 + d bytes of period d."""
    b = Build(f"dist-{d}-{lead}-{total}")
    tail = _tail(b.rnd) if total is None else b.rnd.randint(6, 20)
    if total is not None:
        lead = total - tail - 8 - d
    if d < 8:
        m = b.marker(8 + d, period=d)
        b.fill(lead, m)
        p = b.put(m)
        b.fill(tail)
        return b.case("dist", has_ref(p + d, 8, d), f"d={d} at {p + d}")
    m = b.marker(8)
    b.fill(lead, m)
    p1 = b.put(m)
    b.fill(d - 8, m)
    p2 = b.put(m)
    b.fill(tail, not_first=b.b[p1 + 8])
    label = "dist" if total is None else "dist:large"
    claim = has_ref(p2, 8, d) if d <= MAX_OFF else literal_span(p2, 8)
    return b.case(label, claim, f"d={d} at {p2} of {len(b)}")


def alias_case(k):
    """the marker at p and at p + 65536 + k: only a position kept in 16 bits
    sees a distance of k"""
    b = Build(f"alias-{k}")
    m = b.marker(8)
    b.fill(b.rnd.randint(1, 40) if k > 4000 else b.rnd.randint(2100, 2600), m)      # 66-72 KiB in all
    p1 = b.put(m)
    b.fill(65536 + k - 8, m)
    p2 = b.put(m)
    b.fill(_tail(b.rnd), not_first=b.b[p1 + 8])
    return b.case("alias64k", literal_span(p2, 8), f"k={k} at {p2} of {len(b)}")


def pos0_case(P, total=None):
    """the value begins with the marker (R3: ref > in_data)"""
    b = Build(f"pos0-{P}-{total}")
    m = b.marker(8)
    b.put(m)
    b.fill(P - 8, m)
    b.put(m)
    b.fill(_tail(b.rnd) if total is None else total - len(b), not_first=b.b[8])
    if P <= MAX_OFF:
        claim = all_of(literal_span(P, 1), has_ref(P + 1, 7, P))
    else:
        claim = literal_span(P, 8)
    return b.case("pos0", claim, f"P={P} of {len(b)}")


def collide_case(lead, control=False, gap=(5, 9)):
    """A, a trigram B of A's slot visited as a literal, A again (R1: the slot
    holds B, whose bytes differ, so A's second start is a literal)"""
    b = Build(f"collide-{lead}-{gap}")                       # the control: the same bytes but for B
    A = b.marker(7)
    B = bytes(b.rnd.choice(colliders(A[:3], b.hi, b.hi + 128)))
    b.fill(lead, A)
    pA1 = b.put(A)
    if control:
        b.fill(gap[0] + 3 + gap[1], A)
    else:
        b.fill(gap[0], B)
        b.put(B)
        b.fill(gap[1], A)
    pA2 = b.put(A)
    b.fill(_tail(b.rnd), not_first=b.b[pA1 + 7])
    d = pA2 - pA1
    if control:
        return b.case("collide:control", has_ref(pA2, 7, d), f"A at {pA1}, {pA2}")
    return b.case("collide", all_of(literal_span(pA2, 1), has_ref(pA2 + 1, 6, d)), f"A at {pA1}, {pA2}")


SKIP_M = 24
SKIP_K = {"start": 0, "interior-first": 1, "interior": 13, "interior-last": SKIP_M - 3, "m-2": SKIP_M - 2,
          "m-1": SKIP_M - 1, "after": SKIP_M}


def skip_case(where, lead):
    """X, X + G matched as one reference of SKIP_M bytes, then a probe with the
    trigram at offset k of X + G (R2: which positions of a match are inserted)"""
    k = SKIP_K[where]
    b = Build(f"skip-{where}-{lead}")
    XG = b.marker(SKIP_M + 6)
    X = XG[:SKIP_M]
    uniq = b.marker(4)
    probe = XG[k:k + 3] + bytes([b.other(XG[k + 3])]) + uniq
    b.fill(lead, X)
    pX1 = b.put(X)
    b.fill(b.rnd.randint(4, 30), X)
    pX2 = b.put(XG)
    b.fill(b.rnd.randint(4, 30), probe)
    pQ = b.put(probe)
    b.fill(_tail(b.rnd))
    target = (pX1 if where.startswith("interior") else pX2) + k
    claim = all_of(has_ref(pX2, SKIP_M, pX2 - pX1), has_ref(pQ, 3, pQ - target))
    return b.case("skip", claim, f"{where}: probe at {pQ} -> {target}")


# agreements (bytes, from the trigram's first) of neighbouring chain members,
# from the probe backwards: the probe with Y_m, Y_m with Y_m-1, ...
CHAINS = ([3], [9], [4, 8], [8, 4], [8, 8], [16, 16], [17, 17], [9, 9], [3, 3], [5, 5, 16], [17, 6, 6],
          [7, 9, 3, 16], [16, 17, 8, 9, 7], [6, 7, 4, 5, 17], [3, 4, 5, 6, 7, 8, 9, 16])
SUFFIX = 20


def chain_case(ag, lead, variant=None):
    """Bodies Y_1..Y_m, each pre_i + T + S_i: once visited, then again matched
    whole with T interior (not inserted, R2).  The probe T + S carries T: the
    same-slot chain behind it passes the m skipped copies before the first
    inserted position, T of Y_m's first copy.  ``beyond``: that position lies
    more than 8192 back; ``masked``: a collider of T, visited as a literal,
    lies between the first copies and the second ones."""
    m = len(ag)
    for attempt in range(50):
        b = Build(f"chain-{ag}-{lead}-{variant}-{attempt}")
        T = b.marker(3)
        rb = lambda k: bytes(b.hi + b.rnd.randrange(128) for _ in range(k))
        S = {m: rb(SUFFIX)}
        for i in range(m - 1, 0, -1):                       # Y_i agrees with Y_i+1 in ag[m - i] bytes
            c = ag[m - i] - 3
            S[i] = S[i + 1][:c] + bytes([b.other(S[i + 1][c])]) + rb(SUFFIX - c - 1)
        c = ag[0] - 3
        probe = T + S[m][:c] + bytes([b.other(S[m][c])]) + rb(SUFFIX - c - 1)
        Y = {i: b.marker(4) + T + S[i] for i in range(1, m + 1)}
        for y in list(Y.values()) + [probe]:
            b.reserve(y)
        first, second, pB = {}, {}, None
        b.fill(lead, Y[1])
        for i in range(1, m + 1):
            first[i] = b.put(Y[i])
            nxt = Y[i + 1] if i < m else (Y[1] if variant is None else b"")
            b.fill(b.rnd.randint(4, 8), nxt)
        if variant == "masked":
            B = bytes(b.rnd.choice(colliders(T, b.hi, b.hi + 128)))
            b.fill(3, B)
            pB = b.put(B)
            b.fill(5, Y[1])
        elif variant == "beyond":
            b.fill(first[1] + 8100 - len(b), Y[1])
        for i in range(1, m + 1):
            second[i] = b.put(Y[i])
            b.fill(b.rnd.randint(4, 8) if i < m or variant != "beyond" else 150, Y[i + 1] if i < m else probe,
                   not_first=b.b[first[i] + len(Y[i])])
        pQ = b.put(probe)
        b.fill(_tail(b.rnd))
        v = bytes(b.b)
        # the construction holds when the slot of T occurs at the T's alone, no
        # match runs over a first copy's T or the probe's, and every second
        # copy is one reference (judged by the model; else drawn again)
        at = set(np.nonzero(slots_of(v) == slot(*T))[0].tolist())
        want = {first[i] + 4 for i in Y} | {second[i] + 4 for i in Y} | {pQ} | ({pB} if pB is not None else set())
        toks = tokens(model_compress(v, roomy(len(v))))
        whole = all(Tok("ref", second[i], len(Y[i]), second[i] - first[i]) in toks for i in Y)
        inside = lambda p: any(t.kind == "ref" and t.pos < p < t.pos + t.length for t in toks)
        if at == want and whole and not any(inside(first[i] + 4) for i in Y) and not inside(pQ):
            break
    else:
        raise AssertionError("no chain")
    copies = all_of(*[has_ref(second[i], len(Y[i]), second[i] - first[i]) for i in Y])
    note = f"m={m} ag={ag} probe at {pQ}"
    if variant == "beyond":
        assert pQ - (first[m] + 4) > MAX_OFF and pQ - (second[m] + 4) <= MAX_OFF
        return b.case("chain:beyond", all_of(copies, literal_span(pQ, 3)), note)
    if variant == "masked":
        return b.case("chain:masked", all_of(copies, literal_span(pQ, 1)), note)
    return b.case("chain", all_of(copies, has_ref(pQ, ag[0], pQ - (first[m] + 4))), note)


LEN_L = tuple(range(3, 11)) + tuple(range(15, 21)) + (23, 24, 25) + tuple(range(31, 35)) + \
    tuple(range(263, 267)) + tuple(range(527, 531))


def len_case(L, lead):
    """a body of L bytes and its copy, a differing byte behind it (R4)"""
    b = Build(f"len-{L}-{lead}")
    body = b.marker(L)
    b.fill(lead, body)
    p1 = b.put(body)
    b.fill(b.rnd.randint(5, 40), body)
    p2 = b.put(body)
    b.fill(_tail(b.rnd), not_first=b.b[p1 + L])
    claims, pos, rem = [], p2, L
    while rem >= 3:
        n = min(rem, MAX_REF)
        claims.append(has_ref(pos, n, p2 - p1))
        pos, rem = pos + n, rem - n
    if rem:
        claims.append(literal_span(pos, rem))
    return b.case("len", all_of(*claims), f"L={L} at {p2}")


def end_case(L, t, lead=1):
    """the copy with t bytes behind it (R3 ip + 4 < in_end, R4 maxlen): the model's tokens"""
    b = Build(f"end-{L}-{t}-{lead}")
    body = b.marker(L)
    b.fill(lead, body)
    p1 = b.put(body)
    b.fill(b.rnd.randint(5, 12), body)
    b.put(body)
    b.fill(t, not_first=b.b[p1 + L])
    v = bytes(b.b)
    return b.case("end", same_tokens(model_compress(v, roomy(len(v)))), f"L={L} t={t}")


RUN_N = tuple(range(5, 13)) + tuple(range(63, 67)) + tuple(range(264, 271)) + tuple(range(528, 532)) + \
    tuple(range(959, 963)) + (4096, 8192, 8193, 16384, 65536)


def run_case(period, n):
    """one byte, or two or three, repeated: every lane of a window hits one slot"""
    rnd = random.Random(f"run-{period}-{n}")
    pat = bytes(rnd.sample(range(256), period))
    v = (pat * (n // period + 1))[:n]
    return Case(v, roomy(n), "run", same_tokens(model_compress(v, roomy(n))), f"period {period}, {n} bytes")


WINDOW_P2 = (2047, 2048, 2049, 2879, 2880, 2881)        # 63, 64, 65 mod 64; 959, 960, 961 mod 960
WINDOW_D = (3, 63, 64, 65, 959, 960, 961, 1920)


def window_case(p2, d):
    """the second marker at p2, the first d back: around the edges of the
    kernels' 64-position windows and 960-position blocks"""
    b = Build(f"window-{p2}-{d}")
    if d < 8:
        m = b.marker(8 + d, period=d)
        b.fill(p2 - d, m)
        b.put(m)
    else:
        m = b.marker(8)
        b.fill(p2 - d, m)
        p1 = b.put(m)
        b.fill(d - 8, m)
        assert b.put(m) == p2
    b.fill(_tail(b.rnd), not_first=None if d < 8 else b.b[p1 + 8])
    return b.case("window", has_ref(p2, 8, d), f"at {p2}, d={d}")


def triple_case(base):
    """T + u, T + v, T + u inside one 64-position window: the last takes the
    middle one (R1), though it agrees longer with the first"""
    assert base % 64 == 0 and base >= 64
    b = Build(f"triple-{base}")
    T, u, v = b.marker(3), b.marker(5), b.marker(5)
    while v[0] == u[0]:
        v = b.marker(5)
    b.fill(base + 5, T + u)
    p1 = b.put(T + u)
    b.fill(base + 20 - len(b), T + v)
    p2 = b.put(T + v)
    b.fill(base + 40 - len(b), T + u)
    p3 = b.put(T + u)
    b.fill(_tail(b.rnd))
    assert (p1, p2, p3) == (base + 5, base + 20, base + 40)
    return b.case("window:triple", all_of(has_ref(p2, 3, 15), has_ref(p3, 3, 20)), f"window at {base}")


LIT_K = (0, 1, 31, 32, 33, 63, 64, 65)


def lit_case(k, e, lead=1):
    """k literals between two matches, e literals behind the last (R5: header
    patch, rollover at 32, the empty run undone): the model's tokens"""
    b = Build(f"lit-{k}-{e}-{lead}")
    m = b.marker(8)
    b.fill(lead, m)
    p1 = b.put(m)
    b.fill(b.rnd.randint(4, 70), m)
    b.put(m)
    b.fill(k, m, not_first=b.b[p1 + 8])
    b.put(m)
    b.fill(e, not_first=b.b[p1 + 8])
    v = bytes(b.b)
    return b.case("lit", same_tokens(model_compress(v, roomy(len(v)))), f"k={k} e={e}")


@functools.lru_cache(maxsize=None)
def base_cases():
    """every family but ``cap``"""
    res = []
    for d in (1, 2, 3):
        res += [dist_case(d, lead) for lead in (1,) + SIZE_LEADS]
    for d in (8190, 8191, 8192, 8193, 8194):
        res += [dist_case(d, 1), dist_case(d, 9000)]
    res += [dist_case(d, total=n) for n in (16384, 65536, 70000) for d in (8191, 8192, 8193)]
    res += [alias_case(k) for k in (1, 50, 8191)]
    res += [pos0_case(P) for P in (12, 100, 4000, 8192, 8193)]
    res += [pos0_case(100, 12000), pos0_case(8192, 40000)]
    for lead in (1, 70, 5000) + SIZE_LEADS:
        res += [collide_case(lead), collide_case(lead, control=True)]
    for where in SKIP_K:
        res += [skip_case(where, lead) for lead in (1, 5000) + SIZE_LEADS]
    for i, ag in enumerate(CHAINS):
        res.append(chain_case(ag, 1 + 7 * i))
        res.append(chain_case(ag, ((5000,) + SIZE_LEADS)[i % 3]))
    res += [chain_case([5, 9], 1, "beyond"), chain_case([5, 9], 30000, "beyond")]
    res += [chain_case(ag, lead, "masked") for ag, lead in (([5, 9], 1), ([8], 40), ([4, 4, 6], 9000), ([5, 9], 30000))]
    res += [len_case(L, 1 + L % 61) for L in LEN_L]
    res += [len_case(L, lead) for L in (8, 9, 18, 19, 264, 265, 528) for lead in (5000,) + SIZE_LEADS]
    res += [end_case(L, t) for L in range(3, 21) for t in range(7)]
    res += [end_case(L, t, lead) for L, t in ((19, 0), (20, 0), (8, 2), (17, 1)) for lead in SIZE_LEADS]
    res += [run_case(p, n) for p in (1, 2, 3) for n in RUN_N]
    res.append(run_case(1, 70000))
    res += [window_case(p2, d) for p2 in WINDOW_P2 for d in WINDOW_D]
    res += [window_case(p2 + 960 * k, d) for k in (10, 40) for p2 in WINDOW_P2 for d in (64, 960)]
    res += [triple_case(base) for base in (192, 192 + 64 * 75, 192 + 64 * 150, 192 + 64 * 600)]
    res += [lit_case(k, e) for k in LIT_K for e in range(4)]
    res += [lit_case(k, e, lead) for k, e in ((0, 0), (32, 1), (65, 3)) for lead in SIZE_LEADS]
    return tuple(res)


CAP_KINDS = ("match", "literal", "tail", "fits")


@functools.lru_cache(maxsize=None)
def cap_cases(count=40, full=6):
    """R6: ``count`` small cases (at most 300 bytes, taken family by family)
    at the caps 1..8 and r - 6 .. r + 2 around their uncapped result r,
    ``full`` of them at every cap from 1 to r + 2.  The label names the
    check the model says refuses."""
    small = [c for c in base_cases() if 8 <= len(c.value) <= 300]
    by_family = collections.OrderedDict()
    for c in small:
        by_family.setdefault(family(c.label), []).append(c)
    # first the value that ends in a 19-byte reference (the unrolled compares
    # run past maxlen): :176 refuses it at caps r and r + 1, where it would fit
    picked = [c for c in small if c.label == "end" and c.note == "L=19 t=0"]
    seen, k = {c.value for c in picked}, 0
    while len(picked) < count and any(k < len(cs) for cs in by_family.values()):
        for cs in by_family.values():                         # family by family, spread over each
            c = cs[(k * 37) % len(cs)]
            if k < len(cs) and len(picked) < count and c.value not in seen:
                seen.add(c.value)
                picked.append(c)
        k += 1
    res = []
    for i, c in enumerate(picked):
        whole = model_compress(c.value, roomy(len(c.value)))
        r = len(whole)
        caps = range(1, r + 3) if i < full else sorted(set(range(1, 9)) | set(range(max(1, r - 6), r + 3)))
        for cap in caps:
            got, kind = model_compress(c.value, cap, why=True)
            claim = (lambda x, w=whole: x == w) if kind == "fits" else (lambda x: x is None)
            res.append(Case(c.value, cap, "cap:" + kind, claim, f"{c.label} {c.note}, r={r}"))
    return tuple(res)


def all_cases():
    return base_cases() + cap_cases()


# the least number of cases of a label that the families above imply
MIN_COUNT = {"dist": 14, "dist:large": 9, "alias64k": 3, "pos0": 5, "collide": 3, "collide:control": 3,
             "skip": 3 * len(SKIP_K), "chain": len(CHAINS), "chain:beyond": 1, "chain:masked": 1,
             "len": len(LEN_L), "end": 18 * 7, "run": 3 * len(RUN_N), "window": 48, "window:triple": 1,
             "lit": 8 * 4, "cap:match": 20, "cap:literal": 20, "cap:tail": 20, "cap:fits": 20}


# ---- stream layers --------------------------------------------------------------

def stream_windows(n):
    """64-position windows a value takes in a workgroup's stream (ks_windows)"""
    return (n - 2 + 63) >> 6 if n >= 8 else 0


def _text(rnd, n):
    """n bytes with matches and literals: words of a small vocabulary"""
    words = [rnd.randbytes(rnd.randint(3, 9)) for _ in range(24)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words)
        if rnd.random() < 0.3:
            out += rnd.randbytes(rnd.randint(1, 5))
    return bytes(out[:n])


NEIGHBOUR_N = (8, 9, 63, 64, 65, 100, 960, 961, 4096, 8192)


def neighbour_layers(G):
    """three layers of G values: column j twice the same value, then that
    value shifted by one byte.  The stale entry of every slot then names the
    same text in the previous value, at most 8192 stream positions back."""
    vals = {}
    for n in NEIGHBOUR_N:
        for k in range(2):
            rnd = random.Random(f"neighbour-{n}-{k}")
            v = _text(rnd, n)
            vals[(n, k)] = (v, bytes([rnd.randrange(256)]) + v[:-1])
    layers = [[], [], []]
    for j in range(G):
        n = NEIGHBOUR_N[j % len(NEIGHBOUR_N)]
        v, shifted = vals[(n, (j // len(NEIGHBOUR_N)) % 2)]
        cap = roomy(n) if (j // 20) % 2 == 0 else tight(n)
        layers[0].append(Case(v, cap, "neighbour", anything, f"{n} bytes"))
        layers[1].append(Case(v, cap, "neighbour", anything, f"{n} bytes, again"))
        layers[2].append(Case(shifted, cap, "neighbour:shift", anything, f"{n} bytes, shifted"))
    return layers


@functools.lru_cache(maxsize=None)
def wrap_value(seed, n, far):
    """-> (value, [(position of the second marker, distance)]): overlapping
    marker pairs, the long ones (distances ``far``) chained so that every
    position between the first and the last marker lies inside a pair, short
    ones (3..200) every 256 bytes"""
    b = Build(f"wrap-{seed}-{n}")
    rnd = b.rnd
    taken = np.zeros(n, bool)
    places = []                                               # (pos, text, first's position or None, d)

    def place(pos, text, first, d):
        lo, hi = max(0, pos - 4), pos + len(text) + 4
        if pos < 1 or hi > n - 6 or taken[lo:hi].any():
            return False
        taken[lo:hi] = True
        places.append((pos, text, first, d))
        return True

    a, k = 2, 0
    while True:                                               # the long pairs, each begun inside the one before
        d = far[1] if k == 0 and seed == 0 else rnd.randint(*far)
        if a + d + 12 > n - 6:
            break
        m = b.marker(8)
        assert place(a, m, None, d) and place(a + d, m, a, d)
        a, k = a + d - rnd.randint(40, 120), k + 1
    assert k >= 1
    short = (3, 12, 13, 17, 63, 64, 65, 100, 200)
    for i, pos in enumerate(range(300, n - 300, 256)):
        d = short[i % len(short)]
        pos += rnd.randint(0, 60)
        if d < 8:
            m = b.marker(8 + d, period=d)
            place(pos, m, pos, d)
        else:
            m = b.marker(8)
            lo, hi = pos - 4, pos + d + 12                    # both halves at once: d - 8 >= 4 filler bytes between
            if not taken[lo:hi].any():
                taken[lo:hi] = True
                places += [(pos, m, None, d), (pos + d, m, pos, d)]
    pairs, after = [], None
    for pos, text, first, d in sorted(places):
        b.fill(pos - len(b), text, not_first=after)
        assert b.put(text) == pos
        after = None
        if first == pos:                                      # the periodic text holds both halves
            pairs.append((pos + d, d))
        elif first is not None:
            pairs.append((pos, d))
            after = b.b[first + 8]
    b.fill(n - len(b), not_first=after)
    return bytes(b.b), tuple(pairs)


def wrap_case(seed, n, far):
    v, pairs = wrap_value(seed, n, far)
    return Case(v, roomy(n), "wrap", all_of(*[has_ref(p, 8, d) for p, d in pairs]), f"{n} bytes, {len(pairs)} pairs")


WRAP_LEADS = (0, 2050, 1026, 3010)


def wrap_layers(G, n, layers, far):
    """a lead layer (column j: a value of WRAP_LEADS[j % 4] bytes, so that the
    stream's 65536 boundary falls inside a later value; 0: a 3-byte value,
    which takes no window) and ``layers`` layers of n-byte wrap values: even
    columns keep one value, odd ones rotate through the three"""
    W = [wrap_case(k, n, far) for k in range(3)]
    leads = {}
    for ln in WRAP_LEADS:
        leads[ln] = Case(_text(random.Random(f"lead-{ln}"), ln) if ln else b"abc", roomy(max(ln, 3)), "wrap:lead",
                         anything, f"lead of {ln} bytes")
    res = [[leads[WRAP_LEADS[j % 4]] for j in range(G)]]
    for k in range(layers):
        layer = []
        for j in range(G):
            c = W[(j + k * (j % 2)) % 3]
            layer.append(c if (j // 4) % 2 == 0 else c._replace(cap=tight(n), label="wrap:tight", claim=anything))
        res.append(layer)
    return res


def boundary_inside(layers):
    """columns whose stream position 65536 falls strictly inside a value
    (not at its first window): [(column, layer)]"""
    res = []
    for j in range(len(layers[0])):
        g = 0
        for k, layer in enumerate(layers):
            w = 64 * stream_windows(len(layer[j].value))
            if g < 65536 < g + w:
                res.append((j, k))
            g += w
    return res
