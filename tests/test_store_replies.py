"""lzf_gpu_store_replies: one reply frame per entry of an index list, in a reply
arena in device memory -- the reply of GET for the requests of many clients,
and of the single-key INC / DEC after lzf_gpu_store_minc(single = 1).

The expected bytes come from the Python model below.  It restates the reply
buffer of gbClientEnqueueData (src/net.c:1170-1202), the item reply of
gbClientEnqueueItem (src/net.c:1216-1254) and the validity rule
(src/query.c:204-224).  The framing is parity-unpinned: src/net.c cannot be
built here, so nothing compares these frames with the reference's own output;
the model and the kernels are two readings of the same source lines.  The
value of an LZF item is compared with the original input the store was built
from, never with a decoder's output.

Every buffer a test hands over with a size is allocated larger, with guard
bytes before and after it, which are checked afterwards.  Every GPU batch
first asserts, from the model alone, that each outcome it means to cover is
present."""
import ctypes
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests.oracle_lib import ROOT, synth

try:                                    # before liblzf_hip.so loads: one HIP runtime in the process
    import torch as _torch  # noqa: F401
except ImportError:
    _torch = None

import gibson_amd

ENC_PLAIN, ENC_LZF, ENC_NUMBER, ENC_NULL = 0, 1, 2, 0xFF
ERR, NOT_FOUND, E_NAN, E_LOCKED, R_OK, VAL = 0, 1, 2, 4, 5, 6              # src/query.h:64-70
DONE, DEAD, EXPIRED, LOCKED, NAN, CONVERTED, UNCHANGED, EDECODE = range(8)
GET, VALUE = 0, 1
OK, TOO_BIG = 0, 1
PAD = 0xFFFFFFFF
CODE_OF = {DONE: VAL, CONVERTED: VAL, DEAD: NOT_FOUND, EXPIRED: NOT_FOUND, LOCKED: E_LOCKED, NAN: E_NAN,
           UNCHANGED: E_NAN}
NEW_NAMES = ("lzf_gpu_store_replies_work_size", "lzf_gpu_store_replies", "lzf_host_reply_code")


# ---- CPU ---------------------------------------------------------------------

def test_library_exports_the_reply_calls():
    L = gibson_amd.lib()
    for n in NEW_NAMES:
        assert hasattr(L, n), n
        assert n in gibson_amd.lzf.EXPORTS
    for n in ("store_replies", "store_replies_work", "reply_code"):
        assert callable(getattr(gibson_amd, n)), n
    assert (gibson_amd.REPLY_GET, gibson_amd.REPLY_VALUE) == (0, 1)
    assert (gibson_amd.REPLY_OK, gibson_amd.REPLY_TOO_BIG) == (0, 1)
    assert (gibson_amd.REPL_ERR, gibson_amd.REPL_ERR_NOT_FOUND, gibson_amd.REPL_ERR_NAN, gibson_amd.REPL_ERR_LOCKED,
            gibson_amd.REPL_OK, gibson_amd.REPL_VAL) == (0, 1, 2, 4, 5, 6)
    assert gibson_amd.ENT_EDECODE == 7 and gibson_amd.ENT_UNCHANGED == 6
    # the header states the same numbers
    src = open(os.path.join(ROOT, "include", "lzf_gpu.h")).read()
    for name, v in (("LZF_REPL_ERR", 0), ("LZF_REPL_ERR_NOT_FOUND", 1), ("LZF_REPL_ERR_NAN", 2),
                    ("LZF_REPL_ERR_LOCKED", 4), ("LZF_REPL_OK", 5), ("LZF_REPL_VAL", 6), ("LZF_ENT_EDECODE", 7),
                    ("LZF_REPLY_GET", 0), ("LZF_REPLY_VALUE", 1), ("LZF_REPLY_OK", 0), ("LZF_REPLY_TOO_BIG", 1)):
        line = [x for x in src.splitlines() if x.startswith("#define %s " % name)][0]
        assert int(line.split()[2]) == v, line


def test_reply_call_rejects_bad_arguments_without_device():
    # argument validation happens before any HIP call, so this runs on CPU;
    # only calls that must be refused are made (the pointers are host memory)
    L = gibson_amd.lib()
    null = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(512)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    names = ("idx", "op", "store", "voff", "vsize", "enc", "vlen", "time", "ttl", "last", "replies", "used", "roff",
             "rlen", "est", "result", "work")

    def call(mode=GET, n=1, count=1, max_val_len=16, **nulls):
        a = {k: p for k in names}
        a["op"] = p if mode == VALUE else null
        for k, v in nulls.items():
            a[k] = v
        return L.lzf_gpu_store_replies(a["idx"], n, mode, a["op"], a["store"], a["voff"], a["vsize"], a["enc"],
                                       a["vlen"], count, a["time"], a["ttl"], 5, a["last"], max_val_len,
                                       a["replies"], 64, a["used"], a["roff"], a["rlen"], a["est"], a["result"],
                                       a["work"], null)

    optional = {"op", "time", "ttl", "last"}
    for mode in (GET, VALUE):
        for k in names:
            if k not in optional:
                assert call(mode, **{k: null}) == -1, (mode, k)
        for k in ("time", "ttl"):                    # exactly one NULL time array
            assert call(mode, **{k: null}) == -1, (mode, k)
        assert call(mode, n=0) == -1
        assert call(mode, count=0) == -1
        assert call(mode, max_val_len=(64 << 20) + 1) == -1
    assert call(GET, op=p) == -1                     # op_status must match the mode
    assert call(VALUE, op=null) == -1
    for mode in (-1, 2, 7):
        assert call(mode) == -1 and call(mode, op=p) == -1


def test_reply_work_size():
    ws = gibson_amd.lib().lzf_gpu_store_replies_work_size
    prev = 0
    for n in (1, 2, 1023, 1024, 1025, 3000, 262145, 1 << 20, (1 << 31) + 5, 2**32 - 2, 2**32 - 1):
        w = ws(n)
        assert w > 0 and w >= prev and w >= 40 * n, n
        prev = w
    assert ws(2**32 - 1) < 2**40                     # 64-bit arithmetic: no wrap
    assert ws(0) > 0


def test_host_reply_code():
    f = gibson_amd.lib().lzf_host_reply_code
    for st in list(range(9)) + [255]:
        assert f(st) == CODE_OF.get(st, ERR) == gibson_amd.reply_code(st), st
    assert [f(s) for s in range(9)] == [VAL, NOT_FOUND, NOT_FOUND, E_LOCKED, E_NAN, VAL, E_NAN, ERR, ERR]


# ---- the model -----------------------------------------------------------------

def frame(code, enc, payload):
    """gbClientEnqueueData's buffer, src/net.c:1170-1202"""
    return struct.pack("<hBI", code, enc, len(payload)) + bytes(payload)


def code_reply(code):
    """gbClientEnqueueCode: PLAIN, size 1, one 0x00 byte"""
    return frame(code, ENC_PLAIN, b"\0")


class Model:
    """the replies of one call over ``idx``, every entry judged on ``h.enc`` as
    it is before the call.  orig[i]: the input item i was stored from; failed:
    the items whose LZF stream is known not to decode to vlen"""

    def __init__(self, mode, idx, h, orig, time, ttl, now, max_val_len, op_status=None, failed=()):
        self.st, self.rep, self.slot, self.valid, self.expired = [], [], [], [], []
        self.failed_k = []
        for k, i in enumerate(idx):
            i = int(i)
            if mode == GET:
                if i >= h.n or h.enc[i] == ENC_NULL:
                    s, code = DEAD, NOT_FOUND
                elif ttl is not None and ttl[i] > 0 and now - int(time[i]) >= ttl[i]:
                    s, code = EXPIRED, NOT_FOUND
                    self.expired.append(i)
                else:
                    s, code = DONE, VAL
                    self.valid.append(i)
            else:
                s = int(op_status[k])
                code = CODE_OF.get(s, ERR)
                if code == VAL and (i >= h.n or h.enc[i] == ENC_NULL):
                    code = ERR
            r, slot = code_reply(code), 8
            if code == VAL:
                e = int(h.enc[i])
                if e == ENC_LZF:                                   # src/net.c:1233-1250: decoded, sent PLAIN
                    vl = int(h.vlen[i])
                    if vl > max_val_len or i in failed:
                        s, r = EDECODE, code_reply(ERR)
                        slot = 8 if vl > max_val_len else max(8, 7 + vl)
                        self.failed_k.append(k)
                    else:
                        assert len(orig[i]) == vl
                        r = frame(VAL, ENC_PLAIN, orig[i])
                        slot = max(8, len(r))
                else:
                    r = frame(VAL, e, h.stored(i))
                    slot = max(8, len(r))
            self.st.append(s)
            self.rep.append(r)
            self.slot.append(slot)
        self.n = len(self.st)
        self.off = np.concatenate([[0], np.cumsum(self.slot[:-1], dtype=np.int64)]).astype(np.int64)
        self.need = int(np.sum(self.slot, dtype=np.int64))
        self.values = sum(1 for r in self.rep if struct.unpack_from("<h", r)[0] == VAL)
        self.fail = len(self.failed_k)
        nexp = len(self.expired) if mode == GET else 0
        self.counts = [self.values, nexp, self.n - self.values - nexp - self.fail]

    def result(self, status=OK):
        return self.counts + [status, self.need, self.fail]

    def image(self, cap, fill):
        """the arena's expected bytes and which of them are specified"""
        img, known = np.full(cap, fill, np.uint8), np.ones(cap, bool)
        for k in range(self.n):
            o = int(self.off[k])
            img[o:o + len(self.rep[k])] = np.frombuffer(self.rep[k], np.uint8)
            if self.st[k] == EDECODE:
                known[o + 8:o + self.slot[k]] = False              # the rest of a failed slot is unspecified
        return img, known


# ---- GPU ---------------------------------------------------------------------

FILL = 0xA5
GUARD = 0x5A
ROOM = 4096                              # guard bytes around the arena and the work area
EDGE = 64                                # guard elements around the small outputs
NOW = 1_700_000_000
BIG = [4096, 4097, 16384, 16385, 70000]
SMALL = [1, 2, 7, 8, 15, 16, 17, 63, 64, 65]
KINDS = (0, 1, 4)                        # text, json, random bytes (synth.h)


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    gibson_amd.lib()
    return t


def _helpers():
    from tests import test_store_mget as m
    return m


class Guarded:
    """a tensor of n elements with EDGE guard elements on both sides"""

    def __init__(self, torch, n, dtype, fill, edge=EDGE, shift=0):
        g = {torch.uint8: GUARD, torch.int32: 0x5A5A5A5A, torch.int64: 0x5A5A5A5A5A5A5A5A}[dtype]
        self.g, self.n, self.lo = g, n, edge + shift
        self.buf = torch.full((edge + shift + n + edge,), g, dtype=dtype, device="cuda")
        self.t = self.buf[self.lo:self.lo + n]
        self.t.fill_(fill)

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:self.lo] == self.g).all() and (b[self.lo + self.n:] == self.g).all())


class Run:
    """one lzf_gpu_store_replies call; no synchronisation"""

    def __init__(self, torch, d, idx, mode, cap, max_val_len, base=0, now=NOW, op_status=None, arena=None, off=None,
                 size=None, last=True):
        m = _helpers()
        self.d, self.cap = d, cap
        self.idx = idx if hasattr(idx, "numel") else m._i32(torch, np.asarray(idx, np.uint32))
        n = int(self.idx.numel())
        self.arena = Guarded(torch, cap, torch.uint8, FILL, edge=ROOM, shift=base)
        self.used = Guarded(torch, 1, torch.int64, -1)
        self.off = Guarded(torch, n, torch.int64, -1)
        self.len = Guarded(torch, n, torch.int32, -1)
        self.est = Guarded(torch, n, torch.uint8, 0x77)
        self.result = Guarded(torch, 6, torch.int64, -1)
        self.work = Guarded(torch, int(gibson_amd.lib().lzf_gpu_store_replies_work_size(n)), torch.uint8, GUARD,
                            edge=ROOM)
        gibson_amd.store_replies(self.idx, mode, d.arena if arena is None else arena, d.off if off is None else off,
                                 d.size if size is None else size, d.enc, d.vlen, d.time, d.ttl, now, max_val_len,
                                 self.arena.t, self.used.t, self.off.t, self.len.t, self.est.t, self.result.t,
                                 op_status=op_status, last_access=d.last if last else None, work=self.work.t)

    def outputs(self, torch):
        torch.cuda.synchronize()
        return {"arena": self.arena.t.cpu().numpy(), "used": int(self.used.t.item()),
                "off": self.off.t.cpu().numpy(), "len": self.len.t.cpu().numpy(), "est": self.est.t.cpu().numpy(),
                "result": self.result.t.cpu().numpy()}

    def check(self, torch, m, status=OK):
        o = self.outputs(torch)
        print("replies result", o["result"].tolist(), "used", o["used"], "expected", m.result(status))
        for g in (self.arena, self.used, self.off, self.len, self.est, self.result, self.work):
            assert g.intact()
        assert o["result"].tolist() == m.result(status)
        assert (o["off"] == m.off).all()
        assert o["len"].tolist() == [len(r) for r in m.rep]
        assert o["est"].tolist() == m.st
        if status == TOO_BIG:
            assert o["used"] == 0
            assert (o["arena"] == FILL).all()                      # no byte of the arena is written
            return o
        assert o["used"] == m.need <= self.cap
        img, known = m.image(self.cap, FILL)
        bad = np.nonzero((o["arena"] != img) & known)[0]
        assert not len(bad), (len(bad), "first wrong byte", int(bad[0]))
        return o


def check_side_effects(d, enc_before, valid, expired, last_before=None, now=NOW):
    _helpers().check_side_effects(d, enc_before, valid, expired, last_before, now)


def build_mixed(torch):
    """about 1500 items through lzf_gpu_set_store at compression 64 -- text,
    json and random bytes of the edge lengths, the decode-class edges and random
    lengths up to 3000 -- some 8-byte ones turned into NUMBER items, with dead
    items and TTLs of every kind; and a list of 2500 entries over it"""
    m = _helpers()
    rnd = random.Random(0x9E71)
    sizes = [(n, k) for n in SMALL + BIG for k in KINDS]
    while len(sizes) < 1500:
        sizes.append((rnd.randint(1, 3000), KINDS[len(sizes) % 3]))
    rnd.shuffle(sizes)
    values = [synth(k, 0x5EED9E71, i, n) for i, (n, k) in enumerate(sizes)]
    keys = [b"item:%d" % i for i in range(len(values))]
    h = m.build_store(torch, values, 64, keys)
    for i in np.nonzero((h.vlen == 8) & (h.enc == ENC_PLAIN))[0][:2]:
        h.enc[i] = ENC_NUMBER
    rs = np.random.RandomState(0x9E71)
    big = [i for i, (n, _) in enumerate(sizes) if n in BIG or n in SMALL]     # every edge length is in the list, valid
    dead = np.array([i for i in rs.choice(h.n, 120, replace=False) if i not in big])
    ttl = rs.choice([-1, 0, 5, 600, 32767], h.n).astype(np.int32)
    ttl[big] = 0
    age = rs.randint(0, 1200, h.n).astype(np.int64)
    hd = h.dead(dead)
    idx = np.concatenate([rs.randint(0, h.n, 2500 - len(big) - 6), big, [PAD, h.n, h.n + 5, PAD, 2**31, h.n]])
    idx = idx.astype(np.uint32)
    rs.shuffle(idx)
    return {"values": values, "host": hd, "fresh": h, "dead": dead, "ttl": ttl, "time": NOW - age, "idx": idx,
            "max": 70000}


@pytest.fixture(scope="module")
def mixed(torch):
    mx = build_mixed(torch)
    h = mx["host"]
    mx["model"] = Model(GET, mx["idx"], h, mx["values"], mx["time"], mx["ttl"], NOW, mx["max"])
    return mx


def assert_mixed_outcomes(mx, m):
    """from the model alone: what the mixed batch means to cover is there"""
    h, idx = mx["host"], mx["idx"]
    assert len(idx) == 2500 and m.n == 2500 and set(m.st) == {DONE, DEAD, EXPIRED}
    assert len(m.expired) >= 100 and m.counts[2] >= 100 and not m.fail
    encs = h.enc[m.valid]
    assert set(encs.tolist()) == {ENC_PLAIN, ENC_LZF, ENC_NUMBER}
    lzf = h.vlen[[i for i in m.valid if h.enc[i] == ENC_LZF]]
    assert (lzf <= 4096).sum() >= 100 and ((lzf > 4096) & (lzf <= 16384)).sum() >= 2 and (lzf > 16384).sum() >= 2
    assert set(BIG) <= set(lzf.tolist())                            # the decode-class edges, as LZF items
    plain = h.vlen[[i for i in m.valid if h.enc[i] == ENC_PLAIN]]
    assert set(SMALL + BIG) <= set(plain.tolist())                  # and as PLAIN items (random bytes)
    assert len(set(m.valid)) < len(m.valid) and len(set(m.expired)) < len(m.expired)   # duplicates
    assert (idx == PAD).sum() == 2 and (idx >= h.n).sum() == 6
    assert (h.enc[idx[idx < h.n]] == ENC_NULL).sum() >= 50


def run_mixed(torch, mx, m, base):
    h = mx["host"]
    d = _helpers().Dev(torch, h, mx["time"], mx["ttl"])
    r = Run(torch, d, mx["idx"], GET, m.need + 100, mx["max"], base=base)
    o = r.check(torch, m)
    check_side_effects(d, h.enc, m.valid, m.expired)
    assert (d.arena.cpu().numpy()[len(h.arena):] == GUARD).all()
    o["enc"], o["last"] = d.enc.cpu().numpy(), d.last.cpu().numpy()
    return o


ROUTE = "LZF_GPU_REPLY_ONE_ROUTE"       # "1" and unset: one decode launch; "0": one per decode size class


def child_mixed(path):
    """the mixed batch at both arena offsets in this process, under the
    route the process was started with and then under the other one (the
    variable is read per call), checked against the model, the outputs saved
    for the parent"""
    import torch
    assert os.environ[ROUTE] == "1"
    mx = build_mixed(torch)
    m = Model(GET, mx["idx"], mx["host"], mx["values"], mx["time"], mx["ttl"], NOW, mx["max"])
    out = {}
    for route in ("1", "0"):
        os.environ[ROUTE] = route
        for base in (0, 7):
            for k, v in run_mixed(torch, mx, m, base).items():
                out["%s%d_%s" % (k, base, route)] = np.asarray(v)
    np.savez(path, **out)
    print("child ok")


# 1
@pytest.mark.gpu
def test_mixed_store_every_byte(torch, mixed, tmp_path):
    m = mixed["model"]
    assert_mixed_outcomes(mixed, m)
    mine = {base: run_mixed(torch, mixed, m, base) for base in (0, 7)}
    # the same call with LZF_GPU_REPLY_ONE_ROUTE=1 (one decode launch for all the sizes) in a fresh process,
    # which then runs it with one launch per decode size class as well
    path = str(tmp_path / "one_route.npz")
    code = "from tests import test_store_replies as t; t.child_mixed(%r)" % path
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, LZF_GPU_REPLY_ONE_ROUTE="1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("child ok"), r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(path)
    for route in ("1", "0"):
        for base in (0, 7):
            for k, v in mine[base].items():
                assert (np.asarray(v) == got["%s%d_%s" % (k, base, route)]).all(), (k, base, route)


# 2
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_list_sizes_around_a_tile(torch, mixed, n):
    h = mixed["host"]
    rs = np.random.RandomState(n)
    small = np.nonzero((h.vlen <= 300) & (h.enc != ENC_NULL))[0]
    idx = rs.choice(small, n).astype(np.uint32)                       # with repeats
    if n == 1:
        idx[0] = int(np.nonzero((h.enc == ENC_LZF) & (h.vlen <= 300))[0][0])
    m = Model(GET, idx, h, mixed["values"], None, None, NOW, 300)
    assert m.values == n and (n == 1 or {ENC_PLAIN, ENC_LZF} <= set(h.enc[idx].tolist()))
    d = _helpers().Dev(torch, h)
    Run(torch, d, idx, GET, m.need + 9, 300).check(torch, m)
    check_side_effects(d, h.enc, m.valid, [])


# 3
@pytest.mark.gpu
def test_all_misses_is_ok(torch, mixed):
    h, time, ttl = mixed["host"], mixed["time"], mixed["ttl"]
    every = Model(GET, np.arange(h.n), h, mixed["values"], time, ttl, NOW, mixed["max"])
    idx = np.concatenate([mixed["dead"][:20], every.expired[:20], [h.n, PAD]]).astype(np.uint32)
    m = Model(GET, idx, h, mixed["values"], time, ttl, NOW, mixed["max"])
    assert m.result() == [0, 20, 22, OK, 8 * 42, 0] and all(r == code_reply(NOT_FOUND) for r in m.rep)
    assert code_reply(NOT_FOUND) == bytes([1, 0, 0, 1, 0, 0, 0, 0])
    d = _helpers().Dev(torch, h, time, ttl)
    Run(torch, d, idx, GET, 8 * 42, mixed["max"]).check(torch, m)     # unlike MGET's NOT_FOUND: a reply each
    check_side_effects(d, h.enc, [], every.expired[:20])


# 4
@pytest.mark.gpu
def test_too_big(torch, mixed):
    h, time, ttl = mixed["host"], mixed["time"], mixed["ttl"]
    idx = mixed["idx"][:400]
    m = Model(GET, idx, h, mixed["values"], time, ttl, NOW, mixed["max"])
    assert m.values >= 200 and len(m.expired) >= 10 and m.counts[2] >= 10
    assert ENC_LZF in h.enc[m.valid] and ENC_PLAIN in h.enc[m.valid]
    d = _helpers().Dev(torch, h, time, ttl)
    Run(torch, d, idx, GET, m.need - 1, mixed["max"]).check(torch, m, TOO_BIG)
    check_side_effects(d, h.enc, m.valid, m.expired)                  # done whatever the status
    d = _helpers().Dev(torch, h, time, ttl)
    Run(torch, d, idx, GET, m.need, mixed["max"], base=7).check(torch, m)   # fits exactly
    check_side_effects(d, h.enc, m.valid, m.expired)


# 5
def crafted_store(oracle):
    """a store laid out by hand: per decode class a sound LZF item on either
    side of each faulty one, PLAIN items and a PLAIN item of size 0 between
    them.  -> (Host, originals, failed items, the fault of each)"""
    from tests.lzf_tokens import lit, ref
    m = _helpers()
    rnd = random.Random(0xBAD5)
    items, orig, failed, why = [], [], [], {}

    def add(enc, stored, vlen, original, fault=None):
        items.append((enc, bytes(stored), vlen))
        orig.append(original)
        if fault:
            failed.append(len(items) - 1)
            why[len(items) - 1] = fault

    def sound(n, seed):
        v = synth(1, 0xBAD5, seed, n)
        s = oracle.compress(v, n - 1)
        assert s is not None
        return v, s

    for c, n in enumerate((3000, 10000, 30000)):
        v, s = sound(n, 10 * c)
        add(ENC_LZF, s, n, v)
        add(ENC_LZF, lit(b"ab") + ref(5, 8) + lit(b"tail"), n, None, "back")    # a reference before the output start
        add(ENC_PLAIN, b"plain-%d" % c, 7, None)
        v, s = sound(n, 10 * c + 1)
        add(ENC_LZF, s[:len(s) - 5], n, None, "cut")                             # cut short through val_size
        add(ENC_PLAIN, b"", 0, None)
        v, s = sound(n - 1, 10 * c + 2)
        add(ENC_LZF, s, n, None, "len+1")                                        # val_len one too large
        v, s = sound(n + 1, 10 * c + 3)
        add(ENC_LZF, s, n, None, "len-1")                                        # val_len one too small
        v, s = sound(n, 10 * c + 4)
        add(ENC_LZF, s, n, v)
        add(ENC_PLAIN, bytes(rnd.randrange(256) for _ in range(33)), 33, None)
    v, s = sound(40001, 99)
    add(ENC_LZF, s, 40001, None, "bound")                                        # val_len above max_val_len
    v, s = sound(40000, 98)
    add(ENC_LZF, s, 40000, v)
    for i in failed:                                                              # each fault is one, by the oracle
        got, _ = oracle.decompress(items[i][1], items[i][2])
        assert why[i] == "bound" or got is None or len(got) != items[i][2], why[i]
    arena = bytearray(b"\xEE" * 5)
    off, size = [], []
    for _, stored, _ in items:
        off.append(len(arena))
        size.append(len(stored))
        arena += stored + b"\xEE" * rnd.randint(0, 3)
    keys = [b"c%d" % i for i in range(len(items))]
    h = m.Host(np.frombuffer(bytes(arena), np.uint8), off, size, [e for e, _, _ in items], [n for _, _, n in items],
               keys)
    return h, orig, failed, why


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["1", "0"])
@pytest.mark.parametrize("one_class", [False, True])
def test_decode_failures_are_per_entry(torch, oracle, monkeypatch, one_class, route):
    monkeypatch.setenv(ROUTE, route)                 # read per call: one decode launch, or one per size class
    h, orig, failed, why = crafted_store(oracle)
    bound = 40000
    idx = np.arange(h.n, dtype=np.uint32)
    if one_class:                                    # a bound inside the first class: one decode launch
        idx = np.array([i for i in idx if h.vlen[i] <= 3001], np.uint32)
        bound = 3000
    m = Model(GET, idx, h, orig, None, None, NOW, bound, failed=set(failed))
    faults = {why[int(idx[k])] for k in m.failed_k}
    if one_class:
        assert faults == {"back", "cut", "len+1", "len-1"} and m.fail == 4
    else:
        assert faults == {"back", "cut", "len+1", "len-1", "bound"} and m.fail == 13
        cls = [0 if h.vlen[int(idx[k])] <= 4096 else 1 if h.vlen[int(idx[k])] <= 16384 else 2 for k in m.failed_k]
        assert min(cls.count(c) for c in (0, 1, 2)) >= 4               # failures in every decode class
    assert m.values >= 3 and 7 in [len(r) for r in m.rep]              # a size-0 PLAIN item: 7 bytes in 8
    for k in m.failed_k:
        assert m.st[k] == EDECODE and m.rep[k] == code_reply(ERR) == bytes([0, 0, 0, 1, 0, 0, 0, 0])
    d = _helpers().Dev(torch, h)
    for base in (0, 7):
        Run(torch, d, idx, GET, m.need + 50, bound, base=base).check(torch, m)
    assert (d.arena.cpu().numpy()[len(h.arena):] == GUARD).all()
    assert (d.enc.cpu().numpy() == h.enc).all()


# 6
@pytest.mark.gpu
def test_value_mode_after_single_minc(torch):
    m = _helpers()
    rnd = random.Random(0x1AC6)
    values, kind = [], []
    for i in range(240):
        k = ("num8", "digits", "nan", "lzf")[i % 4]
        if k == "num8":
            values.append(struct.pack("<q", rnd.randrange(-2**40, 2**40)))
        elif k == "digits":
            values.append(b"%d" % rnd.randrange(-10**9, 10**9))
        elif k == "nan":
            values.append(synth(0, 0x1AC6, i, rnd.randint(3, 40)))
        else:
            values.append(synth(1, 0x1AC6, i, rnd.randint(200, 900)))
        kind.append(k)
    h = m.build_store(torch, values, 64, [b"v%d" % i for i in range(len(values))])
    for i, k in enumerate(kind):
        assert h.enc[i] == (ENC_LZF if k == "lzf" else ENC_PLAIN)
        if k == "num8":
            h.enc[i] = ENC_NUMBER
    rs = np.random.RandomState(0x1AC6)
    dead = rs.choice(h.n, 30, replace=False)
    h = h.dead(dead)
    ttl = np.where(rs.rand(h.n) < 0.15, 5, 0).astype(np.int32)        # age 100: these are expired
    lock = np.where(rs.rand(h.n) < 0.2, -1, 0).astype(np.int64)
    time = np.full(h.n, NOW - 100, np.int64)
    idx = np.concatenate([rs.permutation(h.n)[:200], [PAD, h.n + 1]]).astype(np.uint32)
    delta = -3
    # gbQueryIncDecHandler (src/query.c:853-886): validity before the lock, an LZF item is not a number
    st, val = [], []
    for i in idx:
        i, v = int(i), 0
        if i >= h.n or h.enc[i] == ENC_NULL:
            s = DEAD
        elif ttl[i] > 0:
            s = EXPIRED
        elif lock[i] == -1:
            s = LOCKED
        elif kind[i] == "num8":
            s, v = DONE, struct.unpack("<q", values[i])[0] + delta
        elif kind[i] == "digits":
            s, v = CONVERTED, int(values[i]) + delta
        else:
            s = NAN
        st.append(s)
        val.append(v)
    assert set(st) == {DONE, DEAD, EXPIRED, LOCKED, NAN, CONVERTED}
    assert any(s == NAN and kind[int(i)] == "lzf" for s, i in zip(st, idx))
    assert any(s == NAN and kind[int(i)] == "nan" for s, i in zip(st, idx))
    exp = [frame(VAL, ENC_NUMBER, struct.pack("<q", v)) if s in (DONE, CONVERTED) else code_reply(CODE_OF[s])
           for s, v in zip(st, val)]
    assert {struct.unpack_from("<h", r)[0] for r in exp} == {VAL, NOT_FOUND, E_LOCKED, E_NAN}

    d = m.Dev(torch, h, time, ttl)
    used0 = len(h.arena)
    cap = used0 + 8 * len(idx)
    arena = Guarded(torch, cap, torch.uint8, FILL, edge=ROOM)
    arena.t[:used0] = torch.from_numpy(h.arena).cuda()
    d_used = torch.tensor([used0], dtype=torch.int64, device="cuda")
    d_lock = m._i64(torch, lock)
    d_idx = m._i32(torch, idx)
    est = Guarded(torch, len(idx), torch.uint8, 0x77)
    ev = Guarded(torch, len(idx), torch.int64, -1)
    res = torch.full((6,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    w = gibson_amd.store_minc(d_idx, delta, arena.t, d_used, d.off, d.size, d.enc, d.time, d.ttl, d_lock, NOW, res,
                              status, single=True, last_access=d.last, entry_status=est.t, entry_value=ev.t)
    torch.cuda.synchronize()
    del w
    assert int(status.item()) == 0 and est.t.cpu().numpy().tolist() == st and ev.t.cpu().numpy().tolist() == val
    enc1, last1 = d.enc.cpu().numpy().copy(), d.last.cpu().numpy().copy()
    # the model over the store as the operator left it: the reply call reads the items, not entry_value
    h1 = m.Host(arena.t.cpu().numpy()[:int(d_used.item())], d.off.cpu().numpy(), d.size.cpu().numpy().view(np.uint32),
                enc1, h.vlen, h.keys)
    mod = Model(VALUE, idx, h1, values, None, None, NOW, 900, op_status=st)
    assert mod.rep == exp and mod.st == st and mod.counts == [mod.values, 0, len(idx) - mod.values]
    r = Run(torch, d, d_idx, VALUE, mod.need + 3, 900, base=7, op_status=est.t, arena=arena.t)
    r.check(torch, mod)
    assert (d.enc.cpu().numpy() == enc1).all() and (d.last.cpu().numpy() == last1).all()   # untouched by the reply call
    assert arena.intact() and est.intact() and ev.intact()
    # statuses no operator leaves, an LZF item under DONE, and a REPL_VAL entry without an item
    lzf_live = [i for i in range(h.n) if h1.enc[i] == ENC_LZF][:3]
    gone = int(np.nonzero(h1.enc == ENC_NULL)[0][0])
    idx2 = np.array(lzf_live + [gone, PAD, 0, 1, 2], np.uint32)
    st2 = [DONE, CONVERTED, UNCHANGED, DONE, CONVERTED, EDECODE, 8, 255]
    mod2 = Model(VALUE, idx2, h1, values, None, None, NOW, 900, op_status=st2)
    assert [struct.unpack_from("<h", x)[0] for x in mod2.rep] == [VAL, VAL, E_NAN, ERR, ERR, ERR, ERR, ERR]
    r = Run(torch, d, idx2, VALUE, mod2.need, 900, op_status=m._u8(torch, st2), arena=arena.t)
    r.check(torch, mod2)
    assert (d.enc.cpu().numpy() == enc1).all() and (d.last.cpu().numpy() == last1).all()


# 7
@pytest.mark.gpu
def test_one_stream_one_synchronise(torch):
    """set_store -> key_index_insert -> key_index_lookup -> store_replies, the
    index list never leaving the device, compared after a single synchronise"""
    m = _helpers()
    rnd = random.Random(0x57E4)
    values = [synth(KINDS[i % 3], 0x57E4, i, rnd.choice((1, 8, 63, 64, 200, 900, 5000))) for i in range(600)]
    keys = [b"key:%d:%s" % (i, b"x" * (i % 7)) for i in range(len(values))]
    n = len(values)
    query = [keys[i] for i in rnd.sample(range(n), 300)] + [b"key:absent", b"nokey", keys[5], keys[5]]
    rnd.shuffle(query)
    want = [keys.index(q) if q in keys else PAD for q in query]
    assert want.count(PAD) == 2 and want.count(5) >= 2

    d_in, d_off, d_len, ln = m.set_store_args(torch, values)
    room = int(ln.sum()) + 8 * n + 16
    arena = Guarded(torch, room, torch.uint8, FILL, edge=ROOM)
    used = torch.zeros(1, dtype=torch.int64, device="cuda")
    sstatus = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    off = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    size = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    enc = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    kl = np.array([len(k) for k in keys], np.uint32)
    koff = np.concatenate([[0], np.cumsum(kl[:-1], dtype=np.int64)]).astype(np.int64)
    d_keys = m._u8(torch, np.frombuffer(b"".join(keys) + b"\0", np.uint8))
    d_koff, d_klen = m._i64(torch, koff), m._i32(torch, kl)
    ql = np.array([len(q) for q in query], np.uint32)
    qoff = np.concatenate([[0], np.cumsum(ql[:-1], dtype=np.int64)]).astype(np.int64)
    d_q, d_qoff, d_qlen = m._u8(torch, np.frombuffer(b"".join(query) + b"\0", np.uint8)), m._i64(torch, qoff), \
        m._i32(torch, ql)
    table = torch.full((gibson_amd.key_index_bytes(2048),), 0xFF, dtype=torch.uint8, device="cuda")
    tused = torch.zeros(1, dtype=torch.int32, device="cuda")
    ires = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    istatus = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    idx = torch.full((len(query),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    lres = torch.full((3,), -1, dtype=torch.int64, device="cuda")

    class D:
        pass
    d = D()
    d.arena, d.off, d.size, d.enc, d.vlen = arena.t, off, size, enc, m._i32(torch, ln)
    d.time = d.ttl = None
    d.last = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    cap = 8 * len(query) + int(ln.sum()) * 2
    torch.cuda.synchronize()
    w = gibson_amd.set_store(d_in, d_off, d_len, 64, int(ln.max()), int(ln.sum()), arena.t, used, off, size, enc,
                             sstatus)
    gibson_amd.key_index_insert(table, tused, d_keys, d_koff, d_klen, enc, 0, n, ires, istatus)
    gibson_amd.key_index_lookup(table, d_keys, d_koff, d_klen, enc, d_q, d_qoff, d_qlen, idx, lres)
    r = Run(torch, d, idx, GET, cap, int(ln.max()))
    torch.cuda.synchronize()                                          # the only one before the results are read
    del w
    assert int(sstatus.item()) == 0 and int(istatus.item()) == 0
    assert idx.cpu().numpy().view(np.uint32).tolist() == want
    h = m.Host(arena.t.cpu().numpy()[:int(used.item())], off.cpu().numpy(), size.cpu().numpy().view(np.uint32),
               enc.cpu().numpy(), ln, keys)
    assert {ENC_PLAIN, ENC_LZF} == set(h.enc.tolist())
    mod = Model(GET, want, h, values, None, None, NOW, int(ln.max()))
    assert mod.values == len(query) - 2 and mod.counts[2] == 2
    r.check(torch, mod)
    last = np.full(n, -1, np.int64)
    last[np.array(mod.valid)] = NOW
    assert (d.last.cpu().numpy() == last).all() and arena.intact()
