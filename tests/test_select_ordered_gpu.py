"""lzf_gpu_store_select_ordered on the GPU against lzf_host_store_select_ordered,
the host twin that tests/test_select_ordered.py holds to the reference's
recorded trie order: bit for bit, between guard bands on sel and result and
past the work area.  The twin walks a trie, the kernels hash births and sort
rows, so the two are different routes to one list.

Then end to end: the ordered list, still in HBM, feeds lzf_gpu_store_mget and
lzf_gpu_store_keys, and the frames equal those built on the CPU from the
model's list."""
import random

import numpy as np
import pytest

from tests import trie_model as tm
from tests.oracle_lib import synth

import gibson_amd

PAD = tm.PAD
GUARD = 0x5A
SEL_GUARD = 0x5A5A5A5A
UNSET = -0x0123456789ABCDEF
ROOM = 4096
NOW = 1_700_000_000
ENC_NULL = tm.ENC_NULL


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    gibson_amd.lib()
    return t


def _dev(torch, a, dt):
    return torch.from_numpy(np.array(a).view(dt)).cuda()


class Store:
    """a store image on the device and on the host"""

    def __init__(self, torch, keys, live, shift=0):
        self.keys, self.live = keys, live
        self.arrays = tm.store_arrays(keys, live, shift)
        blob, koff, klen, enc = self.arrays
        self.d = (_dev(torch, blob, np.uint8), _dev(torch, koff, np.int64), _dev(torch, klen, np.int32),
                  _dev(torch, enc, np.uint8))

    def twin(self, prefix, limit, cap, cand_cap, node_cap):
        blob, koff, klen, enc = self.arrays
        sel, res = gibson_amd.host_select_ordered(blob, koff, klen, enc, np.frombuffer(prefix, np.uint8), cap, limit,
                                                  cand_cap, node_cap)
        return sel.tolist(), [int(x) for x in res]

    def needs(self, prefix):
        _, _, cands, words = tm.rule_order(self.keys, self.live, prefix)
        return max(1, cands), max(1, words)

    def run(self, torch, prefix, limit, cap, cand_cap, node_cap, mis=0):
        """one call between guards -> (sel, result) as lists"""
        count = len(self.keys)
        sel = torch.full((cap + 16,), SEL_GUARD, dtype=torch.int32, device="cuda")
        res = torch.full((5 + 4,), UNSET, dtype=torch.int64, device="cuda")
        wsize = int(gibson_amd.lib().lzf_gpu_store_select_ordered_work_size(count, cand_cap, node_cap, cap))
        work = torch.full((mis + wsize + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
        gibson_amd.store_select_ordered(*self.d, _dev(torch, np.frombuffer(prefix, np.uint8), np.uint8), sel[:cap],
                                        res[:5], limit=limit, cand_cap=cand_cap, node_cap=node_cap,
                                        work=work[mis:mis + wsize])
        torch.cuda.synchronize()
        s, r, w = sel.cpu().numpy().view(np.uint32), res.cpu().numpy(), work.cpu().numpy()
        assert (s[cap:] == SEL_GUARD).all() and (r[5:] == UNSET).all()
        assert (w[:mis] == GUARD).all() and (w[mis + wsize:] == GUARD).all()
        return s[:cap].tolist(), r[:5].tolist()

    def check(self, torch, prefix, limit, cap, cand_cap=None, node_cap=None, mis=0):
        need = self.needs(prefix)
        cand_cap, node_cap = cand_cap or need[0], node_cap or need[1]
        want = self.twin(prefix, limit, cap, cand_cap, node_cap)
        got = self.run(torch, prefix, limit, cap, cand_cap, node_cap, mis)
        print("prefix", prefix[:8], "limit", limit, "cap", cap, "caps", cand_cap, node_cap, "result", got[1], "twin",
              want[1])
        assert got[1] == want[1]
        bad = [r for r in range(cap) if got[0][r] != want[0][r]]
        assert not bad, (len(bad), "first wrong entry", bad[0], got[0][bad[0]], want[0][bad[0]])
        return want


def random_store(count, seed, dense=False):
    """keys of 1-40 bytes: most under k:, a small alphabet next so that nodes
    are shared, longer random tails; overwrites kill the key's earlier item,
    and a quarter of the rest is deleted (dense: few overwrites, other stems
    and deletes, so that most items match)"""
    rnd = random.Random(seed)
    keys, live, at = [], [], {}
    again, other, alive = (0.02, 0.03, 0.95) if dense else (0.15, 0.15, 0.75)
    for i in range(count):
        if keys and rnd.random() < again:
            key = rnd.choice(keys)
        else:
            stem = b"k:" if rnd.random() >= other else rnd.choice([b"k", b"j:", b"k;"])
            key = stem + bytes(rnd.choice(b"abc") for _ in range(rnd.randint(0, 6)))
            key = (key + bytes(rnd.choice(b"abcdefghij:_0123456789") for _ in range(rnd.choice([3, 5, 8, 31] if dense else [0, 0, 3, 31]))))[:40]
        if key in at:
            live[at[key]] = False
        at[key] = i
        keys.append(key)
        live.append(rnd.random() < alive)
    return keys, live


COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)


@pytest.mark.gpu
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("shift,mis,room", [(0, 0, 1), (3, 2, 4)])
def test_kernel_equals_twin(torch, count, shift, mis, room):
    # room 1: node_cap at exactly the node words needed, the table at its fullest; 4: four times that
    # 5000 dense: more than 4096 matches, five tiles, three merge passes with an odd run out
    keys, live = random_store(count, 0x0D0 + count, dense=count == 5000)
    st = Store(torch, keys, live, shift)
    prefix = b"k:" if count > 1 else keys[0][:1]
    cands, words = st.needs(prefix)
    full = tm.rule_order(keys, live, prefix)[0]
    if count >= 1023:
        assert full != sorted(full) and len(full) > count // 4
    if count == 5000:
        assert len(full) > 4096
    for limit, cap in ((-1, len(full) + 5), (max(1, len(full) // 3), max(1, len(full))), (0, max(1, len(full) - 1))):
        want = st.check(torch, prefix, limit, cap, cands, words * room, mis)
        kept = full[:limit] if limit > 0 else full
        assert want[0][:min(cap, len(kept))] == kept[:cap]             # the twin is the model's list


@pytest.mark.gpu
@pytest.mark.parametrize("matches", (1023, 1024, 1025, 2047, 2048, 2049))
def test_match_counts_around_one_and_two_tiles(torch, matches):
    rnd = random.Random(0xA70 + matches)
    tails = set()
    while len(tails) < matches + 200:
        tails.add(bytes(rnd.choice(b"abcd") for _ in range(rnd.randint(1, 9))))
    tails = sorted(tails)
    rnd.shuffle(tails)
    items = [(b"m:" + t, k < matches) for k, t in enumerate(tails)] + [(b"n:" + t, True) for t in tails[:100]]
    rnd.shuffle(items)
    keys, live = [k for k, _ in items], [l for _, l in items]
    st = Store(torch, keys, live)
    full, n, cands, _ = tm.rule_order(keys, live, b"m:")
    assert n == matches and cands == matches + 200 and full != sorted(full)
    want = st.check(torch, b"m:", -1, matches + 3)
    assert want[0][:matches] == full
    st.check(torch, b"m:", matches - 1, matches)


@pytest.mark.gpu
@pytest.mark.parametrize("name", tm.FAMILIES)
def test_crafted_family(torch, name):
    steps, prefix = tm.family(name)
    script = tm.Script(steps)
    full = tm.rule_order(script.keys, script.live, prefix)[0]
    if not name.startswith("none"):
        assert full != sorted(full), "ascending index would pass: the batch shows nothing"
    st = Store(torch, script.keys, script.live, shift=1)
    for limit in sorted({-1, 0, 1, max(1, len(full) // 2), max(1, len(full)), len(full) + 1}):
        kept = full[:limit] if limit > 0 else full
        for cap in sorted({max(1, len(kept) - 1), max(1, len(kept)), len(kept) + 3}):
            want = st.check(torch, prefix, limit, cap)
            assert want[0][:min(cap, len(kept))] == kept[:cap]


@pytest.mark.gpu
def test_short_work_is_refused_whole_and_the_repeat_succeeds(torch):
    keys, live = random_store(2049, 0xE304)
    st = Store(torch, keys, live)
    full, matches, cands, words = tm.rule_order(keys, live, b"k:")
    for cand_cap, node_cap in ((cands - 1, words), (cands, words - 1)):
        sel, res = st.run(torch, b"k:", -1, len(full) + 2, cand_cap, node_cap)
        assert sel == [PAD] * (len(full) + 2)
        assert res == [0, matches, cands, words, gibson_amd.ORDER_EWORK]
        assert (sel, res) == st.twin(b"k:", -1, len(full) + 2, cand_cap, node_cap)
        # the repeat with the needs the refusal reported
        again = st.check(torch, b"k:", -1, len(full) + 2, res[2], res[3])
        assert again[0][:len(full)] == full and again[1][4] == gibson_amd.ORDER_OK


@pytest.mark.gpu
def test_two_calls_into_fresh_work_areas_agree(torch):
    steps, prefix = tm.family("hot")
    script = tm.Script(steps)
    st = Store(torch, script.keys, script.live)
    cands, words = st.needs(prefix)
    first = st.run(torch, prefix, -1, cands, cands, words)
    second = st.run(torch, prefix, -1, cands, cands, words, mis=2)
    assert first == second and first[1][0] == first[1][1] > 3000


# ---- end to end: select_ordered -> mget, select_ordered -> keys ------------------

@pytest.fixture(scope="module")
def lifecycle(torch):
    """300 items from three SET batches of 100 into one arena.  A key set again
    kills its earlier item (the overwrite), DELs follow the first batch and a
    TTL sweep the second; every step runs on the device and in the model."""
    from tests import test_store_mget as sm
    rnd = random.Random(0xE2E)
    count, per = 300, 100
    values = [synth(i % 6, 0xE2E0, i, rnd.randint(1, 300)) for i in range(count)]
    age = np.array([rnd.randint(0, 100) for _ in range(count)], np.int64)
    ttl = np.array([rnd.choice([0, 0, -1, 60, 200]) for _ in range(count)], np.int32)
    time = NOW - 40 - age                                      # the sweep runs at NOW - 40, the MGET at NOW
    room = sm.BASE + sum(len(v) for v in values) + 8 * count + 16
    arena = torch.full((room,), sm.FILL, dtype=torch.uint8, device="cuda")
    used = torch.tensor([sm.BASE], dtype=torch.int64, device="cuda")
    vo = torch.full((count,), -1, dtype=torch.int64, device="cuda")
    vs = torch.full((count,), -1, dtype=torch.int32, device="cuda")
    en = torch.full((count,), ENC_NULL, dtype=torch.uint8, device="cuda")
    d_time, d_ttl = _dev(torch, time, np.int64), _dev(torch, ttl, np.int32)
    keys, live, at, keep = [], [], {}, []
    for b in range(count // per):
        lo, hi = b * per, (b + 1) * per
        kill = []
        for i in range(lo, hi):
            if keys and rnd.random() < 0.25:
                key = rnd.choice(keys)
            else:
                key = rnd.choice([b"u:", b"u:", b"u:", b"v:"]) + bytes(rnd.choice(b"abc") for _ in range(rnd.randint(0, 5)))
            if key in at and live[at[key]]:
                kill.append(at[key])
                live[at[key]] = False
            at[key] = i
            keys.append(key)
            live.append(True)
        d_in, d_off, d_len, ln = sm.set_store_args(torch, values[lo:hi])
        status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        keep.append(gibson_amd.set_store(d_in, d_off, d_len, 64, int(ln.max()), int(ln.sum()), arena, used, vo[lo:hi],
                                         vs[lo:hi], en[lo:hi], status))
        if b == 0:                                             # DELs
            for i in rnd.sample([i for i in range(hi) if live[i]], 15):
                kill.append(i)
                live[i] = False
        if kill:
            gibson_amd.store_delete(_dev(torch, np.array(kill, np.uint32), np.int32), en)
        if b == 1:                                             # the TTL sweep
            expired = torch.zeros(1, dtype=torch.int32, device="cuda")
            gibson_amd.store_expire(d_time, d_ttl, NOW - 40, en, expired)
            swept = [i for i in range(hi) if live[i] and ttl[i] > 0 and NOW - 40 - int(time[i]) >= ttl[i]]
            for i in swept:
                live[i] = False
            torch.cuda.synchronize()
            assert int(expired.item()) == len(swept) > 3
        torch.cuda.synchronize()
        assert int(status.item()) == 0
    h = sm.Host(arena.cpu().numpy()[:int(used.item())], vo.cpu().numpy(), vs.cpu().numpy().view(np.uint32),
                en.cpu().numpy(), [len(v) for v in values], keys)
    assert ((h.enc != ENC_NULL) == np.array(live)).all() and 100 < sum(live) < 250
    return {"sm": sm, "host": h, "live": live, "time": time, "ttl": ttl}


def ordered_list(torch, d, count, prefix, limit, cap):
    sel = torch.full((cap,), SEL_GUARD, dtype=torch.int32, device="cuda")
    res = torch.full((5,), UNSET, dtype=torch.int64, device="cuda")
    w = gibson_amd.store_select_ordered(d.keys, d.koff, d.klen, d.enc, _dev(torch, np.frombuffer(prefix, np.uint8), np.uint8),
                                        sel, res, limit=limit, cand_cap=count, node_cap=int(d.keys.numel()))
    return sel, res, w


@pytest.mark.gpu
def test_select_ordered_then_mget(torch, oracle, lifecycle):
    sm, h = lifecycle["sm"], lifecycle["host"]
    limit, cap = 40, 64
    order, matches, _, _ = tm.rule_order(h.keys, lifecycle["live"], b"u:", limit)
    assert len(order) == limit < matches and order != sorted(order)
    valid, expired, skipped = sm.model(order, h.enc, h.n, lifecycle["time"], lifecycle["ttl"], NOW)
    assert expired and len(valid) > 20 and not skipped
    d = sm.Dev(torch, h, lifecycle["time"], lifecycle["ttl"], key_shift=3)
    sel, res, w = ordered_list(torch, d, h.n, b"u:", limit, cap)
    m = sm.Mget(torch, d, sel, 1 << 16)                        # no synchronisation in between
    m.check(torch, sm.expect_frame(oracle, h, valid, 1 << 16, True),
            [len(valid), len(expired), cap - limit, gibson_amd.MGET_OK])
    assert sel.cpu().numpy().view(np.uint32).tolist() == order + [PAD] * (cap - limit)
    assert res.cpu().numpy().tolist()[:2] == [limit, matches]
    # the frame in ascending index, what the plain select gives, is another one
    plain = sorted(i for i in range(h.n) if lifecycle["live"][i] and h.keys[i].startswith(b"u:"))[:limit]
    assert sm.model(plain, h.enc, h.n, lifecycle["time"], lifecycle["ttl"], NOW)[0] != valid


@pytest.mark.gpu
def test_select_ordered_then_keys(torch, lifecycle):
    from tests.test_store_meta_keys_gc import keys_model
    sm, h = lifecycle["sm"], lifecycle["host"]
    order, matches, _, _ = tm.rule_order(h.keys, lifecycle["live"], b"u:")
    cap, max_response = h.n, 1 << 16
    exp, found, status, _ = keys_model(h.keys, h.enc, order, True, max_response)
    assert found == matches == len(order) and status == gibson_amd.MGET_OK and order != sorted(order)
    d = sm.Dev(torch, h, key_shift=1)
    sel, res, w = ordered_list(torch, d, h.n, b"u:", -1, cap)
    frame = torch.full((7 + max_response + ROOM,), GUARD, dtype=torch.uint8, device="cuda")
    flen = torch.full((1,), UNSET, dtype=torch.int64, device="cuda")
    result = torch.full((2,), UNSET, dtype=torch.int64, device="cuda")
    w2 = gibson_amd.store_keys(sel, d.keys, d.koff, d.klen, d.enc, frame[:7 + max_response], max_response, flen, result)
    torch.cuda.synchronize()
    assert result.cpu().numpy().tolist() == [found, status] and int(flen.item()) == len(exp)
    f = frame.cpu().numpy().tobytes()
    assert f[:len(exp)] == exp and f[len(exp):] == bytes([GUARD]) * (len(f) - len(exp))
