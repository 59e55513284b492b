"""The ordered prefix select on the CPU: the recorded behaviour of the
reference's trie (tests/golden/trie_order.json), the two models of
tests/trie_model.py, and lzf_host_store_select_ordered, the host twin that the
kernel is held to in tests/test_select_ordered_gpu.py.

The fixture holds search results recorded from the reference's own trie.c; the
restatement of trie.c must reproduce every one of them, and so must the rule
the device computes and the host twin, each over the store image the script
leaves: items numbered in insert order, dead items keeping their keys."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests.oracle_lib import ROOT
from tests import trie_model as tm

import gibson_amd

PAD = tm.PAD
EARG = -1                                          # LZF_GPU_EARG


def _steps(text):
    out = []
    for w in text.split():
        if w[0] == "s":
            key, lim = w[1:].split(":")
            out.append(("s", bytes.fromhex(key), int(lim)))
        else:
            out.append((w[0], bytes.fromhex(w[1:])))
    return out


def _text(steps):
    return " ".join(st[0] + bytes(st[1]).hex() + (":%d" % st[2] if st[0] == "s" else "") for st in steps)


def same(got, want):
    """a recorded list, or the length and digest that stand for a long one"""
    if isinstance(want, dict):
        return len(got) == want["n"] and hashlib.sha256(",".join(map(str, got)).encode()).hexdigest() == want["sha256"]
    return got == want


@pytest.fixture(scope="module")
def recorded():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "trie_order.json")))
    out = []
    for s in doc["scripts"]:
        if "steps" in s:
            steps = _steps(s["steps"])
        else:                                              # a family: the steps this tree builds, pinned by digest
            steps = tm.family_script(s["name"])
            assert hashlib.sha256(_text(steps).encode()).hexdigest() == s["steps_sha256"], s["name"]
        out.append((s["name"], tm.Script(steps), s["results"]))
    return out


def test_fixture_covers_random_scripts_and_every_family(recorded):
    names = [n for n, _, _ in recorded]
    assert sum(n.startswith("random-") for n in names) == 80
    assert set(tm.FAMILIES) <= set(names)
    assert sum(len(r) for _, _, r in recorded) > 1000


def test_trie_restatement_reproduces_every_recorded_search(recorded):
    for name, script, results in recorded:
        assert len(results) == len(script.searches), name
        for (_, _, prefix, limit, got), want in zip(script.searches, results):
            assert same(got, want), (name, prefix, limit)


def test_rule_reproduces_every_recorded_search(recorded):
    for name, script, results in recorded:
        for (n, live, prefix, limit, _), want in zip(script.searches, results):
            assert same(tm.rule_order(script.keys[:n], live, prefix, limit)[0], want), (name, prefix, limit)


def twin(keys, live, prefix, limit, cap, shift=0, cand_cap=None, node_cap=None):
    blob, koff, klen, enc = tm.store_arrays(keys, live, shift)
    sel, res = gibson_amd.host_select_ordered(blob, koff, klen, enc, np.frombuffer(prefix, np.uint8), cap, limit,
                                              cand_cap, node_cap)
    return sel.tolist(), [int(x) for x in res]


def check_twin(keys, live, prefix, limit, want, what):
    """the twin's list and result at caps below, at and above the result"""
    _, matches, cands, words = tm.rule_order(keys, live, prefix)
    for cap in sorted({max(1, len(want) - 1), max(1, len(want)), len(want) + 3}):
        sel, res = twin(keys, live, prefix, limit, cap)
        k = min(len(want), cap)
        assert sel == want[:k] + [PAD] * (cap - k), (what, cap)
        assert res == [k, matches, cands, words, gibson_amd.ORDER_OK], (what, cap)


def test_host_twin_equals_every_recorded_search(recorded):
    for name, script, results in recorded:
        for (n, live, prefix, limit, trie), want in zip(script.searches, results):
            if n:                                          # the restatement's list, which the test above ties to the record
                assert same(trie, want)
                check_twin(script.keys[:n], live, prefix, limit, trie, (name, prefix, limit))


@pytest.mark.parametrize("name", tm.FAMILIES)
def test_host_twin_on_a_crafted_family(name):
    steps, prefix = tm.family(name)
    script = tm.Script(steps + [("s", prefix, -1)])
    full = script.searches[0][4]
    if not name.startswith("none"):
        assert full != sorted(full), "the order must differ from ascending index, or the plain select would pass"
    assert tm.rule_order(script.keys, script.live, prefix)[0] == full
    for limit in sorted({-1, 0, 1, max(1, len(full) // 2), max(1, len(full)), len(full) + 1}):
        want = full[:limit] if limit > 0 else full
        check_twin(script.keys, script.live, prefix, limit, want, (name, limit))


def test_host_twin_orders_two_live_items_of_one_key_by_index():
    keys, live = [b"p:b", b"p:a", b"p:b", b"p:a"], [True, True, True, True]
    assert twin(keys, live, b"p:", -1, 6)[0] == [0, 2, 1, 3, PAD, PAD]
    assert tm.rule_order(keys, live, b"p:")[0] == [0, 2, 1, 3]


def test_host_twin_refuses_short_work_whole():
    steps, prefix = tm.family("prefix-key")
    script = tm.Script(steps)
    want, matches, cands, words = tm.rule_order(script.keys, script.live, prefix)
    for cand_cap, node_cap in ((cands - 1, words), (cands, words - 1)):
        sel, res = twin(script.keys, script.live, prefix, -1, 8, cand_cap=cand_cap, node_cap=node_cap)
        assert sel == [PAD] * 8 and res == [0, matches, cands, words, gibson_amd.ORDER_EWORK]
    sel, res = twin(script.keys, script.live, prefix, -1, 8, cand_cap=cands, node_cap=words)
    assert sel == want + [PAD] * (8 - len(want)) and res[4] == gibson_amd.ORDER_OK


def test_host_twin_reads_keys_at_any_offset():
    steps, prefix = tm.family("dead-birth-overwritten")
    script = tm.Script(steps)
    want = tm.rule_order(script.keys, script.live, prefix)[0]
    for shift in (0, 1, 3):
        assert twin(script.keys, script.live, prefix, -1, len(want), shift=shift)[0] == want


def test_argument_errors():
    L = gibson_amd.lib()
    a = np.zeros(8, np.uint64)
    p = a.ctypes.data

    def host(keys=p, koff=p, klen=p, enc=p, count=1, prefix=p, plen=1, cand=1, node=1, sel=p, cap=1, result=p):
        return L.lzf_host_store_select_ordered(keys, koff, klen, enc, count, prefix, plen, -1, cand, node, sel, cap, result)

    def dev(keys=p, koff=p, klen=p, enc=p, count=1, prefix=p, plen=1, cand=1, node=1, sel=p, cap=1, result=p, work=p):
        return L.lzf_gpu_store_select_ordered(keys, koff, klen, enc, count, prefix, plen, -1, cand, node, sel, cap,
                                              result, work, None)

    assert host() == 0
    for f in (host, dev):
        for bad in ({"keys": None}, {"koff": None}, {"klen": None}, {"enc": None}, {"prefix": None}, {"sel": None},
                    {"result": None}, {"count": 0}, {"plen": 0}, {"cap": 0}, {"cand": 0}, {"node": 0}):
            assert f(**bad) == EARG, (f.__name__, bad)
    assert dev(work=None) == EARG
    assert dev(node=2**63) == EARG          # a table no 64-bit size holds


# count, cand_cap, node_cap -> bytes.  8 state words; per item tile 16 ballot words and 3 sums; the table, a
# power of two of at least 2 * node_cap words of 8 bytes; per candidate tile 2 sums; per candidate an 8-byte
# row offset and 5 u32; 4 bytes per node word; 16 bytes of slack for the caller's pointer
WORK = {
    (1, 1, 1): 64 + 19 * 8 + 2 * 8 + 2 * 8 + 28 + 4 + 16,
    (1024, 1024, 1024): 64 + 19 * 8 + 2048 * 8 + 2 * 8 + 28 * 1024 + 4 * 1024 + 16,
    (1025, 1, 3): 64 + 2 * 19 * 8 + 8 * 8 + 2 * 8 + 28 + 12 + 16,
    (5000, 2049, 40000): 64 + 5 * 19 * 8 + 131072 * 8 + 3 * 2 * 8 + 28 * 2049 + 4 * 40000 + 16,
    (2**32 - 1, 2**32 - 1, 2**40): 64 + 2**22 * 19 * 8 + 2**41 * 8 + 2**22 * 2 * 8 + 28 * (2**32 - 1) + 4 * 2**40 + 16,
}


def test_work_size():
    fn = gibson_amd.lib().lzf_gpu_store_select_ordered_work_size
    for (count, cand, node), want in WORK.items():
        for cap in (1, 77):                                # cap sizes nothing
            assert int(fn(count, cand, node, cap)) == want, (count, cand, node)
    assert int(fn(1, 1, 2**62 + 1, 1)) == 2**64 - 1        # saturates
    assert int(fn(1, 1, 2**64 - 1, 1)) == 2**64 - 1
    assert WORK[(1, 1, 1)] == 296 and WORK[(5000, 2049, 40000)] == 1266836


def test_order_check_runs_clean_under_the_host_sanitizers():
    csrc = os.path.join(ROOT, "gibson_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "build/order_check"])
    out = subprocess.run([os.path.join(csrc, "build", "order_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "order_check: ok" in out.stdout


def test_layout_is_in_carve_check():
    src = open(os.path.join(ROOT, "gibson_amd", "csrc", "carve_check.cpp")).read()
    assert "lzf_order_carve" in src and src.count('fill("order.') == 15
