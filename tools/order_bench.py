#!/usr/bin/env python3
"""What the ordered prefix select costs: against the plain select, for the
price of the order, and against what a caller did before it.

usage: order_bench.py [--items N] [--repeats R] [--warmup W] [--scale S] [--seed N] [--once]

One process.  A store of N (1 M) items with keys of 16-40 bytes, made on the
host from a seed, 10 % of them dead.  A key is "s", one of three stems -- "a:"
on about 1 item in 1000, "b:" on about 1 in 10, "c:" on the rest -- and then
letters of a small alphabet, so that the prefixes "sa:", "sb:", "sc:" and "s"
select about 1 K, 100 K, 900 K and all of the items.

Per prefix, HIP events around every call, W (2) warm-ups and R (7) timed
repeats that alternate the legs:
  (a) select    lzf_gpu_store_select_prefix over the store;
  (b) ordered   lzf_gpu_store_select_ordered, cand_cap and node_cap at what the
                call reports it needs (one untimed call first, as a caller's
                repeat after LZF_ORDER_EWORK would find them);
  (c) host      what a caller does today: download the keys and the three
                descriptor arrays, lzf_host_store_select_ordered on one thread,
                upload the list (a host clock around work that ends in a
                device synchronise).
The ordered list is compared with the host's first.  Also printed: the work
bytes of (b), the candidates, the matches and the node words.

--once runs each ordered call once and nothing else, for a kernel trace taken
in a run of its own.  Prints one JSON object.  --scale divides the item count
(rehearsals)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gibson_amd  # noqa: E402
from mixed_bench import stats, timed  # noqa: E402

ALPHABET = np.frombuffer(b"abcdefgh_01", np.uint8)
PREFIXES = (b"sa:", b"sb:", b"sc:", b"s")     # about N / 1000, N / 10, 9 N / 10 and all N


def make_store(count, seed):
    """keys "s" + stem + letters on the host: (blob, key_off, key_len, enc)"""
    rs = np.random.RandomState(seed)
    klen = rs.randint(16, 41, count).astype(np.uint32)
    koff = (np.cumsum(klen, dtype=np.int64) - klen).astype(np.uint64)
    blob = ALPHABET[rs.randint(0, len(ALPHABET), int(klen.sum()))]
    r = rs.randint(0, 1000, count)
    stem = np.where(r < 1, ord("a"), np.where(r < 101, ord("b"), ord("c"))).astype(np.uint8)
    at = koff.astype(np.int64)
    blob[at], blob[at + 1], blob[at + 2] = ord("s"), stem, ord(":")
    enc = np.where(rs.randint(0, 10, count) == 0, 0xFF, 0x00).astype(np.uint8)
    return blob, koff, klen, enc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0x0DE2)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("order_bench: no GPU")
    dev = torch.device("cuda", 0)
    count = max(1024, a.items // a.scale)
    blob, koff, klen, enc = make_store(count, a.seed)
    d_keys, d_koff = torch.from_numpy(blob).to(dev), torch.from_numpy(koff.view(np.int64)).to(dev)
    d_klen, d_enc = torch.from_numpy(klen.view(np.int32)).to(dev), torch.from_numpy(enc).to(dev)
    out = {"items": count, "key_bytes": int(klen.sum()), "dead": int((enc == 0xFF).sum()), "prefixes": []}
    for prefix in PREFIXES:
        p_host = np.frombuffer(prefix, np.uint8)
        d_prefix = torch.from_numpy(p_host.copy()).to(dev)
        sel = torch.empty(count, dtype=torch.int32, device=dev)
        res = torch.zeros(5, dtype=torch.int64, device=dev)
        res2 = torch.zeros(2, dtype=torch.int32, device=dev)
        # the needs, as a refused first call reports them
        w = gibson_amd.store_select_ordered(d_keys, d_koff, d_klen, d_enc, d_prefix, sel, res, cand_cap=1, node_cap=1)
        torch.cuda.synchronize()
        need = res.cpu().numpy().tolist()
        assert need[4] == gibson_amd.ORDER_EWORK or need[2] <= 1
        cand_cap, node_cap = max(1, need[2]), max(1, need[3])
        work = gibson_amd.store_select_ordered_work(count, cand_cap, node_cap, count, dev)
        swork = gibson_amd.store_select_work(count, dev)

        def ordered():
            gibson_amd.store_select_ordered(d_keys, d_koff, d_klen, d_enc, d_prefix, sel, res, cand_cap=cand_cap,
                                            node_cap=node_cap, work=work)

        def select():
            gibson_amd.store_select_prefix(d_keys, d_koff, d_klen, d_enc, d_prefix, sel, res2, work=swork)

        def host():
            k, o, ln, e = d_keys.cpu().numpy(), d_koff.cpu().numpy(), d_klen.cpu().numpy(), d_enc.cpu().numpy()
            s, _ = gibson_amd.host_select_ordered(k, o.view(np.uint64), ln.view(np.uint32), e, p_host, count)
            up = torch.from_numpy(s.view(np.int32)).to(dev)
            torch.cuda.synchronize()
            return up

        def host_timed():
            torch.cuda.synchronize()
            t = time.perf_counter()
            host()
            return (time.perf_counter() - t) * 1e3

        if a.once:
            ordered()
            torch.cuda.synchronize()
            continue
        ordered()
        torch.cuda.synchronize()
        got, r = sel.cpu().numpy().view(np.uint32).copy(), res.cpu().numpy().tolist()
        want = host().cpu().numpy().view(np.uint32)
        assert r[4] == gibson_amd.ORDER_OK and (got == want).all(), "the ordered list differs from the host's"
        for _ in range(a.warmup):
            select(), ordered()
            torch.cuda.synchronize()
        legs = {"select": [], "ordered": [], "host": []}
        for _ in range(max(a.repeats, 5)):
            legs["select"].append(timed(select))
            legs["ordered"].append(timed(ordered))
            legs["host"].append(host_timed())
        out["prefixes"].append({"prefix": prefix.decode(), "matches": r[1], "candidates": r[2], "node_words": r[3],
                                "work_bytes": int(work.numel()), "select_work_bytes": int(swork.numel()),
                                **{k: stats(v) for k, v in legs.items()}})
        del w, work
    print(json.dumps(out))


if __name__ == "__main__":
    main()
