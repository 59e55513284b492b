#!/usr/bin/env python3
"""What the device key index costs: insert and lookup against a
device-to-device copy of the bytes each call must read.

usage: kidx_bench.py [--items N] [--k K] [--repeats R] [--warmup W] [--scale S] [--seed N]

One process.  A store of N (1 M = 2^20) items whose keys, 16-40 bytes over a
small alphabet, are made on the device (distinct but for chance), and two
tables:
  load 0.50   all N items into 2 N slots;
  load 0.75   the first 3 N / 4 items into N slots, the fullest table the
              insert's bound allows.
Per table, HIP events around every call, warm-ups and R timed repeats (at
least 5), each leg alternating with its copy:
  insert        the clear (outside the timed region), then one
                lzf_gpu_key_index_insert of all the table's items;
  lookup_k      K (100 000) random present keys, from a query arena of their own;
  lookup_all    as many random present keys as the table has items;
  lookup_absent the lookup_all keys with the last byte replaced by one outside
                the alphabet.
The copy of a leg moves as many bytes as the call must read: per query its
key bytes and 12 bytes of q_off / q_len, 8 bytes per slot examined (result[2]
of the call itself), and per hit the stored key's bytes and 13 bytes of
key_off / key_len / enc.  For the insert: each item's key bytes and 13
descriptor bytes twice (claim and settle both hash the key) and 8 bytes per
slot examined twice, the count taken from a lookup of the same keys
afterwards.  The ratio is call over copy; a copy also writes what it reads,
which the calls do not (the lookup writes 4 bytes per query, the insert 8 per
item).  Nothing here is a threshold.

Every lookup's idx is checked against the items the keys were drawn from.
Prints one JSON object.  --scale divides every count (rehearsals)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import gibson_amd  # noqa: E402
from mget_bench import make_keys  # noqa: E402
from mixed_bench import stats, timed  # noqa: E402


def gather_keys(keys, koff, klen, pick):
    """the keys of the items ``pick`` packed into an arena of their own"""
    q_len = klen[pick].to(torch.int64)
    q_off = torch.cumsum(q_len, 0) - q_len
    src = torch.repeat_interleave(koff[pick] - q_off, q_len) + torch.arange(int(q_len.sum().item()), device=keys.device)
    return torch.cat([keys[src], keys.new_zeros(16)]), q_off, q_len.to(torch.int32)


def leg_pair(call, nbytes, dev, a):
    """alternating repeats of ``call`` and of a copy of ``nbytes`` bytes"""
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for _ in range(a.warmup):
        call["warm"]()
        dst.copy_(src)
    ts = {"call": [], "copy": []}
    for _ in range(a.repeats):
        call["before"]()
        ts["call"].append(timed(call["run"]))
        ts["copy"].append(timed(lambda: dst.copy_(src)))
    legs = {k: stats(v) for k, v in ts.items()}
    return {"bytes_read": nbytes, "legs": legs,
            "copy_gb_per_s": round(2 * nbytes / legs["copy"]["median_ms"] / 1e6, 1),
            "call_read_gb_per_s": round(nbytes / legs["call"]["median_ms"] / 1e6, 1),
            "call_over_copy": round(legs["call"]["median_ms"] / legs["copy"]["median_ms"], 3)}


def bench_table(a, dev, gen, keys, koff, klen, n, slots):
    count = klen.numel()
    enc = torch.zeros(count, dtype=torch.uint8, device=dev)
    table = torch.empty(gibson_amd.key_index_bytes(slots), dtype=torch.uint8, device=dev)
    used = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ires = torch.zeros(4, dtype=torch.int64, device=dev)
    lres = torch.zeros(3, dtype=torch.int64, device=dev)

    def clear():
        table.fill_(0xFF)
        used.zero_()
        enc.zero_()                                    # a chance duplicate key is superseded again

    def insert():
        gibson_amd.key_index_insert(table, used, keys, koff, klen, enc, 0, n, ires, status)

    def clear_insert():
        clear()
        insert()

    clear_insert()
    torch.cuda.synchronize()
    out = {"items": n, "slots": slots, "load": round(n / slots, 3), "status": int(status.item()),
           "insert_result": ires.cpu().tolist(), "used": int(used.item())}
    key_bytes = int(klen[:n].sum().item())

    def lookup_leg(pick, absent):
        q, q_off, q_len = gather_keys(keys, koff, klen, pick)
        if absent:
            q[q_off + q_len - 1] = ord("~")
        idx = torch.empty(pick.numel(), dtype=torch.int32, device=dev)

        def run():
            gibson_amd.key_index_lookup(table, keys, koff, klen, enc, q, q_off, q_len, idx, lres)

        run()
        torch.cuda.synchronize()
        hits, misses, examined = lres.cpu().tolist()
        if absent:
            ok = hits == 0 and bool((idx == -1).all())
        else:
            # a chance duplicate maps to the higher item: compare through the table's own answer
            ok = misses == 0 and bool(((idx.to(torch.int64) == pick) | (enc[pick] == gibson_amd.ENC_NULL)).all())
        q_bytes = int(q_len.sum().item())
        nbytes = q_bytes + 12 * pick.numel() + 8 * examined + (0 if absent else q_bytes + 13 * pick.numel())
        r = leg_pair({"warm": run, "before": lambda: None, "run": run}, nbytes, dev, a)
        r.update({"queries": pick.numel(), "hits": hits, "misses": misses, "slots_examined": examined,
                  "examined_per_query": round(examined / pick.numel(), 3), "idx_ok": ok,
                  "ns_per_query": round(r["legs"]["call"]["median_ms"] * 1e6 / pick.numel(), 3)})
        return r, examined

    k = min(max(a.k // a.scale, 1), n)
    pick_k = torch.randint(0, n, (k,), device=dev, generator=gen)
    pick_all = torch.randint(0, n, (n,), device=dev, generator=gen)
    out["lookup_k"], _ = lookup_leg(pick_k, False)
    out["lookup_all"], _ = lookup_leg(pick_all, False)
    out["lookup_absent"], _ = lookup_leg(pick_all, True)
    _, chain = lookup_leg(torch.arange(n, device=dev), False)          # every item's own chain, once
    nbytes = 2 * (key_bytes + 13 * n) + 2 * 8 * chain
    r = leg_pair({"warm": clear_insert, "before": clear, "run": insert}, nbytes, dev, a)
    r["ns_per_item"] = round(r["legs"]["call"]["median_ms"] * 1e6 / n, 3)
    out["insert"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    a = ap.parse_args()
    a.repeats = max(a.repeats, 5)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    count = max(a.items // a.scale, 64)
    slots = 16
    while slots < count:
        slots *= 2
    keys, koff, klen = make_keys(count, dev, gen)
    res = {"repeats": a.repeats, "warmup": a.warmup, "seed": a.seed, "scale": a.scale,
           "library": os.environ.get("LZF_HIP_LIB") or "in-tree", "device": torch.cuda.get_device_name(0),
           "key_bytes": int(klen.sum().item()),
           "tables": [bench_table(a, dev, gen, keys, koff, klen, min(count, slots), 2 * slots),
                      bench_table(a, dev, gen, keys, koff, klen, min(count, slots - slots // 4), slots)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
