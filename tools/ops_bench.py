#!/usr/bin/env python3
"""What INC / DEC and the lock-aware DEL cost over the device store, against
the nearest operators the store had before them.

usage: ops_bench.py [--items N] [--n K] [--repeats R] [--warmup W] [--scale S] [--seed N]

One process.  A store of N (4 M = 2^22) items of 8 stored bytes each, packed
densely from byte 3 of the arena (so no value is 8-aligned), with item_time,
item_ttl and item_lock arrays under which nothing expires and nothing is
locked, and a list of K (1 M = 2^20) distinct random entries.  HIP events
around every call, warm-ups and R timed repeats (at least 5), the legs of a
pair alternating:
  minc_number   every item a NUMBER: one lzf_gpu_store_minc (delta 1) over the
                list, against one lzf_gpu_store_count over the same list;
  minc_convert  every item 8 ASCII digits, PLAIN: one lzf_gpu_store_minc that
                converts every entry (8 bytes parsed, a fresh 8-byte slot
                each), against the same count.  The store is put back before
                each repeat, outside the timed region;
  mdel          one lzf_gpu_store_mdel over the list, against
                lzf_gpu_store_count followed by lzf_gpu_store_delete.  enc is
                put back before each repeat, outside the timed region.
Each leg's result words are checked once.  Nothing here is a threshold.

Prints one JSON object.  --scale divides every count (rehearsals)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import gibson_amd  # noqa: E402
from mixed_bench import stats, timed  # noqa: E402

NOW = 1_700_000_000
BASE = 3


def pair(a, legs, before):
    """alternating repeats of the calls in ``legs`` ({name: fn}); ``before``
    runs ahead of each timed call, outside the timed region"""
    for _ in range(a.warmup):
        for fn in legs.values():
            before()
            fn()
    ts = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, fn in legs.items():
            before()
            ts[k].append(timed(fn))
    return {k: stats(v) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 22)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    a = ap.parse_args()
    a.repeats = max(a.repeats, 5)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    count = max(a.items // a.scale, 64)
    n = min(max(a.n // a.scale, 16), count)
    used0 = BASE + 8 * count
    cap = used0 + 8 * n
    arena = torch.randint(ord("1"), ord("9") + 1, (cap + 16,), dtype=torch.uint8, device=dev, generator=gen)
    off0 = BASE + 8 * torch.arange(count, dtype=torch.int64, device=dev)
    off = off0.clone()
    size = torch.full((count,), 8, dtype=torch.int32, device=dev)
    enc = torch.empty(count, dtype=torch.uint8, device=dev)
    used = torch.empty(1, dtype=torch.int64, device=dev)
    time = torch.full((count,), NOW - 10, dtype=torch.int64, device=dev)
    ttl = torch.zeros(count, dtype=torch.int32, device=dev)
    lock = torch.zeros(count, dtype=torch.int64, device=dev)
    last = torch.zeros(count, dtype=torch.int64, device=dev)
    idx = torch.randperm(count, device=dev, generator=gen)[:n].to(torch.int32)
    res6 = torch.zeros(6, dtype=torch.int64, device=dev)
    res3 = torch.zeros(3, dtype=torch.int64, device=dev)
    res2 = torch.zeros(2, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    work = gibson_amd.store_minc_work(n, dev)

    arena0 = arena[:used0].clone()

    def reset(e):
        def f():
            arena[:used0].copy_(arena0)
            enc.fill_(e)
            off.copy_(off0)
            used.fill_(used0)
        return f

    def minc():
        gibson_amd.store_minc(idx, 1, arena[:cap], used, off, size, enc, time, ttl, lock, NOW, res6, status,
                              last_access=last, work=work)

    def count_():
        gibson_amd.store_count(idx, enc, time, ttl, NOW, res2, last_access=last)

    def mdel():
        gibson_amd.store_mdel(idx, enc, time, ttl, lock, NOW, res3)

    def count_delete():
        gibson_amd.store_count(idx, enc, time, ttl, NOW, res2, last_access=last)
        gibson_amd.store_delete(idx, enc)

    out = {"items": count, "entries": n, "repeats": a.repeats, "warmup": a.warmup, "seed": a.seed, "scale": a.scale,
           "library": os.environ.get("LZF_HIP_LIB") or "in-tree", "device": torch.cuda.get_device_name(0)}

    def leg(name, legs, before, check, base):
        before()
        check()
        r = {"legs": pair(a, legs, before)}
        first = next(iter(legs))
        r["ns_per_entry"] = round(r["legs"][first]["median_ms"] * 1e6 / n, 3)
        r[first + "_over_" + base] = round(r["legs"][first]["median_ms"] / r["legs"][base]["median_ms"], 3)
        out[name] = r

    def check_number():
        minc()
        torch.cuda.synchronize()
        assert res6.cpu().tolist() == [n, 0, 0, 0, 0, 0] and int(status.item()) == 0, res6.cpu().tolist()

    def check_convert():
        minc()
        torch.cuda.synchronize()
        assert res6.cpu().tolist() == [n, 0, 0, 0, n, 0] and int(used.item()) == cap, res6.cpu().tolist()

    def check_mdel():
        mdel()
        torch.cuda.synchronize()
        assert res3.cpu().tolist() == [n, 0, 0], res3.cpu().tolist()
        left = int((enc != gibson_amd.ENC_NULL).sum().item())
        reset(gibson_amd.ENC_NUMBER)()
        count_delete()
        torch.cuda.synchronize()
        assert res2.cpu().tolist() == [n, 0] and int((enc != gibson_amd.ENC_NULL).sum().item()) == left == count - n

    leg("minc_number", {"minc": minc, "count": count_}, reset(gibson_amd.ENC_NUMBER), check_number, "count")
    leg("minc_convert", {"minc": minc, "count": count_}, reset(gibson_amd.ENC_PLAIN), check_convert, "count")
    leg("mdel", {"mdel": mdel, "count_delete": count_delete}, reset(gibson_amd.ENC_NUMBER), check_mdel,
        "count_delete")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
