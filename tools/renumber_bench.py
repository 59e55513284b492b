#!/usr/bin/env python3
"""What renumbering the device store costs against a plain copy of the bytes
it moves, and what it buys the sweeps that come after.

usage: renumber_bench.py [--dead 0.1,0.5,0.9] [--repeats R] [--warmup W] [--scale S] [--seed N]
                         [--once FRACTION]

One process, one store built on the host: 4 M items (divided by --scale) with
seeded random keys of 16-40 bytes under the prefix "k:", all ten item arrays.
Per dead fraction a seeded random subset of the items is deleted
(lzf_gpu_store_delete); then, HIP events around every call, warm-ups and R
timed repeats (at least 7) that alternate
  (a) renumber  lzf_gpu_store_renumber into a second set of arrays and a
                second key arena (*dst_keys_used is zeroed before every call,
                outside the timed region);
  (b) copy      one device-to-device copy of exactly the bytes (a) must move:
                57 bytes of members per live item and the live key bytes;
  (c) rebuild   lzf_gpu_key_index_rebuild over the new arrays, count = dst_cap;
  (d) insert    hipMemset of the table and *used, then
                lzf_gpu_key_index_insert(0, dst_cap) over the same arrays;
  (e) / (f)     lzf_gpu_store_select_prefix of a prefix that matches nothing,
                over the old arrays (count items) and over the new ones (live
                items);
  (g) / (h)     lzf_gpu_store_expire with no TTL set, before and after.
Prints one JSON object: per dead fraction the report, per leg median, min, max
and every repeat, and the figures (a) / (b), (c) / (d), (e) / (f), (g) / (h).

--once FRACTION runs the renumbering of that dead fraction three times and
nothing else: the form to put under a kernel trace, whose per-kernel times
give the key pack's share."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gibson_amd  # noqa: E402
from mixed_bench import stats, timed  # noqa: E402

MEMBER_BYTES = 8 + 4 + 1 + 4 + 8 + 4 + 8 + 4 + 8 + 8    # the ten members of one item


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dead", default="0.1,0.5,0.9")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--once", type=float, default=None)
    a = ap.parse_args()
    a.repeats = max(a.repeats, 7)
    fractions = [a.once] if a.once is not None else [float(x) for x in a.dead.split(",")]
    dev = torch.device("cuda", 0)
    count = (4 << 20) // a.scale
    rs = np.random.RandomState(a.seed)
    klen = rs.randint(16, 41, count).astype(np.int64)
    koff = np.cumsum(klen) - klen
    kbytes = int(klen.sum())
    arena = rs.randint(0, 256, kbytes + 16).astype(np.uint8)
    arena[koff] = ord("k")
    arena[koff + 1] = ord(":")

    def up(x, dt):
        return torch.from_numpy(np.ascontiguousarray(x, dt)).to(dev)

    keys = up(arena, np.uint8)
    src = {"val_off": up(np.arange(count) * 64, np.int64), "val_size": up(np.full(count, 64), np.int32),
           "enc": torch.zeros(count, dtype=torch.uint8, device=dev), "val_len": up(np.full(count, 64), np.int32),
           "key_off": up(koff, np.int64), "key_len": up(klen, np.int32),
           "item_time": torch.zeros(count, dtype=torch.int64, device=dev),
           "item_ttl": torch.zeros(count, dtype=torch.int32, device=dev),
           "item_lock": torch.zeros(count, dtype=torch.int64, device=dev),
           "last_access": torch.zeros(count, dtype=torch.int64, device=dev)}
    dst = {n: torch.empty_like(t) for n, t in src.items()}
    dst_keys = torch.empty(kbytes + 16, dtype=torch.uint8, device=dev)
    dst_used = torch.zeros(1, dtype=torch.int64, device=dev)
    remap = torch.empty(count, dtype=torch.int32, device=dev)
    report = torch.zeros(4, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    work = gibson_amd.store_renumber_work(count, dev)
    slots = 16
    while slots - slots // 4 < count:
        slots *= 2
    table = torch.empty(gibson_amd.key_index_bytes(slots), dtype=torch.uint8, device=dev)
    kused = torch.zeros(1, dtype=torch.int32, device=dev)
    kres = torch.zeros(4, dtype=torch.int64, device=dev)
    kst = torch.zeros(1, dtype=torch.int32, device=dev)
    prefix = up(np.frombuffer(b"k:\xff\xff\xff\xff\xff\xff", np.uint8), np.uint8)
    sel = torch.empty(1024, dtype=torch.int32, device=dev)
    sres = torch.zeros(2, dtype=torch.int32, device=dev)
    swork = gibson_amd.store_select_work(count, dev)
    expired = torch.zeros(1, dtype=torch.int32, device=dev)
    bounce = torch.empty(count * MEMBER_BYTES + kbytes, dtype=torch.uint8, device=dev)
    bounce2 = torch.empty_like(bounce)
    res = {"items": count, "key_bytes": kbytes, "repeats": a.repeats, "warmup": a.warmup, "seed": a.seed,
           "slots": slots, "library": os.environ.get("LZF_HIP_LIB") or "in-tree",
           "device": torch.cuda.get_device_name(0), "dead": []}
    for f in fractions:
        idx = rs.choice(count, int(round(f * count)), replace=False).astype(np.uint32)
        src["enc"].zero_()
        gibson_amd.store_delete(torch.from_numpy(idx.view(np.int32)).to(dev), src["enc"])
        items = gibson_amd.StoreItems(**src)

        def renumber():
            gibson_amd.store_renumber(items, keys, dst, dst_keys, dst_used, report, status, remap=remap, work=work)

        if a.once is not None:
            for _ in range(3):
                dst_used.zero_()
                renumber()
            torch.cuda.synchronize()
            print(json.dumps({"once": f, "status": int(status.item()), "report": report.cpu().numpy().tolist()}))
            return
        dst_used.zero_()
        renumber()
        torch.cuda.synchronize()
        live, live_keys, dead, dead_keys = (int(x) for x in report.cpu().numpy())
        ok = int(status.item()) == 0 and int(dst_used.item()) == live_keys
        moved = live * MEMBER_BYTES + live_keys
        new = {n: t[:live] for n, t in dst.items()}

        def copy():
            bounce2[:moved].copy_(bounce[:moved])

        def rebuild():
            gibson_amd.key_index_rebuild(table, kused, dst_keys, dst["key_off"], dst["key_len"], dst["enc"], kres, kst)

        def insert():
            table.fill_(0xFF)
            kused.zero_()
            gibson_amd.key_index_insert(table, kused, dst_keys, dst["key_off"], dst["key_len"], dst["enc"], 0, count,
                                        kres, kst)

        def select(k, o, ln, e):
            return lambda: gibson_amd.store_select_prefix(k, o, ln, e, prefix, sel, sres, swork)

        def expire(t, ttl, e):
            return lambda: gibson_amd.store_expire(t, ttl, 1 << 30, e, expired)

        legs = {"renumber": renumber, "copy": copy, "rebuild": rebuild, "insert": insert,
                "select_before": select(keys, src["key_off"], src["key_len"], src["enc"]),
                "select_after": select(dst_keys, new["key_off"], new["key_len"], new["enc"]),
                "expire_before": expire(src["item_time"], src["item_ttl"], src["enc"]),
                "expire_after": expire(new["item_time"], new["item_ttl"], new["enc"])}
        for _ in range(a.warmup):
            for name, fn in legs.items():
                dst_used.zero_()
                fn()
        torch.cuda.synchronize()
        ok = ok and int(status.item()) == 0 and int(kst.item()) == 0
        ts = {name: [] for name in legs}
        for _ in range(a.repeats):                    # alternating
            for name, fn in legs.items():
                dst_used.zero_()
                ts[name].append(timed(fn))
        st = {k: stats(v) for k, v in ts.items()}
        ratio = lambda x, y: round(st[x]["median_ms"] / st[y]["median_ms"], 3)
        res["dead"].append({"fraction": f, "live_items": live, "live_key_bytes": live_keys, "dead_items": dead,
                            "dead_key_bytes": dead_keys, "moved_bytes": moved, "ok": ok, "legs": st,
                            "copy_gb_per_s": round(2 * moved / st["copy"]["median_ms"] / 1e6, 1),
                            "renumber_over_copy": ratio("renumber", "copy"),
                            "rebuild_over_insert": ratio("rebuild", "insert"),
                            "select_before_over_after": ratio("select_before", "select_after"),
                            "expire_before_over_after": ratio("expire_before", "expire_after")})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
