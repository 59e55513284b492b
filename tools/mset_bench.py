#!/usr/bin/env python3
"""What MSET by prefix costs over the device store, against what the store
offered before it and against the floor of its copy.

usage: mset_bench.py [--repeats R] [--warmup W] [--scale S] [--compression C]

One process.  Per shape -- a 4 KiB JSON value over 256 K entries, a 64-byte
value over 1 M entries -- a store of K items in which every item is valid and
unlocked, a list of all K entries in a random order, and one value.  HIP events
around every call, warm-ups and R timed repeats (at least 5), the legs
alternating:
  mset        one lzf_gpu_store_mset over the list: one compress, K
              descriptors, K copies of the S stored bytes;
  set_store   what the store offered before: one lzf_gpu_set_store with K
              descriptors aliasing the same value, which compresses it K times
              and makes K new items (the key index's update not counted);
  copy        a plain device-to-device copy of S * K bytes, the floor for the
              replicate.
*store_used is put back before each repeat, outside the timed region.  The
mset leg's result words and every copy's bytes are checked once, against the
set_store leg's first item.  Nothing here is a threshold.

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
SHAPES = (("json4k_x256k", 1, 4096, 1 << 18), ("json64_x1m", 1, 64, 1 << 20))


def shape(a, dev, kind, vlen, k):
    gen = torch.Generator(device=dev)
    gen.manual_seed(0xC0FFEE)
    value = torch.empty(vlen, dtype=torch.uint8, device=dev)
    gibson_amd.synth_fill(kind, 0x5EED0002, 0, 1, 1, vlen, value)
    cap = BASE + vlen * k + 64
    arena = torch.zeros(cap, dtype=torch.uint8, device=dev)
    used = torch.empty(1, dtype=torch.int64, device=dev)
    off = torch.zeros(k, dtype=torch.int64, device=dev)
    size = torch.zeros(k, dtype=torch.int32, device=dev)
    vl = torch.zeros(k, dtype=torch.int32, device=dev)
    enc = torch.zeros(k, dtype=torch.uint8, device=dev)
    time = torch.full((k,), NOW - 10, dtype=torch.int64, device=dev)
    ttl = torch.zeros(k, dtype=torch.int32, device=dev)
    lock = torch.zeros(k, dtype=torch.int64, device=dev)
    last = torch.zeros(k, dtype=torch.int64, device=dev)
    idx = torch.randperm(k, device=dev, generator=gen).to(torch.int32)
    res5 = torch.zeros(5, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    work = gibson_amd.store_mset_work(k, vlen, dev)
    # the set_store leg: K new items whose descriptors all name the one value
    s_off = torch.zeros(k, dtype=torch.int64, device=dev)
    s_len = torch.full((k,), vlen, dtype=torch.int32, device=dev)
    n_off = torch.zeros(k, dtype=torch.int64, device=dev)
    n_size = torch.zeros(k, dtype=torch.int32, device=dev)
    n_enc = torch.zeros(k, dtype=torch.uint8, device=dev)
    s_work = gibson_amd.set_store_work(k, vlen * k, dev)

    def reset():
        used.fill_(BASE)

    def mset():
        gibson_amd.store_mset(idx, value, a.compression, arena, used, off, size, enc, vl, time, ttl, lock, NOW, res5,
                              status, last_access=last, work=work)

    def set_store():
        gibson_amd.set_store(value, s_off, s_len, a.compression, vlen, vlen * k, arena, used, n_off, n_size, n_enc,
                             status, work=s_work)

    # once, checked: the set_store leg's first item is the stored form, and every copy of the mset leg equals it
    reset()
    set_store()
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    s_bytes, s_enc = int(n_size[0].item()), int(n_enc[0].item())
    first = arena[BASE:BASE + s_bytes].clone()
    arena.zero_()
    reset()
    mset()
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and res5.cpu().tolist() == [k, 0, 0, s_bytes, s_enc], res5.cpu().tolist()
    assert int(used.item()) == BASE + s_bytes * k
    assert bool((arena[BASE:BASE + s_bytes * k].view(k, s_bytes) == first).all())
    assert bool((off[idx.long()] == BASE + s_bytes * torch.arange(k, device=dev)).all())

    src = arena[BASE:BASE + s_bytes * k].clone()
    dst = torch.empty_like(src)

    def copy():
        dst.copy_(src)

    legs = {"mset": mset, "set_store": set_store, "copy": copy}
    for _ in range(a.warmup):
        for fn in legs.values():
            reset()
            fn()
    ts = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, fn in legs.items():
            reset()
            ts[name].append(timed(fn))
    r = {"value_bytes": vlen, "entries": k, "stored_bytes": s_bytes, "stored_encoding": s_enc,
         "replicated_bytes": s_bytes * k, "legs": {name: stats(v) for name, v in ts.items()}}
    m = r["legs"]["mset"]["median_ms"]
    r["ns_per_entry"] = round(m * 1e6 / k, 3)
    r["set_store_over_mset"] = round(r["legs"]["set_store"]["median_ms"] / m, 3)
    r["mset_over_copy"] = round(m / r["legs"]["copy"]["median_ms"], 3)
    r["mset_write_gb_per_s"] = round(s_bytes * k / (m * 1e6), 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--compression", type=int, default=64)
    a = ap.parse_args()
    a.repeats = max(a.repeats, 5)
    dev = torch.device("cuda", 0)
    out = {"repeats": a.repeats, "warmup": a.warmup, "scale": a.scale, "compression": a.compression,
           "library": os.environ.get("LZF_HIP_LIB") or "in-tree", "device": torch.cuda.get_device_name(0)}
    for name, kind, vlen, k in SHAPES:
        out[name] = shape(a, dev, kind, vlen, max(k // a.scale, 16))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
