#!/usr/bin/env python3
"""What the index-list MGET and the prefix select of the device store cost
against what a caller had before them.

usage: mget_bench.py [--items N] [--k K] [--select 1048576,16777216] [--repeats R] [--warmup W] [--scale S]
                     [--seed N] [--legs mget,select]

One process.  Keys of 16-40 bytes over a small alphabet, made on the device.

mget: a store of N (1 M) device-generated 4 KiB json values
(lzf_gpu_synth_fill) stored by lzf_gpu_set_store at compression 64, and a
seeded random list of K (100 000) distinct items.  HIP events around every
call, warm-ups and R timed repeats (at least 5) that alternate
  (a) mget      lzf_gpu_store_mget over the list, with the time arrays (no
                item expires) and last_access;
  (b) baseline  what a caller does without it: five index_select gathers of
                the descriptors (key_off, key_len, val_off, val_size, val_len;
                enc of the subset is gathered once, outside the timed region)
                and lzf_gpu_kv_frame with the element count known on the host.
The margin is the baseline's spread, (max - min) / median: (a) passes when its
median is no more than that above the baseline's.  The two frames are compared
byte for byte first.

select: per count of keys, lzf_gpu_store_select_prefix of a 3-byte prefix
against a device-to-device copy of what it reads: the key bytes and the three
descriptor arrays (key_off, key_len, enc).  The selected list is checked
against torch first.

Prints one JSON object.  --scale divides every count (rehearsals)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gibson_amd  # noqa: E402
from mixed_bench import make_batch, stats, timed  # noqa: E402

ALPHABET = b"abcdefgh:_01"
NOW = 1_700_000_000


def make_keys(count, dev, gen):
    """(keys, key_off, key_len) on the device: 16-40 bytes each, dense"""
    klen = torch.randint(16, 41, (count,), device=dev, generator=gen, dtype=torch.int64)
    koff = torch.cumsum(klen, 0) - klen
    total = int(klen.sum().item())
    table = torch.tensor(list(ALPHABET), dtype=torch.uint8, device=dev)
    keys = table[torch.randint(0, len(ALPHABET), (total + 16,), device=dev, generator=gen)]
    return keys, koff, klen.to(torch.int32)


def spread(leg):
    return (leg["max_ms"] - leg["min_ms"]) / leg["median_ms"]


def bench_mget(a, dev, gen):
    b = make_batch([(a.items, 4096, 4096)], (1,), a.scale, dev)
    lens = b["np_len"].astype(np.int64)
    count, in_bytes = len(lens), int(lens.sum())
    k = min(max(a.k // a.scale, 1), count)
    store = torch.empty(in_bytes + 8 * count + 16, dtype=torch.uint8, device=dev)
    used = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    val_off = torch.zeros(count, dtype=torch.int64, device=dev)
    val_size = torch.zeros(count, dtype=torch.int32, device=dev)
    enc = torch.zeros(count, dtype=torch.uint8, device=dev)
    work = gibson_amd.set_store(b["src"], b["off"], b["len"], 64, b["max"], in_bytes, store, used, val_off, val_size,
                                enc, status)
    torch.cuda.synchronize()
    del work
    val_len = b["len"]
    stored_lzf = int((enc == gibson_amd.ENC_LZF).sum().item())
    keys, koff, klen = make_keys(count, dev, gen)
    item_time = torch.full((count,), NOW - 5, dtype=torch.int64, device=dev)
    item_ttl = torch.zeros(count, dtype=torch.int32, device=dev)
    last = torch.zeros(count, dtype=torch.int64, device=dev)
    rs = np.random.RandomState(a.seed)
    idx_np = rs.choice(count, k, replace=False)
    idx32 = torch.from_numpy(idx_np.astype(np.uint32).view(np.int32)).to(dev)
    idx64 = torch.from_numpy(idx_np.astype(np.int64)).to(dev)
    max_response = int(lens[idx_np].sum()) + k * (9 + 40) + 4
    frames = [torch.zeros(max_response + 7, dtype=torch.uint8, device=dev) for _ in range(2)]
    flen = torch.zeros(2, dtype=torch.int64, device=dev)
    result = torch.zeros(4, dtype=torch.int64, device=dev)
    mwork = gibson_amd.store_mget_work(k, dev)
    fwork = torch.empty(int(gibson_amd.lib().lzf_gpu_kv_frame_work_size(k)), dtype=torch.uint8, device=dev)
    g_enc = enc.index_select(0, idx64)

    def mget():
        gibson_amd.store_mget(idx32, keys, koff, klen, store, val_off, val_size, enc, val_len, item_time, item_ttl,
                              NOW, b["max"], frames[0], max_response, flen[0:1], result, last_access=last, work=mwork)

    def baseline():
        g = [t.index_select(0, idx64) for t in (koff, klen, val_off, val_size, val_len)]
        gibson_amd.kv_frame(keys, g[0], g[1], store, g[2], g[3], g_enc, g[4], k, b["max"], frames[1], max_response,
                            flen[1:2], work=fwork)

    for _ in range(a.warmup):
        mget()
        baseline()
    torch.cuda.synchronize()
    n0, n1 = int(flen[0].item()), int(flen[1].item())
    same = n0 == n1 > 0 and bool(torch.equal(frames[0][:n0], frames[1][:n1]))
    ts = {"mget": [], "baseline": []}
    for _ in range(a.repeats):                        # alternating
        ts["mget"].append(timed(mget))
        ts["baseline"].append(timed(baseline))
    legs = {name: stats(v) for name, v in ts.items()}
    margin = spread(legs["baseline"])
    return {"items": count, "input_bytes": in_bytes, "store_status": int(status.item()), "store_bytes": int(used.item()),
            "stored_lzf": stored_lzf, "k": k, "frame_bytes": n0, "result": result.cpu().numpy().tolist(),
            "frames_equal": same, "legs": legs, "baseline_spread": round(margin, 4),
            "mget_over_baseline": round(legs["mget"]["median_ms"] / legs["baseline"]["median_ms"], 3),
            "mget_within_margin": legs["mget"]["median_ms"] <= legs["baseline"]["median_ms"] * (1 + margin)}


def bench_select(a, dev, gen, count):
    count = max(count // a.scale, 64)
    keys, koff, klen = make_keys(count, dev, gen)
    enc = torch.zeros(count, dtype=torch.uint8, device=dev)
    prefix = torch.tensor(list(b"ab:"), dtype=torch.uint8, device=dev)
    sel = torch.empty(count, dtype=torch.int32, device=dev)
    res = torch.zeros(2, dtype=torch.int32, device=dev)
    work = gibson_amd.store_select_work(count, dev)
    copies = [torch.empty_like(t) for t in (keys, koff, klen, enc)]

    def select():
        gibson_amd.store_select_prefix(keys, koff, klen, enc, prefix, sel, res, work=work)

    def copy():
        for d, s in zip(copies, (keys, koff, klen, enc)):
            d.copy_(s)

    for _ in range(a.warmup):
        select()
        copy()
    torch.cuda.synchronize()
    hit = (keys[koff] == prefix[0]) & (keys[koff + 1] == prefix[1]) & (keys[koff + 2] == prefix[2])
    exp = torch.nonzero(hit).flatten().to(torch.int32)
    matches = int(res[1].item())
    ok = matches == exp.numel() == int(res[0].item()) and bool(torch.equal(sel[:matches], exp)) and \
        bool((sel[matches:] == -1).all())
    del hit, exp
    ts = {"select": [], "copy": []}
    for _ in range(a.repeats):                        # alternating
        ts["select"].append(timed(select))
        ts["copy"].append(timed(copy))
    legs = {name: stats(v) for name, v in ts.items()}
    read = int(keys.numel()) + count * (8 + 4 + 1)
    return {"keys": count, "key_bytes": int(keys.numel()), "bytes_read": read, "matches": matches, "select_ok": ok,
            "legs": legs, "copy_gb_per_s": round(2 * read / legs["copy"]["median_ms"] / 1e6, 1),
            "select_read_gb_per_s": round(read / legs["select"]["median_ms"] / 1e6, 1),
            "select_over_copy": round(legs["select"]["median_ms"] / legs["copy"]["median_ms"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=100000)
    ap.add_argument("--select", default="1048576,16777216")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--legs", default="mget,select")
    a = ap.parse_args()
    a.repeats = max(a.repeats, 5)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    res = {"repeats": a.repeats, "warmup": a.warmup, "seed": a.seed, "scale": a.scale,
           "library": os.environ.get("LZF_HIP_LIB") or "in-tree", "device": torch.cuda.get_device_name(0)}
    legs = a.legs.split(",")
    if "mget" in legs:
        res["mget"] = bench_mget(a, dev, gen)
    if "select" in legs:
        res["select"] = [bench_select(a, dev, gen, int(c)) for c in a.select.split(",")]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
