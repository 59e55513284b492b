#!/usr/bin/env python3
"""What compacting the device store costs against a plain copy of the bytes
it keeps.

usage: compact_bench.py [--dead 0.1,0.5,0.9] [--repeats R] [--warmup W] [--scale S] [--seed N]

One process, one device-generated batch (lzf_gpu_synth_fill): 256 K x 4 KiB
json stored by lzf_gpu_set_store at compression 0 (the json4k store of
tools/store_bench.py).  Per dead fraction a seeded random subset of the items
is deleted (lzf_gpu_store_delete); then, HIP events around every call,
warm-ups and R timed repeats (at least 5) that alternate
  (a) compact  lzf_gpu_store_compact of the live items into a second arena
               (the arrays are put back to the store's before every call,
               outside the timed region);
  (b) copy     a device-to-device copy of exactly the live byte count.
Prints one JSON object: per dead fraction the usage report, per leg median,
min, max and every repeat, and the figure (a) / (b).

--scale divides the count (rehearsals).  LZF_GPU_STORE_TILE_KB /
LZF_GPU_STORE_PACK=realign pick the pack kernel's tile and load form
(lzf_store.hip), as for set_store."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gibson_amd  # noqa: E402
from mixed_bench import UNIFORM4K, make_batch, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dead", default="0.1,0.5,0.9")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    a = ap.parse_args()
    a.repeats = max(a.repeats, 5)
    fractions = [float(x) for x in a.dead.split(",")]
    dev = torch.device("cuda", 0)
    b = make_batch(UNIFORM4K, (1,), a.scale, dev)
    lens = b["np_len"].astype(np.int64)
    count, in_bytes = len(lens), int(lens.sum())

    store = torch.empty(in_bytes + 8 * count + 16, dtype=torch.uint8, device=dev)
    used = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    val_off = torch.zeros(count, dtype=torch.int64, device=dev)
    val_size = torch.zeros(count, dtype=torch.int32, device=dev)
    enc = torch.zeros(count, dtype=torch.uint8, device=dev)
    work = gibson_amd.set_store(b["src"], b["off"], b["len"], 0, b["max"], in_bytes, store, used, val_off, val_size,
                                enc, status)
    torch.cuda.synchronize()
    del work
    packed = int(used.item())
    res = {"workload": "json4k", "values": count, "input_bytes": in_bytes, "store_status": int(status.item()),
           "store_bytes": packed, "repeats": a.repeats, "warmup": a.warmup, "seed": a.seed,
           "library": os.environ.get("LZF_HIP_LIB") or "in-tree", "device": torch.cuda.get_device_name(0),
           "pack_tile_kb": int(os.environ.get("LZF_GPU_STORE_TILE_KB") or 64),
           "pack_loads": os.environ.get("LZF_GPU_STORE_PACK") or "unaligned", "dead": []}
    src = store[:packed]                              # the arena as far as it is used
    dst = torch.empty(packed + 16, dtype=torch.uint8, device=dev)
    cwork = gibson_amd.store_compact_work(count, dev)
    report = torch.zeros(4, dtype=torch.int64, device=dev)
    c_off, c_size = torch.empty_like(val_off), torch.empty_like(val_size)
    c_used = torch.zeros(1, dtype=torch.int64, device=dev)
    c_status = torch.zeros(1, dtype=torch.int32, device=dev)
    rs = np.random.RandomState(a.seed)
    for f in fractions:
        idx = rs.choice(count, int(round(f * count)), replace=False).astype(np.uint32)
        c_enc = enc.clone()
        gibson_amd.store_delete(torch.from_numpy(idx.view(np.int32)).to(dev), c_enc)
        gibson_amd.store_usage(val_size, c_enc, report, cwork)
        torch.cuda.synchronize()
        live_items, live, dead_items, dead_bytes = (int(x) for x in report.cpu().numpy())

        def reset():
            c_off.copy_(val_off)
            c_size.copy_(val_size)
            c_used.zero_()

        def compact():
            gibson_amd.store_compact(src, c_off, c_size, c_enc, dst, c_used, report, c_status, cwork)

        def copy():
            dst[:live].copy_(src[:live])

        for _ in range(a.warmup):
            reset()
            compact()
            copy()
        torch.cuda.synchronize()
        ok = int(c_status.item()) == 0 and int(c_used.item()) == live
        ts = {"compact": [], "copy": []}
        for _ in range(a.repeats):                    # alternating
            reset()
            ts["compact"].append(timed(compact))
            ts["copy"].append(timed(copy))
        legs = {k: stats(v) for k, v in ts.items()}
        res["dead"].append({"fraction": f, "live_items": live_items, "live_bytes": live, "dead_items": dead_items,
                            "dead_bytes": dead_bytes, "compact_ok": ok, "legs": legs,
                            "copy_gb_per_s": round(2 * live / legs["copy"]["median_ms"] / 1e6, 1),
                            "compact_over_copy": round(legs["compact"]["median_ms"] / legs["copy"]["median_ms"], 3)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
