#!/usr/bin/env python3
"""What the device SET path costs on top of the compress batch it contains.

usage: store_bench.py [--workload json4k|mixedsize] [--repeats R] [--warmup W]
                      [--legs store,compress,copy] [--scale S]

One process, one device-generated batch (lzf_gpu_synth_fill), HIP events
around every call, warm-ups, then R timed repeats (at least 5) that alternate
  (a) store     lzf_gpu_set_store into an empty store arena;
  (b) compress  lzf_gpu_compress_batch alone on the lengths, caps and dense
                slots set_store hands its compress step (0 for a value at or
                below the threshold): unchanged code, the yardstick;
  (c) copy      a device-to-device copy of exactly the packed byte count.
Prints one JSON object: per leg median, min, max and every repeat, and the
figure of merit (a - b) / c: the decision and the packing in units of a plain
copy of the same bytes.

Workloads
  json4k     256 K x 4 KiB json (the values of BASELINE configs[1]),
             compression 0: every value is a candidate.
  mixedsize  the batch of tools/mixed_bench.py, compression 4096: the 160 K
             values of at most 4 KiB are stored plain without a compress.

--legs compress runs (b) only: with LZF_HIP_LIB naming a build of an earlier
commit, that is the figure to hold this commit's (b) against.  --scale divides
the counts (rehearsals).  LZF_GPU_STORE_TILE_KB / LZF_GPU_STORE_PACK=realign
pick the pack kernel's tile and load form (lzf_store.hip)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gibson_amd  # noqa: E402
from mixed_bench import MIXEDSIZE, UNIFORM4K, make_batch, stats, timed  # noqa: E402


def needcompr(n):
    """gb_needcompr (gibson_amd/csrc/gb_policy.h) over an int64 array"""
    return np.minimum((n - 4) & 0xFFFFFFFF, n + n // 16 + 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="json4k", choices=("json4k", "mixedsize"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="store,compress,copy")
    ap.add_argument("--scale", type=int, default=1)
    a = ap.parse_args()
    a.repeats = max(a.repeats, 5)
    legs = a.legs.split(",")
    dev = torch.device("cuda", 0)
    if a.workload == "json4k":
        b, compression = make_batch(UNIFORM4K, (1,), a.scale, dev), 0
    else:
        b, compression = make_batch(MIXEDSIZE, (2, 1, 3), a.scale, dev), 4096
    lens = b["np_len"].astype(np.int64)
    count, in_bytes = len(lens), int(lens.sum())

    # what set_store hands its compress step
    cand = lens > compression
    caps = np.where(cand, needcompr(lens), 0)
    slot_off = np.concatenate([[0], np.cumsum(caps[:-1])]).astype(np.int64)
    c_len = torch.from_numpy(np.where(cand, lens, 0).astype(np.int32)).to(dev)
    c_cap = torch.from_numpy(caps.astype(np.uint32).view(np.int32)).to(dev)
    c_off = torch.from_numpy(slot_off).to(dev)
    c_out = torch.empty(int(caps.sum()) + 16, dtype=torch.uint8, device=dev)
    c_olen = torch.zeros(count, dtype=torch.int32, device=dev)

    store = torch.empty(in_bytes + 8 * count + 16, dtype=torch.uint8, device=dev)
    used = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    val_off = torch.zeros(count, dtype=torch.int64, device=dev)
    val_size = torch.zeros(count, dtype=torch.int32, device=dev)
    enc = torch.zeros(count, dtype=torch.uint8, device=dev)
    work = gibson_amd.set_store_work(count, in_bytes, dev) if "store" in legs else None
    packed = [0]

    def run(leg):
        if leg == "store":
            used.zero_()
            gibson_amd.set_store(b["src"], b["off"], b["len"], compression, b["max"], in_bytes, store, used, val_off,
                                 val_size, enc, status, work)
        elif leg == "compress":
            gibson_amd.compress_batch(b["src"], b["off"], c_len, c_out, c_off, c_cap, c_olen, b["max"])
        else:
            b["dec"][:packed[0]].copy_(store[:packed[0]])

    res = {"workload": a.workload, "values": count, "input_bytes": in_bytes, "max_len": b["max"],
           "compression": compression, "repeats": a.repeats, "warmup": a.warmup,
           "library": os.environ.get("LZF_HIP_LIB") or "in-tree", "device": torch.cuda.get_device_name(0),
           "pack_tile_kb": int(os.environ.get("LZF_GPU_STORE_TILE_KB") or 64),
           "pack_loads": os.environ.get("LZF_GPU_STORE_PACK") or "unaligned", "legs": {}}
    if "store" in legs:
        run("store")
        torch.cuda.synchronize()
        packed[0] = int(used.item())
        e = enc.cpu().numpy()
        res.update({"status": int(status.item()), "packed_bytes": packed[0], "stored_lzf": int((e == 1).sum()),
                    "stored_plain": int((e == 0).sum())})
        # the same decisions as the compress batch alone makes
        run("compress")
        torch.cuda.synchronize()
        ol = c_olen.cpu().numpy().view(np.uint32).astype(np.int64)
        res["sizes_equal_compress_batch"] = bool(np.array_equal(val_size.cpu().numpy().view(np.uint32).astype(np.int64),
                                                                np.where(ol > 0, ol, lens)))
    else:
        packed[0] = in_bytes // 2                     # no store leg: the copy moves half the input bytes
    for _ in range(a.warmup):
        for leg in legs:
            run(leg)
    torch.cuda.synchronize()
    ts = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg in legs:                              # alternating
            ts[leg].append(timed(lambda: run(leg)))
    for leg in legs:
        res["legs"][leg] = stats(ts[leg])
    if all(leg in legs for leg in ("store", "compress", "copy")):
        s, c, d = (res["legs"][leg]["median_ms"] for leg in ("store", "compress", "copy"))
        res["store_minus_compress_ms"] = round(s - c, 3)
        res["copy_gb_per_s"] = round(2 * packed[0] / d / 1e6, 1)        # read + write
        res["decision_and_pack_over_copy"] = round((s - c) / d, 3)
    res["kernel_info"] = gibson_amd.kernel_info()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
