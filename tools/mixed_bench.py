#!/usr/bin/env python3
"""The mixed-size calls against the uniform calls on one seeded batch.

usage: mixed_bench.py [--workload mixedsize|uniform4k] [--repeats R] [--warmup W]
                      [--legs uniform,mixed] [--scale S]

One process, one device-generated batch (lzf_gpu_synth_fill), HIP events
around every call, warm-ups, then R timed repeats (at least 5) that alternate
the uniform call (lzf_gpu_compress_batch / lzf_gpu_decompress_batch) and the
mixed call (lzf_gpu_compress_mixed / lzf_gpu_decompress_mixed) on the same
descriptors.  Prints one JSON object: per leg the compress and decompress ms
(median, min, max and every repeat), the mixed call's plan, the time of every
class run alone as a uniform batch of its class (events around each), its
scratch_chunks, and the scratch the library allocated.

Workloads
  mixedsize  160 K values of 64-4096 B, 48 K of 4-8 KiB, 64 K of 8-16 KiB,
             40 K of 16-64 KiB and 256 of 64 KiB-1 MiB (log-uniform inside a
             class; sentence text, json and mixed generators by thirds; the
             request order a seeded shuffle): every class passes its own
             crossover threshold, and the uniform call sees one batch whose
             bound is the largest value's.
  uniform4k  256 K x 4 KiB json: one class, so the mixed call's time over the
             uniform call's is its overhead (partition, the one wait, scatter).

--legs uniform runs the uniform calls only: with LZF_HIP_LIB naming a build of
an earlier commit, that is the figure to hold this commit's uniform leg against.
--scale divides every class's count (rehearsals)."""
import argparse
import json
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gibson_amd  # noqa: E402

K = 1024
SEEDS = {1: 0x5EED0002, 2: 0x5EED0003, 3: 0x5EED0005}     # json, sentence text, mixed (BASELINE seeds)
MIXEDSIZE = [(160 * K, 64, 4096), (48 * K, 4097, 8192), (64 * K, 8193, 16384), (40 * K, 16385, 65536),
             (256, 65537, 1 << 20)]
UNIFORM4K = [(256 * K, 4096, 4096)]


def make_batch(spec, kinds, scale, dev):
    """Every value gets a slot of its class's largest size, filled whole by
    the device generator; the value is the slot's first `len` bytes.  The
    stream goes to the same offsets of a second arena (out_cap = len - 4, the
    server's policy)."""
    rnd = np.random.RandomState(0x5EED07)
    slot_off, lens, fills, pos = [], [], [], 0
    for count, lo, hi in spec:
        count = max(count // scale, 3)
        ln = np.exp(rnd.uniform(np.log(lo), np.log(hi + 1), count)).astype(np.int64).clip(lo, hi)
        part = (count + len(kinds) - 1) // len(kinds)
        for j, kind in enumerate(kinds):
            n = min(part, count - j * part)
            if n > 0:
                fills.append((kind, pos + j * part * hi, n, hi))
        slot_off.append(pos + np.arange(count, dtype=np.int64) * hi)
        lens.append(ln)
        pos += count * hi
    slot_off, lens = np.concatenate(slot_off), np.concatenate(lens)
    order = rnd.permutation(len(lens))               # the request order: classes interleaved
    slot_off, lens = slot_off[order], lens[order]
    src = torch.empty(pos + 16, dtype=torch.uint8, device=dev)
    first = 0
    for kind, at, n, size in fills:
        gibson_amd.synth_fill(kind, SEEDS[kind], first, 1, n, size, src[at:])
        first += n
    torch.cuda.synchronize()
    return {"src": src, "out": torch.empty(pos + 16, dtype=torch.uint8, device=dev),
            "dec": torch.empty(pos + 16, dtype=torch.uint8, device=dev),
            "off": torch.from_numpy(slot_off).to(dev), "len": torch.from_numpy(lens.astype(np.int32)).to(dev),
            "cap": torch.from_numpy((lens - 4).clip(0).astype(np.int32)).to(dev),
            "olen": torch.zeros(len(lens), dtype=torch.int32, device=dev),
            "dlen": torch.zeros(len(lens), dtype=torch.int32, device=dev),
            "err": torch.zeros(len(lens), dtype=torch.int32, device=dev),
            "np_len": lens.astype(np.uint32), "max": int(lens.max()), "bytes": int(lens.sum()), "arena": pos}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def chunks():
    m = re.search(r"scratch_chunks=(\d+)", gibson_amd.kernel_info())
    return int(m.group(1)) if m else 0


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
            "repeats_ms": [round(t, 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="mixedsize", choices=("mixedsize", "uniform4k"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="uniform,mixed")
    ap.add_argument("--scale", type=int, default=1)
    a = ap.parse_args()
    a.repeats = max(a.repeats, 5)
    legs = a.legs.split(",")
    dev = torch.device("cuda", 0)
    b = make_batch(MIXEDSIZE if a.workload == "mixedsize" else UNIFORM4K,
                   (2, 1, 3) if a.workload == "mixedsize" else (1,), a.scale, dev)
    count = len(b["np_len"])
    work = gibson_amd.mixed_work(count, dev) if "mixed" in legs else None

    def compress(leg, sub=None, bound=None):
        off, ln, cap, olen = sub or (b["off"], b["len"], b["cap"], b["olen"])
        if leg == "mixed":
            gibson_amd.compress_mixed(b["src"], off, ln, b["out"], off, cap, olen, b["max"], work)
        else:
            gibson_amd.compress_batch(b["src"], off, ln, b["out"], off, cap, olen, bound or b["max"])
        return olen

    res = {"workload": a.workload, "values": count, "input_bytes": b["bytes"], "max_len": b["max"],
           "repeats": a.repeats, "warmup": a.warmup, "library": os.environ.get("LZF_HIP_LIB") or "in-tree",
           "device": torch.cuda.get_device_name(0), "legs": {}}

    # the scratch each leg makes the library allocate, from a released state
    for leg in legs:
        gibson_amd.release()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        compress(leg)
        torch.cuda.synchronize()
        res["legs"][leg] = {"scratch_bytes": int(free0 - torch.cuda.mem_get_info()[0]),
                            "scratch_chunks_last_launch": chunks()}
    for _ in range(a.warmup):
        for leg in legs:
            compress(leg)
    torch.cuda.synchronize()
    ct = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg in legs:                              # alternating
            ct[leg].append(timed(lambda: compress(leg)))
    ref = None
    for leg in legs:                                  # same lengths from every leg
        got = compress(leg).clone()
        torch.cuda.synchronize()
        if ref is None:
            ref = got
        res["legs"][leg]["out_len_equal_to_first_leg"] = bool(torch.equal(ref, got))
        res["legs"][leg]["compress"] = stats(ct[leg])
    if "mixed" in legs:
        res["plan_compress"] = gibson_amd.mixed_last_plan()
    ok = ref > 0
    res["compressed_values"], res["ratio"] = int(ok.sum()), round(float(ref.sum()) / b["bytes"], 4)

    # decompress: the streams just made (a value that stayed plain gets cap 0)
    d_in_len = torch.where(ok, ref, torch.ones_like(ref))
    d_cap = torch.where(ok, b["len"], torch.zeros_like(b["len"]))

    def decompress(leg, sub=None, bound=None):
        off, il, cp, dl, er = sub or (b["off"], d_in_len, d_cap, b["dlen"], b["err"])
        if leg == "mixed":
            gibson_amd.decompress_mixed(b["out"], off, il, b["dec"], off, cp, dl, er, b["max"], work)
        else:
            gibson_amd.decompress_batch(b["out"], off, il, b["dec"], off, cp, dl, er, bound or b["max"])
        return dl

    for _ in range(a.warmup):
        for leg in legs:
            decompress(leg)
    dt = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg in legs:
            dt[leg].append(timed(lambda: decompress(leg)))
    for leg in legs:
        dl = decompress(leg)
        torch.cuda.synchronize()
        res["legs"][leg]["decompress_round_trip"] = bool(torch.equal(dl[ok], b["len"][ok]))
        res["legs"][leg]["decompress"] = stats(dt[leg])
    if "mixed" in legs:
        res["plan_decompress"] = gibson_amd.mixed_last_plan()

    # every class alone, as the uniform batch the mixed call makes of it
    if "mixed" in legs:
        for kind, name, fn, by, arrays in (
                (gibson_amd.KIND_COMPRESS, "classes_compress", compress, b["np_len"],
                 (b["off"], b["len"], b["cap"], b["olen"])),
                (gibson_amd.KIND_DECOMPRESS, "classes_decompress", decompress, d_cap.cpu().numpy().astype(np.uint32),
                 (b["off"], d_in_len, d_cap, b["dlen"], b["err"]))):
            perm, cc, cm = gibson_amd.host_size_partition(by, b["max"], kind)
            route = res["plan_compress" if kind == gibson_amd.KIND_COMPRESS else "plan_decompress"]["route"]
            rows, at = [], 0
            for c in range(gibson_amd.NCLASS):
                n = int(cc[c])
                if n:
                    sel = torch.from_numpy(perm[at:at + n].astype(np.int64)).to(dev)
                    sub = tuple(x[sel].contiguous() for x in arrays)      # class-contiguous descriptors
                    fn("uniform", sub, max(int(cm[c]), 1))
                    ts = [timed(lambda: fn("uniform", sub, max(int(cm[c]), 1))) for _ in range(3)]
                    scratch = kind == gibson_amd.KIND_COMPRESS and route[c] in (1, 2)
                    rows.append({"class": c, "values": n, "max_len": int(cm[c]), "route": route[c],
                                 "median_ms": round(statistics.median(ts), 3),
                                 "scratch_chunks": chunks() if scratch else None})
                at += n
            res[name] = rows
            res[name + "_sum_ms"] = round(sum(r["median_ms"] for r in rows), 3)

    if len(legs) == 2:
        for op in ("compress", "decompress"):
            u, m = res["legs"]["uniform"][op], res["legs"]["mixed"][op]
            res[op + "_mixed_over_uniform"] = round(m["median_ms"] / u["median_ms"], 4)
            res[op + "_mixed_minus_uniform_us"] = round((m["median_ms"] - u["median_ms"]) * 1e3, 1)
            res[op + "_spread_ms"] = round(max(u["max_ms"] - u["min_ms"], m["max_ms"] - m["min_ms"]), 3)
    res["kernel_info"] = gibson_amd.kernel_info()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
