#!/usr/bin/env python3
"""What the per-request replies of the device store (lzf_gpu_store_replies)
cost against the nearest thing a caller had, and whether the decode launch per
size class pays.

usage: reply_bench.py [--items N] [--k K] [--repeats R] [--warmup W] [--scale S] [--seed N] [--legs a,b]
                      [--out DIR] [--route both|split|one_route]

One process.  HIP events around every call, warm-ups and R timed repeats (at
least 7), the legs of a shape alternating.

a: the MGET bench's shape: a store of N (1 M) device-generated 4 KiB json
   values stored by lzf_gpu_set_store at compression 64, and a seeded random
   list of K (100 000) distinct items, in GET mode with the time arrays (no
   item expires) and last_access.  Legs:
     replies  lzf_gpu_store_replies over the list, one decode launch per size
              class (LZF_GPU_REPLY_ONE_ROUTE=0);
     replies_one_route  the same with one decode launch (=1, the default);
     mget     lzf_gpu_store_mget over the same list (unchanged code: one
              REPL_KVAL frame for all of them);
     copy     a device-to-device copy of *rep_used bytes.
   With max_val_len = 4096 only the first decode class can hold an entry, so
   the class split and the one-route form are the same launches here; both are
   timed all the same.
b: a list of K entries over a store with the `mixedsize` length distribution
   of mixed_bench.py (64 B - 1 MiB, five size bands, the request order a
   seeded shuffle).  Legs:
     split      LZF_GPU_REPLY_ONE_ROUTE=0: one decode launch per size class;
     one_route  LZF_GPU_REPLY_ONE_ROUTE=1: one launch bounded by max_val_len
                (what the library does when the variable is unset).
   The two arenas are compared byte for byte first.  --route split or
   one_route runs that form alone (for a kernel trace of it).

Before the timing the replies of a sample of entries are checked against the
store's input bytes.  Prints one JSON object and, with --out, writes it to
DIR/reply_bench.json.  --scale divides every count (rehearsals)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gibson_amd  # noqa: E402
from mget_bench import make_keys, spread  # noqa: E402
from mixed_bench import MIXEDSIZE, make_batch, stats, timed  # noqa: E402

NOW = 1_700_000_000
ENV = "LZF_GPU_REPLY_ONE_ROUTE"


class Store:
    """a batch of device-generated values stored by lzf_gpu_set_store"""

    def __init__(self, b, dev):
        lens = b["np_len"].astype(np.int64)
        self.b, self.lens, self.count, self.in_bytes = b, lens, len(lens), int(lens.sum())
        self.store = torch.empty(self.in_bytes + 8 * self.count + 16, dtype=torch.uint8, device=dev)
        self.used = torch.zeros(1, dtype=torch.int64, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.val_off = torch.zeros(self.count, dtype=torch.int64, device=dev)
        self.val_size = torch.zeros(self.count, dtype=torch.int32, device=dev)
        self.enc = torch.zeros(self.count, dtype=torch.uint8, device=dev)
        work = gibson_amd.set_store(b["src"], b["off"], b["len"], 64, b["max"], self.in_bytes, self.store, self.used,
                                    self.val_off, self.val_size, self.enc, self.status)
        torch.cuda.synchronize()
        del work
        self.val_len = b["len"]
        self.item_time = torch.full((self.count,), NOW - 5, dtype=torch.int64, device=dev)
        self.item_ttl = torch.zeros(self.count, dtype=torch.int32, device=dev)
        self.last = torch.zeros(self.count, dtype=torch.int64, device=dev)

    def info(self):
        return {"items": self.count, "input_bytes": self.in_bytes, "store_status": int(self.status.item()),
                "store_bytes": int(self.used.item()),
                "stored_lzf": int((self.enc == gibson_amd.ENC_LZF).sum().item()), "max_val_len": self.b["max"]}


class Replies:
    def __init__(self, s, idx_np, dev):
        self.s, self.k = s, len(idx_np)
        self.idx = torch.from_numpy(idx_np.astype(np.uint32).view(np.int32)).to(dev)
        self.cap = int(np.maximum(s.lens[idx_np] + 7, 8).sum())
        self.arena = torch.zeros(self.cap, dtype=torch.uint8, device=dev)
        self.used = torch.zeros(1, dtype=torch.int64, device=dev)
        self.off = torch.zeros(self.k, dtype=torch.int64, device=dev)
        self.len = torch.zeros(self.k, dtype=torch.int32, device=dev)
        self.est = torch.zeros(self.k, dtype=torch.uint8, device=dev)
        self.result = torch.zeros(6, dtype=torch.int64, device=dev)
        self.work = gibson_amd.store_replies_work(self.k, dev)

    def __call__(self):
        s = self.s
        gibson_amd.store_replies(self.idx, gibson_amd.REPLY_GET, s.store, s.val_off, s.val_size, s.enc, s.val_len,
                                 s.item_time, s.item_ttl, NOW, s.b["max"], self.arena, self.used, self.off, self.len,
                                 self.est, self.result, last_access=s.last, work=self.work)

    def sample_ok(self, idx_np, every):
        """the replies of every `every`-th entry against the input bytes"""
        s = self.s
        torch.cuda.synchronize()
        off, ln = self.off.cpu().numpy(), self.len.cpu().numpy()
        src_off = s.b["off"].cpu().numpy()
        for k in range(0, self.k, every):
            i, n = int(idx_np[k]), int(s.lens[idx_np[k]])
            got = self.arena[int(off[k]):int(off[k]) + int(ln[k])].cpu().numpy().tobytes()
            want = s.b["src"][int(src_off[i]):int(src_off[i]) + n].cpu().numpy().tobytes()
            if got != bytes([6, 0, 0]) + n.to_bytes(4, "little") + want:
                return False
        return True


def one_route(on):
    os.environ[ENV] = "1" if on else "0"


def bench_a(a, dev, gen):
    s = Store(make_batch([(a.items, 4096, 4096)], (1,), a.scale, dev), dev)
    k = min(max(a.k // a.scale, 1), s.count)
    idx_np = np.random.RandomState(a.seed).choice(s.count, k, replace=False)
    r = Replies(s, idx_np, dev)
    keys, koff, klen = make_keys(s.count, dev, gen)
    max_response = int(s.lens[idx_np].sum()) + k * (9 + 40) + 4
    frame = torch.zeros(max_response + 7, dtype=torch.uint8, device=dev)
    flen = torch.zeros(1, dtype=torch.int64, device=dev)
    mres = torch.zeros(4, dtype=torch.int64, device=dev)
    mwork = gibson_amd.store_mget_work(k, dev)
    dst = torch.empty_like(r.arena)

    def mget():
        gibson_amd.store_mget(r.idx, keys, koff, klen, s.store, s.val_off, s.val_size, s.enc, s.val_len, s.item_time,
                              s.item_ttl, NOW, s.b["max"], frame, max_response, flen, mres, last_access=s.last,
                              work=mwork)

    def replies_one():
        one_route(True)
        r()

    def replies_split():
        one_route(False)
        r()

    replies_split()
    ok = r.sample_ok(idx_np, max(k // 200, 1))
    used = int(r.used.item())

    def copy():
        dst[:used].copy_(r.arena[:used])

    legs = {"replies": replies_split, "replies_one_route": replies_one, "mget": mget, "copy": copy}
    for _ in range(a.warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ts = {name: [] for name in legs}
    for _ in range(a.repeats):                        # alternating
        for name, f in legs.items():
            ts[name].append(timed(f))
    out = {name: stats(v) for name, v in ts.items()}
    med = {name: v["median_ms"] for name, v in out.items()}
    res = s.info()
    res.update({"k": k, "reply_bytes": used, "result": r.result.cpu().numpy().tolist(), "sample_ok": ok,
                "mget_result": mres.cpu().numpy().tolist(), "mget_frame_bytes": int(flen.item()), "legs": out,
                "replies_over_mget": round(med["replies"] / med["mget"], 3),
                "replies_over_copy": round(med["replies"] / med["copy"], 3),
                "split_over_one_route": round(med["replies"] / med["replies_one_route"], 3),
                "spread": {name: round(spread(v), 4) for name, v in out.items()}})
    return res


def bench_b(a, dev):
    s = Store(make_batch(MIXEDSIZE, (2, 1, 3), a.scale, dev), dev)
    k = min(max(a.k // a.scale, 1), s.count)
    idx_np = np.random.RandomState(a.seed + 1).choice(s.count, k, replace=False)
    r = Replies(s, idx_np, dev)
    lens = s.lens[idx_np]
    lzf = (s.enc.cpu().numpy() == gibson_amd.ENC_LZF)[idx_np]
    classes = [int((lzf & (lens <= 4096)).sum()), int((lzf & (lens > 4096) & (lens <= 16384)).sum()),
               int((lzf & (lens > 16384)).sum())]

    def split():
        one_route(False)
        r()

    def one():
        one_route(True)
        r()

    legs = {"split": split, "one_route": one}
    same = None
    if a.route == "both":
        one()
        ok = r.sample_ok(idx_np, max(k // 200, 1))
        first = r.arena.clone()
        res_one = r.result.cpu().numpy().tolist()
        r.arena.zero_()
        split()
        torch.cuda.synchronize()
        same = bool(torch.equal(first, r.arena)) and res_one == r.result.cpu().numpy().tolist()
        ok = ok and r.sample_ok(idx_np, max(k // 200, 1))
        del first
    else:                                             # a kernel trace of one form alone
        legs = {a.route: legs[a.route]}
        legs[a.route]()
        ok = r.sample_ok(idx_np, max(k // 200, 1))
    for _ in range(a.warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ts = {name: [] for name in legs}
    for _ in range(a.repeats):                        # alternating
        for name, f in legs.items():
            ts[name].append(timed(f))
    out = {name: stats(v) for name, v in ts.items()}
    res = s.info()
    res.update({"k": k, "reply_bytes": int(r.used.item()), "result": r.result.cpu().numpy().tolist(),
                "lzf_entries_by_class": classes, "sample_ok": ok, "arenas_equal": same, "legs": out,
                "spread": {name: round(spread(v), 4) for name, v in out.items()}})
    if a.route == "both":
        res["split_over_one_route"] = round(out["split"]["median_ms"] / out["one_route"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1 << 20)
    ap.add_argument("--k", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--out", default=None)
    ap.add_argument("--route", default="both", choices=("both", "split", "one_route"))
    a = ap.parse_args()
    a.repeats = max(a.repeats, 7)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    res = {"repeats": a.repeats, "warmup": a.warmup, "seed": a.seed, "scale": a.scale,
           "library": os.environ.get("LZF_HIP_LIB") or "in-tree", "device": torch.cuda.get_device_name(0)}
    legs = a.legs.split(",")
    if "a" in legs:
        res["a"] = bench_a(a, dev, gen)
        torch.cuda.empty_cache()
    if "b" in legs:
        res["b"] = bench_b(a, dev)
    text = json.dumps(res)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "reply_bench.json"), "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
