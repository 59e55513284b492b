#!/usr/bin/env python3
"""What request ingest costs: lzf_gpu_request_parse and
lzf_gpu_store_append_keys against a plain copy of the bytes they touch, and
against what a caller does today on the host.

usage: ingest_bench.py [--workloads set64,set4k,get] [--repeats R] [--warmup W] [--scale S] [--seed N]
                       [--once WORKLOAD]

One process.  Per workload 1 M requests (divided by --scale) with seeded random
keys of 16-40 bytes, built on the host and uploaded once:
  set64  SET "10 <key> <64-byte value>"
  set4k  SET "10 <key> <4096-byte value>"
  get    GET "<key>"
HIP events around every device call, warm-ups and R timed repeats (at least 7)
that alternate
  (a) parse        lzf_gpu_request_parse of the batch;
  (b) parse_copy   one device-to-device copy of exactly the bytes (a) must read
                   and write: 12 bytes of descriptor and the scanned bytes of
                   every request (opcode, ttl token, key and the byte behind
                   it), 34 bytes of outputs;
  (c) append       lzf_gpu_store_append_keys (SET only; *keys_used is zeroed
                   before every call, outside the timed region);
  (d) append_copy  the copy of what (c) must read and write: 26 bytes of parse
                   outputs and the key bytes, 48 bytes of item members, set_len
                   and void_idx and the key bytes again.
The host yardstick is timed with the wall clock, once per repeat: (e)
lzf_host_request_parse on one thread, (f) a host key pack (one numpy gather of
the key bytes into a dense arena -- a C caller's memcpy loop would be faster),
(g) the upload of the descriptor arrays and the packed keys from pageable
memory.  Prints one JSON object: per workload and leg median, min, max and
every repeat, the copies' GB/s, and the ratios (a) / (b), (c) / (d), ((e) +
(g)) / (a) and ((f)) / (c).

--once WORKLOAD runs the parse and the append of that workload three times and
nothing else: the form to put under a kernel trace, whose per-kernel times
give the split over the append's three launches."""
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

PARSE_IN, PARSE_OUT = 8 + 4, 1 + 1 + 8 + 4 + 8 + 4 + 8
APPEND_IN, APPEND_OUT = 1 + 1 + 8 + 4 + 4 + 8, 8 + 4 + 8 + 4 + 8 + 8 + 4 + 4


def build(rs, n, op, head, vlen):
    """n requests [i16 op][head][key][' ' value] -> arena, off, len, key lengths, scanned bytes"""
    klen = rs.randint(16, 41, n).astype(np.int64)
    tail = (1 + vlen) if vlen else 0
    ln = 2 + len(head) + klen + tail
    off = np.cumsum(ln) - ln
    arena = np.full(int(ln.sum()) + 16, ord("v"), np.uint8)
    arena[off], arena[off + 1] = op, 0
    for j, c in enumerate(head):
        arena[off + 2 + j] = c
    kat = off + 2 + len(head)
    pos = np.arange(int(klen.sum()), dtype=np.int64) - np.repeat(np.cumsum(klen) - klen, klen) + np.repeat(kat, klen)
    arena[pos] = rs.randint(ord("a"), ord("z") + 1, len(pos)).astype(np.uint8)
    if vlen:
        arena[kat + klen] = ord(" ")
    scanned = int((2 + len(head) + klen + (1 if vlen else 0)).sum())
    return arena, off.astype(np.uint64), ln.astype(np.uint32), klen, scanned


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="set64,set4k,get")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xC0FFEE)
    ap.add_argument("--once", default=None)
    a = ap.parse_args()
    a.repeats = max(a.repeats, 7)
    dev = torch.device("cuda", 0)
    n = (1 << 20) // a.scale
    shapes = {"set64": (gibson_amd.OP_SET, b"10 ", 64), "set4k": (gibson_amd.OP_SET, b"10 ", 4096),
              "get": (gibson_amd.OP_GET, b"", 0)}
    res = {"requests": n, "repeats": a.repeats, "warmup": a.warmup, "seed": a.seed,
           "library": os.environ.get("LZF_HIP_LIB") or "in-tree", "device": torch.cuda.get_device_name(0),
           "workloads": []}
    for name in [a.once] if a.once else a.workloads.split(","):
        op, head, vlen = shapes[name]
        rs = np.random.RandomState(a.seed)
        arena, off, ln, klen, scanned = build(rs, n, op, head, vlen)
        kbytes = int(klen.sum())
        up = lambda x: torch.from_numpy(x.view({8: np.int64, 4: np.int32, 1: np.uint8}[x.dtype.itemsize])).to(dev)
        d_req, d_off, d_len = up(arena), up(off), up(ln)
        parsed = gibson_amd.ParsedRequests.empty(n, dev)
        pres = torch.zeros(gibson_amd.REQ_NSTATUS, dtype=torch.int64, device=dev)
        z = lambda dt: torch.zeros(n, dtype=dt, device=dev)
        keys = torch.empty(kbytes + 16, dtype=torch.uint8, device=dev)
        keys_used = torch.zeros(1, dtype=torch.int64, device=dev)
        key_off, key_len, item_time, item_ttl = z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int32)
        item_lock, last_access, set_len, void = z(torch.int64), z(torch.int64), z(torch.int32), z(torch.int32)
        ares = torch.zeros(4, dtype=torch.int64, device=dev)
        work = gibson_amd.store_append_keys_work(n, dev)
        parse_bytes = n * (PARSE_IN + PARSE_OUT) + scanned
        append_bytes = n * (APPEND_IN + APPEND_OUT) + 2 * kbytes
        bounce = torch.empty(max(parse_bytes, append_bytes), dtype=torch.uint8, device=dev)
        bounce2 = torch.empty_like(bounce)

        def parse():
            gibson_amd.request_parse(d_req, d_off, d_len, 512, 1 << 20, parsed, pres, expect_op=op)

        def append():
            gibson_amd.store_append_keys(d_req, parsed, keys, keys_used, key_off, key_len, 0, 1000, 100, set_len, void,
                                         ares, item_time=item_time, item_ttl=item_ttl, item_lock=item_lock,
                                         last_access=last_access, work=work)

        if a.once:
            for _ in range(3):
                keys_used.zero_()
                parse()
                if op == gibson_amd.OP_SET:
                    append()
            torch.cuda.synchronize()
            print(json.dumps({"once": name, "statuses": pres.cpu().numpy().tolist(), "append": ares.cpu().numpy().tolist()}))
            return
        legs = {"parse": parse, "parse_copy": lambda: bounce2[:parse_bytes // 2].copy_(bounce[:parse_bytes // 2])}
        if op == gibson_amd.OP_SET:
            legs["append"] = append
            legs["append_copy"] = lambda: bounce2[:append_bytes // 2].copy_(bounce[:append_bytes // 2])
        host = {}

        def host_parse():
            host["out"], host["result"] = gibson_amd.host_request_parse(arena, off, ln, 512, 1 << 20, op)

        def host_pack():
            o = host["out"]
            kl = o.key_len.astype(np.int64)
            starts = np.cumsum(kl) - kl
            pos = np.arange(int(kl.sum()), dtype=np.int64) - np.repeat(starts, kl) + np.repeat(o.key_off.astype(np.int64), kl)
            host["keys"], host["key_off"] = arena[pos], starts

        def upload():
            o = host["out"]
            sent = [o.key_off.view(np.int64), o.key_len.view(np.int32)]
            if op == gibson_amd.OP_SET:
                sent += [o.val_off.view(np.int64), o.val_len.view(np.int32), o.num, host["keys"], host["key_off"]]
            host["sent"] = [torch.from_numpy(x).to(dev) for x in sent]

        host_legs = {"host_parse": host_parse}
        if op == gibson_amd.OP_SET:
            host_legs["host_pack"] = host_pack
        host_legs["upload"] = upload
        for _ in range(a.warmup):
            for fn in legs.values():
                keys_used.zero_()
                fn()
        torch.cuda.synchronize()
        counts = pres.cpu().numpy().tolist()
        ok = counts[gibson_amd.REQ_OK] == n
        if op == gibson_amd.OP_SET:
            ok = ok and ares.cpu().numpy().tolist() == [n, 0, kbytes, gibson_amd.STORE_OK]
            ok = ok and int(set_len.sum().item()) == n * vlen
        ts = {k: [] for k in list(legs) + list(host_legs)}
        for _ in range(a.repeats):                    # alternating
            for k, fn in legs.items():
                keys_used.zero_()
                ts[k].append(timed(fn))
            for k, fn in host_legs.items():
                ts[k].append(wall(fn))
        ok = ok and host["result"].tolist() == counts
        st = {k: stats(v) for k, v in ts.items()}
        med = lambda k: st[k]["median_ms"]
        w = {"workload": name, "request_bytes": int(ln.sum()), "key_bytes": kbytes, "parse_bytes": parse_bytes,
             "ok": bool(ok), "legs": st,
             "parse_copy_gb_per_s": round(parse_bytes / med("parse_copy") / 1e6, 1),
             "parse_mreq_per_s": round(n / med("parse") / 1e3, 1),
             "parse_over_copy": round(med("parse") / med("parse_copy"), 3),
             "host_parse_and_upload_over_parse": round((med("host_parse") + med("upload")) / med("parse"), 1)}
        if op == gibson_amd.OP_SET:
            w.update({"append_bytes": append_bytes,
                      "append_copy_gb_per_s": round(append_bytes / med("append_copy") / 1e6, 1),
                      "append_over_copy": round(med("append") / med("append_copy"), 3),
                      "host_pack_over_append": round(med("host_pack") / med("append"), 1)})
        res["workloads"].append(w)
        del d_req, bounce, bounce2
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
