#!/usr/bin/env python3
"""What request dispatch costs: lzf_gpu_request_bucket and
lzf_gpu_request_stitch against a plain copy of the bytes they must read and
write, and against what a caller does today on one host thread.

usage: dispatch_bench.py [--repeats R] [--warmup W] [--scale S] [--seed N] [--once]

One process.  1 M parsed requests (divided by --scale) of the realistic mix --
70 % GET, 20 % SET, the rest spread over the other operators, 3 % refused --
synthesized as parse outputs (the bucket reads no request byte) and uploaded
once.  SET and GET are ARENA classes, DEL / LOCK / UNLOCK CODE classes, the
rest HOST.  HIP events around every device call, warm-ups and R timed repeats
(at least 7) that alternate
  (a) bucket       lzf_gpu_request_bucket;
  (b) bucket_copy  one device-to-device copy of exactly the bytes (a) must read
                   and write: 34 bytes of parse outputs in, the same 34 bytes
                   gathered plus perm and slot out;
  (c) stitch       lzf_gpu_request_stitch;
  (d) stitch_copy  the copy of what (c) must read and write: op, status and
                   slot, 12 bytes of reply slice per ARENA request, a byte of
                   entry status per CODE request, a byte of refusal per SET,
                   and 13 bytes of reply table out.
The host yardstick is timed with the wall clock, once per repeat, one thread:
  (e) download     op and status to the host;
  (f) download5    the five descriptor arrays, which the gathers need on the
                   host (a caller that parsed on the host has them already);
  (g) sort         the class of every request from a 256 x 256 table, a stable
                   numpy argsort by class, its inverse, class_first;
  (h) gather       the seven arrays through the permutation;
  (i) upload       the seven gathered arrays, perm and slot, from pageable memory;
  (j) override     the stitch's seven rules as numpy selects over host arrays;
  (k) host_stitch  lzf_host_request_stitch, the same rules in C.
Prints one JSON object: per leg median, min, max and every repeat, the copies'
GB/s, and the ratios (a) / (b), (c) / (d), ((e) + (g) + (h) + (i)) / (a) and
(j) / (c).

--once runs the bucket and the stitch three times and nothing else: the form
to put under a kernel trace, whose per-kernel times give the split over the
bucket's three launches."""
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

G = gibson_amd
NC = G.RQ_NCLASS
FIELDS = G.ParsedRequests.FIELDS
NP_DT = {"op": np.uint8, "status": np.uint8, "key_off": np.uint64, "key_len": np.uint32, "val_off": np.uint64,
         "val_len": np.uint32, "num": np.int64}
BUCKET_BYTES = 34 + 34 + 4 + 4
ARENA, CODE = (G.OP_SET, G.OP_GET), (G.OP_DEL, G.OP_LOCK, G.OP_UNLOCK)


def class_table():
    t = np.zeros((256, 256), np.uint8)
    for c in range(1, 22):
        t[c, G.REQ_OK] = t[c, G.REQ_NAN] = c
    t[G.OP_END, G.REQ_OK] = t[G.OP_END, G.REQ_NAN] = NC - 1
    return t


def realistic(rs, n):
    x = rs.rand(n)
    op = np.where(x < 0.70, G.OP_GET, np.where(x < 0.90, G.OP_SET, rs.randint(1, 22, n))).astype(np.uint8)
    status = np.where(rs.rand(n) < 0.03, rs.choice([G.REQ_ERR, G.REQ_BADOP, G.REQ_SHORT], n), G.REQ_OK).astype(np.uint8)
    klen = rs.randint(16, 41, n).astype(np.uint32)
    return {"op": op, "status": status, "key_off": (np.cumsum(klen.astype(np.uint64) + 70) - klen).astype(np.uint64),
            "key_len": klen, "val_off": rs.randint(0, 1 << 40, n).astype(np.uint64),
            "val_len": rs.randint(1, 257, n).astype(np.uint32), "num": rs.randint(-1, 100, n).astype(np.int64)}


CODE_OF_ENT = np.array([G.REPL_OK, G.REPL_ERR_NOT_FOUND, G.REPL_ERR_NOT_FOUND, G.REPL_ERR_LOCKED, G.REPL_ERR_NAN, G.REPL_OK,
                        G.REPL_ERR_NAN, G.REPL_ERR, G.REPL_ERR], np.int64)


def numpy_override(op, st, j, c, mode, base, ent, refused, rep_off, rep_len, code_base, rep_cap):
    """the stitch's seven rules on the host, one numpy mask after another;
    `todo` is who is still without a rule -> out_off, out_len, out_kind"""
    n = len(op)
    m, e, todo = mode[c], ent[j], np.ones(n, bool)
    off, ln, kind, code = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.full(n, -1)

    def take(mask):
        nonlocal todo
        mine = mask & todo
        todo = todo & ~mask
        return mine

    kind[take(st == G.REQ_BADOP)] = G.OUT_CLOSE
    code[take((st != G.REQ_OK) & (st != G.REQ_NAN))] = G.REPL_ERR
    gone = (m == G.STITCH_CODE) & ((e == G.ENT_DEAD) | (e == G.ENT_EXPIRED))
    nan = take(st == G.REQ_NAN)
    code[nan] = np.where(gone[nan], G.REPL_ERR_NOT_FOUND, G.REPL_ERR_NAN)
    kind[take(m == G.STITCH_HOST)] = G.OUT_HOST
    code[take((op == G.OP_SET) & (refused[j] != 0))] = G.REPL_ERR_LOCKED
    arena = take(m == G.STITCH_ARENA)
    a_off, a_len = base[c] + rep_off[j], rep_len[j]
    cap = np.uint64(rep_cap)
    bad = (a_off < base[c]) | (a_off > cap) | (a_len > cap - np.minimum(a_off, cap))
    good = arena & ~bad
    off[good], ln[good] = a_off[good], a_len[good]
    code[arena & bad] = G.REPL_ERR
    code[todo] = CODE_OF_ENT[np.minimum(e[todo], 8)]
    framed = code >= 0
    off[framed], ln[framed] = (code_base + 8 * code[framed]).astype(np.uint64), 8
    return off, ln, kind


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0xD15A7C4)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    a.repeats = max(a.repeats, 7)
    dev = torch.device("cuda", 0)
    n = (1 << 20) // a.scale
    rs = np.random.RandomState(a.seed)
    p = realistic(rs, n)
    signed = {8: np.int64, 4: np.int32, 1: np.uint8}
    up = lambda x: torch.from_numpy(x.view(signed[x.dtype.itemsize])).to(dev)
    parsed = G.ParsedRequests(*(up(p[f]) for f in FIELDS))
    bk = G.BucketedRequests.empty(n, dev)
    work = G.request_bucket_work(n, dev)
    table = class_table()
    cls = table[p["op"], p["status"]]
    sizes = np.bincount(cls, minlength=NC)

    # the stitch's inputs: what the per-class calls would have left, in bucket order
    mode, base = [G.STITCH_HOST] * NC, [0] * NC
    for c in ARENA:
        mode[c] = G.STITCH_ARENA
    for c in CODE:
        mode[c] = G.STITCH_CODE
    rep_len = rs.randint(8, 264, n).astype(np.uint32)
    rep_off = np.zeros(n, np.uint64)
    at, room = np.concatenate([[0], np.cumsum(sizes)]), 0
    for c in ARENA:
        sl = slice(int(at[c]), int(at[c + 1]))
        rep_off[sl] = np.cumsum(rep_len[sl].astype(np.uint64)) - rep_len[sl]
        base[c] = room
        room += int(rep_len[sl].sum())
    code_base = (room + 255) // 256 * 256
    replies = torch.zeros(code_base + 64, dtype=torch.uint8, device=dev)
    ent = rs.choice(np.array([0, 0, 0, 1, 2, 3], np.uint8), n)
    refused = (rs.rand(n) < 0.01).astype(np.uint8)
    d_rep_off, d_rep_len, d_ent, d_refused = up(rep_off), up(rep_len), up(ent), up(refused)
    out_off = torch.zeros(n, dtype=torch.int64, device=dev)
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    out_kind = torch.zeros(n, dtype=torch.uint8, device=dev)
    sres = torch.zeros(5, dtype=torch.int64, device=dev)
    n_arena, n_code = int(sum(sizes[c] for c in ARENA)), int(sum(sizes[c] for c in CODE))
    stitch_bytes = n * (1 + 1 + 4) + 12 * n_arena + n_code + int(sizes[G.OP_SET]) + n * (8 + 4 + 1)
    bucket_bytes = n * BUCKET_BYTES

    def bucket():
        G.request_bucket(parsed, bk, work=work)

    def stitch():
        G.request_stitch(parsed.op, parsed.status, bk.slot, bk.class_first, mode, base, replies, code_base, out_off,
                         out_len, out_kind, sres, b_rep_off=d_rep_off, b_rep_len=d_rep_len, b_ent=d_ent,
                         b_refused=d_refused)

    if a.once:
        for _ in range(3):
            bucket()
            stitch()
        torch.cuda.synchronize()
        print(json.dumps({"once": True, "class_first": bk.class_first.cpu().numpy().tolist(),
                          "stitch": sres.cpu().numpy().tolist()}))
        return
    bounce = torch.empty(max(bucket_bytes, stitch_bytes) // 2, dtype=torch.uint8, device=dev)
    bounce2 = torch.empty_like(bounce)
    legs = {"bucket": bucket, "bucket_copy": lambda: bounce2[:bucket_bytes // 2].copy_(bounce[:bucket_bytes // 2]),
            "stitch": stitch, "stitch_copy": lambda: bounce2[:stitch_bytes // 2].copy_(bounce[:stitch_bytes // 2])}
    host = {}

    def download():
        host["op"], host["status"] = parsed.op.cpu().numpy(), parsed.status.cpu().numpy()

    def download5():
        host["rest"] = [getattr(parsed, f).cpu().numpy() for f in FIELDS[2:]]

    def sort():
        c = table[host["op"], host["status"]]
        perm = np.argsort(c, kind="stable").astype(np.uint32)
        slot = np.empty(n, np.uint32)
        slot[perm] = np.arange(n, dtype=np.uint32)
        host["perm"], host["slot"], host["cls"] = perm, slot, c
        host["first"] = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=NC))]).astype(np.uint32)

    def gather():
        host["b"] = [x[host["perm"]] for x in [host["op"], host["status"]] + host["rest"]]

    def upload():
        host["sent"] = [torch.from_numpy(x.view(signed[x.dtype.itemsize])).to(dev)
                        for x in host["b"] + [host["perm"], host["slot"]]]

    mode_np, base_np = np.array(mode, np.uint8), np.array(base, np.uint64)

    def override():
        host["off"], host["len"], host["kind"] = numpy_override(host["op"], host["status"], host["slot"], host["cls"],
                                                                mode_np, base_np, ent, refused, rep_off, rep_len,
                                                                code_base, code_base + 64)

    host_replies = np.zeros(code_base + 64, np.uint8)

    def host_stitch():
        host["twin"] = G.host_request_stitch(host["op"], host["status"], host["slot"], host["first"], mode, base,
                                             host_replies, code_base, b_rep_off=rep_off, b_rep_len=rep_len, b_ent=ent,
                                             b_refused=refused)

    host_legs = {"download": download, "download5": download5, "sort": sort, "gather": gather, "upload": upload,
                 "override": override, "host_stitch": host_stitch}
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in list(legs) + list(host_legs)}
    for _ in range(a.repeats):                        # alternating
        for k, fn in legs.items():
            ts[k].append(timed(fn))
        for k, fn in host_legs.items():
            ts[k].append(wall(fn))
    # the device's outputs against the host's, and the numpy override against the C twin
    ok = (bk.perm.cpu().numpy().view(np.uint32) == host["perm"]).all()
    ok = ok and (bk.class_first.cpu().numpy().view(np.uint32) == host["first"]).all()
    ok = ok and all((getattr(bk.b, f).cpu().numpy().view(NP_DT[f]) == x.view(NP_DT[f])).all() for f, x in zip(FIELDS, host["b"]))
    t_off, t_len, t_kind, t_res = host["twin"]
    ok = ok and (out_off.cpu().numpy().view(np.uint64) == t_off).all() and (out_kind.cpu().numpy() == t_kind).all()
    ok = ok and (out_len.cpu().numpy().view(np.uint32) == t_len).all()
    ok = ok and sres.cpu().numpy().tolist() == [int(x) for x in t_res]
    ok = ok and (host["off"] == t_off).all() and (host["len"] == t_len).all() and (host["kind"] == t_kind).all()
    st = {k: stats(v) for k, v in ts.items()}
    med = lambda k: st[k]["median_ms"]
    host_bucket = med("download") + med("sort") + med("gather") + med("upload")
    print(json.dumps({
        "requests": n, "repeats": a.repeats, "warmup": a.warmup, "seed": a.seed,
        "library": os.environ.get("LZF_HIP_LIB") or "in-tree", "device": torch.cuda.get_device_name(0),
        "class_sizes": sizes.tolist(), "stitch_result": [int(x) for x in t_res], "ok": bool(ok),
        "bucket_bytes": bucket_bytes, "stitch_bytes": stitch_bytes, "legs": st,
        "bucket_copy_gb_per_s": round(bucket_bytes / med("bucket_copy") / 1e6, 1),
        "stitch_copy_gb_per_s": round(stitch_bytes / med("stitch_copy") / 1e6, 1),
        "bucket_mreq_per_s": round(n / med("bucket") / 1e3, 1), "stitch_mreq_per_s": round(n / med("stitch") / 1e3, 1),
        "bucket_over_copy": round(med("bucket") / med("bucket_copy"), 3),
        "stitch_over_copy": round(med("stitch") / med("stitch_copy"), 3),
        "host_bucket_ms": round(host_bucket, 3), "host_bucket_over_bucket": round(host_bucket / med("bucket"), 1),
        "host_bucket_with_download5_over_bucket": round((host_bucket + med("download5")) / med("bucket"), 1),
        "override_over_stitch": round(med("override") / med("stitch"), 1),
        "host_stitch_over_stitch": round(med("host_stitch") / med("stitch"), 1)}))


if __name__ == "__main__":
    main()
