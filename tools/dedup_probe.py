#!/usr/bin/env python3
"""Cost and gain of dedup (encode repeated blocks once) on the bench text.

One process, 3 warm-ups and 10 alternating rounds per case; blocks of 1 MiB of the bench stream
(kolm.datagen.enwik_like, seed ENWIK_SEED), resident on the device, hot-path candidates
(kolm_encode_blocks_device):
  hash      256 blocks: k_block_fp's device time (ms_hash of kolm_find_duplicates_device's report)
            against a hipMemcpyAsync device-to-device copy of the same bytes in the same round.
            The hash reads N bytes, the copy moves 2 N: the mark is hash <= copy.
  distinct  256 distinct blocks, dedup off against on in turn: the overhead of one streaming read,
            one read-back and a host sort of 256 entries (no duplicate: the original buffer is
            encoded as with dedup off)
  pairs     128 distinct blocks, each appearing twice (A0 .. A127 A0 .. A127), off against on:
            expected near the 128-block call plus the two gathers
Median and min-max of the wall time of each call, the ratio on / off, and the dedup report's
device times.  Writes profiles/r11/dedup.json (--out).

    python tools/dedup_probe.py [--blocks 256] [--block-size 1048576] [--runs 10] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "kolmogorovlike-datacompressor_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from kolm import _lib, datagen  # noqa: E402
from verify_probe import HipCopy, stats  # noqa: E402


def bench_text(n):
    return datagen.enwik_like(n, seed=datagen.ENWIK_SEED)


def hash_case(ctx, data, bs, runs, warmup):
    n = len(data)
    d_in = _lib.input_buffer(ctx, data)
    d_cp = _lib.DeviceBuffer(ctx, n + 64)
    copy = HipCopy(d_in.ptr, d_cp.ptr, n)
    bounds = list(range(0, n, bs)) + [n]
    t = {"hash": [], "copy": [], "find_wall": []}
    try:
        for it in range(warmup + runs):
            t0 = time.perf_counter()
            rep, r = _lib.find_duplicates_device(ctx, d_in.ptr, bounds)
            wall = 1e3 * (time.perf_counter() - t0)
            assert r["blocks"] == len(bounds) - 1 and r["bytes"] == n
            cp = copy.run()
            if it >= warmup:
                t["hash"].append(r["ms_hash"])
                t["copy"].append(cp)
                t["find_wall"].append(wall)
    finally:
        copy.free()
        d_in.free()
        d_cp.free()
    res = {k: stats(v) for k, v in t.items()}
    res["hash_over_copy"] = res["hash"]["median_ms"] / res["copy"]["median_ms"]
    res["hash_gb_per_s"] = n / 1e9 / (res["hash"]["median_ms"] / 1e3)
    res["copy_gb_per_s"] = 2 * n / 1e9 / (res["copy"]["median_ms"] / 1e3)
    res["blocks_distinct"] = int(len(set(int(x) for x in rep)))
    return res


def encode_case(ctx, data, bs, runs, warmup, want_distinct):
    n = len(data)
    nb = (n + bs - 1) // bs
    mask = _lib.KOLM_HOTPATH_MASK
    d_in = _lib.input_buffer(ctx, data)
    arena = _lib.DeviceBuffer(ctx, _lib.arena_capacity(n, nb, mask))
    t = {"encode_off": [], "encode_on": [], "device_off": [], "device_on": [], "hash": [], "compare": [], "compact": [],
         "expand": []}
    try:
        for it in range(warmup + runs):
            row, outs = {}, {}
            for key in (("off", "on") if it % 2 == 0 else ("on", "off")):  # alternating order
                t0 = time.perf_counter()
                _, meth, off, st = _lib.encode_blocks_device(ctx, d_in.ptr, n, bs, arena.ptr, arena.nbytes, mask,
                                                             dedup=key == "on")
                row["encode_" + key] = 1e3 * (time.perf_counter() - t0)
                row["device_" + key] = st["ms_total"]
                outs[key] = (meth.copy(), off.copy())
                if key == "on":
                    r = _lib.last_dedup()
                    assert r["blocks"] == nb and r["blocks_encoded"] == want_distinct and r["collisions"] == 0
                    row.update(hash=r["ms_hash"], compare=r["ms_compare"], compact=r["ms_compact"], expand=r["ms_expand"])
            assert (outs["on"][0] == outs["off"][0]).all() and (outs["on"][1] == outs["off"][1]).all()
            if it >= warmup:
                for k, v in row.items():
                    t[k].append(v)
    finally:
        d_in.free()
        arena.free()
    res = {k: stats(v) for k, v in t.items()}
    res["on_over_off"] = res["encode_on"]["median_ms"] / res["encode_off"]["median_ms"]
    res["blocks"], res["blocks_encoded"] = nb, want_distinct
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-size", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r11", "dedup.json"))
    args = ap.parse_args()
    ctx = _lib.device_ctx(_lib.ensure_init(0))
    nb, bs = args.blocks, args.block_size
    text = bench_text(nb * bs)
    res = {"block_size": bs, "blocks": nb, "runs": args.runs, "warmup": args.warmup, "hot_path": True, "cases": {}}
    cases = (("hash", lambda: hash_case(ctx, text, bs, args.runs, args.warmup)),
             ("distinct", lambda: encode_case(ctx, text, bs, args.runs, args.warmup, nb)),
             ("pairs", lambda: encode_case(ctx, text[:nb // 2 * bs] * 2, bs, args.runs, args.warmup, nb // 2)))
    for name, fn in cases:
        r = fn()
        res["cases"][name] = r
        print(json.dumps({name: r}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
