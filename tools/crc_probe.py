#!/usr/bin/env python3
"""Cost of the block CRC-32 (k_crc32) on the bench text.

One process.  Blocks of 1 MiB of the bench stream (kolm.datagen.enwik_like, seed ENWIK_SEED):
  kernel  256 blocks resident on the device.  Three measurements alternate in every round, three
          rounds of `--runs` repetitions each after the warm-up: k_crc32 (the device time
          kolm_crc32_blocks_device reports: HIP events around the kernel), k_block_fp (ms_hash of
          kolm_find_duplicates_device's report: the same bytes through the same loads, the
          reference point) and a hipMemcpyAsync device-to-device copy of the buffer (HIP events).
          The two kernels read N bytes, the copy moves 2 N.  Reported: ms (median, min, max) and
          TB/s of each, and k_crc32 over k_block_fp.
  check   a container of 32 blocks: kolm.check (decode + k_crc32 over the scratch, no original)
          against kolm.verify (decode + k_verify_cmp against the uploaded original), alternating:
          wall ms of each call, ms_decode and ms_crc against ms_decode and ms_compare.
Writes profiles/r13/crc.json (--out).  The committed file also holds an "encode" case: the bench A/B of
the parent commit against this build with checksums off and on (bench.py runs, their command in the
case), which this tool does not produce.

    python tools/crc_probe.py [--blocks 256] [--block-size 1048576] [--runs 5] [--out PATH]
"""
import argparse
import json
import os
import sys
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "kolmogorovlike-datacompressor_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import kolm  # noqa: E402
from kolm import _lib, datagen  # noqa: E402
from verify_probe import HipCopy, stats  # noqa: E402


def bench_text(n):
    return datagen.enwik_like(n, seed=datagen.ENWIK_SEED)


def kernel_case(ctx, data, bs, runs, warmup):
    n = len(data)
    d_in = _lib.input_buffer(ctx, data)
    d_cp = _lib.DeviceBuffer(ctx, n + 64)
    copy = HipCopy(d_in.ptr, d_cp.ptr, n)
    bounds = list(range(0, n, bs)) + [n]
    t = {"crc": [], "fp": [], "copy": []}
    try:
        crcs = None
        for rnd in range(3):  # the three alternate three times
            for it in range((warmup if rnd == 0 else 0) + runs):
                crcs, ms = _lib.crc32_blocks_device(ctx, d_in.ptr, bounds)
                _, r = _lib.find_duplicates_device(ctx, d_in.ptr, bounds)
                cp = copy.run()
                if rnd or it >= warmup:
                    t["crc"].append(ms)
                    t["fp"].append(r["ms_hash"])
                    t["copy"].append(cp)
        for i in (0, len(crcs) // 2, len(crcs) - 1):  # the result is zlib's
            assert crcs[i] == zlib.crc32(data[bounds[i]:bounds[i + 1]]), i
    finally:
        copy.free()
        d_in.free()
        d_cp.free()
    res = {k: stats(v) for k, v in t.items()}
    res["crc_tb_per_s"] = n / 1e12 / (res["crc"]["median_ms"] / 1e3)
    res["fp_tb_per_s"] = n / 1e12 / (res["fp"]["median_ms"] / 1e3)
    res["copy_tb_per_s"] = 2 * n / 1e12 / (res["copy"]["median_ms"] / 1e3)
    res["crc_over_fp"] = res["crc"]["median_ms"] / res["fp"]["median_ms"]
    res["crc_over_copy"] = res["crc"]["median_ms"] / res["copy"]["median_ms"]
    res["bytes"] = n
    return res


def check_case(data, bs, runs, warmup):
    blob = kolm.compress_blocks_fixed(data, bs, hot_path=True, checksums=True)
    cs = kolm.last_checksums()
    assert cs.stream_crc == zlib.crc32(data)
    t = {"check_wall": [], "verify_wall": [], "check_decode": [], "check_crc": [], "verify_decode": [],
         "verify_compare": []}
    for it in range(warmup + runs):
        row = {}
        for key in (("check", "verify") if it % 2 == 0 else ("verify", "check")):
            t0 = time.perf_counter()
            r = kolm.check(blob, cs) if key == "check" else kolm.verify(blob, data)
            row[key + "_wall"] = 1e3 * (time.perf_counter() - t0)
            assert r["ok"] and r["blocks"] == len(cs.lens)
            row[key + "_decode"] = r["ms_decode"]
            row["check_crc" if key == "check" else "verify_compare"] = r["ms_crc" if key == "check" else "ms_compare"]
        if it >= warmup:
            for k, v in row.items():
                t[k].append(v)
    res = {k: stats(v) for k, v in t.items()}
    res["blocks"], res["bytes"], res["container_bytes"] = len(cs.lens), len(data), len(blob)
    res["crc_over_compare"] = res["check_crc"]["median_ms"] / res["verify_compare"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--check-blocks", type=int, default=32)
    ap.add_argument("--block-size", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r13", "crc.json"))
    args = ap.parse_args()
    ctx = _lib.device_ctx(_lib.ensure_init(0))
    nb, bs = args.blocks, args.block_size
    text = bench_text(nb * bs)
    res = {"block_size": bs, "blocks": nb, "runs": args.runs, "warmup": args.warmup, "cases": {}}
    cases = (("kernel", lambda: kernel_case(ctx, text, bs, args.runs, args.warmup)),
             ("check", lambda: check_case(text[:args.check_blocks * bs], bs, args.runs, args.warmup)))
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
