#!/usr/bin/env python3
"""Cost of random-access reads (kolm.open_container) against a device-to-device copy and against
kolm.decompress of the whole container.

One process: `--blocks` x 1 MiB enwik_like blocks compressed with the hot-path candidates, one
Reader over the container, warm-ups and alternating timed rounds.  Measured per round:
  (a) gather bandwidth: one contiguous range of nearly the whole stream into device memory at the
      (source, destination) misalignment pairs (0, 0) and (3, 9) — ms_gather of kolm_read_stats
      is k_range_gather's own device time — beside hipMemcpyAsync device-to-device of the same
      bytes;
  (b) many small ranges: 65536 seeded ranges of 256 B..4 KiB into device memory (ms_gather, GB/s,
      ranges/s) beside the copy of the same total bytes;
  (c) end to end, wall time: reader.read of 4 KiB inside one block and read_many of 1000 small
      ranges, each beside kolm.decompress of the whole container; blocks_decoded is reported.
Writes min / median / max to profiles/r10/range.json (--out).

    python tools/range_probe.py [--blocks 256] [--runs 5] [--warmup 2] [--out PATH]
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

import kolm  # noqa: E402
from kolm import _lib, datagen  # noqa: E402
from verify_probe import HipCopy, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-size", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10", "range.json"))
    args = ap.parse_args()
    bs, n = args.block_size, args.blocks * args.block_size
    ctx = _lib.device_ctx(_lib.ensure_init(0))
    data = b"".join(datagen.enwik_like(min(32 << 20, n - o), seed=1 + o // (32 << 20)) for o in range(0, n, 32 << 20))
    blob = kolm.compress_blocks_fixed(data, bs, hot_path=True)
    rng = np.random.default_rng(10)
    small = []
    for _ in range(65536):
        m = int(rng.integers(256, 4097))
        small.append((int(rng.integers(0, n - m + 1)), m))
    small_bytes = sum(m for _, m in small)
    if small_bytes > n:  # the packed small ranges land in the n + 64 bytes of `out`
        sys.exit(f"--blocks {args.blocks}: the 65536 small ranges hold {small_bytes} bytes, more than the {n} of the data")
    thousand = small[:1000]
    big = n - 64
    out = _lib.DeviceBuffer(ctx, n + 64)
    cp = _lib.DeviceBuffer(ctx, n + 64)
    copy_big = HipCopy(out.ptr, cp.ptr, big)
    copy_small = HipCopy(out.ptr, cp.ptr, small_bytes)
    t = {k: [] for k in ("gather_0_0", "gather_3_9", "copy_big", "small_gather", "copy_small", "decode_all",
                         "read_4k_wall", "read_1000_wall", "decompress_wall")}
    seen = {}
    with kolm.open_container(blob, ctx) as rd:
        for it in range(args.warmup + args.runs):
            row = {}
            for key, (sm, dm) in (("gather_0_0", (0, 0)), ("gather_3_9", (3, 9))):
                rd.read_many_device([(sm, big)], out.ptr + dm, big)
                st = kolm.last_read()
                row[key], row["decode_all"] = st["ms_gather"], st["ms_decode"]
            assert out.download(4096, 9) == data[3:3 + 4096]
            row["copy_big"] = copy_big.run()
            offs = rd.read_many_device(small, out.ptr, small_bytes)
            row["small_gather"] = kolm.last_read()["ms_gather"]
            o, m = small[-1]
            assert out.download(m, offs[-1]) == data[o:o + m]
            row["copy_small"] = copy_small.run()
            t0 = time.perf_counter()
            got = rd.read(5 * bs + 12345, 4096)
            row["read_4k_wall"] = 1e3 * (time.perf_counter() - t0)
            seen["read_4k_blocks_decoded"] = kolm.last_read()["blocks_decoded"]
            assert got == data[5 * bs + 12345:5 * bs + 12345 + 4096]
            t0 = time.perf_counter()
            got = rd.read_many(thousand)
            row["read_1000_wall"] = 1e3 * (time.perf_counter() - t0)
            seen["read_1000_blocks_decoded"] = kolm.last_read()["blocks_decoded"]
            assert got[-1] == data[thousand[-1][0]:thousand[-1][0] + thousand[-1][1]]
            t0 = time.perf_counter()
            whole = kolm.decompress(blob)
            row["decompress_wall"] = 1e3 * (time.perf_counter() - t0)
            assert len(whole) == n and whole[-4096:] == data[-4096:]
            del whole
            if it >= args.warmup:
                for k, v in row.items():
                    t[k].append(v)
    for c in (copy_big, copy_small):
        c.free()
    for b in (out, cp):
        b.free()
    res = {k: stats(v) for k, v in t.items()}
    med = lambda k: res[k]["median_ms"]  # noqa: E731
    res.update(seen)
    res.update({"blocks": args.blocks, "block_size": bs, "runs": args.runs, "warmup": args.warmup,
                "container_bytes": len(blob), "big_bytes": big, "small_ranges": len(small), "small_bytes": small_bytes,
                "gather_0_0_over_copy": med("gather_0_0") / med("copy_big"),
                "gather_3_9_over_copy": med("gather_3_9") / med("copy_big"),
                "gather_0_0_gb_per_s": 2 * big / 1e6 / med("gather_0_0"),
                "gather_3_9_gb_per_s": 2 * big / 1e6 / med("gather_3_9"),
                "copy_big_gb_per_s": 2 * big / 1e6 / med("copy_big"),
                "small_gather_over_copy": med("small_gather") / med("copy_small"),
                "small_gather_gb_per_s": 2 * small_bytes / 1e6 / med("small_gather"),
                "small_ranges_per_s": len(small) / (med("small_gather") / 1e3),
                "decompress_over_read_4k": med("decompress_wall") / med("read_4k_wall"),
                "decompress_over_read_1000": med("decompress_wall") / med("read_1000_wall")})
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    print(json.dumps({k: v["median_ms"] for k, v in res.items() if isinstance(v, dict)}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
