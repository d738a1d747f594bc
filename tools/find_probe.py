#!/usr/bin/env python3
"""Cost of searching a container on the device (Reader.find / count) against its decode and
against kolm.decompress plus a search on the host.

Expectation from the code, stated before any run: k_find_count reads every decoded byte once, as
k_crc32 does, and does a few dozen integer operations per position and pattern, so for one
pattern the search should add a few percent to the decode of the same blocks; 16 patterns cost 16
masked compares per position and should stay well below the decode.  The measured values stand
beside that, whichever way they fall.

One process: `--blocks` x 1 MiB enwik_like blocks compressed with the hot-path candidates, one
Reader over the container, warm-ups and alternating timed rounds.  Measured per round:
  (a) ms_find and ms_decode (kolm_find_stats: HIP events around the search and decode kernels) of
      Reader.find for a rare 12-byte pattern, a frequent 3-byte pattern (the match count is
      reported) and 16 patterns at once, and of Reader.count for the same (no emit launch);
  (b) the count kernel's read rate: kolm_find_device with max_results = 0 over the same bytes
      resident in device memory, beside k_crc32 over them (kolm_crc32_blocks_device);
  (c) wall time of Reader.find beside kolm.decompress(container) plus the host search
      (repeated bytes.find), for the rare and the frequent pattern.
Every result is compared with the host search once.  Writes min / median / max to
profiles/r15/find.json (--out).

    python tools/find_probe.py [--blocks 256] [--runs 5] [--warmup 2] [--out PATH]
"""
import argparse
import json
import os
import sys
import time
from collections import Counter

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "kolmogorovlike-datacompressor_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import kolm  # noqa: E402
from kolm import _lib, datagen  # noqa: E402
from verify_probe import stats  # noqa: E402


def host_find(data, p):
    out, o = [], data.find(p)
    while o >= 0:
        out.append(o)
        o = data.find(p, o + 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-size", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r15", "find.json"))
    args = ap.parse_args()
    bs, n = args.block_size, args.blocks * args.block_size
    ctx = _lib.device_ctx(_lib.ensure_init(0))
    data = b"".join(datagen.enwik_like(min(32 << 20, n - o), seed=1 + o // (32 << 20)) for o in range(0, n, 32 << 20))
    blob = kolm.compress_blocks_fixed(data, bs, hot_path=True)
    mid = n // 2 + 12345
    rare = data[mid:mid + 12]
    freq = Counter(data[i:i + 3] for i in range(1 << 18)).most_common(1)[0][0]
    many = [data[k:k + 6 + i % 9] for i, k in enumerate(range(7777, 7777 + 16 * 65537, 65537))]
    want_rare, want_freq = host_find(data, rare), host_find(data, freq)
    resident = _lib.DeviceBuffer(ctx, n + 64)
    resident.upload(data)
    bounds = list(range(0, n, bs)) + [n]
    keys = ("find_rare", "find_freq", "find_16", "count_rare", "count_freq", "count_16")
    t = {f"{k}_{w}": [] for k in keys for w in ("ms_find", "ms_decode")}
    t.update({k: [] for k in ("count_kernel_rare", "count_kernel_16", "crc32_kernel", "find_rare_wall", "find_freq_wall",
                              "decompress_wall", "host_search_rare_wall", "host_search_freq_wall")})
    seen = {}
    with kolm.open_container(blob, ctx) as rd:
        for it in range(args.warmup + args.runs):
            row = {}
            for key, fn in (("find_rare", lambda: rd.find(rare)), ("find_freq", lambda: rd.find(freq)),
                            ("find_16", lambda: rd.find_many(many)), ("count_rare", lambda: rd.count(rare)),
                            ("count_freq", lambda: rd.count(freq)), ("count_16", lambda: rd.count_many(many))):
                t0 = time.perf_counter()
                got = fn()
                wall = 1e3 * (time.perf_counter() - t0)
                st = kolm.last_find()
                row[f"{key}_ms_find"], row[f"{key}_ms_decode"] = st["ms_find"], st["ms_decode"]
                if key in ("find_rare", "find_freq"):
                    row[f"{key}_wall"] = wall
                    assert got == (want_rare if key == "find_rare" else want_freq)
                seen[f"{key}_matches"], seen[f"{key}_emit_launches"] = st["matches"], st["emit_launches"]
                del got
            assert seen["count_rare_matches"] == len(want_rare) and seen["count_freq_matches"] == len(want_freq)
            row["count_kernel_rare"] = _lib.find_device(ctx, resident.ptr, n, [rare], 0)[3]
            row["count_kernel_16"] = _lib.find_device(ctx, resident.ptr, n, many, 0)[3]
            row["crc32_kernel"] = _lib.crc32_blocks_device(ctx, resident.ptr, bounds)[1]
            t0 = time.perf_counter()
            whole = kolm.decompress(blob)
            row["decompress_wall"] = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            assert host_find(whole, rare) == want_rare
            row["host_search_rare_wall"] = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            assert len(host_find(whole, freq)) == len(want_freq)
            row["host_search_freq_wall"] = 1e3 * (time.perf_counter() - t0)
            del whole
            if it >= args.warmup:
                for k, v in row.items():
                    t[k].append(v)
    resident.free()
    res = {k: stats(v) for k, v in t.items()}
    med = lambda k: res[k]["median_ms"]  # noqa: E731
    res.update(seen)
    res.update({"blocks": args.blocks, "block_size": bs, "runs": args.runs, "warmup": args.warmup,
                "container_bytes": len(blob), "bytes": n, "rare_pattern": rare.decode("latin-1"),
                "freq_pattern": freq.decode("latin-1"), "lens_16": [len(p) for p in many],
                "find_rare_over_decode": med("find_rare_ms_find") / med("find_rare_ms_decode"),
                "find_freq_over_decode": med("find_freq_ms_find") / med("find_freq_ms_decode"),
                "find_16_over_decode": med("find_16_ms_find") / med("find_16_ms_decode"),
                "count_kernel_rare_gb_per_s": n / 1e6 / med("count_kernel_rare"),
                "count_kernel_16_gb_per_s": n / 1e6 / med("count_kernel_16"),
                "crc32_kernel_gb_per_s": n / 1e6 / med("crc32_kernel"),
                "host_rare_over_find_rare_wall": (med("decompress_wall") + med("host_search_rare_wall")) / med("find_rare_wall"),
                "host_freq_over_find_freq_wall": (med("decompress_wall") + med("host_search_freq_wall")) / med("find_freq_wall")})
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    print(json.dumps({k: v["median_ms"] for k, v in res.items() if isinstance(v, dict)}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
