#!/usr/bin/env python3
"""Cost of searching a container for a pattern set (Reader.find_set / count_set) against its
decode, against the size of the set, and against the existing route (find_many in chunks of 16).

Expectation from the code, stated before any run: k_findset_count pays per position a few
single-pattern compares' worth of integer work plus one random LDS read for the filter bit, so its
ms_find should be nearly flat in the set size while few positions pass the filter, and rise with
the share of positions that hit a bucket (each hit: a slot probe in global memory, then the
bucket's patterns verified one by one, divergent within the wave).  Nothing is pre-set as a
threshold: the 16-pattern set's ms_find stands beside find_many's for the same 16 patterns
whichever way it falls, and so does the growth from 16 to 65 536 patterns.

One process: the round-15 probe's container (`--blocks` x 1 MiB enwik_like blocks, hot-path
candidates), one Reader, warm-ups and alternating timed rounds.  Sets of 16, 256, 4 096 and
65 536 patterns: the round-15 probe's 16 patterns first, then words of 6..14 bytes, half drawn
from the text and half random strings of bytes >= 0x80, which the text does not hold.  Per round
and set: ms_find / ms_decode of find_set and count_set (kolm_find_stats); for the 16- and
256-pattern sets also find_many in chunks of 16 over the same reader (summed ms_find, summed
ms_decode, wall time).  The set route's pairs are compared once with the chunked route's (a
cross-check between two device routes; the tests hold the oracles).  Writes min / median / max to
profiles/r16/findset.json (--out).

    python tools/findset_probe.py [--blocks 256] [--runs 5] [--warmup 2] [--out PATH]
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
from verify_probe import stats  # noqa: E402

SIZES = (16, 256, 4096, 65536)


def make_patterns(data, npat):
    n = len(data)
    pats = [data[k:k + 6 + i % 9] for i, k in enumerate(range(7777, 7777 + 16 * 65537, 65537))]
    seen = set(pats)
    assert len(seen) == 16
    rng = np.random.default_rng(16)
    while len(pats) < npat:
        ln = 6 + len(pats) % 9
        if len(pats) % 2:
            p = rng.integers(128, 256, ln, dtype=np.uint8).tobytes()
        else:
            o = int(rng.integers(0, n - ln))
            p = data[o:o + ln]
        if p not in seen:
            seen.add(p)
            pats.append(p)
    return pats


def chunked(rd, pats, limit):
    """find_many in chunks of 16: (sorted pairs or None, summed ms_find, summed ms_decode)."""
    pairs, ms_find, ms_decode = [], 0.0, 0.0
    for c in range(0, len(pats), 16):
        got = rd.find_many(pats[c:c + 16], limit=limit)
        st = kolm.last_find()
        ms_find, ms_decode = ms_find + st["ms_find"], ms_decode + st["ms_decode"]
        pairs += [(o, c + i) for o, i in got]
    pairs.sort()
    return pairs, ms_find, ms_decode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-size", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r16", "findset.json"))
    args = ap.parse_args()
    bs, n = args.block_size, args.blocks * args.block_size
    ctx = _lib.device_ctx(_lib.ensure_init(0))
    data = b"".join(datagen.enwik_like(min(32 << 20, n - o), seed=1 + o // (32 << 20)) for o in range(0, n, 32 << 20))
    assert max(data[:1 << 20]) < 128
    blob = kolm.compress_blocks_fixed(data, bs, hot_path=True)
    allp = make_patterns(data, SIZES[-1])
    t, seen = {}, {}
    with kolm.open_container(blob, ctx) as rd:
        sets = {k: kolm.PatternSet(allp[:k], ctx) for k in SIZES}
        for k in (16, 256):  # the two routes agree
            assert rd.find_set(sets[k]) == chunked(rd, allp[:k], None)[0]
        for it in range(args.warmup + args.runs):
            row = {}
            for k in SIZES:
                for key, fn in ((f"find_set_{k}", lambda: rd.find_set(sets[k])), (f"count_set_{k}", lambda: rd.count_set(sets[k]))):
                    t0 = time.perf_counter()
                    got = fn()
                    row[f"{key}_wall"] = 1e3 * (time.perf_counter() - t0)
                    st = kolm.last_find()
                    row[f"{key}_ms_find"], row[f"{key}_ms_decode"] = st["ms_find"], st["ms_decode"]
                    seen[f"{key}_matches"], seen[f"{key}_emit_launches"] = st["matches"], st["emit_launches"]
                    seen[f"{key}_blocks_decoded"] = st["blocks_decoded"]
                    del got
                if k <= 256:
                    t0 = time.perf_counter()
                    _, f, d = chunked(rd, allp[:k], None)
                    row[f"find_many_chunks_{k}_wall"] = 1e3 * (time.perf_counter() - t0)
                    row[f"find_many_chunks_{k}_ms_find"], row[f"find_many_chunks_{k}_ms_decode"] = f, d
            if it >= args.warmup:
                for key, v in row.items():
                    t.setdefault(key, []).append(v)
        info = {str(k): sets[k].info for k in SIZES}
        for s in sets.values():
            s.close()
    res = {k: stats(v) for k, v in t.items()}
    med = lambda k: res[k]["median_ms"]  # noqa: E731
    res.update(seen)
    res.update({"blocks": args.blocks, "block_size": bs, "runs": args.runs, "warmup": args.warmup, "bytes": n,
                "container_bytes": len(blob), "info": info,
                "find_set_16_over_find_many_16_ms_find": med("find_set_16_ms_find") / med("find_many_chunks_16_ms_find"),
                "find_set_256_over_find_many_chunks_256_ms_find": med("find_set_256_ms_find") / med("find_many_chunks_256_ms_find"),
                "find_set_256_over_find_many_chunks_256_wall": med("find_set_256_wall") / med("find_many_chunks_256_wall"),
                "count_set_65536_over_count_set_16_ms_find": med("count_set_65536_ms_find") / med("count_set_16_ms_find"),
                "find_set_4096_ms_find_over_ms_decode": med("find_set_4096_ms_find") / med("find_set_4096_ms_decode")})
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    print(json.dumps({k: v["median_ms"] for k, v in res.items() if isinstance(v, dict) and "median_ms" in v}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
