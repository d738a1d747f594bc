#!/usr/bin/env python3
"""Cost of a class-pattern search of a container on the device (Reader.find_classes /
count_classes, the ignore_case searches) against the literal search, against the decode of the same
blocks and against kolm.decompress plus Python's re on the host.

Expectation from the code, stated before any run: k_findcls_count forms the same 16 windows per
thread as k_find_count and filters every position with the same masked 64-bit compare, so a
pattern whose first 8 classes are masked equalities (a literal, an ignore_case word) should cost
what the literal search costs plus the larger LDS image of the patterns (T and the rows: up to
10.6 KiB a workgroup against 4.4 KiB), a few percent of the decode.  \\d{4}-\\d{2}-\\d{2} has
table classes at 6 of its first 8 positions; the filter sees their hulls ((b & 0xF0) == 0x30) and
the two '-', so only positions that look like DDDD-DD- up to the hull reach the table; on text
few do, and the cost should stay near the literal's.  Sixteen patterns cost sixteen compares per
position, as in the literal search.  The measured values stand beside that, whichever way they fall.

One process: `--blocks` x 1 MiB enwik_like blocks (dates planted every 64 KiB) compressed with the
hot-path candidates, one Reader over the container, warm-ups and alternating timed rounds.  Per
round ms_find and ms_decode (kolm_find_stats) of
  1. count of the rare 12-byte literal, and count_classes of the same literal as classes;
  2. count of one 8-letter word under ignore_case;
  3. count_classes of \\d{4}-\\d{2}-\\d{2} (the positions that pass its filter are counted on the host);
  4. count_many of 16 words under ignore_case;
  5. find_classes listing the matches of 2 and 3, with its wall time, beside the wall time of
     kolm.decompress plus re.finditer over the result for the same two patterns.
Every result is compared with re once.  Writes min / median / max to profiles/r19/findcls.json (--out).

    python tools/findcls_probe.py [--blocks 256] [--runs 5] [--warmup 2] [--out PATH]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "kolmogorovlike-datacompressor_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import kolm  # noqa: E402
from kolm import _lib, classes, datagen  # noqa: E402
from verify_probe import stats  # noqa: E402

DATE = rb"\d{4}-\d{2}-\d{2}"


def host_re(data, expr, flags=0):
    return [m.start() for m in re.finditer(b"(?=(" + expr + b"))", data, re.DOTALL | flags)]


def filter_passes(data, pat):
    """Positions whose 8-byte window passes the candidate filter of `pat`: the hulls of its first
    min(len, 8) classes (findcls_core.h)."""
    a = np.frombuffer(data, np.uint8)
    n = len(a) - len(pat) + 1
    ok = np.ones(n, bool)
    for k, c in enumerate(pat.classes[:8]):
        v, o = 0xFF, 0
        for b in c:
            v, o = v & b, o | b
        mask = ~(o ^ v) & 0xFF
        if mask:
            ok &= (a[k:k + n] & mask) == v
    return int(ok.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-size", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r19", "findcls.json"))
    args = ap.parse_args()
    bs, n = args.block_size, args.blocks * args.block_size
    ctx = _lib.device_ctx(_lib.ensure_init(0))
    d = bytearray(b"".join(datagen.enwik_like(min(32 << 20, n - o), seed=1 + o // (32 << 20)) for o in range(0, n, 32 << 20)))
    for k, o in enumerate(range(40_000, n - 10, 65_521)):
        d[o:o + 10] = b"%04d-%02d-%02d" % (1970 + k % 80, 1 + k % 12, 1 + k % 28)
    data = bytes(d)
    del d
    blob = kolm.compress_blocks_fixed(data, bs, hot_path=True)
    mid = n // 2 + 12345
    rare = data[mid:mid + 12]
    words = [w for w in dict.fromkeys(re.findall(rb"[a-z]{8}", data[:1 << 20]))][:16]
    word = words[0]
    rare_cls, date = classes.ClassPattern.literal(rare), classes.compile(DATE)
    want_word, want_date = host_re(data, word, re.IGNORECASE), host_re(data, DATE)
    want_rare = host_re(data, re.escape(rare))
    keys = ("count_rare", "count_rare_classes", "count_word_ic", "count_date", "count_16_ic", "find_word_ic", "find_date")
    t = {f"{k}_{w}": [] for k in keys for w in ("ms_find", "ms_decode")}
    t.update({k: [] for k in ("find_word_ic_wall", "find_date_wall", "decompress_wall", "host_re_word_ic_wall",
                              "host_re_date_wall")})
    seen = {}
    with kolm.open_container(blob, ctx) as rd:
        for it in range(args.warmup + args.runs):
            row = {}
            for key, fn in (("count_rare", lambda: rd.count(rare)), ("count_rare_classes", lambda: rd.count_classes(rare_cls)[0]),
                            ("count_word_ic", lambda: rd.count(word, ignore_case=True)),
                            ("count_date", lambda: rd.count_classes(date)[0]),
                            ("count_16_ic", lambda: rd.count_many(words, ignore_case=True)),
                            ("find_word_ic", lambda: rd.find(word, ignore_case=True)),
                            ("find_date", lambda: [o for o, _ in rd.find_classes(date)])):
                t0 = time.perf_counter()
                got = fn()
                wall = 1e3 * (time.perf_counter() - t0)
                st = kolm.last_find()
                row[f"{key}_ms_find"], row[f"{key}_ms_decode"] = st["ms_find"], st["ms_decode"]
                if key.startswith("find_"):
                    row[f"{key}_wall"] = wall
                    assert got == (want_word if key == "find_word_ic" else want_date)
                elif key in ("count_rare", "count_rare_classes"):
                    assert got == len(want_rare)
                seen[f"{key}_matches"], seen[f"{key}_emit_launches"] = st["matches"], st["emit_launches"]
                del got
            assert seen["count_word_ic_matches"] == len(want_word) and seen["count_date_matches"] == len(want_date)
            if it >= args.warmup:  # the host path: decode everything, copy it out, then re
                t0 = time.perf_counter()
                whole = kolm.decompress(blob)
                row["decompress_wall"] = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                assert host_re(whole, word, re.IGNORECASE) == want_word
                row["host_re_word_ic_wall"] = 1e3 * (time.perf_counter() - t0)
                t0 = time.perf_counter()
                assert host_re(whole, DATE) == want_date
                row["host_re_date_wall"] = 1e3 * (time.perf_counter() - t0)
                del whole
                for k, v in row.items():
                    t[k].append(v)
            print(f"round {it + 1} of {args.warmup + args.runs}", flush=True)
    res = {k: stats(v) for k, v in t.items()}
    med = lambda k: res[k]["median_ms"]  # noqa: E731
    res.update(seen)
    res.update({"blocks": args.blocks, "block_size": bs, "runs": args.runs, "warmup": args.warmup,
                "container_bytes": len(blob), "bytes": n, "rare_pattern": rare.decode("latin-1"),
                "word": word.decode(), "words_16": [w.decode() for w in words], "date_expression": DATE.decode(),
                "date_filter_passes": filter_passes(data, date), "date_table_classes": classes.table_classes([date]),
                "classes_over_literal_rare": med("count_rare_classes_ms_find") / med("count_rare_ms_find"),
                "count_word_ic_over_decode": med("count_word_ic_ms_find") / med("count_word_ic_ms_decode"),
                "count_date_over_decode": med("count_date_ms_find") / med("count_date_ms_decode"),
                "count_16_ic_over_decode": med("count_16_ic_ms_find") / med("count_16_ic_ms_decode"),
                "host_over_find_word_ic_wall": (med("decompress_wall") + med("host_re_word_ic_wall")) / med("find_word_ic_wall"),
                "host_over_find_date_wall": (med("decompress_wall") + med("host_re_date_wall")) / med("find_date_wall")})
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict)}))
    print(json.dumps({k: v["median_ms"] for k, v in res.items() if isinstance(v, dict)}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
