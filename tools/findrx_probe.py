#!/usr/bin/env python3
"""Cost of a regular-expression search of a container on the device (Reader.find_regex /
count_regex) against the class-pattern search of the same expression, against the decode of the
same blocks and against kolm.decompress plus Python's re on the host.

Expectation from the code, stated before any run: k_findrx_count reads the buffer once, like
k_findcls_count (0.30 ms over 256 MiB in profiles/r19/findcls.json, most of it the read), and adds
per tile the copy of the table and the map into LDS (a few hundred bytes to a few KiB from L2) and
the translation of 273 words to class ids (4 368 LDS byte reads a tile).  Per position and
expression it then pays two dependent LDS reads (the class id, the table entry) where the class
kernel pays one masked 64-bit compare in registers, and on text nearly every walk ends there.  The
class-id reads of a wave are 16 bytes apart (a 4-way bank conflict).  So one expression should land
between 1 and 3 times k_findcls_count, a frequent expression whose walks run 10 to 20 steps
([A-Z][a-z]+ [A-Z][a-z]+ walks only from capitals, about 2 % of text) little above a rare one, and 16
expressions near 16 times the walking part of one: 2 to 6 ms, still under a quarter of the decode
(about 25 ms).  The date expression as a Regex should cost what any single expression costs,
above count_classes of it by the two LDS reads.  End to end the device call should stay near the
decode's 25 ms against 2 s or more for decompress plus re.  The measured values stand beside
that, whichever way they fall.

One process: `--blocks` x 1 MiB enwik_like blocks (dates planted every 64 KiB, as in round 19)
compressed with the hot-path candidates, one Reader over the container, warm-ups and alternating
timed rounds.  Per round ms_find and ms_decode (kolm_find_stats) of count_regex and find_regex of
  rare      ERROR|WARN(ING)?|kolmogorov
  frequent  [A-Z][a-z]+ [A-Z][a-z]+
  sixteen   16 expressions (the two above, the date, words, numbers, punctuation); find_regex lists
            the first million of their matches
  date      \\d{4}-\\d{2}-\\d{2}, next to count_classes of it in the same round
with the wall time of every find_regex, beside the wall time of kolm.decompress plus re.finditer over
the result for rare, frequent and date.  Every result is compared with re once.  Writes min / median
/ max to profiles/r20/findrx.json (--out).

    python tools/findrx_probe.py [--blocks 256] [--runs 3] [--warmup 1] [--out PATH]
"""
import argparse
import json
import os
import re
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "kolmogorovlike-datacompressor_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import kolm  # noqa: E402
from kolm import _lib, classes, datagen, regex  # noqa: E402
from verify_probe import stats  # noqa: E402

DATE = rb"\d{4}-\d{2}-\d{2}"
RARE = rb"ERROR|WARN(ING)?|kolmogorov"
FREQUENT = rb"[A-Z][a-z]+ [A-Z][a-z]+"
SIXTEEN = [RARE, FREQUENT, DATE, rb"https?://[^ ]+", rb"\d{1,3}(\.\d{1,3}){3}", rb"[a-z0-9._]+@[a-z]+\.(com|org)", rb"t(he|o) ",
           rb"(in|on|at) [a-z]+", rb"\d+", rb"[.,;]+ [A-Z]", rb"e{2,}|o{2,}", rb"qu?", rb"[a-z]+ing ", rb"[^a-z ]{3,}",
           rb"[Cc]ompress(ion|ed)?", rb"\n\n+"]


LIST_16 = 1_000_000  # the 16 expressions match tens of millions of starts: this many are listed


def host_re(data, expr):
    """Every start with a match (all expressions here have witnesses far below 256 bytes on this text)."""
    return [m.start() for m in re.finditer(b"(?=(" + expr + b"))", data, re.DOTALL)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--block-size", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r20", "findrx.json"))
    args = ap.parse_args()
    bs, n = args.block_size, args.blocks * args.block_size
    ctx = _lib.device_ctx(_lib.ensure_init(0))
    d = bytearray(b"".join(datagen.enwik_like(min(32 << 20, n - o), seed=1 + o // (32 << 20)) for o in range(0, n, 32 << 20)))
    for k, o in enumerate(range(40_000, n - 10, 65_521)):
        d[o:o + 10] = b"%04d-%02d-%02d" % (1970 + k % 80, 1 + k % 12, 1 + k % 28)
    for k, o in enumerate(range(90_000, n - 10, 1_048_573 * 3)):
        d[o:o + 7] = (b"ERROR  ", b"WARNING", b"WARN   ")[k % 3]
    data = bytes(d)
    del d
    blob = kolm.compress_blocks_fixed(data, bs, hot_path=True)
    rx = {"rare": [regex.compile(RARE)], "frequent": [regex.compile(FREQUENT)], "sixteen": [regex.compile(e) for e in SIXTEEN],
          "date": [regex.compile(DATE)]}
    date_cls = classes.compile(DATE)
    want = {"rare": host_re(data, RARE), "frequent": host_re(data, FREQUENT), "date": host_re(data, DATE)}
    want16 = [len(host_re(data, e)) for e in SIXTEEN]
    tables = {k: regex.table(v) for k, v in rx.items()}
    t = {f"{op}_{k}_{w}": [] for op in ("count", "find") for k in rx for w in ("ms_find", "ms_decode")}
    t.update({f"find_{k}_wall": [] for k in rx})
    t.update({k: [] for k in ("count_classes_date_ms_find", "count_classes_date_ms_decode", "decompress_wall",
                              "host_re_rare_wall", "host_re_frequent_wall", "host_re_date_wall")})
    seen = {}
    with kolm.open_container(blob, ctx) as rd:
        for it in range(args.warmup + args.runs):
            row = {}
            for k, r in rx.items():
                got = rd.count_regex(r)
                st = kolm.last_find()
                row[f"count_{k}_ms_find"], row[f"count_{k}_ms_decode"] = st["ms_find"], st["ms_decode"]
                assert got == (want16 if k == "sixteen" else [len(want[k])]), (k, got)
                if k == "date":  # the class kernel on the same expression, in the same round
                    assert rd.count_classes(date_cls) == got
                    st = kolm.last_find()
                    row["count_classes_date_ms_find"], row["count_classes_date_ms_decode"] = st["ms_find"], st["ms_decode"]
                t0 = time.perf_counter()
                got = rd.find_regex(r, limit=LIST_16 if k == "sixteen" else None)
                row[f"find_{k}_wall"] = 1e3 * (time.perf_counter() - t0)
                st = kolm.last_find()
                row[f"find_{k}_ms_find"], row[f"find_{k}_ms_decode"] = st["ms_find"], st["ms_decode"]
                seen[f"{k}_matches"], seen[f"{k}_emit_launches"] = st["matches"], st["emit_launches"]
                if k != "sixteen":
                    assert [o for o, _ in got] == want[k], k
                else:
                    assert len(got) == min(LIST_16, sum(want16))
                del got
            if it >= args.warmup:  # the host path: decode everything, copy it out, then re
                t0 = time.perf_counter()
                whole = kolm.decompress(blob)
                row["decompress_wall"] = 1e3 * (time.perf_counter() - t0)
                for k, e in (("rare", RARE), ("frequent", FREQUENT), ("date", DATE)):
                    t0 = time.perf_counter()
                    assert host_re(whole, e) == want[k]
                    row[f"host_re_{k}_wall"] = 1e3 * (time.perf_counter() - t0)
                del whole
                for k, v in row.items():
                    t[k].append(v)
            print(f"round {it + 1} of {args.warmup + args.runs}", flush=True)
    res = {k: stats(v) for k, v in t.items()}
    med = lambda k: res[k]["median_ms"]  # noqa: E731
    res.update(seen)
    res.update({"blocks": args.blocks, "block_size": bs, "runs": args.runs, "warmup": args.warmup,
                "container_bytes": len(blob), "bytes": n, "expressions_16": [e.decode() for e in SIXTEEN],
                "table": {k: {"states": tb.nstates, "classes": tb.ncls, "entries": tb.entries} for k, tb in tables.items()},
                "regex_over_classes_date": med("count_date_ms_find") / med("count_classes_date_ms_find")})
    for k in rx:
        res[f"count_{k}_over_decode"] = med(f"count_{k}_ms_find") / med(f"count_{k}_ms_decode")
    for k in ("rare", "frequent", "date"):
        res[f"host_over_find_{k}_wall"] = (med("decompress_wall") + med(f"host_re_{k}_wall")) / med(f"find_{k}_wall")
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict) or k == "table"}))
    print(json.dumps({k: v["median_ms"] for k, v in res.items() if isinstance(v, dict) and k != "table"}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
