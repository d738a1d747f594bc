#!/usr/bin/env python3
"""Cost of the line index: counting delimiters, locating and reading lines, and grep over a container.

Expectation from the code, stated before any run: k_delim_count reads every byte once through the
loads of k_crc32, keeps no table in LDS and does a handful of integer operations per 16-byte word,
so it should take at most k_crc32's time over the same bytes; a line query decodes the one or two
blocks that hold its bounding delimiters, so its cost should be that decode plus a few launches.
The measured values stand beside that, whichever way they fall.

One process: `--blocks` x 1 MiB enwik_like blocks compressed with the hot-path candidates, one
Reader over the container with its line index attached, warm-ups and alternating timed rounds.
Measured per round:
  (a) k_delim_count over the resident text (kolm_delim_count_device: HIP events around the kernel),
      the same with the 4 KiB pieces' counts and their scan (kolm_delim_count_pieces_device), and
      k_crc32 over the same bytes (kolm_crc32_blocks_device);
  (b) ms_lines and ms_decode (kolm_lines_stats) of kolm.line_index_of, of read_lines(first, 100)
      and of line_of on the offsets Reader.find gives for a rare 12-byte and a frequent 3-byte
      pattern (round 15's patterns), with the blocks each decodes;
  (c) wall time of read_lines(first, 100) beside kolm.decompress + bytes.split, and of grep of the
      rare pattern beside Reader.find alone and beside decompress + bytes.find + split; the
      decodes of each step of grep (blocks of find, line_of, line_spans, read_many).
Every result is compared with the host's once.  Writes min / median / max to profiles/r17/lines.json
(--out).  The committed file also holds an "encode" case: the bench A/B of the parent commit against
this build with the switch off and on (bench.py runs), which this tool does not produce.

    python tools/lines_probe.py [--blocks 256] [--runs 5] [--warmup 2] [--first 1000000] [--out PATH]
"""
import argparse
import bisect
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
    ap.add_argument("--first", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r17", "lines.json"))
    args = ap.parse_args()
    bs, n = args.block_size, args.blocks * args.block_size
    ctx = _lib.device_ctx(_lib.ensure_init(0))
    data = b"".join(datagen.enwik_like(min(32 << 20, n - o), seed=1 + o // (32 << 20)) for o in range(0, n, 32 << 20))
    blob = kolm.compress_blocks_fixed(data, bs, hot_path=True)
    mid = n // 2 + 12345
    rare = data[mid:mid + 12]
    freq = Counter(data[i:i + 3] for i in range(1 << 18)).most_common(1)[0][0]
    want_rare, want_freq = host_find(data, rare), host_find(data, freq)
    lines = data.split(b"\n")
    pos = host_find(data, b"\n")
    first = min(args.first, max(0, len(lines) - 100))
    want_index = [data[o:o + bs].count(b"\n") for o in range(0, n, bs)]
    want_grep = [(k, lines[k]) for k in sorted({bisect.bisect_left(pos, o) for o in want_rare})]
    resident = _lib.DeviceBuffer(ctx, n + 64)
    resident.upload(data)
    bounds = list(range(0, n, bs)) + [n]
    t = {k: [] for k in ("count_kernel", "count_pieces_kernel", "crc32_kernel", "index_of_ms_lines", "index_of_ms_decode",
                         "read_lines_ms_lines", "read_lines_ms_decode", "line_of_rare_ms_lines", "line_of_rare_ms_decode",
                         "line_of_freq_ms_lines", "line_of_freq_ms_decode", "read_lines_wall", "decompress_wall",
                         "split_wall", "grep_rare_wall", "find_rare_wall", "host_find_rare_wall")}
    seen = {}
    index = kolm.line_index_of(blob)
    assert index.counts == want_index
    with kolm.open_container(blob, ctx, lines=index) as rd:
        assert rd.line_count() == len(lines)
        for it in range(args.warmup + args.runs):
            row = {}
            for key in (("count_kernel", "count_pieces_kernel", "crc32_kernel") if it % 2 == 0 else
                        ("crc32_kernel", "count_pieces_kernel", "count_kernel")):
                if key == "count_kernel":
                    got, row[key] = _lib.delim_count_device(ctx, resident.ptr, bounds, 10)
                    assert got == want_index
                elif key == "count_pieces_kernel":
                    got, _, row[key] = _lib.delim_count_pieces_device(ctx, resident.ptr, bounds, 10)
                    assert got == want_index
                else:
                    row[key] = _lib.crc32_blocks_device(ctx, resident.ptr, bounds)[1]
            assert kolm.line_index_of(blob) == index
            st = kolm.last_lines()
            row["index_of_ms_lines"], row["index_of_ms_decode"] = st["ms_lines"], st["ms_decode"]
            seen["index_of_blocks_decoded"] = st["blocks_decoded"]
            t0 = time.perf_counter()
            got = rd.read_lines(first, 100)
            row["read_lines_wall"] = 1e3 * (time.perf_counter() - t0)
            assert got == lines[first:first + 100]
            st = kolm.last_lines()
            row["read_lines_ms_lines"], row["read_lines_ms_decode"] = st["ms_lines"], st["ms_decode"]
            seen["read_lines_blocks_decoded_spans"] = st["blocks_decoded"]
            seen["read_lines_blocks_decoded_read"] = kolm.last_read()["blocks_decoded"]
            for key, offs in (("line_of_rare", want_rare), ("line_of_freq", want_freq)):
                got = rd.line_of(offs)
                st = kolm.last_lines()
                row[f"{key}_ms_lines"], row[f"{key}_ms_decode"] = st["ms_lines"], st["ms_decode"]
                seen[f"{key}_queries"], seen[f"{key}_blocks_decoded"] = st["queries"], st["blocks_decoded"]
                if it == 0:
                    assert got == [bisect.bisect_left(pos, o) for o in offs]
                del got
            t0 = time.perf_counter()
            got = rd.grep(rare)
            row["grep_rare_wall"] = 1e3 * (time.perf_counter() - t0)
            assert got == want_grep
            seen["grep_rare_lines"] = len(got)
            seen["grep_rare_blocks_decoded"] = {"find": kolm.last_find()["blocks_decoded"],
                                                "line_spans": kolm.last_lines()["blocks_decoded"],
                                                "read_many": kolm.last_read()["blocks_decoded"]}
            rd.line_of(want_rare)
            seen["grep_rare_blocks_decoded"]["line_of"] = kolm.last_lines()["blocks_decoded"]
            t0 = time.perf_counter()
            assert rd.find(rare) == want_rare
            row["find_rare_wall"] = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            whole = kolm.decompress(blob)
            row["decompress_wall"] = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            sp = whole.split(b"\n")
            row["split_wall"] = 1e3 * (time.perf_counter() - t0)
            assert sp[first:first + 100] == lines[first:first + 100]
            t0 = time.perf_counter()
            assert host_find(whole, rare) == want_rare
            row["host_find_rare_wall"] = 1e3 * (time.perf_counter() - t0)
            del whole, sp
            if it >= args.warmup:
                for k, v in row.items():
                    t[k].append(v)
    resident.free()
    res = {k: stats(v) for k, v in t.items()}
    med = lambda k: res[k]["median_ms"]  # noqa: E731
    res.update(seen)
    res.update({"blocks": args.blocks, "block_size": bs, "runs": args.runs, "warmup": args.warmup, "bytes": n,
                "container_bytes": len(blob), "lines": len(lines), "first": first, "rare_pattern": rare.decode("latin-1"),
                "freq_pattern": freq.decode("latin-1"), "rare_matches": len(want_rare), "freq_matches": len(want_freq),
                "count_kernel_tb_per_s": n / 1e9 / med("count_kernel"),
                "count_pieces_kernel_tb_per_s": n / 1e9 / med("count_pieces_kernel"),
                "crc32_kernel_tb_per_s": n / 1e9 / med("crc32_kernel"),
                "count_over_crc32": med("count_kernel") / med("crc32_kernel"),
                "index_of_lines_over_decode": med("index_of_ms_lines") / med("index_of_ms_decode"),
                "host_over_read_lines_wall": (med("decompress_wall") + med("split_wall")) / med("read_lines_wall"),
                "grep_over_find_wall": med("grep_rare_wall") / med("find_rare_wall"),
                "host_over_grep_wall": (med("decompress_wall") + med("host_find_rare_wall") + med("split_wall")) / med("grep_rare_wall")})
    print(json.dumps({k: v for k, v in res.items() if not isinstance(v, dict) or k == "grep_rare_blocks_decoded"}))
    print(json.dumps({k: v["median_ms"] for k, v in res.items() if isinstance(v, dict) and "median_ms" in v}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
