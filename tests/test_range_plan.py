"""kolm_range_plan (csrc/kolm_range.cpp: host only, no device) against a brute-force restatement:
for every range the set of blocks that overlap it, computed here block by block.  The plan's
groups, payload runs and copy segments are then replayed on a byte stream in numpy: the groups'
decoded scratch is rebuilt from the stream, the segments are copied, and the result must be the
ranges' slices back to back, every output byte written exactly once.  Block lengths: the golden
fixed and CDC containers' TOCs and synthetic lists (1-byte blocks, equal blocks, a short last
block).  Second: the ctypes layout of kolm_read_stats against include/kolm.h (CPU)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kolm
from kolm import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kolm.h")
GOLDEN = os.path.join(REPO, "tests", "golden")
UNLIMITED = (1 << 31) - 1


def block_lists(golden_containers):
    out = {"ones": [1] * 40, "equal": [1000] * 7, "short_last": [1000] * 6 + [123], "tiny_mix": [1, 1, 5, 1, 16, 1, 40],
           "single": [77]}
    for z, names in ((golden_containers, ("mix_b1000/full", "mix_b1000/ids0_8")),
                     (np.load(os.path.join(GOLDEN, "cdc.npz")), None)):
        for k in (names or [k for k in z.keys() if k.endswith("/full")]):
            out[k] = list(kolm.read_container(z[k].tobytes())[4])
    return out


def make_ranges(lens, seed):
    total = sum(lens)
    starts = np.concatenate(([0], np.cumsum(lens))).tolist()
    edges = starts[1:-1]
    r = [(0, 0), (total, 0), (0, total), (total - 1, 1), (0, 1)]
    if edges:
        e1 = edges[0]
        r += [(e1, 0), (e1 - 1, 2), (e1, total - e1)]                  # empty at an edge; one edge; to the end
        r += [(e1 - 1, 2), (max(e1 - 3, 0), min(7, total - max(e1 - 3, 0)))]  # a duplicate, an overlap
    if len(edges) >= 2:
        r.append((edges[0] - 1, edges[1] - edges[0] + 2))                # two edges
        r.append((edges[0] - 1, edges[-1] - edges[0] + 2))               # every edge
    rng = np.random.default_rng(seed)
    for _ in range(200):
        o = int(rng.integers(0, total + 1))
        n = int(rng.integers(0, min(total - o, 3 * max(lens)) + 1))
        r.append((o, n))
    return r


def brute_selected(lens, ranges):
    sel, pos = set(), 0
    for b, n in enumerate(lens):
        for o, m in ranges:
            if max(o, pos) < min(o + m, pos + n):  # a non-empty intersection
                sel.add(b)
                break
        pos += n
    return sorted(sel)


def check_plan(lens, ranges, limit):
    total = sum(lens)
    starts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    p = _lib.range_plan(lens, ranges, limit)
    assert p["sel"] == brute_selected(lens, ranges)
    # groups: consecutive selected blocks, at or under the limit unless single, filled greedily
    assert [b for g in p["groups"] for b in g] == p["sel"]
    gbytes = [sum(lens[b] for b in g) for g in p["groups"]]
    for gi, g in enumerate(p["groups"]):
        assert g and (gbytes[gi] <= limit or len(g) == 1)
        if gi:
            assert gbytes[gi - 1] + lens[g[0]] > limit
    # runs: blocks consecutive in the container, inside one group, as long as possible
    assert [b for r in p["runs"] for b in r] == p["sel"]
    gof = {b: gi for gi, g in enumerate(p["groups"]) for b in g}
    for ri, r in enumerate(p["runs"]):
        assert r == list(range(r[0], r[0] + len(r))) and len({gof[b] for b in r}) == 1
        if ri:
            prev = p["runs"][ri - 1]
            assert prev[-1] + 1 != r[0] or gof[prev[-1]] != gof[r[0]]
    # the copy segments replayed on a stream: scratch = the group's blocks back to back
    stream = ((np.arange(total, dtype=np.int64) * 2654435761) >> 7 & 0xFF).astype(np.uint8)
    want = np.concatenate([stream[o:o + n] for o, n in ranges]) if ranges else np.zeros(0, np.uint8)
    got = np.zeros(len(want), np.uint8)
    hits = np.zeros(len(want), np.int32)
    assert len(p["segs"]) == len(p["groups"])
    for g, segs in zip(p["groups"], p["segs"]):
        scratch = np.concatenate([stream[starts[b]:starts[b + 1]] for b in g])
        last = -1
        for s, d, n in segs:
            assert n > 0 and s + n <= len(scratch) and d + n <= len(want)
            assert d > last  # request order within the group
            last = d
            got[d:d + n] = scratch[s:s + n]
            hits[d:d + n] += 1
    assert (hits == 1).all()  # the segments tile every non-empty range exactly once
    assert (got == want).all()
    # a range has one segment per group it has bytes in
    nseg = sum(len(s) for s in p["segs"])
    assert nseg == sum(len({gof[b] for b in brute_selected(lens, [r])}) for r in ranges)


def test_plan_against_brute_force(golden_containers):
    lists = block_lists(golden_containers)
    assert any(k.startswith("c_") for k in lists) and "mix_b1000/full" in lists
    for seed, (name, lens) in enumerate(sorted(lists.items())):
        if not lens:  # the container of an empty input: only empty ranges at 0 exist
            check_plan(lens, [(0, 0), (0, 0)], 1)
            with pytest.raises(ValueError):
                _lib.range_plan(lens, [(0, 1)])
            continue
        ranges = make_ranges(lens, seed)
        for limit in (1, max(lens), UNLIMITED):
            check_plan(lens, ranges, limit)
        check_plan(lens, [], UNLIMITED)
        check_plan(lens, [(0, 0), (sum(lens), 0)], 1)


def test_default_limit_and_environment(monkeypatch):
    lens = [1000] * 8
    whole = [(0, 8000)]
    monkeypatch.delenv("KOLM_READ_BYTES", raising=False)
    assert len(_lib.range_plan(lens, whole)["groups"]) == 1       # 1 GiB
    monkeypatch.setenv("KOLM_READ_BYTES", "2500")                 # read per call
    p = _lib.range_plan(lens, whole)
    assert [len(g) for g in p["groups"]] == [2, 2, 2, 2] and [len(s) for s in p["segs"]] == [1, 1, 1, 1]
    assert len(_lib.range_plan(lens, whole, 8000)["groups"]) == 1  # an explicit limit wins
    monkeypatch.setenv("KOLM_READ_BYTES", str(1 << 40))            # capped at 2^31 - 1
    assert len(_lib.range_plan([1 << 30] * 3, [(0, 3 << 30)])["groups"]) == 3


def test_ranges_outside_the_data_are_refused():
    lens = [100, 100, 50]
    for bad in ((200, 51), (251, 0), (0, 251), (1 << 63, 1 << 63)):
        with pytest.raises(ValueError) as e:
            _lib.range_plan(lens, [(0, 10), (5, 0), bad, (300, 1)])
        assert "range 2" in str(e.value)
    assert _lib.range_plan(lens, [(250, 0), (0, 250)])["sel"] == [0, 1, 2]


def test_capacity_query_fills_the_counts():
    L = _lib.load()
    lens = np.asarray([10, 10, 10, 10], np.uint32)
    offs = np.asarray([5, 35], np.uint64)
    ns = np.asarray([10, 2], np.uint64)
    counts = np.zeros(4, np.uint64)
    rc = L.kolm_range_plan(lens.ctypes.data, 4, offs.ctypes.data, ns.ctypes.data, 2, 0, None, None, None, None, None,
                           None, counts.ctypes.data)
    assert rc == _lib.KOLM_ECAP and counts.tolist() == [3, 1, 2, 2]  # blocks 0, 1, 3; one group; two runs
    caps = np.asarray([3, 1, 1, 2], np.uint64)  # one run too few
    bufs = [np.zeros(8, np.uint32) for _ in range(4)]
    segs = np.zeros(3 * 4, np.uint64)
    rc = L.kolm_range_plan(lens.ctypes.data, 4, offs.ctypes.data, ns.ctypes.data, 2, 0, *[b.ctypes.data for b in bufs],
                           segs.ctypes.data, caps.ctypes.data, counts.ctypes.data)
    assert rc == _lib.KOLM_ECAP and counts.tolist() == [3, 1, 2, 2]


def test_read_stats_layout_matches_header(tmp_path):
    assert ctypes.sizeof(_lib.ReadStats) == 4 * 4 + 2 * 8 + 2 * 8
    fields = [f for f, _ in _lib.ReadStats._fields_]
    assert set(fields) == {"ranges", "bytes_returned", "blocks_decoded", "bytes_decoded", "groups", "compactions",
                           "ms_decode", "ms_gather"}
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kolm.h"\nint main(void){printf("%zu %zu'
                   + "".join(" %zu" for _ in fields) + '\\n", sizeof(kolm_range_seg), sizeof(kolm_read_stats)'
                   + "".join(f", offsetof(kolm_read_stats, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.RangeSeg) == 24
    assert got[1] == ctypes.sizeof(_lib.ReadStats)
    assert got[2:] == [getattr(_lib.ReadStats, f).offset for f in fields]
