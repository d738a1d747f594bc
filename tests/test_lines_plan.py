"""The host side of the line index (no device): kolm_lines_locate and kolm_lines_locate_offsets
(csrc/kolm_lines.cpp) against bisect over prefix sums computed here, the LineIndex sidecar
(kolm/lines.py) with every rejection of from_bytes, and the ctypes layout of kolm_lines_stats
against include/kolm.h."""
import bisect
import ctypes
import itertools
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from kolm import _lib
from kolm.lines import KolmLineIndexError, LineIndex, as_line_index, delim_byte

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kolm.h")

# zero-delimiter blocks at the front, in the middle and at the end; a single block; all zero
COUNTS = {"front": [0, 0, 3, 1, 2], "middle": [2, 0, 0, 5, 0, 1], "end": [4, 1, 0, 0], "single": [7], "one": [1],
          "mixed": [0, 1, 0, 0, 9, 0, 2, 0], "big": [0xFFFFFFFF, 0, 0xFFFFFFFF, 5]}


def prefix(counts):
    return [0] + list(itertools.accumulate(counts))


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_locate_against_bisect(name):
    counts = COUNTS[name]
    pre = prefix(counts)
    D = pre[-1]
    idx = sorted(set(list(range(min(D, 40))) + [D - 1, D // 2] + [p for p in pre[:-1] if p < D] + [p - 1 for p in pre if p > 0]))
    idx = idx + idx[::-1]  # any order, repeats
    want = []
    for k in idx:
        b = bisect.bisect_right(pre, k) - 1
        assert counts[b] > 0 and pre[b] <= k < pre[b + 1]  # never a block without delimiters
        want.append((b, k - pre[b]))
    assert _lib.lines_locate(counts, idx) == want
    assert _lib.lines_locate(counts, []) == []
    for bad in ([D], [0, D + 5], [1 << 63]):
        with pytest.raises(ValueError, match=f"entry {len(bad) - 1}"):
            _lib.lines_locate(counts, bad)


def test_locate_nothing_to_find():
    for counts in ([], [0], [0, 0, 0]):
        assert _lib.lines_locate(counts, []) == []
        with pytest.raises(ValueError, match="entry 0"):
            _lib.lines_locate(counts, [0])


@pytest.mark.parametrize("lens,counts", [
    ([5, 0, 5], [1, 0, 2]),                    # an empty block in the middle
    ([0, 0, 4, 1], [0, 0, 0, 1]),              # empty blocks at the front
    ([3, 2, 0, 0], [3, 0, 0, 0]),              # ... at the end
    ([9], [4]),                                # a single block
    ([0], [0]), ([], []),                      # nothing at all
    ([1000, 4096, 4097, 1, 8193], [10, 0, 4097, 1, 0]),
])
def test_locate_offsets_against_bisect(lens, counts):
    starts, pre = prefix(lens), prefix(counts)
    total = starts[-1]
    offs = sorted(set(list(range(min(total, 30))) + starts + [s - 1 for s in starts if s > 0] + [total, total // 2]))
    offs = offs[::-1] + offs
    want = []
    for o in offs:
        if o == total:
            b = len(lens)
        else:
            b = bisect.bisect_right(starts, o) - 1
            assert lens[b] > 0 and starts[b] <= o < starts[b + 1]  # never an empty block
        want.append((b, o - starts[b], pre[b]))
    assert _lib.lines_locate_offsets(lens, counts, offs) == want
    with pytest.raises(ValueError, match="entry 1"):
        _lib.lines_locate_offsets(lens, counts, [0, total + 1])


def test_line_index_round_trip():
    blocks = [b"a\nb\n", b"", b"no delimiter", b"\n\n\n", b"tail"]
    for delim in (b"\n", b"\0", 0xFF, b"a"):
        li = LineIndex.of_blocks(1, 2048, blocks, delim)
        d = bytes([delim_byte(delim)])
        assert li.counts == [b.count(d) for b in blocks] and li.lens == [len(b) for b in blocks]
        assert li.delimiters == b"".join(blocks).count(d) and li.nlines == len(b"".join(blocks).split(d))
        blob = li.to_bytes()
        assert blob[:4] == b"KOLL" and len(blob) == 24 + 8 * len(blocks) + 4
        assert struct.unpack_from("<BBBBIQI", blob, 4) == (1, 1, d[0], 0, 2048, sum(len(b) for b in blocks), len(blocks))
        back = LineIndex.from_bytes(blob)
        assert back == li and as_line_index(blob) == li and as_line_index(li) is li
        assert back != LineIndex.of_blocks(1, 2048, blocks, d[0] ^ 1)
    empty = LineIndex(0, 4096, 0, [], b"\n", [])
    assert empty.nlines == 1 and LineIndex.from_bytes(empty.to_bytes()) == empty
    assert "expected 3 delimiters, got 2" in str(KolmLineIndexError(5, 3, 2)) and KolmLineIndexError(5, 3, 2).block == 5


def reseal(body: bytes) -> bytes:
    return body + struct.pack("<I", zlib.crc32(body))


def test_from_bytes_rejections():
    li = LineIndex.of_blocks(0, 1000, [b"x\n" * 500, b"y\n" * 100], b"\n")
    blob = li.to_bytes()
    body = blob[:-4]
    cases = [
        ("bad magic", reseal(b"KOLS" + body[4:])),
        ("unsupported version 2", reseal(body[:4] + b"\x02" + body[5:])),
        ("unsupported version 1", reseal(body[:7] + b"\x01" + body[8:])),  # the zero byte
        ("too short", blob[:20]),
        ("sidecar of", blob + b"\0"),
        ("sidecar of", reseal(body[:-8])),  # one block's pair missing: the count field says two
        ("own CRC-32", blob[:30] + bytes([blob[30] ^ 1]) + blob[31:]),
        ("own CRC-32", blob[:-1] + bytes([blob[-1] ^ 0x80])),
        ("add up to", reseal(body[:12] + struct.pack("<Q", li.total_len + 1) + body[20:])),  # sum of lens
        ("cannot hold", reseal(body[:-4] + struct.pack("<I", 201))),  # more delimiters than bytes
    ]
    for text, bad in cases:
        with pytest.raises(ValueError, match=text):
            LineIndex.from_bytes(bad)
    with pytest.raises(ValueError, match="one count per block"):
        LineIndex(0, 1000, 5, [5], b"\n", [])
    for bad in (b"", b"ab", 256, -1):
        with pytest.raises(ValueError, match="one byte"):
            delim_byte(bad)


def test_lines_stats_layout_matches_header(tmp_path):
    assert ctypes.sizeof(_lib.LinesStats) == 4 * 4 + 8 + 2 * 8
    fields = [f for f, _ in _lib.LinesStats._fields_]
    assert set(fields) == {"queries", "blocks_decoded", "groups", "reserved", "bytes_decoded", "ms_decode", "ms_lines"}
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kolm.h"\nint main(void){printf("%zu %d'
                   + "".join(" %zu" for _ in fields) + '\\n", sizeof(kolm_lines_stats), KOLM_ELINES'
                   + "".join(f", offsetof(kolm_lines_stats, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.LinesStats)
    assert got[1] == _lib.KOLM_ELINES == -10
    assert got[2:] == [getattr(_lib.LinesStats, f).offset for f in fields]
