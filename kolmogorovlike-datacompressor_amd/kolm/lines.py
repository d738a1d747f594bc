"""Line index of a container's decoded bytes, kept beside it (not in PY).

The KOLR container speaks in byte offsets and does not change.  A ``LineIndex`` holds, for one
delimiter byte (default ``b"\\n"``), every block's count of bytes equal to it.  With it every line
question is block-local: delimiter number k lies in the one block a search of the counts' prefix
sums names, so only that block is decoded (kolm.open_container(..., lines=...): Reader.line_count,
line_spans, line_of, read_lines, grep).  Lines are ``data.split(delim)``: D + 1 lines for D
delimiters, delimiters belong to no line, empty lines exist, an empty stream has one empty line.
It travels as a small sidecar file, little-endian:

    b"KOLL" | u8 version (1) | u8 mode | u8 delim | u8 0 | u32 size_field | u64 total_len |
    u32 nblocks | nblocks x (u32 len, u32 count) | u32 CRC-32 of everything before it

Plain ``struct`` + ``zlib``: no device and no native library is involved here.  The encode entry
points fill an index on the device (``lines=True``; ``kolm.last_line_index()``), ``kolm.line_index``
counts a resident input and ``kolm.line_index_of`` an existing container.
"""
from __future__ import annotations

import struct
import zlib
from typing import List, Sequence

MAGIC = b"KOLL"
VERSION = 1
_HEAD = struct.Struct("<4sBBBBIQI")


def delim_byte(delim) -> int:
    """The delimiter as a byte value: an int 0..255 or a bytes-like of length one."""
    if isinstance(delim, int) and not isinstance(delim, bool):
        d = delim
    else:
        b = bytes(delim)
        if len(b) != 1:
            raise ValueError("the delimiter is one byte")
        d = b[0]
    if not 0 <= d <= 255:
        raise ValueError("the delimiter is one byte")
    return d


class KolmLineIndexError(ValueError):
    """The attached line index does not describe the decoded bytes: the block, the count the index
    holds and the count found.  No result is returned."""

    def __init__(self, block: int, expected: int, got: int):
        super().__init__(f"line index: block {block}: expected {expected} delimiters, got {got}")
        self.block, self.expected, self.got = block, expected, got


class LineIndex:
    """The index: mode / size_field / total_len as in the container's header, every block's length
    and its count of bytes equal to delim (an int 0..255)."""

    def __init__(self, mode: int, size_field: int, total_len: int, lens: Sequence[int], delim, counts: Sequence[int]):
        self.mode, self.size_field, self.total_len = int(mode), int(size_field), int(total_len)
        self.lens: List[int] = [int(n) for n in lens]
        self.delim = delim_byte(delim)
        self.counts: List[int] = [int(c) for c in counts]
        if len(self.lens) != len(self.counts):
            raise ValueError("line index: one count per block length")
        if sum(self.lens) != self.total_len:
            raise ValueError(f"line index: block lengths add up to {sum(self.lens)}, expect {self.total_len}")
        for i, (n, c) in enumerate(zip(self.lens, self.counts)):
            if not 0 <= c <= n:
                raise ValueError(f"line index: block {i} of {n} bytes cannot hold {c} delimiters")

    @property
    def delimiters(self) -> int:
        """D: the delimiters of the whole stream."""
        return sum(self.counts)

    @property
    def nlines(self) -> int:
        """D + 1: the lines of the whole stream (an empty stream has one empty line)."""
        return self.delimiters + 1

    @classmethod
    def of_blocks(cls, mode: int, size_field: int, blocks: Sequence[bytes], delim=b"\n") -> "LineIndex":
        """The index of the given original blocks, computed with bytes.count on the host."""
        d = bytes([delim_byte(delim)])
        return cls(mode, size_field, sum(len(b) for b in blocks), [len(b) for b in blocks], d,
                   [bytes(b).count(d) for b in blocks])

    def __eq__(self, other) -> bool:
        return isinstance(other, LineIndex) and (
            self.mode, self.size_field, self.total_len, self.lens, self.delim, self.counts) == (
            other.mode, other.size_field, other.total_len, other.lens, other.delim, other.counts)

    def __repr__(self) -> str:
        return (f"LineIndex(mode={self.mode}, size_field={self.size_field}, total_len={self.total_len}, "
                f"blocks={len(self.lens)}, delim=0x{self.delim:02x}, lines={self.nlines})")

    def to_bytes(self) -> bytes:
        body = _HEAD.pack(MAGIC, VERSION, self.mode, self.delim, 0, self.size_field, self.total_len, len(self.lens))
        body += b"".join(struct.pack("<II", n, c) for n, c in zip(self.lens, self.counts))
        return body + struct.pack("<I", zlib.crc32(body))

    @classmethod
    def from_bytes(cls, blob: bytes) -> "LineIndex":
        blob = bytes(blob)
        if len(blob) < _HEAD.size + 4:
            raise ValueError("line index: sidecar too short")
        magic, version, mode, delim, zero, size_field, total_len, nb = _HEAD.unpack_from(blob)
        if magic != MAGIC:
            raise ValueError("line index: bad magic")
        if version != VERSION or zero != 0:
            raise ValueError(f"line index: unsupported version {version}")
        if len(blob) != _HEAD.size + 8 * nb + 4:
            raise ValueError(f"line index: sidecar of {len(blob)} bytes, expect {_HEAD.size + 8 * nb + 4} for {nb} blocks")
        if struct.unpack_from("<I", blob, len(blob) - 4)[0] != zlib.crc32(blob[:-4]):
            raise ValueError("line index: the sidecar's own CRC-32 does not match")
        pairs = struct.unpack_from(f"<{2 * nb}I", blob, _HEAD.size)
        return cls(mode, size_field, total_len, pairs[0::2], delim, pairs[1::2])


def as_line_index(obj) -> LineIndex:
    """A LineIndex, or the sidecar bytes of one."""
    return obj if isinstance(obj, LineIndex) else LineIndex.from_bytes(obj)
