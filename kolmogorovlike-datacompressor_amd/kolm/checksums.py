"""Block and stream CRC-32 of a container's decoded bytes, kept beside it (not in PY).

The KOLR container carries no checksum and does not grow one (the reference's reader rejects
trailing bytes).  A ``Checksums`` manifest holds the standard CRC-32 (zlib / gzip / PNG:
``zlib.crc32``) of every block's original bytes and, combined, of the whole stream — the value
``gzip -l -v`` or ``python -c "zlib.crc32"`` prints for the original file.  It travels as a small
sidecar file, little-endian:

    b"KOLS" | u8 version (1) | u8 mode | u16 0 | u32 size_field | u64 total_len | u32 nblocks |
    u32 stream_crc | nblocks x (u32 len, u32 crc) | u32 CRC-32 of everything before it

Plain ``struct`` + ``zlib``: no device and no native library is involved here.  The encode entry
points fill a manifest on the device (``checksums=True``; ``kolm.last_checksums()``), and
``kolm.decompress`` / ``kolm.check`` / ``kolm.open_container`` check decoded bytes against one.
"""
from __future__ import annotations

import struct
import zlib
from functools import lru_cache
from typing import List, Sequence

MAGIC = b"KOLS"
VERSION = 1
_HEAD = struct.Struct("<4sBBHIQII")
_POLY = 0xEDB88320  # reflected; bit 31 is the coefficient of x^0 (zlib's convention)


def _multmodp(a: int, b: int) -> int:
    """a b mod P."""
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (_POLY if b & 1 else 0)
    return p


@lru_cache(maxsize=4096)
def _xpow8(n: int) -> int:
    """x^(8 n) mod P (square and multiply; the exponent counts modulo 2^32 - 1)."""
    e = (8 * n) % 0xFFFFFFFF
    p, sq = 0x80000000, 0x40000000
    while e:
        if e & 1:
            p = _multmodp(p, sq)
        sq = _multmodp(sq, sq)
        e >>= 1
    return p


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """CRC-32 of A + B from the CRC-32 of A, of B and len(B) (zlib's crc32_combine)."""
    if len_b < 0:
        raise ValueError("len_b must not be negative")
    return _multmodp(_xpow8(int(len_b)), crc_a & 0xFFFFFFFF) ^ (crc_b & 0xFFFFFFFF)


def combine_all(lens: Sequence[int], crcs: Sequence[int]) -> int:
    """CRC-32 of the stream whose blocks have these lengths and CRC-32 words."""
    c = 0
    for n, w in zip(lens, crcs):
        c = crc32_combine(c, w, n)
    return c


class KolmChecksumError(ValueError):
    """Decoded bytes do not match the manifest: block, its method id, the expected and the
    computed CRC-32.  No data is returned."""

    def __init__(self, block: int, method: int, expected: int, got: int):
        super().__init__(f"checksum: block {block} (method {method}): expected CRC-32 {expected:08x}, got {got:08x}")
        self.block, self.method, self.expected, self.got = block, method, expected, got


class Checksums:
    """The manifest: mode / size_field / total_len as in the container's header, every block's
    length and CRC-32, and stream_crc = CRC-32 of the whole original data."""

    def __init__(self, mode: int, size_field: int, total_len: int, lens: Sequence[int], crcs: Sequence[int],
                 stream_crc: int = None):
        self.mode, self.size_field, self.total_len = int(mode), int(size_field), int(total_len)
        self.lens: List[int] = [int(n) for n in lens]
        self.crcs: List[int] = [int(c) & 0xFFFFFFFF for c in crcs]
        if len(self.lens) != len(self.crcs):
            raise ValueError("checksums: one CRC-32 per block length")
        if sum(self.lens) != self.total_len:
            raise ValueError(f"checksums: block lengths add up to {sum(self.lens)}, expect {self.total_len}")
        combined = combine_all(self.lens, self.crcs)
        if stream_crc is not None and (int(stream_crc) & 0xFFFFFFFF) != combined:
            raise ValueError(f"checksums: stream CRC-32 {int(stream_crc) & 0xFFFFFFFF:08x} is not the combination of "
                             f"the blocks' ({combined:08x})")
        self.stream_crc = combined

    @classmethod
    def of_blocks(cls, mode: int, size_field: int, blocks: Sequence[bytes]) -> "Checksums":
        """The manifest of the given original blocks, computed with zlib on the host."""
        return cls(mode, size_field, sum(len(b) for b in blocks), [len(b) for b in blocks],
                   [zlib.crc32(b) for b in blocks])

    def __eq__(self, other) -> bool:
        return isinstance(other, Checksums) and (self.mode, self.size_field, self.total_len, self.lens, self.crcs) == (
            other.mode, other.size_field, other.total_len, other.lens, other.crcs)

    def __repr__(self) -> str:
        return (f"Checksums(mode={self.mode}, size_field={self.size_field}, total_len={self.total_len}, "
                f"blocks={len(self.lens)}, stream_crc=0x{self.stream_crc:08x})")

    def to_bytes(self) -> bytes:
        body = _HEAD.pack(MAGIC, VERSION, self.mode, 0, self.size_field, self.total_len, len(self.lens), self.stream_crc)
        body += b"".join(struct.pack("<II", n, c) for n, c in zip(self.lens, self.crcs))
        return body + struct.pack("<I", zlib.crc32(body))

    @classmethod
    def from_bytes(cls, blob: bytes) -> "Checksums":
        blob = bytes(blob)
        if len(blob) < _HEAD.size + 4:
            raise ValueError("checksums: sidecar too short")
        magic, version, mode, zero, size_field, total_len, nb, stream_crc = _HEAD.unpack_from(blob)
        if magic != MAGIC:
            raise ValueError("checksums: bad magic")
        if version != VERSION or zero != 0:
            raise ValueError(f"checksums: unsupported version {version}")
        if len(blob) != _HEAD.size + 8 * nb + 4:
            raise ValueError(f"checksums: sidecar of {len(blob)} bytes, expect {_HEAD.size + 8 * nb + 4} for {nb} blocks")
        if struct.unpack_from("<I", blob, len(blob) - 4)[0] != zlib.crc32(blob[:-4]):
            raise ValueError("checksums: the sidecar's own CRC-32 does not match")
        pairs = struct.unpack_from(f"<{2 * nb}I", blob, _HEAD.size)
        return cls(mode, size_field, total_len, pairs[0::2], pairs[1::2], stream_crc)


def as_checksums(obj) -> Checksums:
    """A Checksums, or the sidecar bytes of one."""
    return obj if isinstance(obj, Checksums) else Checksums.from_bytes(obj)
