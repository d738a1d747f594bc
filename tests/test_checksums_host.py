"""The checksum manifest and the host side of the checks (kolm/checksums.py, kolm.decompress with
device=False): the sidecar's round trip and every rejection of from_bytes, and the reference's own
containers (tests/golden/containers.npz) decoded by the host decoders against a manifest built
with zlib from the golden inputs.  No device."""
import struct
import zlib

import pytest

import kolm
from kolm.checksums import Checksums, KolmChecksumError, combine_all, crc32_combine


def manifest_of(blob: bytes, data: bytes) -> Checksums:
    mode, size_field, total, mids, orig, _ = kolm.read_container(blob)
    assert total == len(data)
    blocks, pos = [], 0
    for n in orig:
        blocks.append(data[pos:pos + n])
        pos += n
    return Checksums.of_blocks(mode, size_field, blocks)


def sample() -> Checksums:
    blocks = [b"123456789", b"", bytes(1), bytes(2), bytes(range(256)) * 40]
    return Checksums.of_blocks(1, 4096, blocks)


def test_combine_is_zlibs():
    a, b = bytes(range(256)) * 33, b"kolm" * 1000
    for lb in (0, 1, 7, len(b)):
        assert crc32_combine(zlib.crc32(a), zlib.crc32(b[:lb]), lb) == zlib.crc32(a + b[:lb])
    assert crc32_combine(0, zlib.crc32(b), len(b)) == zlib.crc32(b)
    with pytest.raises(ValueError):
        crc32_combine(1, 2, -1)


def test_manifest_round_trip():
    cs = sample()
    assert cs.crcs[:4] == [0xCBF43926, 0, 0xD202EF8D, 0x41D912FF]
    data = b"123456789" + bytes(3) + bytes(range(256)) * 40
    assert cs.total_len == len(data) and cs.stream_crc == zlib.crc32(data) == combine_all(cs.lens, cs.crcs)
    blob = cs.to_bytes()
    assert blob[:4] == b"KOLS" and len(blob) == 28 + 8 * 5 + 4
    assert struct.unpack_from("<BBHIQII", blob, 4) == (1, 1, 0, 4096, len(data), 5, cs.stream_crc)
    back = Checksums.from_bytes(blob)
    assert back == cs and back.stream_crc == cs.stream_crc and back.to_bytes() == blob
    empty = Checksums(0, 8192, 0, [], [])
    assert empty.stream_crc == 0 and Checksums.from_bytes(empty.to_bytes()) == empty


def _resealed(body: bytes) -> bytes:
    return body + struct.pack("<I", zlib.crc32(body))


def test_from_bytes_rejections():
    cs = sample()
    blob = cs.to_bytes()
    body = bytearray(blob[:-4])
    with pytest.raises(ValueError, match="too short"):
        Checksums.from_bytes(blob[:20])
    with pytest.raises(ValueError, match="magic"):
        Checksums.from_bytes(_resealed(b"KOLR" + bytes(body[4:])))
    with pytest.raises(ValueError, match="version"):
        Checksums.from_bytes(_resealed(bytes(body[:4]) + b"\x02" + bytes(body[5:])))
    with pytest.raises(ValueError, match="bytes, expect"):  # a block short / a byte too many
        Checksums.from_bytes(blob[:-8] + blob[-4:])
    with pytest.raises(ValueError, match="bytes, expect"):
        Checksums.from_bytes(blob + b"\0")
    flipped = bytearray(blob)
    flipped[30] ^= 1
    with pytest.raises(ValueError, match="own CRC-32"):
        Checksums.from_bytes(bytes(flipped))
    bad = bytearray(body)  # total_len + 1: the lengths no longer add up (trailer made right again)
    struct.pack_into("<Q", bad, 12, cs.total_len + 1)
    with pytest.raises(ValueError, match="add up"):
        Checksums.from_bytes(_resealed(bytes(bad)))
    bad = bytearray(body)  # stream_crc that is not the combination of the blocks
    struct.pack_into("<I", bad, 24, cs.stream_crc ^ 1)
    with pytest.raises(ValueError, match="combination"):
        Checksums.from_bytes(_resealed(bytes(bad)))
    bad = bytearray(body)  # one block CRC changed: the stream CRC no longer matches it
    struct.pack_into("<I", bad, 28 + 4, cs.crcs[0] ^ 0x80)
    with pytest.raises(ValueError, match="combination"):
        Checksums.from_bytes(_resealed(bytes(bad)))


def golden_pairs(golden_containers):
    for k in golden_containers.keys():
        name, what = k.rsplit("/", 1)
        if what in ("full", "ids0_8"):
            yield k, golden_containers[k].tobytes(), golden_containers[f"{name}/input"].tobytes()


def test_host_decompress_checks_the_golden_containers(golden_containers):
    seen = 0
    for name, blob, data in golden_pairs(golden_containers):
        cs = manifest_of(blob, data)
        assert cs.stream_crc == zlib.crc32(data), name
        assert kolm.decompress(blob, device=False, checksums=cs) == data, name
        assert kolm.decompress(blob, device=False, checksums=cs.to_bytes()) == data, name
        seen += 1
    assert seen >= 8


def test_host_decompress_detects_a_flipped_manifest_crc(golden_containers):
    checked = 0
    for name, blob, data in golden_pairs(golden_containers):
        cs = manifest_of(blob, data)
        for b in sorted({0, len(cs.crcs) // 2, len(cs.crcs) - 1} if cs.crcs else ()):
            crcs = list(cs.crcs)
            crcs[b] ^= 0x00010000
            bad = Checksums(cs.mode, cs.size_field, cs.total_len, cs.lens, crcs)
            with pytest.raises(KolmChecksumError) as ei:
                kolm.decompress(blob, device=False, checksums=bad)
            e = ei.value
            mids = kolm.read_container(blob)[3]
            assert (e.block, e.method, e.expected, e.got) == (b, mids[b], crcs[b], cs.crcs[b]), name
            assert isinstance(e, ValueError)
            checked += 1
    assert checked >= 8


def test_host_decompress_rejects_a_manifest_of_other_lengths(golden_containers):
    for name, blob, data in golden_pairs(golden_containers):
        cs = manifest_of(blob, data)
        if len(cs.lens) < 2 or cs.lens[0] < 2:
            continue
        lens = [cs.lens[0] - 1, cs.lens[1] + 1] + cs.lens[2:]  # same total, other cut
        blocks, pos = [], 0
        for n in lens:
            blocks.append(data[pos:pos + n])
            pos += n
        other = Checksums.of_blocks(cs.mode, cs.size_field, blocks)
        assert other.stream_crc == cs.stream_crc
        with pytest.raises(ValueError, match="block lengths") as ei:
            kolm.decompress(blob, device=False, checksums=other)
        assert not isinstance(ei.value, KolmChecksumError)
        with pytest.raises(ValueError, match="another container"):
            kolm.decompress(blob, device=False,
                            checksums=Checksums(cs.mode, cs.size_field + 1, cs.total_len, cs.lens, cs.crcs))
        return
    pytest.fail("no golden container with two blocks")


def test_empty_input_gives_an_empty_manifest_not_none():
    blob = kolm.compress_blocks_fixed(b"", 4096, checksums=True)
    cs = kolm.last_checksums()
    assert cs == Checksums(kolm.MODE_FIXED, 4096, 0, [], []) and cs.stream_crc == zlib.crc32(b"") == 0
    assert kolm.decompress(blob, device=False, checksums=cs.to_bytes()) == b""
    assert kolm.compress_blocks_fixed(b"", 4096) == blob and kolm.last_checksums() is None
    kolm.compress_blocks_cdc(b"", checksums=True)
    assert kolm.last_checksums() == Checksums(kolm.MODE_CDC, 8192, 0, [], [])
    assert kolm.encode_blocks(b"", 4096, checksums=True)[0] == [] and kolm.last_checksums().lens == []
