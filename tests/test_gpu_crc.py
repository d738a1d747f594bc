"""Block and stream CRC-32 on the device (k_crc32): integrity without the original.  zlib.crc32 is
the oracle throughout.  Inputs are a few KiB to a few MiB.
1. crc32_blocks == zlib == the CPU emulation (tools/crc_emu.cpp), word for word: every word / piece /
   run edge, three contents, every misalignment, a block of 2^20 + 5 bytes, an empty block between
   two others, the batch at an aligned and an unaligned device address, fixed geometry with a
   short last block
2. encode with checksums on: the manifest is zlib's, the container is byte for byte the one of the
   same call with checksums off (smoke inputs, CDC, dedup, verify, several device batches); off:
   no manifest
3. decompress / check / Reader pass with the true manifest over every method id 0..10 (the
   reference's containers), checksums_of == the zlib manifest; again in several groups
4. detection: a flipped manifest CRC, a flipped payload byte of a raw / an xor block
5. off means off: no k_crc32 launch."""
import ctypes
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

from kolm import datagen as D
from kolm.checksums import Checksums, KolmChecksumError

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
EMU_SRC = os.path.join(REPO, "tools", "crc_emu.cpp")
LENS = (1, 3, 4, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 32767, 32768, 32769, 100000)
BS = 4096


@pytest.fixture(scope="module")
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("crc") / "crc_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", EMU_SRC, "-o", so], check=True)
    e = ctypes.CDLL(so)
    P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    e.crc_emu_blocks.argtypes = [P, U64, P, U32, U32, U32, P]
    e.crc_emu_blocks.restype = U64
    return e


def content(n, seed=0):
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed * 977)
    return ((i * 131 + (i >> 8) * 7 + 3) & 0xFF).astype(np.uint8).tobytes()


def split(data, lens):
    out, pos = [], 0
    for n in lens:
        out.append(data[pos:pos + n])
        pos += n
    return out


def manifest_of(kolm, blob, data) -> Checksums:
    """The zlib manifest of a container and the data it holds."""
    mode, size_field, total, _, orig, _ = kolm.read_container(blob)
    assert total == len(data)
    return Checksums.of_blocks(mode, size_field, split(data, orig))


# ------------------------------------------------------------------ 1. the kernel

def test_crc32_blocks_equal_zlib_and_the_emulation(kolm_gpu, emu):
    blocks = []
    for n in LENS:
        for kind, body in enumerate((bytes(n), b"\xff" * n, content(n))):
            # a prefix block of a bytes shifts the block (and everything behind it) by a bytes: many
            # geometries in one batch; every misalignment of every block is the loop further down
            for a in (range(16) if n < 32767 or kind == 2 else (0, 7)):
                if a:
                    blocks.append(bytes([0xE0 + a]) * a)
                blocks.append(body)
    blocks += [D.splitmix64_bytes((1 << 20) + 5), b"abc", b"", b"defgh"]
    bounds = np.concatenate(([0], np.cumsum([len(b) for b in blocks]))).tolist()
    batch = b"".join(blocks)
    want = [zlib.crc32(b) for b in blocks]
    host = np.frombuffer(batch, np.uint8)
    b64 = np.asarray(bounds, np.uint64)
    model = np.zeros(len(blocks), np.uint32)
    assert emu.crc_emu_blocks(host.ctypes.data, len(batch), b64.ctypes.data, len(blocks), 0, 0, model.ctypes.data) == 0
    assert [int(x) for x in model] == want
    for off in (0, 5):  # the batch at an aligned and at an unaligned device address
        got = kolm_gpu.crc32_blocks(batch, bounds=bounds, data_offset=off)
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (off, bad[0], bounds[bad[0]], len(blocks[bad[0]]), hex(got[bad[0]]), hex(want[bad[0]]))
        assert got == [int(x) for x in model]
    # every length and content at every misalignment: the blocks back to back, the batch uploaded at
    # data_offset 0..15, so a block that starts at s lies (s + off) mod 16 past a boundary
    sweep = [body for n in LENS for body in (bytes(n), b"\xff" * n, content(n))]
    sb = np.concatenate(([0], np.cumsum([len(b) for b in sweep]))).tolist()
    sbatch, swant = b"".join(sweep), [zlib.crc32(b) for b in sweep]
    seen = [set() for _ in sweep]
    for off in range(16):
        got = kolm_gpu.crc32_blocks(sbatch, bounds=sb, data_offset=off)
        bad = [i for i, (g, w) in enumerate(zip(got, swant)) if g != w]
        assert not bad, (off, bad[0], sb[bad[0]], len(sweep[bad[0]]))
        for i in range(len(sweep)):
            seen[i].add((sb[i] + off) % 16)
    assert all(m == set(range(16)) for m in seen)
    # fixed geometry with a short last block: one piece per block, and two runs per block (the
    # last block then has fewer runs than the others)
    for data, bs in ((content(10 * BS + 100, 3), BS), (D.splitmix64_bytes(100001, seed=2), 40000), (b"x", 8192)):
        got = kolm_gpu.crc32_blocks(data, block_size=bs, data_offset=3)
        assert got == [zlib.crc32(data[i:i + bs]) for i in range(0, len(data), bs)], bs
    assert kolm_gpu.crc32_blocks(b"", block_size=BS) == []
    assert kolm_gpu.crc32_blocks(b"", bounds=[0, 0, 0]) == [0, 0]
    assert kolm_gpu.crc32_blocks(b"123456789", bounds=[0, 9]) == [0xCBF43926]
    with pytest.raises(ValueError):
        kolm_gpu.crc32_blocks(b"abcdef", bounds=[0, 4, 2, 6])


def test_combine_is_zlibs(kolm_gpu):
    a, b = content(12345, 1), content(1 << 16, 2)
    for lb in (0, 1, 1 << 16):
        assert kolm_gpu.crc32_combine(zlib.crc32(a), zlib.crc32(b[:lb]), lb) == zlib.crc32(a + b[:lb])
    l1, l2 = (1 << 31) - 100, 105  # len_b = 2^31 + 5 in one step and in two
    one = kolm_gpu.crc32_combine(7, kolm_gpu.crc32_combine(0x12345678, 0x9ABCDEF0, l2), l1 + l2)
    assert one == kolm_gpu.crc32_combine(kolm_gpu.crc32_combine(7, 0x12345678, l1), 0x9ABCDEF0, l2)


# ------------------------------------------------------------------ 2. the encode side

def _abc():
    a, b, c = D.enwik_like(BS, seed=3), D.splitmix64_bytes(BS), bytes(BS)
    return b"".join({"A": a, "B": b, "C": c}[k] for k in "ABAACBAC") + a[:100]


SMOKE = [(D.enwik_like(40000) + bytes(3000) + D.splitmix64_bytes(5000), 16384),
         (D.enwik_like(50000, seed=7) + bytes(12000) + D.enwik_like(40000, seed=8), 65536)]


def _is_zlibs(cs, data, lens):
    assert cs is not None
    assert cs.lens == lens and cs.total_len == len(data)
    assert cs.crcs == [zlib.crc32(b) for b in split(data, lens)]
    assert cs.stream_crc == zlib.crc32(data)


@pytest.mark.parametrize("case", range(len(SMOKE)))
def test_encode_with_checksums_smoke_inputs(kolm_gpu, case, monkeypatch):
    kolm = kolm_gpu
    data, bs = SMOKE[case]
    lens = [min(bs, len(data) - i) for i in range(0, len(data), bs)]
    off = kolm.compress_blocks_fixed(data, bs, hot_path=True)
    assert kolm.last_checksums() is None
    on = kolm.compress_blocks_fixed(data, bs, hot_path=True, checksums=True)
    assert on == off
    cs = kolm.last_checksums()
    _is_zlibs(cs, data, lens)
    assert (cs.mode, cs.size_field) == (kolm.MODE_FIXED, bs)
    assert Checksums.from_bytes(cs.to_bytes()) == cs
    assert kolm.decompress(on, checksums=cs) == data
    # several device batches: the per-batch words are appended in container order
    monkeypatch.setenv("KOLM_BATCH_BYTES", str(bs))
    assert kolm.compress_blocks_fixed(data, bs, hot_path=True, checksums=True) == off
    _is_zlibs(kolm.last_checksums(), data, lens)
    monkeypatch.delenv("KOLM_BATCH_BYTES")
    # the block entry point
    mids, orig, payloads, _ = kolm.encode_blocks(data, bs, hot_path=True, checksums=True)
    _is_zlibs(kolm.last_checksums(), data, orig)
    assert kolm.encode_blocks(data, bs, hot_path=True)[2] == payloads
    assert kolm.last_checksums() is None


def test_encode_with_checksums_default_candidates_and_the_switch(kolm_gpu):
    kolm = kolm_gpu
    data, bs = SMOKE[0]
    lens = [min(bs, len(data) - i) for i in range(0, len(data), bs)]
    off = kolm.compress_blocks_fixed(data, bs)
    kolm.G_CHECKSUMS = True
    try:
        assert kolm.compress_blocks_fixed(data, bs) == off
        _is_zlibs(kolm.last_checksums(), data, lens)
        assert kolm.compress_blocks_fixed(data, bs, checksums=False) == off
        assert kolm.last_checksums() is None
    finally:
        kolm.G_CHECKSUMS = False
    assert kolm.compress_blocks_fixed(data, bs) == off and kolm.last_checksums() is None


def test_encode_with_checksums_cdc(kolm_gpu):
    kolm = kolm_gpu
    data = D.enwik_like(60000, seed=11) + bytes(9000) + D.splitmix64_bytes(7001)
    off = kolm.compress_blocks_cdc(data, 1024, 4096, 8192, hot_path=True)
    assert kolm.last_checksums() is None
    on = kolm.compress_blocks_cdc(data, 1024, 4096, 8192, hot_path=True, checksums=True)
    assert on == off
    cs = kolm.last_checksums()
    lens = [e - s for s, e in kolm.cdc_fast_boundaries_strict(data, 1024, 4096, 8192)]
    assert len(set(lens)) > 1
    _is_zlibs(cs, data, lens)
    assert (cs.mode, cs.size_field) == (kolm.MODE_CDC, 4096)
    assert kolm.check(on, cs)["ok"]


def test_encode_with_checksums_dedup_and_verify(kolm_gpu, monkeypatch):
    kolm = kolm_gpu
    data = _abc()
    lens = [min(BS, len(data) - i) for i in range(0, len(data), BS)]
    off = kolm.compress_blocks_fixed(data, BS)
    # dedup on: the pass reads the original text, so block numbers are container numbers
    assert kolm.compress_blocks_fixed(data, BS, dedup=True, checksums=True) == off
    assert kolm.last_dedup()["blocks_encoded"] == 4
    _is_zlibs(kolm.last_checksums(), data, lens)
    assert kolm.compress_blocks_fixed(data, BS, verify=True, checksums=True) == off
    assert kolm.last_verify()["blocks"] == 9 and kolm.last_verify()["bad_blocks"] == 0
    _is_zlibs(kolm.last_checksums(), data, lens)
    monkeypatch.setenv("KOLM_BATCH_BYTES", str(4 * BS))  # pieces A B A A | C B A C | tail
    assert kolm.compress_blocks_fixed(data, BS, dedup=True, verify=True, checksums=True) == off
    _is_zlibs(kolm.last_checksums(), data, lens)
    assert kolm.last_verify()["blocks"] == 9


# ------------------------------------------------------------------ 3. the check side

KEYS = {1: "xor", 2: "rice0", 3: "rice1", 4: "rice4", 5: "rice8", 6: "rice16", 7: "lz77", 8: "lfsr", 9: "repair"}


@pytest.fixture(scope="module")
def cases(kolm_gpu, golden_containers, golden_kernels):
    """[(name, container, input)]: the reference's fixed containers (ids 0..9 and 0..8), its v2_new
    containers (id 10, one with an empty block), and one block per id 0..10 under a TOC written
    here, each the reference's own payload of that method."""
    kolm = kolm_gpu
    out = []
    for k in golden_containers.keys():
        name, what = k.rsplit("/", 1)
        if what in ("full", "ids0_8"):
            out.append((k, golden_containers[k].tobytes(), golden_containers[f"{name}/input"].tobytes()))
    z = np.load(os.path.join(GOLDEN, "v2new.npz"))
    with open(os.path.join(GOLDEN, "v2new.json")) as f:
        for c in json.load(f)["containers"]:
            out.append((f"C/{c}/full10", z[f"C/{c}/full10"].tobytes(), z[f"C/{c}/input"].tobytes()))
    mids, orig, pays, data = [], [], [], b""
    for name in ("grad4k", "text_hobbit"):
        inp = golden_kernels[f"{name}/input"].tobytes()
        for m in range(11):
            p = inp if m == 0 else z[f"{name}/v2new"].tobytes() if m == 10 else golden_kernels[f"{name}/{KEYS[m]}"].tobytes()
            mids.append(m), orig.append(len(inp)), pays.append(p)
            data += inp
        mids.append(10), orig.append(0), pays.append(z["empty/v2new"].tobytes())  # an empty block: CRC-32 0
    out.append(("every_method", kolm.write_container(kolm.MODE_CDC, 4096, len(data), mids, orig, pays), data))
    return out


@pytest.mark.parametrize("groups", ("one", "several"))
def test_true_manifest_passes_everywhere(kolm_gpu, cases, groups, monkeypatch):
    kolm = kolm_gpu
    methods, empty_blocks = set(), 0
    for name, blob, data in cases:
        cs = manifest_of(kolm, blob, data)
        assert cs.stream_crc == zlib.crc32(data), name
        if groups == "several" and len(cs.lens) >= 3:  # a single block always forms a group
            two = sorted(cs.lens)[:2]
            monkeypatch.setenv("KOLM_VERIFY_BYTES", str(max(two[0] + two[1] - 1, 1)))
            monkeypatch.setenv("KOLM_READ_BYTES", str(max(two[0] + two[1] - 1, 1)))
        else:
            monkeypatch.delenv("KOLM_VERIFY_BYTES", raising=False)
            monkeypatch.delenv("KOLM_READ_BYTES", raising=False)
        assert kolm.decompress(blob, checksums=cs) == data, name
        rep = kolm.check(blob, cs.to_bytes())
        assert rep["ok"] and rep["bad"] == [] and rep["blocks"] == len(cs.lens) and rep["bytes"] == len(data), name
        assert rep["stream_crc"] == cs.stream_crc, name
        made = kolm.checksums_of(blob)
        assert made == cs and made.stream_crc == cs.stream_crc, name
        with kolm.open_container(blob, checksums=cs) as rd:
            methods.update(m for _, _, m in rd.blocks)
            empty_blocks += sum(1 for _, n, _ in rd.blocks if n == 0)
            n = len(data)
            ranges = [(0, n), (n // 3, n // 2), (max(n - 1, 0), min(n, 1)), (0, 0)]
            assert rd.read_many(ranges) == [data[o:o + k] for o, k in ranges], name
            if groups == "several" and len(cs.lens) >= 3:
                assert kolm.last_read()["groups"] >= 2, name
    assert methods == set(range(11)) and empty_blocks >= 1


# ------------------------------------------------------------------ 4. detection

@pytest.fixture(scope="module")
def raw_xor_case(kolm_gpu):
    """A container of 8 blocks of 4 KiB with ids 0 (raw) and 1 (xor) alternating: a flipped payload
    byte of either decodes to other bytes and cannot make a decoder misbehave."""
    kolm = kolm_gpu
    data = D.enwik_like(6 * BS, seed=5) + D.splitmix64_bytes(2 * BS - 77, seed=6)
    blocks = [data[i:i + BS] for i in range(0, len(data), BS)]
    mids = [i & 1 for i in range(len(blocks))]
    pays = [kolm.encode_xor(b)[0] if m else b for b, m in zip(blocks, mids)]
    blob = kolm.write_container(kolm.MODE_FIXED, BS, len(data), mids, [len(b) for b in blocks], pays)
    assert kolm.decompress(blob) == data
    return blob, data, mids


def flip_payload_byte(kolm, blob, block, at):
    _, _, _, _, _, off, start = kolm.read_toc(blob)
    bad = bytearray(blob)
    p0, p1 = int(start) + int(off[block]), int(start) + int(off[block + 1])
    # an xor payload is a ULEB128 stream: change a one-byte code into another one-byte code (a
    # byte below 0x80 behind a byte below 0x80), so the payload stays well-formed and of its
    # length; in a raw payload every byte qualifies or the search moves on a little
    at = next(i for i in range(p0 + at, p1) if bad[i] < 0x80 and bad[i - 1] < 0x80)
    bad[at] ^= 0x01
    return bytes(bad)


def test_flipped_manifest_crc_is_reported_for_exactly_that_block(kolm_gpu, raw_xor_case):
    kolm = kolm_gpu
    blob, data, mids = raw_xor_case
    cs = manifest_of(kolm, blob, data)
    for b in (0, 3, 7):
        crcs = list(cs.crcs)
        crcs[b] ^= 1
        bad = Checksums(cs.mode, cs.size_field, cs.total_len, cs.lens, crcs)
        with pytest.raises(KolmChecksumError) as ei:
            kolm.decompress(blob, checksums=bad)
        e = ei.value
        assert (e.block, e.method, e.expected, e.got) == (b, mids[b], crcs[b], cs.crcs[b])
        rep = kolm.check(blob, bad)
        assert not rep["ok"] and rep["reason"] == 1 and rep["bad"] == [(b, mids[b], crcs[b], cs.crcs[b], 1)]
        assert rep["stream_crc"] == cs.stream_crc  # of the bytes the container holds


@pytest.mark.parametrize("block", (2, 5))  # a raw and an xor block
def test_flipped_payload_byte_is_detected(kolm_gpu, lib, raw_xor_case, block, monkeypatch):
    kolm = kolm_gpu
    blob, data, mids = raw_xor_case
    cs = manifest_of(kolm, blob, data)
    bad = flip_payload_byte(kolm, blob, block, 1234)
    wrong = kolm.decompress(bad)  # unchecked: it decodes, to other bytes, in that block only
    diff = [i for i in range(len(cs.lens)) if wrong[i * BS:(i + 1) * BS] != data[i * BS:(i + 1) * BS]]
    assert diff == [block]
    got = zlib.crc32(wrong[block * BS:(block + 1) * BS])
    with pytest.raises(KolmChecksumError) as ei:
        kolm.decompress(bad, checksums=cs)
    e = ei.value
    assert (e.block, e.method, e.expected, e.got) == (block, mids[block], cs.crcs[block], got)
    with pytest.raises(KolmChecksumError):
        kolm.decompress(bad, device=False, checksums=cs)
    rep = kolm.check(bad, cs)
    assert not rep["ok"] and rep["bad"] == [(block, mids[block], cs.crcs[block], got, 1)]
    assert rep["stream_crc"] == zlib.crc32(wrong)
    ctx = lib.device_ctx(lib.ensure_init())
    for read_bytes in (None, str(2 * BS)):  # one group; several (the bad block is not in the first)
        if read_bytes:
            monkeypatch.setenv("KOLM_READ_BYTES", read_bytes)
        with kolm.open_container(bad, ctx, checksums=cs) as rd:
            # a read that does not touch the block succeeds
            lo, hi = block * BS, (block + 1) * BS
            assert rd.read_many([(0, lo), (hi, len(data) - hi)]) == [data[:lo], data[hi:]]
            # one that touches it raises and returns nothing
            for ranges in ([(0, len(data))], [(10, 20), (hi - 1, 2)]):
                with pytest.raises(KolmChecksumError) as ei:
                    rd.read_many(ranges)
                assert (ei.value.block, ei.value.expected, ei.value.got) == (block, cs.crcs[block], got)
            # and leaves a device buffer untouched
            buf = lib.DeviceBuffer(ctx, len(data) + 128)
            try:
                buf.upload(bytes([0xA5]) * (len(data) + 128))
                with pytest.raises(KolmChecksumError):
                    rd.read_many_device([(0, len(data))], buf.ptr + 64, len(data))
                assert buf.download() == bytes([0xA5]) * (len(data) + 128)
                offs = rd.read_many_device([(0, lo)], buf.ptr + 64, len(data))
                assert offs == [0] and buf.download(lo, 64) == data[:lo]
            finally:
                buf.free()
    # the same reader without a manifest hands the bytes out as they decode
    with kolm.open_container(bad) as rd:
        assert rd.read(0) == wrong


# ------------------------------------------------------------------ 5. off means off

def test_off_launches_nothing(lib):
    ctx = lib.device_ctx(lib.ensure_init())
    data = _abc()
    mask = lib.KOLM_HOTPATH_MASK
    d_in = lib.input_buffer(ctx, data)
    arena = lib.DeviceBuffer(ctx, lib.arena_capacity(len(data), 9, mask))
    want = [zlib.crc32(data[i:i + BS]) for i in range(0, len(data), BS)]
    try:
        lib.check(lib.load().kolm_ctx_set_timing(ctx, 1))
        base = lib.kernel_times(ctx).get("k_crc32", {"launches": 0})["launches"]
        off = lib.encode_blocks_device(ctx, d_in.ptr, len(data), BS, arena.ptr, arena.nbytes, mask)
        pay_off = arena.download(int(off[2][-1]))
        assert lib.kernel_times(ctx).get("k_crc32", {"launches": 0})["launches"] == base
        assert lib.last_crcs() is None and lib.ctx_checksums(ctx) == []
        on = lib.encode_blocks_device(ctx, d_in.ptr, len(data), BS, arena.ptr, arena.nbytes, mask, checksums=True)
        kt = lib.kernel_times(ctx)["k_crc32"]
        assert kt["launches"] == base + 1 and kt["bytes"] >= len(data)
        assert lib.last_crcs() == want == lib.ctx_checksums(ctx)
        assert (on[0] == off[0]).all() and (on[1] == off[1]).all() and (on[2] == off[2]).all()
        assert arena.download(int(on[2][-1])) == pay_off
        lib.encode_blocks_device(ctx, d_in.ptr, len(data), BS, arena.ptr, arena.nbytes, mask)
        assert lib.kernel_times(ctx)["k_crc32"]["launches"] == base + 1
        assert lib.last_crcs() is None and lib.ctx_checksums(ctx) == []
    finally:
        lib.load().kolm_ctx_set_timing(ctx, 0)
        d_in.free()
        arena.free()
