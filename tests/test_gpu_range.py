"""Random-access reads on the device (csrc/k_range.hip, kolm_reader_*, kolm.open_container).

The expected bytes are always slices of the original input: for the golden containers the
reference's own input / container pairs (tests/golden/containers.npz, cdc.npz, v2new.npz), for
containers made here the data that was compressed.  Nothing expected comes from a decode."""
import json
import os

import numpy as np
import pytest

from kolm import datagen as D
from kolm import decode as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


@pytest.fixture(scope="module")
def golden_cases(golden_containers):
    """[(name, container, input)]: fixed (ids 0..9 and 0..8), CDC, and the v2_new containers (id 10)."""
    out = []
    for z in (golden_containers, np.load(os.path.join(GOLDEN, "cdc.npz"))):
        for k in z.keys():
            name, what = k.rsplit("/", 1)
            if what in ("full", "ids0_8"):
                out.append((k, z[k].tobytes(), z[f"{name}/input"].tobytes()))
    z = np.load(os.path.join(GOLDEN, "v2new.npz"))
    with open(os.path.join(GOLDEN, "v2new.json")) as f:
        for c in json.load(f)["containers"]:
            out.append((f"C/{c}/full10", z[f"C/{c}/full10"].tobytes(), z[f"C/{c}/input"].tobytes()))
    return out


KEYS = {1: "xor", 2: "rice0", 3: "rice1", 4: "rice4", 5: "rice8", 6: "rice16", 7: "lz77", 8: "lfsr", 9: "repair"}


@pytest.fixture(scope="module")
def every_method_case(golden_kernels):
    """The MDL winners of the golden containers are ids 0, 2, 6, 7, 9 and 10 only.  This container
    holds one block per id 0..10, each the reference's own payload of that method (kernels.npz,
    v2new.npz) for two golden inputs, under a TOC written here (CDC mode: the lengths differ)."""
    import kolm
    z = np.load(os.path.join(GOLDEN, "v2new.npz"))
    mids, orig, pays, data = [], [], [], b""
    for name in ("grad4k", "text_hobbit"):
        inp = golden_kernels[f"{name}/input"].tobytes()
        assert z[f"{name}/input"].tobytes() == inp
        for m in range(11):
            p = inp if m == 0 else z[f"{name}/v2new"].tobytes() if m == 10 else golden_kernels[f"{name}/{KEYS[m]}"].tobytes()
            mids.append(m), orig.append(len(inp)), pays.append(p)
            data += inp
    return "every_method", kolm.write_container(kolm.MODE_CDC, 4096, len(data), mids, orig, pays), data


def ranges_for(blocks, total, seed):
    r = [(0, total), (0, 0), (total, 0)]
    if total:
        r.append((total - 1, 1))
    for start, _, _ in blocks[1:]:
        r.append((start, 0))
        for j in range(1, 18):
            lo, hi = max(start - j, 0), min(start + j, total)
            r.append((lo, hi - lo))
    rng = np.random.default_rng(seed)
    for _ in range(200):
        o = int(rng.integers(0, total + 1))
        r.append((o, int(rng.integers(0, total - o + 1))))
    return r


# ------------------------------------------------------------------ 1. golden containers

def test_golden_containers(kolm_gpu, golden_cases, every_method_case, monkeypatch):
    kolm = kolm_gpu
    methods = set()
    assert len(golden_cases) > 32
    for seed, (name, blob, data) in enumerate(golden_cases + [every_method_case]):
        with kolm.open_container(blob) as rd:
            assert len(rd) == len(data), name
            methods.update(m for _, _, m in rd.blocks)
            ranges = ranges_for(rd.blocks, len(data), seed)
            monkeypatch.delenv("KOLM_READ_BYTES", raising=False)
            got = rd.read_many(ranges)
            assert got == [data[o:o + n] for o, n in ranges], name
            st = kolm.last_read()
            assert st["groups"] == (1 if data else 0) and st["blocks_decoded"] == sum(1 for b in rd.blocks if b[1])
            if len(rd.blocks) >= 3:  # several groups; the whole-stream range is split across them
                two = sorted(n for _, n, _ in rd.blocks)[:2]
                monkeypatch.setenv("KOLM_READ_BYTES", str(max(two[0] + two[1] - 1, 1)))
                got = rd.read_many(ranges)
                assert got == [data[o:o + n] for o, n in ranges], name
                assert kolm.last_read()["groups"] >= 2
    assert methods == set(range(11))  # ids 0..10 are all covered


# ------------------------------------------------------------------ 2. alignment on the device

def test_every_alignment_into_device_memory(kolm_gpu, lib):
    kolm = kolm_gpu
    data = D.splitmix64_bytes(3 * 4096, seed=21)
    blob = kolm.compress_blocks_fixed(data, 4096)
    ctx = lib.device_ctx(lib.ensure_init())
    with kolm.open_container(blob, ctx) as rd:
        assert [m for _, _, m in rd.blocks] == [0, 0, 0]  # random bytes: raw wins the MDL
        ranges, i = [], 0
        for sm in range(16):
            for n in range(49):
                base = (i * 37 * 16) % (len(data) - 64) // 16 * 16  # crosses the block edges now and then
                ranges.append((base + sm, n))
                i += 1
        total = sum(n for _, n in ranges)
        buf = lib.DeviceBuffer(ctx, total + 128)
        try:
            buf.upload(bytes([0xCC]) * (total + 128))
            offs = rd.read_many_device(ranges, buf.ptr + 64, total)
            got = buf.download()
        finally:
            buf.free()
    assert got[:64] == bytes([0xCC]) * 64 and got[64 + total:] == bytes([0xCC]) * 64
    assert offs == np.concatenate(([0], np.cumsum([n for _, n in ranges])))[:-1].tolist()
    assert {o % 16 for o in offs} == set(range(16))  # the destination alignment varies too
    for (o, n), d in zip(ranges, offs):
        assert got[64 + d:64 + d + n] == data[o:o + n], (o, n)


# ------------------------------------------------------------------ 3. only the touched blocks

def test_only_touched_blocks_are_decoded(kolm_gpu, golden_containers):
    kolm = kolm_gpu
    blob = golden_containers["mix_b1000/full"].tobytes()
    data = golden_containers["mix_b1000/input"].tobytes()
    with kolm.open_container(blob) as rd:
        nb = len(rd.blocks)
        last = rd.blocks[-1][1]  # the last block is the short one
        assert nb == 15 and all(n == 1000 for _, n, _ in rd.blocks[:-1]) and 10 <= last <= 1000

        def stats(ranges):
            assert rd.read_many(ranges) == [data[o:o + n] for o, n in ranges]
            st = kolm.last_read()
            return st["blocks_decoded"], st["bytes_decoded"], st["groups"], st["compactions"]

        assert stats([(5123, 1)]) == (1, 1000, 1, 0)
        assert stats([(5100, 300), (5200, 500)]) == (1, 1000, 1, 0)       # overlapping, one block
        assert stats([(10, 20), (len(data) - 10, 10)]) == (2, 1000 + last, 1, 1)  # first and last block
        assert stats([(1500, 2000)]) == (3, 3000, 1, 0)                   # blocks 1..3, one run
        assert stats([(0, 0), (7000, 0)]) == (0, 0, 0, 0)
        st = kolm.last_read()
        assert st["ranges"] == 2 and st["bytes_returned"] == 0


# ------------------------------------------------------------------ 4. a bad block matters only when touched

def test_bad_block_matters_only_when_touched(kolm_gpu, golden_containers):
    kolm = kolm_gpu
    blob = golden_containers["mix_b1000/full"].tobytes()
    data = golden_containers["mix_b1000/input"].tobytes()
    mode, size_field, total, mids, orig, payloads = kolm.read_container(blob)
    # the edit: the first (block, edit) for which the host decoder raises
    bad = None
    for b in range(1, len(mids) - 1):
        p = payloads[b]
        h = len(p) // 2
        for q in (bytes([p[0] ^ 0x80]) + p[1:], p[:h] + bytes([p[h] ^ 0x80]) + p[h + 1:], p[:-1] + bytes([p[-1] ^ 1])):
            try:
                H.decode_block(mids[b], q, orig[b])
            except Exception:  # noqa: BLE001  (the decoders raise ValueError / IndexError / ...)
                bad = (b, q)
                break
        if bad:
            break
    assert bad is not None
    b, q = bad
    with pytest.raises(Exception):  # the expectation rests on the host decoder
        H.decode_block(mids[b], q, orig[b])
    tampered = kolm.write_container(mode, size_field, total, mids, orig, payloads[:b] + [q] + payloads[b + 1:])
    with kolm.open_container(tampered) as rd:  # the open does not fail
        lo, hi = rd.blocks[b][0], rd.blocks[b][0] + rd.blocks[b][1]
        ok = [(0, lo), (hi, total - hi), (lo - 7, 7), (hi, 9)]
        assert rd.read_many(ok) == [data[o:o + n] for o, n in ok]
        for touching in ([(lo, 1)], [(0, 10), (hi - 1, 2)], [(0, total)]):
            with pytest.raises(ValueError) as e:
                rd.read_many(touching)
            assert f"block {b} " in str(e.value) and f"method {mids[b]}" in str(e.value)
        assert rd.read_many(ok) == [data[o:o + n] for o, n in ok]  # and the reader goes on working


# ------------------------------------------------------------------ 5. file-like read

def test_file_like_read(kolm_gpu, lib, golden_containers):
    kolm = kolm_gpu
    blob = golden_containers["mix_b1000/full"].tobytes()
    data = golden_containers["mix_b1000/input"].tobytes()
    total = len(data)
    ctx = lib.device_ctx(lib.ensure_init())
    rd = kolm.open_container(blob, ctx)
    try:
        assert len(rd) == total
        assert rd.read(0) == kolm.decompress(blob) == data
        assert rd.read(total - 3, 10) == data[-3:]
        assert rd.read(total) == b"" and rd.read(total + 5, 4) == b""
        assert rd.read(1234, 0) == b"" and rd.read(999, 2) == data[999:1001]
        assert rd.blocks[1] == (1000, 1000, kolm.read_container(blob)[3][1])
        # a range past the end: ValueError, and nothing is launched
        lib.check(lib.load().kolm_ctx_set_timing(ctx, 1))
        assert rd.read_many([(0, 10), (2000, 10)]) == [data[:10], data[2000:2010]]
        kt = lib.kernel_times(ctx)
        assert kt["k_range_gather"]["launches"] >= 1 and kt["k_range_gather"]["family"] == 8  # KOLM_KT_EMIT
        for bad in ([(0, 10), (total - 1, 2)], [(total + 1, 0)]):
            with pytest.raises(ValueError):
                rd.read_many(bad)
            with pytest.raises(ValueError) as e:  # the native check, past the binding's own
                lib.reader_read(rd._h, bad)
            assert "range 1" in str(e.value) or "range 0" in str(e.value)
        assert lib.kernel_times(ctx) == kt
    finally:
        lib.load().kolm_ctx_set_timing(ctx, 0)
        rd.close()
    rd.close()  # closing twice is fine
    with pytest.raises(ValueError):
        rd.read(0, 1)
    with pytest.raises(ValueError):
        rd.read_many([(0, 1)])
    with pytest.raises(ValueError):  # a malformed container: as decompress raises
        kolm.open_container(blob[:-1])


# ------------------------------------------------------------------ 6. workload geometry

def test_many_small_ranges_over_1mib_blocks(kolm_gpu):
    kolm = kolm_gpu
    bs = 1 << 20
    data = D.enwik_like(8 * bs, seed=9)
    blob = kolm.compress_blocks_fixed(data, bs, hot_path=True)
    rng = np.random.default_rng(3)
    ranges = []
    for _ in range(1000):
        n = int(rng.integers(100, 4001))
        ranges.append((int(rng.integers(0, len(data) - n + 1)), n))
    ranges.insert(500, (bs // 2 + 5, 3 * bs))  # starts mid-block, ends mid-block
    with kolm.open_container(blob) as rd:
        got = rd.read_many(ranges)
        st = kolm.last_read()
    assert got == [data[o:o + n] for o, n in ranges]
    assert st["blocks_decoded"] == 8 and st["bytes_decoded"] == len(data) and st["compactions"] == 0
    assert st["bytes_returned"] == sum(n for _, n in ranges)


# ------------------------------------------------------------------ 7. host fallback

def test_host_fallback(kolm_gpu, lib, monkeypatch):
    """The goldens hold no id-10 block with a Rice parameter byte above 15 (an encoder writes
    0..15), so the fallback is forced through the binding's method mask: id 10 taken out of
    KOLM_DECODE_MASK as the reader sees it.  The calls that touch an id-10 block then go through
    kolm.decode.decode_block; the others still run on the device."""
    kolm = kolm_gpu
    z = np.load(os.path.join(GOLDEN, "v2new.npz"))
    with open(os.path.join(GOLDEN, "v2new.json")) as f:
        names = list(json.load(f)["containers"])
    for c in names:
        blob, data = z[f"C/{c}/full10"].tobytes(), z[f"C/{c}/input"].tobytes()
        mids = kolm.read_container(blob)[3]
        assert not any(m == 10 and kolm._v2_k_above_15(p) for m, p in zip(mids, kolm.read_container(blob)[5]))
        if 10 in mids and any(m != 10 for m in mids):
            break
    else:
        pytest.fail("no golden container mixes id 10 with other ids")
    monkeypatch.setattr(lib, "KOLM_DECODE_MASK", lib.KOLM_DECODE_MASK & ~(1 << 10))
    with kolm.open_container(blob) as rd:
        v2 = [i for i, (_, _, m) in enumerate(rd.blocks) if m == 10]
        other = [i for i, (_, _, m) in enumerate(rd.blocks) if m != 10]
        assert rd._host_blocks == v2
        s, n, _ = rd.blocks[v2[0]]
        ranges = [(s + n // 3, n // 2), (0, len(data)), (s, 0)]
        assert rd.read_many(ranges) == [data[o:o + m] for o, m in ranges]
        assert kolm.last_read().get("host") is True
        s, n, _ = rd.blocks[other[0]]
        assert rd.read_many([(s, n)]) == [data[s:s + n]]
        assert "host" not in kolm.last_read() and kolm.last_read()["blocks_decoded"] == 1
