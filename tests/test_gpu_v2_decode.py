"""v2_new (id 10) decoded on the GPU (csrc/k_v2dec.hip through kolm_decode_blocks): PY's golden
payloads and containers, every automaton mode over raw planes, hand-made Rice planes (k = 0..15,
codewords across the parse tile's edges), the encoder's own id-10 payloads alone and interleaved
with ids 0..9, the device-resident entry, the k > 15 host route and malformed payloads.  The
expected bytes are the original data (equal to kolm.decode.decode_new_pipeline on the same payload,
pinned by tests/test_v2_decode_core.py and tests/test_host.py)."""
import ctypes
import json
import os

import numpy as np
import pytest

import v2_payloads as V
from kolm import datagen as D
from kolm import decode as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def v2new():
    z = np.load(os.path.join(GOLDEN, "v2new.npz"))
    with open(os.path.join(GOLDEN, "v2new.json")) as f:
        return z, json.load(f)


def decode10(payloads, lens):
    from kolm import _lib
    return _lib.decode_blocks(list(payloads), [10] * len(payloads), list(lens))


def check_batch(cases):
    got = decode10([p for _, p, _ in cases], [len(d) for _, _, d in cases])
    pos = 0
    for name, _, data in cases:
        assert got[pos:pos + len(data)] == data, name
        pos += len(data)
    assert pos == len(got)


def test_golden_payloads(kolm_gpu):
    z, m = v2new()
    cases = [(n, z[f"{n}/v2new"].tobytes(), z[f"{n}/input"].tobytes()) for n in m["kernels"]]
    assert len(cases) == 85 and any(len(d) == 0 for _, _, d in cases)
    check_batch(cases)
    for name, pay, data in cases[:6]:
        assert kolm_gpu.decode_new_pipeline(pay, len(data)) == data, name


def test_automaton_modes_raw_planes(kolm_gpu):
    cases = V.automaton_cases()
    assert len(cases) == 196
    check_batch(cases)
    check_batch([(n, p + b"\xde\xad\xbe\xef", d) for n, p, d in cases])


def test_rice_planes(kolm_gpu):
    check_batch(V.rice_cases())


def _blocks():
    return [D.enwik_like(200_000, seed=3), D.splitmix64_bytes(70_001), bytes(65_536), D.gradient_bmp()[:100_000],
            D.sine_wav()[:50_000], b"a", b"ab" * 3000 + b"c", bytes(i & 0xFF for i in range(4099))]


def _forced(blk, mid):
    from kolm import _lib
    _, meth, p, _ = _lib.encode_blocks(blk, len(blk), cand_mask=1 << mid, force=[mid])
    assert int(meth[0]) == mid
    return p[0]


def test_encoder_round_trip(kolm_gpu):
    from kolm import _lib
    blocks = _blocks()
    pays = [_forced(b, 10) for b in blocks]
    for b, p in zip(blocks, pays):
        if len(b) <= 4099:
            assert H.decode_new_pipeline(p, len(b)) == b
    assert decode10(pays, [len(b) for b in blocks]) == b"".join(blocks)
    # interleaved with every other id in one batch
    mp, mm, ml, want = [], [], [], []
    for i, mid in enumerate(range(10)):
        blk = blocks[(3 * i) % len(blocks)]
        for m, p in ((mid, _forced(blk, mid)), (10, pays[i % len(blocks)])):
            mp.append(p)
            mm.append(m)
            data = blk if m != 10 else blocks[i % len(blocks)]
            ml.append(len(data))
            want.append(data)
    assert _lib.decode_blocks(mp, mm, ml) == b"".join(want)


def test_one_mib_block(kolm_gpu):
    """Multi-tile inverse BBWT with ruling-set nodes on the binary planes."""
    blk = D.enwik_like((1 << 20) + 3)
    assert decode10([_forced(blk, 10)], [len(blk)]) == blk


def test_device_entry(kolm_gpu):
    from kolm import _lib
    L = _lib.load()
    blocks = _blocks()[4:]
    pays = [_forced(b, 10) for b in blocks]
    arena = b"".join(pays)
    off = np.zeros(len(pays) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in pays])
    meth = np.full(len(pays), 10, np.uint32)
    lens = np.asarray([len(b) for b in blocks], np.uint32)
    total = int(lens.sum())
    ctx = ctypes.c_void_p()
    _lib.check(L.kolm_ctx_create(0, ctypes.byref(ctx)))
    try:
        dp, do = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.kolm_dev_alloc(ctx, len(arena) + 64, ctypes.byref(dp)))
        _lib.check(L.kolm_dev_alloc(ctx, total + 64, ctypes.byref(do)))
        _lib.check(L.kolm_memcpy_h2d(ctx, dp, arena, len(arena)))
        ms = ctypes.c_double(-1.0)
        _lib.check(L.kolm_decode_blocks_device(ctx, dp, off.ctypes.data, meth.ctypes.data, lens.ctypes.data,
                                               len(blocks), do, total, ctypes.byref(ms)))
        out = ctypes.create_string_buffer(total)
        _lib.check(L.kolm_memcpy_d2h(ctx, out, do, total))
        assert out.raw == b"".join(blocks)
        assert ms.value > 0.0
        L.kolm_dev_free(ctx, dp)
        L.kolm_dev_free(ctx, do)
    finally:
        L.kolm_ctx_destroy(ctx)


def test_containers_without_host_decoder(kolm_gpu, monkeypatch):
    from kolm.container import read_container

    def refuse(payload, n):
        raise AssertionError("host v2 decoder called")

    monkeypatch.setattr(H, "decode_new_pipeline", refuse)
    z, m = v2new()
    assert len(m["containers"]) == 5
    data = D.enwik_like(20_000, seed=5) + bytes(5000) + D.sine_wav()[:9000]
    sets = [(z[f"C/{c}/full10"].tobytes(), z[f"C/{c}/input"].tobytes()) for c in m["containers"]]
    sets.append((kolm_gpu.compress_blocks_fixed(data, 4096, v2_new=True), data))
    ids = []
    for blob, want in sets:
        ids += list(read_container(blob)[3])
        assert kolm_gpu.decompress(blob) == want
    assert 10 in ids


def test_k_above_15(kolm_gpu):
    from kolm import _lib
    from kolm.container import MODE_FIXED, write_container
    pay, data = V.k16_block()
    with pytest.raises(_lib.KolmError, match=r"block 0 \(method 10\): malformed payload"):
        decode10([pay], [len(data)])
    good = V.VALID_NEIGHBOUR
    blob = write_container(MODE_FIXED, 4, 8, [10, 10], [4, 4], [good, pay])
    assert kolm_gpu.decompress(blob) == bytes(4) + data


@pytest.mark.parametrize("i", range(len(V.MALFORMED)))
def test_malformed_payloads(kolm_gpu, i):
    from kolm import _lib
    bad = V.MALFORMED[i]
    with pytest.raises(_lib.KolmError, match=r"block 0 \(method 10\): malformed payload"):
        decode10([bad], [V.MALFORMED_N])
    with pytest.raises(_lib.KolmError, match=r"block 1 \(method 10\): malformed payload"):
        decode10([V.VALID_NEIGHBOUR, bad, V.VALID_NEIGHBOUR], [4, V.MALFORMED_N, 4])
    assert decode10([bad], [0]) == b""
    assert decode10([V.VALID_NEIGHBOUR], [4]) == bytes(4)
