"""Verify-after-encode on the device (csrc/k_verify.hip, kolm_verify_blocks_device,
kolm_verify_container, the encode entry points' verify switch).

The payloads of tests 1-3 are the reference's own (tests/golden/kernels.npz: xor, rice0/1/4/8/16
for ids 2..6, lz77, lfsr, repair; id 0 is the input itself; tests/golden/v2new.npz for id 10):
no encode is involved there, so a failure is the decoders' or the compare kernel's.  Tampered
payloads are judged by the host decoders (kolm.decode.decode_block) and, for the offset, by
kolm_decode_blocks' own output for the same payload — a pure check of the compare kernel.
"""
import json
import os
import time

import numpy as np
import pytest

from kolm import datagen as D
from kolm import decode as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EQUAL, REJECTED = 0xFFFFFFFF, 0xFFFFFFFE
NAMES = ["abab", "abcabc", "checker8k", "enwik16k", "grad4k", "grad_px4k", "pattern0_4k", "pattern1_4k",
         "pattern2_4k", "pattern6_4k", "pattern10_4k", "pattern15_4k", "ramp8k", "rand1k_seed7", "rand4k", "sine4k",
         "text_hobbit", "tiny06", "tiny07", "tiny12", "tiny20", "tiny40", "tiny49", "utf8_mixed", "zero16k"]
KEYS = {1: "xor", 2: "rice0", 3: "rice1", 4: "rice4", 5: "rice8", 6: "rice16", 7: "lz77", 8: "lfsr", 9: "repair"}


@pytest.fixture(scope="module")
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


@pytest.fixture(scope="module")
def fixtures(golden_kernels):
    """[(name, input, {id: golden payload})] of the 25 fixtures of 64..20000 input bytes."""
    out = []
    for n in NAMES:
        data = golden_kernels[f"{n}/input"].tobytes()
        assert 64 <= len(data) <= 20000
        pays = {0: data}
        pays.update({m: golden_kernels[f"{n}/{k}"].tobytes() for m, k in KEYS.items()})
        out.append((n, data, pays))
    assert len(out) == 25
    return out


def batch(cases):
    """cases: [(data, payload, method)] -> (data bytes, bounds, payloads, methods)."""
    bounds = np.zeros(len(cases) + 1, np.uint64)
    bounds[1:] = np.cumsum([len(d) for d, _, _ in cases])
    return b"".join(d for d, _, _ in cases), bounds, [p for _, p, _ in cases], [m for _, _, m in cases]


# ------------------------------------------------------------------ 1. clean

def test_clean_golden_payloads(lib, fixtures):
    cases = [(data, pays[m], m) for _, data, pays in fixtures for m in range(10)]
    fb, rep = lib.verify_blocks(*batch(cases))
    assert len(fb) == 250 and (fb == EQUAL).all()
    assert rep["blocks"] == 250 and rep["bad_blocks"] == 0 and rep["first_bad_reason"] == 0
    assert rep["bytes"] == 10 * sum(len(d) for _, d, _ in fixtures)
    # second batch: every id-10 payload of the v2_new goldens (85 blocks, the empty one included)
    z = np.load(os.path.join(GOLDEN, "v2new.npz"))
    with open(os.path.join(GOLDEN, "v2new.json")) as f:
        names = json.load(f)["kernels"]
    cases = [(z[f"{n}/input"].tobytes(), z[f"{n}/v2new"].tobytes(), 10) for n in names]
    fb, rep = lib.verify_blocks(*batch(cases))
    assert len(fb) == 85 and (fb == EQUAL).all()
    assert rep["blocks"] == 85 and rep["bad_blocks"] == 0
    assert rep["bytes"] == sum(len(d) for d, _, _ in cases)


# ------------------------------------------------------------------ 2. tampered payloads

def tamper(p, edit):
    q = bytearray(p)
    if edit == "first":
        q[0] ^= 0x80
    elif edit == "middle":
        q[len(q) // 2] ^= 0x80
    else:
        q[-1] ^= 0x01
    return bytes(q)


def host_verdict(mid, payload, data):
    """(bad, raised) by the host decoder."""
    try:
        out = H.decode_block(mid, payload, len(data))
    except Exception:  # noqa: BLE001  (the decoders raise ValueError / IndexError / ...)
        return True, True
    return out != data, False


def first_diff(a, b):
    x = np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)
    i = np.flatnonzero(x)
    return int(i[0]) if len(i) else EQUAL


@pytest.mark.parametrize("edit", ["first", "middle", "last"])
def test_tampered_payloads_agree_with_host_decoders(lib, fixtures, edit):
    cases = [(data, tamper(pays[m], edit), m) for _, data, pays in fixtures for m in range(1, 10)]
    assert len(cases) == 225
    verdict = [host_verdict(m, p, d) for d, p, m in cases]
    nbad = sum(b for b, _ in verdict)
    nraised = sum(r for _, r in verdict)
    print(f"edit {edit}: host bad {nbad}/225, identical {225 - nbad}, raised {nraised}")
    # the test's own preconditions, from the host decoders: it cannot pass vacuously
    if edit == "last":
        assert nbad >= 100 and 225 - nbad >= 60  # the identical ones: Rice padding bits, no false alarm allowed
    else:
        assert nbad >= 200
    fb, rep = lib.verify_blocks(*batch(cases))
    rejected = fb == REJECTED
    print(f"edit {edit}: device bad {int((fb != EQUAL).sum())}/225, rejected {int(rejected.sum())}")
    # the compare kernel alone: where the device decoder accepts the payload, first_bad is the first
    # index at which kolm_decode_blocks' output for the same payload differs from the input
    keep = [i for i in range(225) if not rejected[i]]
    dec = lib.decode_blocks([cases[i][1] for i in keep], [cases[i][2] for i in keep], [len(cases[i][0]) for i in keep])
    pos = 0
    for i in keep:
        d = cases[i][0]
        assert int(fb[i]) == first_diff(dec[pos:pos + len(d)], d), (i, cases[i][2])
        pos += len(d)
    # bad exactly when the host decoder raises or returns other bytes
    for i, (bad, _) in enumerate(verdict):
        assert (int(fb[i]) != EQUAL) == bad, (i, cases[i][2], int(fb[i]))
    assert rep["bad_blocks"] == nbad and rep["blocks"] == 225
    first = min(i for i, (b, _) in enumerate(verdict) if b)
    assert rep["first_bad_block"] == first and rep["first_bad_method"] == cases[first][2]
    assert rep["first_bad_reason"] == (2 if rejected[first] else 1)
    assert rep["first_bad_offset"] == (0 if rejected[first] else int(fb[first]))


def test_raw_block_input_side_flips(lib, fixtures):
    data = fixtures[3][1]  # enwik16k
    n = len(data)
    cases, want = [], []
    for p in (0, 1, 15, 16, 17, n - 1):
        q = bytearray(data)
        q[p] ^= 0x80
        cases.append((bytes(q), data, 0))  # the input differs from what the raw payload decodes to
        want.append(p)
    fb, rep = lib.verify_blocks(*batch(cases))
    assert fb.tolist() == want
    assert rep["bad_blocks"] == 6 and rep["first_bad_block"] == 0 and rep["first_bad_offset"] == 0
    assert rep["first_bad_method"] == 0 and rep["first_bad_reason"] == 1


# ------------------------------------------------------------------ 3. geometry (raw blocks)

LENS = [1, 1, 2, 3, 15, 16, 17, 1, 31, 4101]


def verify_raw(lib, data, payload, lens, offset, before=0xAA, after=0x55):
    """Raw blocks of `lens` bytes: data placed `offset` bytes into its device buffer, with
    `before` / `after` bytes around it; payload = the arena."""
    ctx = lib.device_ctx(lib.ensure_init())
    bounds = np.zeros(len(lens) + 1, np.uint64)
    bounds[1:] = np.cumsum(lens)
    n = int(bounds[-1])
    assert len(data) == len(payload) == n
    dd = lib.DeviceBuffer(ctx, offset + n + 64)
    dp = lib.DeviceBuffer(ctx, n + 64)
    try:
        dd.upload(bytes([before]) * offset + data + bytes([after]) * 64)
        dp.upload(payload)
        return lib.verify_blocks_device(ctx, dd.ptr + offset, bounds, dp.ptr, bounds, [0] * len(lens))
    finally:
        dd.free()
        dp.free()


@pytest.mark.parametrize("offset", range(16))
def test_geometry_every_alignment(lib, offset):
    n = sum(LENS)
    starts = np.concatenate([[0], np.cumsum(LENS)]).tolist()
    data = D.splitmix64_bytes(n, seed=offset + 1)
    nb = len(LENS)
    # equal, whatever lies around the data (two different surroundings: one of them differs from the
    # bytes around the decode scratch): the byte before and the byte after stay unreported
    for before, after in ((0xAA, 0x55), (0x00, 0xFF)):
        fb, rep = verify_raw(lib, data, data, LENS, offset, before, after)
        assert fb.tolist() == [EQUAL] * nb and rep["bad_blocks"] == 0 and rep["bytes"] == n

    def run(flips):
        q = bytearray(data)
        for p in flips:
            q[p] ^= 0x80
        want = [EQUAL] * nb
        for p in sorted(flips, reverse=True):
            b = max(i for i in range(nb) if starts[i] <= p)
            want[b] = p - starts[b]
        fb, rep = verify_raw(lib, data, bytes(q), LENS, offset)
        assert fb.tolist() == want, (offset, flips)
        assert rep["bad_blocks"] == sum(w != EQUAL for w in want)
        assert rep["first_bad_block"] == min(i for i in range(nb) if want[i] != EQUAL)

    run([0, 1])                # two adjacent 1-byte blocks of one 16-byte word
    run([0, n - 1])            # the first and the last byte of the batch
    run([starts[5] + 7, starts[9] + 100, starts[9] + 4000])  # two blocks at once; the lower offset wins
    run([starts[6] + 16, starts[7], starts[8]])              # a block's last byte and its two neighbours
    run(list(range(n)))        # everything


def test_all_different_1mib_block(lib):
    n = 1 << 20
    data = D.enwik_like(n, seed=11)
    other = bytes(np.frombuffer(data, np.uint8) ^ 0xFF)
    t0 = time.perf_counter()
    fb, rep = verify_raw(lib, data, other, [n], 3)
    assert time.perf_counter() - t0 < 5.0
    assert fb.tolist() == [0] and rep["bad_blocks"] == 1 and rep["first_bad_offset"] == 0
    print(f"all-different 1 MiB: compare {rep['ms_compare']:.3f} ms")


# ------------------------------------------------------------------ 4. encode with verify on

@pytest.fixture(scope="module")
def enc_data():
    return D.enwik_like(200_000, seed=3) + D.splitmix64_bytes(70_001) + bytes(65_536)


ENC_CASES = [("fixed", bs, mode) for bs in (65536, 4099) for mode in ("hot", "default", "v2")] + [("cdc", 0, "default")]
_plain = {}


def compress(kolm, data, case, verify):
    kind, bs, mode = case
    kw = {"hot": {"hot_path": True}, "default": {}, "v2": {"v2_new": True}}[mode]
    if kind == "cdc":
        return kolm.compress_blocks_cdc(data, verify=verify, **kw)
    return kolm.compress_blocks_fixed(data, bs, verify=verify, **kw)


def nblocks(kolm, data, case):
    kind, bs, _ = case
    return len(kolm.cdc_fast_boundaries_strict(data)) if kind == "cdc" else (len(data) + bs - 1) // bs


@pytest.mark.parametrize("env", [None, ("KOLM_BATCH_BYTES", "100000"), ("KOLM_VERIFY_BYTES", "100000")])
def test_encode_with_verify_on(kolm_gpu, enc_data, monkeypatch, env):
    kolm = kolm_gpu
    for case in ENC_CASES:
        if case not in _plain:  # the verify-off container, once, in the plain environment
            _plain[case] = compress(kolm, enc_data, case, False)
    if env:
        monkeypatch.setenv(*env)
    for case in ENC_CASES:
        got = compress(kolm, enc_data, case, True)
        assert got == _plain[case], (case, env)
        rep = kolm.last_verify()
        assert rep["blocks"] == nblocks(kolm, enc_data, case), (case, env)
        assert rep["bad_blocks"] == 0 and rep["bytes"] == len(enc_data) and rep["first_bad_reason"] == 0
    assert kolm.decompress(_plain[ENC_CASES[0]]) == enc_data


def test_encode_blocks_verify(kolm_gpu, enc_data):
    kolm = kolm_gpu
    plain = kolm.encode_blocks(enc_data, 65536, hot_path=True)
    got = kolm.encode_blocks(enc_data, 65536, hot_path=True, verify=True)
    assert got[0] == plain[0] and got[2] == plain[2]
    rep = kolm.last_verify()
    assert rep["blocks"] == len(plain[0]) and rep["bad_blocks"] == 0 and rep["bytes"] == len(enc_data)
    got = kolm.encode_blocks(enc_data, 65536, hot_path=True, verify=True, devices=2)  # clamped to the devices present
    assert got[0] == plain[0] and got[2] == plain[2]
    rep = kolm.last_verify()
    assert rep["blocks"] == len(plain[0]) and rep["bad_blocks"] == 0 and rep["bytes"] == len(enc_data)


# ------------------------------------------------------------------ 5. off is untouched

def test_off_launches_no_verify_kernel(lib, enc_data):
    ctx = lib.device_ctx(lib.ensure_init())
    data = enc_data[:131072]
    mask = lib.KOLM_HOTPATH_MASK
    d_in = lib.input_buffer(ctx, data)
    arena = lib.DeviceBuffer(ctx, lib.arena_capacity(len(data), 2, mask))
    try:
        lib.check(lib.load().kolm_ctx_set_timing(ctx, 1))
        off = lib.encode_blocks_device(ctx, d_in.ptr, len(data), 65536, arena.ptr, arena.nbytes, mask)
        kt = lib.kernel_times(ctx)
        assert kt and not [k for k in kt if k.startswith("k_verify")]
        on = lib.encode_blocks_device(ctx, d_in.ptr, len(data), 65536, arena.ptr, arena.nbytes, mask, verify=True)
        kt = lib.kernel_times(ctx)
        assert [k for k in kt if k.startswith("k_verify")] == ["k_verify_cmp"]
        assert kt["k_verify_cmp"]["launches"] == 1 and kt["k_verify_cmp"]["family"] == 8  # KOLM_KT_EMIT
        assert kt["k_verify_cmp"]["bytes"] == 2 * len(data)
        assert (on[1] == off[1]).all() and (on[2] == off[2]).all() and (on[0] == off[0]).all()
        assert lib.verify_report(ctx)["blocks"] == 2
        # and off again: the count stays
        lib.encode_blocks_device(ctx, d_in.ptr, len(data), 65536, arena.ptr, arena.nbytes, mask)
        assert lib.kernel_times(ctx)["k_verify_cmp"]["launches"] == 1
    finally:
        lib.load().kolm_ctx_set_timing(ctx, 0)
        d_in.free()
        arena.free()


# ------------------------------------------------------------------ 6. the error path

def test_injected_corruption_raises(kolm_gpu, monkeypatch):
    kolm = kolm_gpu
    bs = 8192
    data = D.enwik_like(bs, seed=5) + D.splitmix64_bytes(bs) + bytes(bs)
    plain = kolm.compress_blocks_fixed(data, bs, hot_path=True)
    monkeypatch.setenv("KOLM_VERIFY_INJECT", "1")
    assert kolm.compress_blocks_fixed(data, bs, hot_path=True) == plain  # verify off: the switch is ignored
    assert kolm.compress_blocks_fixed(data, bs, hot_path=True, verify=False) == plain
    with pytest.raises(kolm.KolmVerifyError) as ei:
        kolm.compress_blocks_fixed(data, bs, hot_path=True, verify=True)
    e = ei.value
    assert (e.block, e.method, e.offset, e.reason) == (1, 0, 0, 1)
    assert e.code == -8 and "block 1" in str(e) and "offset 0" in str(e)
    rep = kolm.last_verify()
    assert rep["bad_blocks"] == 1 and rep["blocks"] == 3 and rep["first_bad_block"] == 1
    with pytest.raises(kolm.KolmVerifyError) as ei:
        kolm.encode_blocks(data, bs, hot_path=True, verify=True)
    assert (ei.value.block, ei.value.method, ei.value.offset, ei.value.reason) == (1, 0, 0, 1)
    with pytest.raises(kolm.KolmVerifyError) as ei:  # the multi-device entry: the shard's report, block numbers of the call
        kolm.encode_blocks(data, bs, hot_path=True, verify=True, devices=2)
    assert (ei.value.block, ei.value.method, ei.value.offset, ei.value.reason) == (1, 0, 0, 1)
    monkeypatch.setenv("KOLM_VERIFY_INJECT", "0")  # block 0 is text: a Rice / LZ77 payload with its first byte changed
    with pytest.raises(kolm.KolmVerifyError) as ei:
        kolm.compress_blocks_fixed(data, bs, hot_path=True, verify=True)
    assert ei.value.block == 0 and ei.value.method != 0 and ei.value.reason in (1, 2)
    monkeypatch.delenv("KOLM_VERIFY_INJECT")
    assert kolm.compress_blocks_fixed(data, bs, hot_path=True, verify=True) == plain  # the switch was restored
    assert kolm.compress_blocks_fixed(data, bs, hot_path=True) == plain


def test_distributed_rank_verifies_its_shard(kolm_gpu, monkeypatch):
    """kolm.parallel.compress_blocks_fixed_distributed(verify=True) on a one-rank communicator: the
    rank checks its shard on its own device context before the gather."""
    from kolm import _lib
    from kolm.parallel import Comm, compress_blocks_fixed_distributed
    bs = 8192
    data = D.enwik_like(bs, seed=5) + D.splitmix64_bytes(bs) + bytes(bs - 100)
    plain = kolm_gpu.compress_blocks_fixed(data, bs)
    with Comm(1, 0, Comm.unique_id(), device=_lib.ensure_init()) as comm:
        assert compress_blocks_fixed_distributed(data, bs, comm=comm) == plain
        assert compress_blocks_fixed_distributed(data, bs, comm=comm, verify=True) == plain
        rep = kolm_gpu.last_verify()
        assert rep["blocks"] == 3 and rep["bad_blocks"] == 0 and rep["bytes"] == len(data)
        monkeypatch.setenv("KOLM_VERIFY_INJECT", "1")
        assert compress_blocks_fixed_distributed(data, bs, comm=comm) == plain
        with pytest.raises(kolm_gpu.KolmVerifyError) as ei:
            compress_blocks_fixed_distributed(data, bs, comm=comm, verify=True)
        assert (ei.value.block, ei.value.method, ei.value.offset, ei.value.reason) == (1, 0, 0, 1)
        monkeypatch.delenv("KOLM_VERIFY_INJECT")
        assert compress_blocks_fixed_distributed(data, bs, comm=comm, verify=True) == plain


# ------------------------------------------------------------------ 7. kolm.verify

def golden_container_cases(golden_containers):
    out = []
    for z in (golden_containers, np.load(os.path.join(GOLDEN, "cdc.npz"))):
        for k in z.keys():
            name, what = k.rsplit("/", 1)
            if what in ("full", "ids0_8"):
                out.append((k, z[k].tobytes(), z[f"{name}/input"].tobytes()))
    return out


def test_verify_golden_containers(kolm_gpu, golden_containers):
    cases = golden_container_cases(golden_containers)
    assert len(cases) == 32
    for k, blob, data in cases:
        r = kolm_gpu.verify(blob, data)
        assert r["ok"] and r["bad"] == [] and r["reason"] == 0 and r["bytes"] == len(data), k
        assert kolm_gpu.decompress(blob) == data


def test_verify_reports_block_and_offset(kolm_gpu, golden_containers):
    blob = golden_containers["mix_b1000/full"].tobytes()
    data = golden_containers["mix_b1000/input"].tobytes()
    q = bytearray(data)
    q[5123] ^= 0x04
    r = kolm_gpu.verify(blob, bytes(q))
    assert not r["ok"] and r["blocks"] == 15 and r["reason"] == 1
    assert [(b, o, why) for b, _, o, why in r["bad"]] == [(5, 123, 1)]
    mids = kolm_gpu.read_container(blob)[3]
    assert r["bad"][0][1] == mids[5]
    r = kolm_gpu.verify(blob, data + b"x")  # the lengths differ: nothing is decoded
    assert not r["ok"] and r["reason"] == 3 and r["bad"] == []
    with pytest.raises(ValueError) as e1:
        kolm_gpu.decompress(blob[:-1])
    with pytest.raises(ValueError) as e2:
        kolm_gpu.verify(blob[:-1], data)
    assert str(e1.value) == str(e2.value)
