"""Dedup on the device: repeated blocks are found (k_block_fp fingerprints, k_dedup_cmp byte
compare), encoded once, and their payloads copied to the repeats; the outputs are those of a call
without dedup.  Inputs are a few KiB to a few hundred KiB.
1. device fingerprints == the CPU emulation's (tools/dedup_emu.cpp) and the byte-wise definition
2. duplicate_blocks == a dict-of-bytes reference
3. containers with dedup on == containers with dedup off (hot path, default mask, v2_new, CDC),
   blocks_encoded == the distinct blocks; the zero-block golden container; the variable-bounds
   input also through encode_blocks_var under its own bounds (mixed lengths, forced methods)
4. KOLM_DEDUP_BITS=0: every block of one length collides with the first; same container
5. identical blocks under different forced methods
6. verify with dedup on, clean and with an injected corruption of a duplicate block
7. KOLM_BATCH_BYTES: duplicates that straddle two device batches
8. dedup off: no report, no dedup kernel launched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from kolm import datagen as D

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_SRC = os.path.join(REPO, "tools", "dedup_emu.cpp")
LENS = (1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8193)
BS = 4096


@pytest.fixture(scope="module")
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ddp") / "dedup_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", EMU_SRC, "-o", so], check=True)
    e = ctypes.CDLL(so)
    P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    e.ddp_emu_fp.argtypes = [P, U64, P, U32, U32, U32, P]
    e.ddp_emu_fp.restype = U64
    e.ddp_ref_fp.argtypes = [P, U64, P]
    e.ddp_ref_fp.restype = None
    return e


def _abc():
    a, b, c = D.enwik_like(BS, seed=3), D.splitmix64_bytes(BS), bytes(BS)
    return b"".join({"A": a, "B": b, "C": c}[k] for k in "ABAACBAC") + a[:100]


INPUTS = {
    "zeros": bytes(64 * BS),
    "distinct": D.splitmix64_bytes(16 * BS),
    "abc_tail": _abc(),
    "single": D.enwik_like(1000, seed=9),
}
# equal content at different lengths: X, X + one more byte, X again, a prefix of X, that prefix again
_X = D.enwik_like(5000, seed=4)
VAR = (_X + _X + b"q" + _X + _X[:777] + _X[:777] + bytes(33) + bytes(33) + bytes(34),
       [0, 5000, 10001, 15001, 15778, 16555, 16588, 16621, 16655])
# the fifth input: its bytes in fixed blocks and CDC chunks for the container tests, its own bounds
# for duplicate_blocks and the variable-geometry encode (test_var_bounds_encode_identical)
INPUTS["var"] = VAR[0]


def ref_rep(data, bounds):
    first, rep = {}, []
    for i in range(len(bounds) - 1):
        rep.append(first.setdefault(bytes(data[bounds[i]:bounds[i + 1]]), i))
    return rep


def fixed_bounds(n, bs=BS):
    return list(range(0, n, bs)) + [n]


def n_distinct(data, bounds):
    return len(set(ref_rep(data, bounds)))


# ------------------------------------------------------------------ 1. fingerprints

def test_device_fingerprints_equal_the_emulation(kolm_gpu, emu):
    blocks, bounds = [], [0]
    for n in LENS:
        body = (np.arange(n, dtype=np.uint64) * 131 + 3).astype(np.uint8).tobytes()
        for a in range(16):
            for part in ((bytes([0xE0 + a]) * a, body) if a else (body,)):
                blocks.append(part)
                bounds.append(bounds[-1] + len(part))
    for n in (8 * 4096 + 7, 17 * 4096, 140001):  # more pieces than one wave takes in a run
        blocks.append(D.splitmix64_bytes(n))
        bounds.append(bounds[-1] + n)
    batch = b"".join(blocks)
    nb = len(blocks)
    b = np.asarray(bounds, np.uint64)
    host = np.frombuffer(batch, np.uint8)
    want = np.zeros((nb, 2), np.uint64)
    assert emu.ddp_emu_fp(host.ctypes.data, len(batch), b.ctypes.data, nb, 0, 0, want.ctypes.data) == 0
    one = np.zeros(2, np.uint64)
    for i in (0, 1, nb // 2, nb - 1):  # the emulation against the byte-wise definition
        blk = np.frombuffer(blocks[i], np.uint8)
        emu.ddp_ref_fp(blk.ctypes.data, len(blocks[i]), one.ctypes.data)
        assert (one == want[i]).all()
    for off in (0, 5):  # the batch at an aligned and at an unaligned device address
        got = kolm_gpu.block_fingerprints(batch, bounds=bounds, data_offset=off)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (off, int(bad[0]), bounds[int(bad[0])], len(blocks[int(bad[0])]))
    # fixed geometry, a short tail: the same function of the bytes
    data = INPUTS["abc_tail"]
    got = kolm_gpu.block_fingerprints(data, block_size=BS)
    assert (got[0] == got[2]).all() and (got[0] == got[3]).all() and (got[1] == got[5]).all() and (got[4] == got[7]).all()
    assert len({tuple(int(x) for x in f) for f in got}) == 4
    blk = np.frombuffer(data[:BS], np.uint8)
    emu.ddp_ref_fp(blk.ctypes.data, BS, one.ctypes.data)
    assert (got[0] == one).all()


# ------------------------------------------------------------------ 2. the duplicate map

@pytest.mark.parametrize("name", list(INPUTS))
def test_duplicate_blocks_equal_dict_of_bytes(kolm_gpu, name):
    data = INPUTS[name]
    bounds = fixed_bounds(len(data))
    assert kolm_gpu.duplicate_blocks(data, BS) == ref_rep(data, bounds)
    if name == "var":  # and under its own bounds: equal content at different lengths
        data, bounds = VAR
        got = kolm_gpu.duplicate_blocks(data, bounds=bounds)
        assert got == [0, 1, 0, 3, 3, 5, 5, 7] == ref_rep(data, bounds)


def test_duplicate_blocks_unaligned_and_report(lib):
    data = INPUTS["abc_tail"]
    rep, r = lib.duplicate_blocks(data, BS, data_offset=11)
    assert list(rep) == ref_rep(data, fixed_bounds(len(data)))
    assert r["blocks"] == 9 and r["blocks_encoded"] == 4 and r["candidate_pairs"] == 5 and r["collisions"] == 0
    assert r["bytes"] == len(data) and r["bytes_encoded"] == 3 * BS + 100
    assert r["ms_hash"] > 0 and r["ms_compare"] > 0


# ------------------------------------------------------------------ 3. identity

MODES = {"hot": {"hot_path": True}, "default": {}, "v2": {"v2_new": True}}
_plain = {}


def plain(kolm, name, mode):
    """The container without dedup, computed once per (input, mode)."""
    if (name, mode) not in _plain:
        data = INPUTS[name]
        _plain[name, mode] = (kolm.compress_blocks_cdc(data, 1024, 2048, 4096) if mode == "cdc"
                              else kolm.compress_blocks_fixed(data, BS, **MODES[mode]))
    return _plain[name, mode]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(INPUTS))
def test_fixed_container_identical(kolm_gpu, name, mode):
    kolm = kolm_gpu
    data = INPUTS[name]
    want = plain(kolm, name, mode)
    got = kolm.compress_blocks_fixed(data, BS, dedup=True, **MODES[mode])
    assert got == want
    rep = kolm.last_dedup()
    bounds = fixed_bounds(len(data))
    assert rep["blocks"] == len(bounds) - 1 and rep["bytes"] == len(data)
    assert rep["blocks_encoded"] == n_distinct(data, bounds)
    assert rep["collisions"] == 0
    if mode == "hot":
        assert kolm.decompress(got) == data


@pytest.mark.parametrize("name", list(INPUTS))
def test_cdc_container_identical(kolm_gpu, name):
    kolm = kolm_gpu
    data = INPUTS[name]
    want = plain(kolm, name, "cdc")
    got = kolm.compress_blocks_cdc(data, 1024, 2048, 4096, dedup=True)
    assert got == want
    cuts = [s for s, _ in kolm.cdc_fast_boundaries_strict(data, 1024, 2048, 4096)] + [len(data)]
    rep = kolm.last_dedup()
    assert rep["blocks"] == len(cuts) - 1 and rep["blocks_encoded"] == n_distinct(data, cuts)


@pytest.mark.parametrize("mask_name", ["hot", "default", "forced"])
def test_var_bounds_encode_identical(lib, mask_name):
    """Variable geometry with blocks of mixed length and confirmed duplicates: the packed text's
    own bounds, and payloads expanded from representatives of different lengths.  Forced: the
    twin X blocks under different methods are no duplicates, the other pairs (same method) are."""
    data, bounds = VAR
    mask = {"hot": lib.KOLM_HOTPATH_MASK, "default": lib.KOLM_DEFAULT_MASK, "forced": 0x83}[mask_name]
    force = [0, 7, 7, 1, 1, 0, 0, 7] if mask_name == "forced" else None
    want = lib.encode_blocks_var(data, bounds, mask, force=force)
    assert lib.last_dedup() == {}
    got = lib.encode_blocks_var(data, bounds, mask, force=force, dedup=True)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and got[2] == want[2]
    rep = lib.last_dedup()
    distinct = n_distinct(data, bounds) + (1 if force else 0)  # forced: blocks 0 and 2 both encoded
    assert distinct == (6 if force else 5)
    assert rep["blocks"] == 8 and rep["blocks_encoded"] == distinct and rep["collisions"] == 0
    assert rep["candidate_pairs"] == 8 - distinct
    assert rep["bytes_encoded"] == (15845 if force else 10845)  # X, X + q, (X,) the prefix, 33 and 34 zeros
    if force:
        assert list(got[1]) == force
    got = lib.encode_blocks_var(data, bounds, mask, force=force, dedup=True, verify=True)
    assert got[2] == want[2] and lib.last_verify()["blocks"] == 8 and lib.last_verify()["bad_blocks"] == 0


def test_encode_blocks_outputs_identical(kolm_gpu):
    kolm = kolm_gpu
    data = INPUTS["abc_tail"]
    want = kolm.encode_blocks(data, BS)
    got = kolm.encode_blocks(data, BS, dedup=True)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and (got[3] == want[3]).all()
    assert kolm.last_dedup()["blocks_encoded"] == 4
    got = kolm.encode_blocks(data, BS, dedup=True, devices=2)  # clamped to the devices present; dedup per shard
    assert got[0] == want[0] and got[2] == want[2]
    assert kolm.last_dedup()["blocks"] == 9


def test_zero_block_golden_container(kolm_gpu, golden_containers):
    data = golden_containers["config1_zero64k/input"].tobytes()
    assert kolm_gpu.compress_blocks_fixed(data, 65536, dedup=True) == golden_containers["config1_zero64k/full"].tobytes()
    # the same zeros in 16 blocks of 4 KiB: one block encoded
    want = kolm_gpu.compress_blocks_fixed(data, BS)
    assert kolm_gpu.compress_blocks_fixed(data, BS, dedup=True) == want
    assert kolm_gpu.last_dedup()["blocks_encoded"] == 1


# ------------------------------------------------------------------ 4. collisions

def test_fingerprint_collisions_are_settled_by_bytes(kolm_gpu, monkeypatch):
    kolm = kolm_gpu
    data = INPUTS["abc_tail"]
    want = plain(kolm, "abc_tail", "hot")
    monkeypatch.setenv("KOLM_DEDUP_BITS", "0")
    assert kolm.compress_blocks_fixed(data, BS, hot_path=True, dedup=True) == want
    # the plan's rule: one group per length, represented by its first block; a member with other
    # bytes is a collision and is encoded itself
    bounds = fixed_bounds(len(data))
    blocks = [data[bounds[i]:bounds[i + 1]] for i in range(len(bounds) - 1)]
    first = {}
    coll = sum(1 for i, b in enumerate(blocks) if blocks[first.setdefault(len(b), i)] != b)
    dups = sum(1 for i, b in enumerate(blocks) if first[len(b)] != i and blocks[first[len(b)]] == b)
    assert (coll, dups) == (4, 3)
    rep = kolm.last_dedup()
    assert rep["collisions"] == coll and rep["candidate_pairs"] == coll + dups
    assert rep["blocks_encoded"] == len(blocks) - dups
    assert kolm.duplicate_blocks(data, BS) == [0, 1, 0, 0, 4, 5, 0, 7, 8]


# ------------------------------------------------------------------ 5. forced methods

def test_forced_methods_split_duplicates(lib):
    a = D.enwik_like(BS, seed=3)
    data = a * 6
    force = [0, 7, 0, 7, 1, 0]
    mask = (1 << 0) | (1 << 1) | (1 << 7)
    want = lib.encode_blocks(data, BS, mask, force=force)
    got = lib.encode_blocks(data, BS, mask, force=force, dedup=True)
    assert list(got[1]) == force == list(want[1])
    assert got[2] == want[2] and (got[0] == want[0]).all()
    assert got[2][0] == got[2][2] == got[2][5] and got[2][1] == got[2][3] and len({got[2][0], got[2][1], got[2][4]}) == 3
    rep = lib.last_dedup()
    assert rep["blocks_encoded"] == 3 and rep["candidate_pairs"] == 3 and rep["collisions"] == 0


# ------------------------------------------------------------------ 6. verify

def test_verify_checks_the_expanded_payloads(kolm_gpu, monkeypatch):
    kolm = kolm_gpu
    data = INPUTS["abc_tail"]
    want = plain(kolm, "abc_tail", "hot")
    assert kolm.compress_blocks_fixed(data, BS, hot_path=True, dedup=True, verify=True) == want
    v = kolm.last_verify()
    assert v["blocks"] == 9 and v["bad_blocks"] == 0 and v["bytes"] == len(data)
    assert kolm.last_dedup()["blocks_encoded"] == 4
    monkeypatch.setenv("KOLM_VERIFY_INJECT", "6")  # block 6 is the fourth A: a copy of block 0's payload
    with pytest.raises(kolm.KolmVerifyError) as ei:
        kolm.compress_blocks_fixed(data, BS, hot_path=True, dedup=True, verify=True)
    assert ei.value.block == 6 and "block 6" in str(ei.value)
    assert kolm.last_verify()["bad_blocks"] == 1 and kolm.last_dedup()["blocks_encoded"] == 4
    with pytest.raises(kolm.KolmVerifyError) as ei:
        kolm.encode_blocks(data, BS, hot_path=True, dedup=True, verify=True)
    assert ei.value.block == 6
    monkeypatch.delenv("KOLM_VERIFY_INJECT")
    assert kolm.compress_blocks_fixed(data, BS, hot_path=True, dedup=True, verify=True) == want
    assert kolm.compress_blocks_fixed(data, BS, hot_path=True) == want  # both switches went back
    assert kolm.last_dedup() == {}


# ------------------------------------------------------------------ 7. several device batches

def test_duplicates_across_device_batches(kolm_gpu, monkeypatch):
    kolm = kolm_gpu
    data = INPUTS["abc_tail"]
    want = plain(kolm, "abc_tail", "default")
    monkeypatch.setenv("KOLM_BATCH_BYTES", str(4 * BS))  # pieces A B A A | C B A C | tail
    assert kolm.compress_blocks_fixed(data, BS, dedup=True) == want
    rep = kolm.last_dedup()
    assert rep["blocks"] == 9 and rep["blocks_encoded"] == 2 + 3 + 1 and rep["candidate_pairs"] == 2 + 1
    assert kolm.compress_blocks_fixed(data, BS, dedup=True, verify=True) == want
    assert kolm.last_verify()["blocks"] == 9


# ------------------------------------------------------------------ 8. off is untouched

def test_off_reports_nothing_and_launches_nothing(lib):
    ctx = lib.device_ctx(lib.ensure_init())
    data = INPUTS["abc_tail"]
    mask = lib.KOLM_HOTPATH_MASK
    d_in = lib.input_buffer(ctx, data)
    arena = lib.DeviceBuffer(ctx, lib.arena_capacity(len(data), 9, mask))
    names = ("k_block_fp", "k_dedup_cmp", "k_range_gather")
    try:
        lib.check(lib.load().kolm_ctx_set_timing(ctx, 1))
        off = lib.encode_blocks_device(ctx, d_in.ptr, len(data), BS, arena.ptr, arena.nbytes, mask)
        pay_off = arena.download(int(off[2][-1]))
        assert lib.last_dedup() == {}
        r = lib.dedup_report(ctx)
        assert all(r[k] == 0 for k in r)
        before = {k: lib.kernel_times(ctx).get(k, {"launches": 0})["launches"] for k in names}
        on = lib.encode_blocks_device(ctx, d_in.ptr, len(data), BS, arena.ptr, arena.nbytes, mask, dedup=True)
        kt = lib.kernel_times(ctx)
        assert kt["k_block_fp"]["launches"] == before["k_block_fp"] + 1
        assert kt["k_dedup_cmp"]["launches"] == before["k_dedup_cmp"] + 1
        assert kt["k_range_gather"]["launches"] == before["k_range_gather"] + 2  # compaction, expansion
        assert kt["k_block_fp"]["bytes"] >= len(data)
        assert (on[0] == off[0]).all() and (on[1] == off[1]).all() and (on[2] == off[2]).all()
        assert arena.download(int(on[2][-1])) == pay_off
        r = lib.dedup_report(ctx)
        assert r["blocks"] == 9 and r["blocks_encoded"] == 4 and lib.last_dedup() == r
        assert on[3]["cyc_rounds_sum"] <= off[3]["cyc_rounds_sum"]  # the statistics describe the distinct blocks
        # and off again: the counts stay, the report is empty
        lib.encode_blocks_device(ctx, d_in.ptr, len(data), BS, arena.ptr, arena.nbytes, mask)
        assert {k: lib.kernel_times(ctx)[k]["launches"] for k in names} == {k: kt[k]["launches"] for k in names}
        assert lib.last_dedup() == {} and lib.dedup_report(ctx)["blocks"] == 0
    finally:
        lib.load().kolm_ctx_set_timing(ctx, 0)
        d_in.free()
        arena.free()
