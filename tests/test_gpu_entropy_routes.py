"""Every route of the stage after the BBWT gather - move-to-front (csrc/k_mtf.hip), the five Rice
sizes, the xor / lfsr counters, k_mdl and payload emission (csrc/k_entropy.hip) - reached on purpose
and checked exactly.  One test per row of the route matrix of tests/entropy_routes.py;
tests/test_entropy_route_model.py proves on the CPU that every row's input takes the routes the row
claims and that the numpy model equals the oracle on the rows' blocks.

Exactness.  For every block of every row, none sampled: the whole sizes row (candidates 0..6 and 8
from the model, the others disabled), the winner (the model's MDL: strict <, ties to the lowest id,
force overrides) and the payload (the model's bytes; LZ77, forced in the mosaic row, is the
oracle's) are equal, and the payloads of methods 2..6 decode back to the block through the host
decoder.  The entry points refuse the empty candidate mask with KOLM_EARG before any kernel runs, so
the `ties` row requires that answer for it; k_mdl's fall-back to raw when nothing is enabled cannot
be reached through the C ABI and is a rule of the model alone.

Route evidence from the device (rows marked mtf), with timing on: exactly one of k_mtf_wave /
k_mtf_replay was launched, the one the predictor names, and the bytes recorded for k_mtf_summary are
N + 256 * cpb * nb for the predicted chunk size - that is how chunks of 128 / 256 / 512 / 1024 bytes
are shown to have been taken.  Every such row then runs again with KOLM_MTF_WAVE set to the opposite
form: the same expectations, the evidence recomputed by the predictor with the switch.  The
per-thread paths (the summary's and the replay's access paths, registers against LDS, the emitter's
fast and slow forms, the lead of a tile) leave no trace on the device: for them the CPU test is the
evidence."""
import ctypes
import functools

import numpy as np
import pytest

import entropy_routes as E
import oracle as O
from kolm import decode as H

pytestmark = pytest.mark.gpu

KOLM_EARG, KOLM_ERANGE = -1, -7


@pytest.fixture(scope="module")
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


def _encode(lib, blocks, mask, force):
    """The batch through the device entry points (fixed geometry when the blocks allow it, block
    bounds otherwise); force: one method per block, or None.  (sizes, methods, payloads)."""
    ctx = lib.device_ctx(lib.ensure_init())
    data = b"".join(blocks)
    n, nb = len(data), len(blocks)
    lens = [len(b) for b in blocks]
    sizes = np.zeros((nb, lib.KOLM_NCAND), dtype=np.uint32)
    method = np.zeros(nb, dtype=np.uint32)
    off = np.zeros(nb + 1, dtype=np.uint64)
    fz = None if force is None else np.ascontiguousarray(np.asarray(force, dtype=np.int32))
    fp = None if fz is None else fz.ctypes.data
    st = lib.Stats()
    d_in = lib.input_buffer(ctx, data)
    arena = lib.DeviceBuffer(ctx, 9 * n + 64 * nb + 256)
    try:
        if E.is_fixed(lens):
            rc = lib.load().kolm_encode_blocks_device(ctx, d_in.ptr, n, lens[0], mask, fp, arena.ptr, arena.nbytes,
                                                      sizes.ctypes.data, method.ctypes.data, off.ctypes.data,
                                                      ctypes.byref(st))
        else:
            bounds = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
            rc = lib.load().kolm_encode_blocks_device_var(ctx, d_in.ptr, bounds.ctypes.data, nb, mask, fp, arena.ptr,
                                                          arena.nbytes, sizes.ctypes.data, method.ctypes.data,
                                                          off.ctypes.data, ctypes.byref(st))
        lib.check(rc, ctx)
        raw = arena.download(int(off[nb]))
    finally:
        d_in.free()
        arena.free()
    return sizes, method.tolist(), [raw[int(off[i]):int(off[i + 1])] for i in range(nb)]


def _kernels(lib):
    ctx = lib.device_ctx(lib.ensure_init())
    return {k: (v["launches"], v["bytes"]) for k, v in lib.kernel_times(ctx).items()}


def _encode_counted(lib, blocks, mask, force):
    """_encode with that call's launches and recorded bytes per kernel name."""
    ctx = lib.device_ctx(lib.ensure_init())
    try:
        lib.check(lib.load().kolm_ctx_set_timing(ctx, 1))
        before = _kernels(lib)
        out = _encode(lib, blocks, mask, force)
        after = _kernels(lib)
    finally:
        lib.load().kolm_ctx_set_timing(ctx, 0)
    zero = (0, 0)
    return out + ({k: (v[0] - before.get(k, zero)[0], v[1] - before.get(k, zero)[1]) for k, v in after.items()
                   if v[0] - before.get(k, zero)[0]},)


@functools.lru_cache(maxsize=None)
def _decoded(mid, payload, n):
    """The host decoder's output (equal payloads of equal blocks in several rows: decoded once)."""
    return H.decode_block(mid, payload, n)


def _check_run(lib, case, run, switch):
    if run.mask == 0:  # no candidate at all: refused before any kernel runs
        with pytest.raises(lib.KolmError) as e:
            _encode(lib, case.blocks(), run.mask, run.force)
        assert e.value.code == KOLM_EARG
        return
    want_sizes, want_win, want_pay = case.model(run)
    pred = case.predict(run, switch)
    sizes, method, pays, kern = _encode_counted(lib, case.blocks(), run.mask, run.force)
    tag = (case.name, hex(run.mask), switch)
    bad = np.flatnonzero((sizes != want_sizes).any(axis=1))
    assert bad.size == 0, (tag, "sizes", int(bad[0]), sizes[bad[0]].tolist(), want_sizes[bad[0]].tolist())
    assert method == want_win, (tag, "winner", next(i for i in range(len(method)) if method[i] != want_win[i]))
    for i, (blk, p, w) in enumerate(zip(case.blks(), pays, want_pay)):
        assert p == w, (tag, "payload", i, method[i], len(p), len(w))
        if method[i] in E.RICE_IDS:
            assert _decoded(method[i], p, blk.n) == blk.block, (tag, "host decode", i)
    if case.mtf:
        got = {k: v for k, v in kern.items() if k in ("k_mtf_wave", "k_mtf_replay", "k_mtf_summary")}
        print(f"\n{case.name} KOLM_MTF_WAVE={switch}: nb={len(method)} {pred.kernel} csz={pred.csz} cpb={pred.cpb} "
              f"summary bytes {got.get('k_mtf_summary')} / {pred.summary_bytes}  winners {sorted(set(method))}")
        other = "k_mtf_replay" if pred.kernel == "k_mtf_wave" else "k_mtf_wave"
        assert got.get(pred.kernel, (0, 0))[0] == 1 and other not in got, (tag, got)
        assert got["k_mtf_summary"] == (1, pred.summary_bytes), (tag, got)


@pytest.mark.parametrize("name", list(E.CASES))
def test_route(lib, monkeypatch, name):
    case = E.CASES[name]
    monkeypatch.delenv("KOLM_MTF_WAVE", raising=False)
    for run in case.runs():
        _check_run(lib, case, run, None)
    if case.mtf:  # the other replay form on the same bytes
        sw = E.opposite_switch(case)
        monkeypatch.setenv("KOLM_MTF_WAVE", str(sw))
        _check_run(lib, case, case.runs()[0], sw)


# ------------------------------------------------------------------ the direct entries

def _single_blocks():
    """Blocks for the one-block entries: the one-block row's, the deep-index blocks, the all-255 block
    and 64 KiB of the geometry rows' BBWT output (1 KiB chunks in the wave form, 64 chunks of 1 KiB or
    512 of 128 bytes in one block)."""
    out = list(E.CASES["wave_one_block"].blks()) + list(E.CASES["deep_indices"].blks())
    return out + [E.CASES["rice_slow_k2"].blks()[0], E.CASES["replay_512"].blks()[0]]


@pytest.mark.parametrize("switch", [None, "0", "1"])
def test_mtf_encode_direct(lib, monkeypatch, switch):
    """kolm_mtf_encode(L) == m, in the form batches of one block take and in both forced forms."""
    if switch is None:
        monkeypatch.delenv("KOLM_MTF_WAVE", raising=False)
    else:
        monkeypatch.setenv("KOLM_MTF_WAVE", switch)
    for i, b in enumerate(_single_blocks()):
        assert lib.mtf_encode(b.L) == b.m.tobytes(), (switch, i)


def _rice_sequences():
    n = 12 * 1024 + 5
    r = np.random.default_rng(17)
    rare = E.geometric(18, n, 0.5)
    rare[r.integers(0, n, 40)] = r.integers(200, 256, 40)
    return {"all_255": np.full(n, 255, np.uint8), "uniform": r.integers(0, 256, n, dtype=np.uint8), "rare_deep": rare}


@pytest.mark.parametrize("seq", ["all_255", "uniform", "rare_deep"])
def test_rice_encode_direct(lib, seq):
    """kolm_rice_encode for every k the C ABI accepts.  all_255 at k = 0 is the launch whose tiles
    fill the whole dynamic LDS buffer (2048 symbols of 256 bits)."""
    m = _rice_sequences()[seq]
    for k in range(16):
        got = lib.rice_encode(m.tobytes(), k)
        assert got == O.rice_encode(m.tobytes(), k), (seq, k)
        if k in (0, 2, 15):
            assert got == E.rice_code(m, k), (seq, k)


def _direct_blocks():
    return [E.CASES["wave_one_block"].blks()[0], E.CASES["rice_edge_64"].blks()[0], E.CASES["deep_indices"].blks()[0]]


def test_bbwt_mtf_rice_direct(lib, monkeypatch):
    """kolm_bbwt_mtf_rice: flags 0 for every k (rice_common on the device's own MTF output), the
    bitwise variants at k = 2 through the forced batched path."""
    monkeypatch.delenv("KOLM_MTF_WAVE", raising=False)
    for i, b in enumerate(_direct_blocks()):
        for k in range(16):
            assert lib.bbwt_mtf_rice(b.block, 0, k) == O.rice_encode(b.m.tobytes(), k), (i, k)
        for mid, flags in E.FLAG_OF.items():
            got = lib.bbwt_mtf_rice(b.block, flags, 2)
            assert got == E.payload(b.block, b.m, mid), (i, flags)
            assert H.decode_block(mid, got, b.n) == b.block, (i, flags)


def _raw_call(lib, name, data, *mid_args, cap=None):
    """The C entry itself (the Python wrappers size their buffers from k): (rc, out_len, out)."""
    cap = 9 * len(data) + 256 if cap is None else cap
    out = ctypes.create_string_buffer(cap)
    ln = ctypes.c_size_t(123)
    rc = getattr(lib.load(), name)(data, len(data), *mid_args, out, cap, ctypes.byref(ln))
    return rc, ln.value, out


def test_earg_answers(lib):
    """KOLM_EARG: k outside 0..15, flags that are no variant, a bitwise variant with k != 2."""
    lib.ensure_init()
    b = E.CASES["wave_one_block"].blks()[0]
    for k in (-1, 16):
        assert _raw_call(lib, "kolm_rice_encode", b.m.tobytes(), k)[0] == KOLM_EARG, k
        assert _raw_call(lib, "kolm_bbwt_mtf_rice", b.block, 0, k)[0] == KOLM_EARG, k
    for flags in (2, 3, 32, -1):
        assert _raw_call(lib, "kolm_bbwt_mtf_rice", b.block, flags, 2)[0] == KOLM_EARG, flags
    for flags in (1, 4, 8, 16):
        for k in (0, 1, 3, 15):
            assert _raw_call(lib, "kolm_bbwt_mtf_rice", b.block, flags, k)[0] == KOLM_EARG, (flags, k)
    # and the same calls with legal arguments answer KOLM_OK with the model's bytes
    rc, ln, out = _raw_call(lib, "kolm_bbwt_mtf_rice", b.block, 16, 2)
    assert rc == 0 and out.raw[:ln] == E.payload(b.block, b.m, 6)
    rc, ln, out = _raw_call(lib, "kolm_rice_encode", b.m.tobytes(), 15)
    assert rc == 0 and out.raw[:ln] == E.rice_code(b.m, 15)


# ------------------------------------------------------------------ a code of 2^32 bits

def test_rice_code_of_2_to_32_bits_is_refused(lib):
    """2^24 bytes of 255 at k = 0 are exactly 2^32 bits: the block's bit offsets are 32-bit, so the
    call answers KOLM_ERANGE from the count pass and writes nothing (it used to return KOLM_OK with
    wrong bytes).  The capacity given is tiny on purpose: the refusal comes before anything is sized."""
    lib.ensure_init()
    data = bytes([255]) * (1 << 24)
    rc, ln, out = _raw_call(lib, "kolm_rice_encode", data, 0, cap=64)
    assert rc == KOLM_ERANGE and ln == 0 and out.raw == bytes(64)
    assert b"2^32" in lib.load().kolm_last_error()


@pytest.mark.parametrize("n", [1 << 20, (1 << 24) - 4096])
def test_rice_code_just_under_2_to_32_bits(lib, n):
    """The largest input of 255s at k = 0 that stays under 2^32 bits ((2^24 - 4096) bytes: 512 MiB -
    128 KiB of output), and 2^20 bytes, against the closed form: every symbol is 255 ones and a zero,
    32 bytes of which the first 31 are 0xFF and the last 0xFE."""
    lib.ensure_init()
    data = bytes([255]) * n
    out = np.zeros(32 * n + 64, np.uint8)
    ln = ctypes.c_size_t(0)
    lib.check(lib.load().kolm_rice_encode(data, n, 0, out.ctypes.data, out.size, ctypes.byref(ln)))
    assert ln.value == 32 * n
    rows = out[:32 * n].reshape(-1, 32)
    assert (rows[:, :31] == 0xFF).all() and (rows[:, 31] == 0xFE).all() and not out[32 * n:].any()
