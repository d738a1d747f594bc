"""Round 0 of the cyclic sort with keys from the blocks' order-preserving prefix codes
(csrc/alpha_code.h, k_keypos_r0c in csrc/k_lsd.hip) against the oracle, every input in both key
forms (KOLM_R0_CODE = 0: fixed-width codes, 1: prefix codes): text, a batch mixing text / random
bytes (all 8-bit codes) / zeros (one symbol) / two symbols, one dominant byte with rare symbols
(depth cap, 2-bit padding, 32 characters per key), descending runs (every Lyndon factor 1-3 long:
the wrap path everywhere), periodic data, blocks of 1 and 5 bytes, alphabets of exactly 16 (fixed
form by default) and 17 symbols (prefix codes by default), and a 1 MiB text block."""
import functools

import numpy as np
import pytest

import oracle as O
from kolm import _lib
from kolm import datagen as D

pytestmark = pytest.mark.gpu


def _dominant():
    rng = np.random.default_rng(11)
    a = np.full(32768, 0x20, np.uint8)
    idx = rng.choice(32768, 328, replace=False)  # 1 % of the block: 40 rare symbols
    a[idx] = rng.integers(0x41, 0x41 + 40, 328, dtype=np.uint8)
    a[idx[:40]] = np.arange(0x41, 0x41 + 40, dtype=np.uint8)  # every one of them occurs
    return a.tobytes()


def _descending():
    rng = np.random.default_rng(12)
    out = bytearray()
    v = 255
    while len(out) < 8192:  # strictly descending runs with repeats of 1-3: factors of 1-3 bytes
        out += bytes([v]) * int(rng.integers(1, 4))
        v = v - int(rng.integers(1, 9))
        if v < 40:
            v = 255
    return bytes(out[:8192])


def _alphabet(sigma, n, seed):
    return bytes(np.random.default_rng(seed).integers(0, sigma, n, dtype=np.uint8) * 3 + 7)


@functools.lru_cache(maxsize=None)
def _inputs():
    text = D.enwik_like(3 * 65536 + 777, seed=43)
    rnd = D.splitmix64_bytes(4096, seed=6)
    two = bytes(np.random.default_rng(5).choice([97, 98], 4096).astype(np.uint8))
    return (
        ("text_64k_ragged", text, 65536),
        ("mixed_4k", text[:4096 * 3] + rnd + bytes(4096) + two + text[5000:5000 + 3000], 4096),
        ("dominant_32k", _dominant(), 32768),
        ("descending_8k", _descending(), 8192),
        ("periodic", (b"abcab" * 4000)[:19001], 8192),
        ("five_byte_blocks", b"b" + b"a" * 9 + b"xyz", 5),
        ("one_byte_blocks", b"hello world", 1),
        ("sigma_16", _alphabet(16, 20000, 7), 8192),
        ("sigma_17", _alphabet(17, 20000, 8), 8192),
    )


@functools.lru_cache(maxsize=None)
def _want(case):
    """The oracle's candidates 2..6 of every block and the container, computed once per input."""
    _, data, bs = _inputs()[case]
    blocks = [data[i:i + bs] for i in range(0, len(data), bs)]
    cands = [{m: O.candidate(m, b) for m in (2, 3, 4, 5, 6)} for b in blocks]
    return blocks, cands, O.compress_blocks_fixed(data, bs, range(9))


# every input in both forms; the 16 / 17 symbol alphabets (cases 7, 8) also in the default form
@pytest.mark.parametrize("case,mode", [(c, m) for c in range(9) for m in ("0", "1")] + [(7, None), (8, None)])
def test_codes_match_oracle(kolm_gpu, monkeypatch, case, mode):
    name, data, bs = _inputs()[case]
    if mode is None:
        monkeypatch.delenv("KOLM_R0_CODE", raising=False)
    else:
        monkeypatch.setenv("KOLM_R0_CODE", mode)
    blocks, cands, container = _want(case)
    sizes, method, pays, _ = _lib.encode_blocks(data, bs, _lib.KOLM_HOTPATH_MASK)
    assert len(method) == len(blocks)
    for i, blk in enumerate(blocks):
        for m in (2, 3, 4, 5, 6):  # the BBWT family: BBWT -> MTF -> map -> Rice
            assert int(sizes[i][m]) == len(cands[i][m]), (name, mode, i, m)
        want = cands[i].get(int(method[i])) or O.candidate(int(method[i]), blk)
        assert pays[i] == want, (name, mode, i)
    assert kolm_gpu.compress_blocks_fixed(data, bs, hot_path=True) == container, (name, mode)


@functools.lru_cache(maxsize=None)
def _mib():
    data = D.enwik_like(1 << 20, seed=78)
    return data, O.bbwt_forward(data)


@pytest.mark.parametrize("mode", ["0", "1"])
def test_codes_bbwt_1mib(kolm_gpu, monkeypatch, mode):
    """1 MiB of text (the bench's block size): 256 LSD tiles, ~14.5 characters per key."""
    monkeypatch.setenv("KOLM_R0_CODE", mode)
    data, want = _mib()
    assert _lib.bbwt_forward(data) == want


def test_codes_round_sum_batch_invariant(kolm_gpu, monkeypatch):
    """Prefix-code form: h0 is the constant 8 and a block's code depends on its bytes alone, so
    the per-block doubling rounds (cyc_rounds_sum) do not depend on the batch split."""
    monkeypatch.setenv("KOLM_R0_CODE", "1")
    bs = 65536
    data = D.enwik_like(7 * bs, seed=22)
    sums, outs = [], []
    for per in (7, 3, 1):
        monkeypatch.setenv("KOLM_BATCH_BYTES", str(per * bs + 100))
        outs.append(kolm_gpu.compress_blocks_fixed(data, bs, hot_path=True))
        sums.append(kolm_gpu.last_stats()["cyc_rounds_sum"])
    assert outs[0] == outs[1] == outs[2]
    assert sums[0] == sums[1] == sums[2] and sums[0] >= 7, sums
