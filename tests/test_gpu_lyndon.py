"""The Lyndon stage's two routes on the device: factor starts from prefix-minimum candidates
(KOLM_LYN_FAST=1, the default) and the parallel Duval kernels (KOLM_LYN_FAST=0, and every block
the fast route gives up on).  Every case runs with both settings through the public entry points
(kolm.bbwt_forward, _lib.encode_blocks with method 2 forced, _lib.encode_blocks_var); the outputs
must equal each other and the oracle, and kolm_ctx_lyndon_report must show the expected routes.
The method-2 payload (BBWT + MTF + Rice) depends on every factor start of its block."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle as O
from kolm import datagen as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEXT = D.enwik_like(1 << 18, seed=11)
_want = {}


def want2(block: bytes) -> bytes:
    """The oracle's method-2 payload, computed once per distinct block."""
    if block not in _want:
        _want[block] = O.candidate(2, block)
    return _want[block]


def both(monkeypatch, fn):
    """fn() under KOLM_LYN_FAST = 0 and = 1 -> {setting: (result, report)}."""
    from kolm import _lib
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("KOLM_LYN_FAST", mode)
        res = fn()
        out[mode] = (res, _lib.lyndon_report())
    monkeypatch.delenv("KOLM_LYN_FAST")
    return out


def check_batch(monkeypatch, data, blocks, encode, accepted):
    """encode() -> payloads of `blocks`; `accepted` blocks take the fast route when it is on."""
    got = both(monkeypatch, encode)
    nb = len(blocks)
    assert got["0"][1] == {"accepted": 0, "fallback": nb}
    assert got["1"][1] == {"accepted": accepted, "fallback": nb - accepted}
    assert got["0"][0] == got["1"][0]
    for i, blk in enumerate(blocks):
        assert got["1"][0][i] == want2(blk), f"block {i} of {nb}"


@pytest.mark.parametrize("n", [1, 7, 8, 9, 4095, 4096, 4097, 8191, 8192, 8193])
def test_single_block_shapes(kolm_gpu, monkeypatch, n):
    from kolm import _lib
    data = TEXT[100:100 + n]
    check_batch(monkeypatch, data, [data], lambda: _lib.encode_blocks(data, n, force=[2])[2], 1)
    bw = both(monkeypatch, lambda: kolm_gpu.bbwt_forward(data))
    assert bw["0"][0] == bw["1"][0] == O.bbwt_forward(data)
    assert bw["1"][1] == {"accepted": 1, "fallback": 0} and bw["0"][1] == {"accepted": 0, "fallback": 1}


def test_mixed_batch_routes_side_by_side(kolm_gpu, monkeypatch):
    """Accepted and fallback blocks alternate in one batch; the last block is a ragged tail."""
    from kolm import _lib
    bs = 1 << 16
    parts = [TEXT[:bs], bytes(bs), (bytes(range(96)) * 700)[:bs], TEXT[bs:2 * bs],
             b"\x01" + TEXT[3 * bs:4 * bs - 1 - 3000] + bytes(3000), D.splitmix64_bytes(bs), TEXT[5000:5000 + 1234]]
    data = b"".join(parts)
    assert [len(p) for p in parts] == [bs] * 6 + [1234]
    # zeros: one candidate per byte; period 96: common prefixes of whole periods; the zero run at a
    # block's end: 3000 candidates.  Text and random bytes stay far inside both budgets.
    check_batch(monkeypatch, data, parts, lambda: _lib.encode_blocks(data, bs, force=[2] * 7)[2], 4)


def test_variable_geometry(kolm_gpu, monkeypatch):
    """Chunks of 8-16 KiB at odd offsets (no block begins at an aligned address), one of zeros."""
    from kolm import _lib
    rng = np.random.default_rng(12)
    lens = [int(x) | 1 for x in rng.integers(8192, 16384, 9)]
    parts, pos = [], 0
    for i, ln in enumerate(lens):
        parts.append(bytes(ln) if i == 4 else TEXT[pos:pos + ln])
        pos += ln
    data = b"".join(parts)
    bounds = np.concatenate([[0], np.cumsum(lens)])
    check_batch(monkeypatch, data, parts,
                lambda: _lib.encode_blocks_var(data, bounds, force=[2] * len(parts))[2], len(parts) - 1)


def staircase(k: int, n: int, step: int) -> bytes:
    """Exactly k candidates (all factor starts): strictly falling two-byte values in a larger filler."""
    s = bytearray(b"\xf0" * n)
    for i in range(k):
        s[i * step], s[i * step + 1] = 8 - i // 200, 239 - i % 200
    return bytes(s)


def lcp_pair(L: int) -> bytes:
    """Three candidates; the first two share exactly L bytes, no other pair shares any."""
    return b"b" + b"z" * (L - 1) + b"c" + b"b" + b"z" * (L - 1) + b"a"


@pytest.mark.parametrize("name,block,accepted", [
    ("16 candidates", staircase(16, 9000, 500), 1), ("17 candidates", staircase(17, 9000, 500), 0),
    ("lcp 16", lcp_pair(16), 1), ("lcp 17", lcp_pair(17), 0)],
    ids=["cand16", "cand17", "lcp16", "lcp17"])
def test_lowered_caps(kolm_gpu, monkeypatch, name, block, accepted):
    from kolm import _lib
    monkeypatch.setenv("KOLM_LYN_CAND_MAX", "16")
    monkeypatch.setenv("KOLM_LYN_LCP_MAX", "16")
    check_batch(monkeypatch, block, [block], lambda: _lib.encode_blocks(block, len(block), force=[2])[2], accepted)
    monkeypatch.delenv("KOLM_LYN_CAND_MAX")
    monkeypatch.delenv("KOLM_LYN_LCP_MAX")
    check_batch(monkeypatch, block, [block], lambda: _lib.encode_blocks(block, len(block), force=[2])[2], 1)


def test_bench_block_accepted(kolm_gpu, monkeypatch):
    """Block 0 of the benchmark's rank-0 stream (1 MiB): accepted; its payload against the oracle's
    recorded answer — tests/golden/bench_stream.json holds the size of O.candidate(2, block) and,
    method 2 being the block's winner there, its sha256."""
    from kolm import _lib
    with open(os.path.join(GOLDEN, "bench_stream.json")) as f:
        g = json.load(f)["ranks"]["0"]
    rec = g["blocks"][0]
    assert rec["w9"] == 2
    bs = g["block_size"]
    data = D.enwik_like(bs, seed=g["seed"])
    got = both(monkeypatch, lambda: _lib.encode_blocks(data, bs, force=[2])[2][0])
    assert got["1"][1] == {"accepted": 1, "fallback": 0}
    assert got["0"][0] == got["1"][0]
    assert len(got["1"][0]) == rec["sizes"][2]
    assert hashlib.sha256(got["1"][0]).hexdigest() == rec["sha9"]
