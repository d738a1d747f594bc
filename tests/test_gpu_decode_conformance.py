"""Device decoders (csrc/k_decode.hip) against the decoder conformance corpus: payloads no
encoder of this project writes, with PY's verdict recorded beside each
(tests/golden/decode_cases.json; only the JSON is read here).  The rule of
decode_cases.check_against_py holds for the device, and device and host agree on accept or
reject and on the bytes for every case.

Accepted cases decode in one batch per method, every case between two plain blocks of the same
method that must decode exactly (a decoder writing outside its own block's scratch — the LZ77
token slots — corrupts a neighbour); the batch is repeated behind a raw block of 0..7 bytes, so
every payload starts at every arena offset mod 8.  One batch of all methods goes through
kolm_decode_blocks_device into an output buffer with 64 guard bytes on each side.  Rejected
cases go one per batch as (good, bad, good) and the error names block 1."""
import ctypes

import numpy as np
import pytest

import decode_cases as DC
from kolm import decode as H

pytestmark = pytest.mark.gpu

CASES = DC.load()
BY_NAME = {c["name"]: c for c in CASES}
# the plain neighbour of every method: a well-formed corpus case with PY's bytes
PLAIN = {0: "raw_length/exact_7", 1: "xor_values/edge_values", 2: "rice_all_values/shuffled_256",
         3: "rice_bitplane/n_64", 4: "rice_inverse_maps/every_byte_id4", 5: "rice_inverse_maps/every_byte_id5",
         6: "rice_inverse_maps/every_byte_id6", 7: "lz_malformed/well_formed_5", 8: "lfsr_values/edge_values",
         9: "repair_forward/chain"}


def host(c):
    try:
        return H.decode_block(c["mid"], c["payload"], c["n"])
    except (ValueError, RuntimeError):
        return None


HOST = {c["name"]: host(c) for c in CASES}


def plain(mid):
    c = BY_NAME[PLAIN[mid]]
    want = DC.py_bytes(c)
    assert want is not None and HOST[c["name"]] == want
    return c, want


def sandwich(cases, shift):
    """(payloads, methods, lengths, expected bytes per block): a raw block of `shift` bytes,
    then plain, case, plain, case, ..., plain."""
    blocks = [(0, bytes(range(1, shift + 1)), shift, bytes(range(1, shift + 1)))] if shift else []
    for c in cases:
        p, want = plain(c["mid"])
        if not blocks or blocks[-1][0] != c["mid"] or blocks[-1][1] != p["payload"]:
            blocks.append((c["mid"], p["payload"], p["n"], want))
        blocks.append((c["mid"], c["payload"], c["n"], HOST[c["name"]]))
        blocks.append((c["mid"], p["payload"], p["n"], want))
    return [b[1] for b in blocks], [b[0] for b in blocks], [b[2] for b in blocks], [b[3] for b in blocks]


def split(out, lens):
    ob = np.concatenate([[0], np.cumsum(lens)])
    return [out[ob[i]:ob[i + 1]] for i in range(len(lens))]


@pytest.mark.parametrize("mid", range(10))
def test_accepted_cases_between_plain_blocks(kolm_gpu, mid):
    from kolm import _lib
    mine = [c for c in CASES if c["mid"] == mid and HOST[c["name"]] is not None]
    assert len(mine) >= 3
    for c in mine:
        DC.check_against_py(c, HOST[c["name"]])
    seen = set()
    for shift in range(8):
        pays, mids, lens, want = sandwich(mine, shift)
        offs = np.concatenate([[0], np.cumsum([len(p) for p in pays])])
        seen |= {(int(o) % 8) for o, p in zip(offs, pays) if p}
        got = split(_lib.decode_blocks(pays, mids, lens), lens)
        bad = [i for i in range(len(pays)) if got[i] != want[i]]
        assert not bad, (shift, bad[0], pays[bad[0]][:32].hex(), lens[bad[0]])
    assert seen == set(range(8))


@pytest.mark.parametrize("c", [c for c in CASES if HOST[c["name"]] is None],
                         ids=[c["name"] for c in CASES if HOST[c["name"]] is None])
def test_rejected_cases_name_their_block(kolm_gpu, c):
    from kolm import _lib
    DC.check_against_py(c, None)
    p, want = plain(c["mid"])
    with pytest.raises(_lib.KolmError, match="block 1"):
        _lib.decode_blocks([p["payload"], c["payload"], p["payload"]], [c["mid"]] * 3, [p["n"], c["n"], p["n"]])
    # and the neighbours alone still decode
    assert _lib.decode_blocks([p["payload"]] * 2, [c["mid"]] * 2, [p["n"]] * 2) == want * 2


def test_all_methods_one_device_batch_with_guards(kolm_gpu):
    """Every accepted case of every method in ONE batch through kolm_decode_blocks_device
    (payloads and output resident in device memory); the 64 bytes on each side of the output
    are unchanged."""
    from kolm import _lib
    L = _lib.load()
    order = sorted((c for c in CASES if HOST[c["name"]] is not None), key=lambda c: (c["n"] % 5, c["mid"]))
    pays, mids, lens, want = sandwich(order, 3)
    arena = b"".join(pays)
    off = np.zeros(len(pays) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in pays])
    meth = np.asarray(mids, np.uint32)
    ln = np.asarray(lens, np.uint32)
    total = int(ln.sum())
    G = 64
    ctx = ctypes.c_void_p()
    _lib.check(L.kolm_ctx_create(0, ctypes.byref(ctx)))
    try:
        dp, do = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.kolm_dev_alloc(ctx, len(arena) + 64, ctypes.byref(dp)))
        _lib.check(L.kolm_dev_alloc(ctx, total + 2 * G, ctypes.byref(do)))
        try:
            _lib.check(L.kolm_memcpy_h2d(ctx, dp, arena, len(arena)))
            _lib.check(L.kolm_memcpy_h2d(ctx, do, b"\xc3" * (total + 2 * G), total + 2 * G))
            _lib.check(L.kolm_decode_blocks_device(ctx, dp, off.ctypes.data, meth.ctypes.data, ln.ctypes.data,
                                                   len(pays), ctypes.c_void_p(do.value + G), total, None))
            out = ctypes.create_string_buffer(total + 2 * G)
            _lib.check(L.kolm_memcpy_d2h(ctx, out, do, total + 2 * G))
        finally:
            L.kolm_dev_free(ctx, dp)
            L.kolm_dev_free(ctx, do)
    finally:
        L.kolm_ctx_destroy(ctx)
    raw = out.raw
    assert raw[:G] == b"\xc3" * G and raw[G + total:] == b"\xc3" * G
    got = split(raw[G:G + total], lens)
    bad = [i for i in range(len(pays)) if got[i] != want[i]]
    assert not bad, (bad[0], mids[bad[0]], pays[bad[0]][:32].hex())
