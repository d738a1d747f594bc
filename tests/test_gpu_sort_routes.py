"""Every route of the omega-order sort's doubling rounds (csrc/k_sort.hip, sort_pass in
csrc/kolm_api.cpp), reached on purpose and checked exactly.  One test per row of the route matrix
of tests/sort_routes.py; tests/test_sort_route_model.py proves on the CPU that every
row's input is what the row claims.

Route evidence.  With KOLM_R0_CODE=0 the rows' batches get 8-bit fixed codes, round 0 holds exactly
8 characters and the numpy model of sort_routes is exact: the launch count of every sort kernel
(kolm_ctx_kernel_times, by the names sort_pass records), kolm_stats.cyc_active, cyc_rounds and
cyc_rounds_sum must equal the model's.  In the default prefix-code form a key holds 8 or more
characters, so the device's groups refine the model's: cyc_active may only be lower.

Correctness, in both forms.  The method-2 payload (BBWT -> MTF -> Rice) of every block decodes
back to the block through the host decoder: BBWT is a bijection, so that is an exact check of the
sorted order.  The first, the middle, the last and the four largest blocks also equal the oracle's
payload and their payload when encoded alone, a batch of one block that takes the routes of the
smallest batches.  For the three blocks over 200 KB (the 1 MiB block of the u64 row, the 909 KB
block of the early-gather rows, the 342 KB block of equal runs: the oracle's BBWT takes 2..10 s on
each) the expected payload is sort_routes.model_payload: the model's final order through the
oracle's MTF and Rice coders, which the CPU tests show equal to the oracle's on the shorter blocks."""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
import sort_routes as S
from kolm import decode as H

pytestmark = pytest.mark.gpu

EARLY = "k_bbwt_gather (early)"
MED = "k_small_sort<13> (medium)"
MSD = ("k_msd_hist", "k_msd_scan", "k_msd_scatter", "k_copy_back")
TINY = tuple(f"k_tiny_sort<{k}>" for k in (1, 2, 3, 4))
U32, U64 = "k_small_sort_all<u32>", "k_small_sort_all<u64>"

# The rows' evidence in words: (row name prefix, kernels that must run, kernels that must not).  The
# exact counts come from the model (test_route compares every sort kernel's launch count with it).
EVIDENCE = [
    ("tiny_dense", TINY + ("k_keypos",), ("k_keygen_small", U32, U64, MED) + MSD),  # the tiny sorts gather from KP
    ("tiny_sparse", TINY + ("k_keygen_small",), ("k_keypos", U32, U64, MED) + MSD),
    ("small_dense", (U32, "k_keypos"), (U64, MED, "k_finalize_eq") + MSD),
    ("small_sparse", (U32, "k_keygen_small"), ("k_keypos", U64, MED) + MSD),
    ("medium", (MED, "k_keygen_large"), MSD + ("k_finalize_eq",)),
    ("msd_moderate", MSD + ("k_keygen_large", "k_finalize_eq", "k_single"), (MED,)),
    ("msd_levels", MSD + ("k_finalize_eq",), (MED,)),
    ("mixed_medium_msd", (MED,) + MSD, ()),
    # under 64 blocks the buckets of 4500 split off at the first digit and are the medium sort's at the
    # next level; k_finalize_eq then finishes only runs over MED_T (or formed by the last digit)
    ("equal_runs_nb3", (MED,) + MSD, ("k_finalize_eq",)),
    ("equal_runs_nb64", MSD + ("k_finalize_eq",), (MED,)),
    ("equal_runs_over_medium", (MED, "k_finalize_eq") + MSD, ()),
    ("u64_words", (U64, U32), ("k_keypos",)),
    ("early_gather", (EARLY,), ()),
    ("early_off", (), (EARLY,)),
    ("retire", (U32, "k_keypos", "k_keygen_small", EARLY), ()),  # the early gather beside retired blocks
    ("multi_factor_tiny", TINY + ("k_keypos", "k_keygen_small"), (U32,)),
    ("multi_factor_small", TINY + (U32, "k_keypos"), (U64,)),
]


@pytest.fixture(scope="module")
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


def _encode(lib, blocks, mask, force):
    """The batch through the device entry points (fixed geometry when the blocks allow it, block
    bounds otherwise), every block forced to method `force`: (sizes, payloads, stats)."""
    ctx = lib.device_ctx(lib.ensure_init())
    data = b"".join(blocks)
    n, nb = len(data), len(blocks)
    lens = [len(b) for b in blocks]
    fixed = all(x == lens[0] for x in lens[:-1]) and lens[-1] <= lens[0]
    sizes = np.zeros((nb, lib.KOLM_NCAND), dtype=np.uint32)
    method = np.zeros(nb, dtype=np.uint32)
    off = np.zeros(nb + 1, dtype=np.uint64)
    fz = np.full(nb, force, dtype=np.int32)
    st = lib.Stats()
    d_in = lib.input_buffer(ctx, data)
    arena = lib.DeviceBuffer(ctx, 9 * n + 64 * nb + 256)
    try:
        if fixed:
            rc = lib.load().kolm_encode_blocks_device(ctx, d_in.ptr, n, lens[0], mask, fz.ctypes.data, arena.ptr,
                                                      arena.nbytes, sizes.ctypes.data, method.ctypes.data,
                                                      off.ctypes.data, ctypes.byref(st))
        else:
            bounds = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
            rc = lib.load().kolm_encode_blocks_device_var(ctx, d_in.ptr, bounds.ctypes.data, nb, mask, fz.ctypes.data,
                                                          arena.ptr, arena.nbytes, sizes.ctypes.data,
                                                          method.ctypes.data, off.ctypes.data, ctypes.byref(st))
        lib.check(rc, ctx)
        raw = arena.download(int(off[nb]))
    finally:
        d_in.free()
        arena.free()
    assert (method == force).all()
    return sizes, [raw[int(off[i]):int(off[i + 1])] for i in range(nb)], st.as_dict()


def _launches(lib):
    ctx = lib.device_ctx(lib.ensure_init())
    return {k: v["launches"] for k, v in lib.kernel_times(ctx).items()}


def _encode_counted(lib, blocks, mask, force=2):
    """_encode with the launch count per kernel name of that call."""
    ctx = lib.device_ctx(lib.ensure_init())
    try:
        lib.check(lib.load().kolm_ctx_set_timing(ctx, 1))
        before = _launches(lib)
        sizes, pays, st = _encode(lib, blocks, mask, force)
        after = _launches(lib)
    finally:
        lib.load().kolm_ctx_set_timing(ctx, 0)
    return sizes, pays, st, {k: v - before.get(k, 0) for k, v in after.items() if v - before.get(k, 0)}


@functools.lru_cache(maxsize=None)
def _oracle(block):
    return O.candidate(2, block) if len(block) <= S.ORACLE_MAX else S.model_payload(block)


@functools.lru_cache(maxsize=None)
def _decoded(payload, n):
    """The host decoder's output (equal payloads of equal blocks in several rows: decoded once)."""
    return H.decode_block(2, payload, n)


_alone_cache = {}


def _alone(lib, block):
    """The block's method-2 payload as a batch of its own, in the form of the current KOLM_R0_CODE."""
    import os
    key = (block, os.environ.get("KOLM_R0_CODE"))
    if key not in _alone_cache:
        _alone_cache[key] = _encode(lib, [block], S.HOT, 2)[1][0]
    return _alone_cache[key]


def _chosen(blocks):
    """The first, the middle and the last block of the batch, and its four largest."""
    nb = len(blocks)
    big = sorted(range(nb), key=lambda i: -len(blocks[i]))[:4]
    return sorted({0, nb // 2, nb - 1, *big})


def _want_launches(case, m):
    want = m.launches()
    # the early BBWT gather: 16 blocks or more, no Re-Pair, and doubling round 3 reached
    if m.nb >= 16 and case.mask == S.HOT and len(m.rounds) >= 3:
        want[EARLY] = 1
    return want


def _check_payloads(lib, blocks, pays, tag):
    for i, (b, p) in enumerate(zip(blocks, pays)):
        assert _decoded(p, len(b)) == b, (tag, "host decode", i)
    for i in _chosen(blocks):
        assert pays[i] == _oracle(blocks[i]), (tag, "oracle", i)
        assert pays[i] == _alone(lib, blocks[i]), (tag, "alone", i)


@pytest.mark.parametrize("name", list(S.CASES))
def test_route(lib, monkeypatch, name):
    case = S.CASES[name]
    blocks = case.blocks()
    m = case.model()
    assert m.fixed_8bit  # 8-bit fixed codes: the model is exact for KOLM_R0_CODE=0
    want = _want_launches(case, m)

    # fixed 8-bit form: the routes, exactly
    monkeypatch.setenv("KOLM_R0_CODE", "0")
    sizes, pays, st, got = _encode_counted(lib, blocks, case.mask)
    got = {k: v for k, v in got.items() if k in S.SORT_KERNELS or k == EARLY}
    print(f"\n{name}: nb={m.nb} N={m.N} bs={m.bs}")
    print(f"  launches device {sorted(got.items())}\n  launches model  {sorted(want.items())}")
    print(f"  cyc_active {st['cyc_active']} / {m.cyc_active}  cyc_rounds {st['cyc_rounds']} / {m.cyc_rounds}  "
          f"cyc_rounds_sum {st['cyc_rounds_sum']} / {m.rounds_sum}")
    must, must_not = next((a, b) for p, a, b in EVIDENCE if name.startswith(p))
    assert all(got.get(k, 0) >= 1 for k in must), [k for k in must if not got.get(k)]
    assert not any(got.get(k, 0) for k in must_not), [k for k in must_not if got.get(k)]
    large_rounds = sum(1 for x in m.rounds if x["hist"][S.NCLASS])
    if m.nb >= 64:  # every round with groups over TILE runs every MSD level of bitlen(bs)
        assert got.get("k_msd_hist", 0) == S.msd_levels(m.bs) * large_rounds
    assert got == want
    assert st["cyc_active"] == m.cyc_active
    assert st["cyc_rounds"] == m.cyc_rounds
    assert st["cyc_rounds_sum"] == m.rounds_sum
    _check_payloads(lib, blocks, pays, "fixed")

    # default form (prefix-code keys): the same bytes, and never more active slots than the model
    monkeypatch.delenv("KOLM_R0_CODE")
    sizes1, pays1, st1, got1 = _encode_counted(lib, blocks, case.mask)
    print(f"  default form: cyc_active {st1['cyc_active']} cyc_rounds {st1['cyc_rounds']}")
    assert st1["cyc_active"] <= m.cyc_active
    assert st1["cyc_rounds"] <= m.cyc_rounds
    assert got1.get(EARLY, 0) <= want.get(EARLY, 0)
    assert (sizes1 == sizes).all()
    _check_payloads(lib, blocks, pays1, "default")


@pytest.mark.parametrize("name", ["early_off_repair_nb20", "early_off_nb3"])
def test_early_gather_off_same_payloads(lib, monkeypatch, name):
    """Re-Pair in the mask, or fewer than 16 blocks, turns the early gather off: no early launch,
    and the payloads of the BBWT family (methods 2..6) are those of the batch that gathers early
    (the same blocks among 20 under the hot-path mask), which test_route checks against the
    decoder and the oracle."""
    case = S.CASES[name]
    on = S.CASES["early_gather_nb20"].blocks()
    blocks = case.blocks()
    at = [on.index(b) for b in blocks]  # where this batch's blocks are in the early-gather batch
    for mid in (2, 3, 4, 5, 6):
        sz_on, pay_on, _, l_on = _encode_counted(lib, on, S.HOT, mid)
        sz_off, pay_off, _, l_off = _encode_counted(lib, blocks, case.mask, mid)
        assert l_on.get(EARLY, 0) == 1 and l_off.get(EARLY, 0) == 0, mid
        assert [pay_on[i] for i in at] == pay_off, mid
        assert (sz_on[at][:, 2:7] == sz_off[:, 2:7]).all(), mid
