"""The route matrix of tests/sort_routes.py on the CPU: (1) the numpy model of the doubling rounds
against brute force (the rotation prefixes sorted directly), (2) every row of the matrix is what it
claims - the exact group counts, densities, round depths and launch counts that
tests/test_gpu_sort_routes.py relies on, so that no row can pass there vacuously, and (3) BBWT is a
bijection on every case block (the host decode used as the second check on the GPU side)."""
import numpy as np
import pytest

import oracle as O
import sort_routes as S
from kolm import decode as H

MED = "k_small_sort<13> (medium)"
# the group sizes the rows claim, written out here (not taken from the builder's lists)
TINY_SIZES = (2, 3, 4, 5, 8, 9, 16)
SMALL_SIZES = (17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)
EARLY_SIZES = (40, 200, 600, 3000)
MSD = ("k_msd_hist", "k_msd_scan", "k_msd_scatter", "k_copy_back")


# ------------------------------------------------------------------ 1. the model against brute force

def _descending(seed, n):
    """Strictly descending runs with repeats of 1..3: Lyndon factors of 1..3 bytes, every
    rotation wraps inside the first 8 characters."""
    rng = np.random.default_rng(seed)
    out, v = bytearray(), 255
    while len(out) < n:
        out += bytes([v]) * int(rng.integers(1, 4))
        v -= int(rng.integers(1, 9))
        if v < 200:
            v = 255
    return bytes(out[:n])


BRUTE = {
    "single_factor": S.build_block(1, [(3, 20), (5, 12), (2, 40)], filler=40),
    "single_factor_two_valued": S.build_block(2, [S.Fam(6, 24, two=True), S.Fam(4, 20, pin=True)]),
    "multi_factor": S.build_block(3, [(3, 20), (5, 12), (2, 40)], filler=40, lead=False, split=True),
    "multi_factor_plain": S.build_block(3, [(3, 20), (5, 12), (2, 40)], filler=40, lead=False),
    "multi_factor_two_symbols": bytes(np.random.default_rng(4).choice([97, 98], 300).astype(np.uint8)),
    "factors_of_1_to_3_bytes": _descending(5, 250),
    "periodic": S.periodic_block(6, 30, 6),
    "periodic_short_word": S.periodic_block(7, 5, 40),  # the word is shorter than round 0's 8 characters
    "one_symbol": b"a" * 50,
    "one_byte": b"z",
}


def _round_stats(prev_rank):
    """dict(active, hist, sizes, longest) of the groups of a rank array, as the model reports them."""
    cnt = np.bincount(prev_rank)
    g = cnt[cnt >= 2]
    hist = [0] * (S.NCLASS + 1)
    for x in g.tolist():
        hist[S.size_class(x) if x <= S.TILE else S.NCLASS] += 1
    sizes, mult = np.unique(g, return_counts=True)
    return dict(active=int(g.sum()), hist=hist, sizes=dict(zip(sizes.tolist(), mult.tolist())),
                longest=int(g.max()) if g.size else 0)


@pytest.mark.parametrize("name", list(BRUTE))
def test_model_against_brute_force(name):
    block = BRUTE[name]
    m = S.BlockModel(block, keep_ranks=True)
    # the ranks after round r are those of the rotations' first 8 * 2^r characters
    brute = [S.rotation_classes(block, S.H0 << r) for r in range(len(m.ranks) + 1)]
    for r, rk in enumerate(m.ranks):
        assert (rk == brute[r]).all(), (name, r)
    # retirement: the model stops after the first round that changes nothing (round 0: a block
    # of one group), or when no group of two is left
    changed = [bool((brute[r + 1] != brute[r]).any()) for r in range(len(brute) - 1)]
    split0 = bool(brute[0].max() > 0)
    live, want_rounds, last_split = split0, [], 0
    for r in range(1, len(brute)):
        if not live or _round_stats(brute[r - 1])["active"] == 0:
            break
        want_rounds.append(_round_stats(brute[r - 1]))
        live = changed[r - 1]
        if live:
            last_split = r
    assert len(m.rounds) == len(want_rounds), name
    for got, want in zip(m.rounds, want_rounds):
        assert {k: got[k] for k in want} == want, name
    for r, got in enumerate(m.rounds, 1):
        assert got["bucket"] == int(np.bincount(brute[r]).max()), (name, r)
        assert sorted(zip(got["starts"].tolist(), got["lens"].tolist())) == sorted(
            (int(s), int(c)) for s, c in enumerate(np.bincount(brute[r - 1]).tolist()) if c >= 2), (name, r)
    assert m.last_split == last_split, name


def test_brute_force_blocks_cover_the_shapes():
    """What the brute-force inputs are: one factor, many factors, factors shorter than 8, and
    blocks that retire while groups are still tied."""
    nfac = {k: len(O.duval_starts(v)) for k, v in BRUTE.items()}
    assert nfac["single_factor"] == 1 and nfac["single_factor_two_valued"] == 1
    assert nfac["multi_factor"] == 7 and nfac["multi_factor_two_symbols"] > 10  # 3 families, filler, 3 single bytes
    assert nfac["factors_of_1_to_3_bytes"] > 20 and nfac["periodic"] == 6 and nfac["periodic_short_word"] == 40
    for name in ("periodic", "periodic_short_word", "one_symbol"):
        m = S.BlockModel(BRUTE[name])
        assert m.last_split == 0 and len(m.rounds) <= 1, name  # retired with every group still tied
    assert len(S.BlockModel(BRUTE["periodic"]).rounds) == 1 and S.BlockModel(BRUTE["one_symbol"]).rounds == []
    assert len(S.BlockModel(BRUTE["single_factor"]).rounds) >= 3  # h = 8, 16, 32 against words of 40


def test_msd_round_by_hand():
    """msd_round on keys whose digits are chosen by hand (18-bit keys: digits of 8, 8 and 2 bits)."""
    k = np.arange(3000, dtype=np.int64)
    assert S.msd_round([], 18, False) == dict(levels=0, medium=0, eq=0, added=[0] * S.NCLASS)
    # batches under 64 blocks, nothing over MED_T: one medium launch, no level
    assert S.msd_round([k], 18, True) == dict(levels=0, medium=1, eq=0, added=[0] * S.NCLASS)
    # 3000 distinct keys 0..2999: the top digit (key >> 10) has buckets of 1024, 1024 and 952
    r = S.msd_round([k], 18, False)
    assert (r["levels"], r["medium"], r["eq"]) == (3, 0, 0) and r["added"][10] == 3 and sum(r["added"]) == 3
    # one key 3000 times: an equal-key run after the last digit; with 2 distinct low bits: two buckets of 1500
    assert S.msd_round([np.full(3000, 77)], 18, False)["eq"] == 1
    r = S.msd_round([np.full(3000, 76) + (k & 1)], 18, False)
    assert r["eq"] == 0 and r["added"][11] == 2
    # under 64 blocks a group over MED_T runs the levels, each with a medium launch; its buckets of
    # 2049..8192 formed before the last digit are the medium sort's, at the last digit equal-key runs
    big = np.concatenate([np.full(4500, 5 << 10), np.full(4500, 9 << 10)])
    assert S.msd_round([big], 18, True) == dict(levels=3, medium=3, eq=0, added=[0] * S.NCLASS)
    assert S.msd_round([big], 18, False)["eq"] == 2
    low = np.concatenate([np.full(4500, 4), np.full(4500, 5)])
    assert S.msd_round([low], 18, True)["eq"] == 2
    # single elements join class 0
    assert S.msd_round([np.concatenate([np.full(2999, 1), [1 << 17]])], 18, False)["added"][0] == 1
    assert [S.msd_levels(b) for b in (255, 256, 65535, 65536, 65537, 1 << 20, (1 << 24) - 1, 1 << 24)] == [
        1, 2, 2, 3, 3, 3, 3, 4]


# ------------------------------------------------------------------ 2. every row is what it claims

def _large_rounds(m):
    return [r for r, x in enumerate(m.rounds, 1) if x["hist"][S.NCLASS]]


def _claim_tiny(m, L, dense, multi=False):
    for g in TINY_SIZES:
        assert m.groups(1, g) >= 33 * m.nb, g     # offsets 0..32 of a 40-byte word tie on 8 characters
        assert m.groups(3, g) >= 9 * m.nb, g      # h = 32: offsets 0..8 still tie
    assert all(m.dense(r) == dense for r in (1, 2, 3))
    assert all(sum(x["hist"][5:]) == 0 and min(x["hist"][1:5]) > 0 for x in m.rounds[:3])
    if multi:
        # round 4 holds only the three equal one-byte factors at every block's end, which tie for
        # ever: a sparse round that splits nothing and retires the blocks with a group still tied
        assert len(m.rounds) == 4 and m.rounds[3]["sizes"] == {3: m.nb} and not m.dense(4)
        assert all(b.last_split == 3 and b.rounds[3]["bucket"] == 3 for b in m.blocks)
        assert L["k_tiny_sort<2>"] == 4 and L["k_keygen_small"] == 1
    else:
        assert len(m.rounds) == 3 and L["k_tiny_sort<2>"] == 3
        assert L.get("k_keygen_small", 0) == (0 if dense else 3)
    assert all(L[f"k_tiny_sort<{k}>"] == 3 for k in (1, 3, 4))
    assert L.get("k_keypos", 0) == (3 if dense else 0)
    assert not any(k in L for k in MSD + (MED, "k_small_sort_all<u32>", "k_finalize_eq", "k_single"))


def _claim_small(m, L, dense, word, rounds, multi=False):
    per = word - 7  # offsets 0..word-8 tie on 8 characters
    for g in SMALL_SIZES:
        assert m.groups(1, g) >= per, g
        assert S.size_class(g) == {17: 5, 32: 5, 33: 6, 64: 6, 65: 7, 128: 7, 129: 8, 256: 8, 257: 9, 512: 9, 513: 10,
                                   1024: 10, 1025: 11, 2048: 11}[g]
    assert all(m.dense(r) == dense for r in range(1, rounds + 1))
    if multi:  # as in the tiny row: a last sparse round of the tied one-byte factors
        assert len(m.rounds) == rounds + 1 and m.rounds[rounds]["sizes"] == {3: 2} and not m.dense(rounds + 1)
    else:
        assert len(m.rounds) == rounds
    for x in m.rounds[:rounds]:
        assert min(x["hist"][5:12]) >= 5 and x["hist"][S.NCLASS] == 0 and x["longest"] == 2048
    assert L["k_small_sort_all<u32>"] == rounds and "k_small_sort_all<u64>" not in L
    assert L.get("k_keypos", 0) == (rounds if dense else 0) and L["k_keygen_small"] == len(m.rounds)
    assert not any(k in L for k in MSD + (MED, "k_finalize_eq", "k_single"))


def _claim_medium(m, L):
    for g in (2049, 4096, 8192):
        assert m.groups(1, g) == 10 and m.groups(2, g) == 2, g
    assert [x["longest"] for x in m.rounds] == [8192, 8192] and [x["hist"][S.NCLASS] for x in m.rounds] == [30, 6]
    assert _large_rounds(m) == [1, 2] and m.bs == 163841 and S.msd_levels(m.bs) == 3


def _claim_early(m, L, nb, case_blocks):
    assert m.nb == nb and len(m.rounds) == 6
    for g in EARLY_SIZES[:case_blocks]:
        assert [m.groups(r, g) for r in range(1, 8)] == [293, 285, 269, 237, 173, 45, 0], g
    for r in (3, 4, 5, 6):
        x = m.rounds[r - 1]
        long = x["lens"] >= 64  # segments in which k_mark_active writes whole 64-bit words
        assert int(x["lens"][long].sum()) >= (170_000 if case_blocks == 4 else 30_000), r
        if r == 3 and case_blocks == 4:  # their starts fall at every residue mod 64, their ends too
            assert len(set((x["starts"][long] % 64).tolist())) == 64
            assert len(set(((x["starts"][long] + x["lens"][long]) % 64).tolist())) == 64


def _claims(name, case, m, L):
    nb = m.nb
    lvl = S.msd_levels(m.bs)
    if name.startswith("tiny_dense"):
        assert nb == int(name.split("nb")[1]) and m.bs == 2022
        _claim_tiny(m, L, True)
    elif name.startswith("tiny_sparse"):
        assert nb == int(name.split("nb")[1])
        _claim_tiny(m, L, False)
    elif name == "multi_factor_tiny_nb3":
        _claim_tiny(m, L, True, multi=True)
    elif name == "multi_factor_small_nb3":
        _claim_small(m, L, True, 24, 2, multi=True)
    elif name.startswith("small_dense"):
        assert nb == int(name.split("nb")[1])
        _claim_small(m, L, True, 24, 2)
    elif name.startswith("small_sparse"):
        assert nb == int(name.split("nb")[1])
        _claim_small(m, L, False, 12, 1)
    elif name in ("medium_nb3", "medium_nb20"):
        assert nb == int(name.split("nb")[1])
        _claim_medium(m, L)
        assert L[MED] == 2 and not any(k in L for k in MSD + ("k_finalize_eq", "k_single"))
    elif name == "msd_moderate_nb64":
        assert nb == 64
        _claim_medium(m, L)
        assert all(L[k] == 2 * lvl == 6 for k in MSD) and MED not in L
        # round 1 cannot split the groups of offset 0 (their successors still tie): runs of equal keys
        assert m.rounds[0]["bucket"] == 8192 and m.rounds[1]["bucket"] == 1 and L["k_finalize_eq"] == 1
        assert L["k_single"] == 2  # round 2's keys are distinct: some digit buckets hold one element
    elif name.startswith("msd_levels_bs"):
        bs = int(name.split("bs")[1])
        assert nb == 64 and m.bs == bs and lvl == {65535: 2, 65536: 3, 65537: 3}[bs]
        assert _large_rounds(m) == [1, 2] and all(L[k] == 2 * lvl for k in MSD) and MED not in L
        assert m.groups(1, 2100) == 8 and m.groups(2, 2100) == 8
        # the pin: the successors of the copies' first 8 offsets are in the block's highest group
        top = max(int(g.max()) for g in m.rounds[0]["large"])
        assert all(int(g.min()) == top for g in m.rounds[0]["large"] if len(g) == 2100) and top + 27309 == bs
        # round 2 sorts groups of 2100 by 2100 distinct keys: buckets of every digit, down to the classes
        assert any(len(np.unique(g)) == 2100 for g in m.rounds[1]["large"])
    elif name == "mixed_medium_msd_nb3":
        assert nb == 3 and m.groups(1, 8193) == 10 and m.groups(1, 3000) == 10
        assert m.groups(2, 8193) == 2 and m.groups(2, 3000) == 2 and lvl == 3
        # both rounds have a group over MED_T: every level runs with a medium launch before it
        assert L[MED] == 6 and all(L[k] == 6 for k in MSD) and L["k_finalize_eq"] == 1
    elif name == "equal_runs_nb3":
        assert nb == 3 and m.groups(1, 9000) == 1 and m.groups(1, 4500) == 18 and m.rounds[0]["bucket"] == 4500
        assert [x["longest"] for x in m.rounds] == [9000, 4500] and lvl == 3
        # round 1: the group of 9000 runs the three levels; its two buckets of 4500 split off at the
        # first digit and are the medium sort's at the second level (not equal-key runs: under 64
        # blocks k_finalize_eq finishes only runs over MED_T, or ones formed by the last digit)
        g9000 = [g for g in m.rounds[0]["large"] if len(g) == 9000]
        assert [np.unique(g, return_counts=True)[1].tolist() for g in g9000] == [[4500, 4500]]
        assert S.msd_round(m.rounds[0]["large"], S.bitlen(m.bs), True) == dict(levels=3, medium=3, eq=0,
                                                                              added=[0] * S.NCLASS)
        assert L[MED] == 4 and all(L[k] == 3 for k in MSD) and "k_finalize_eq" not in L
    elif name == "equal_runs_nb64":
        assert nb == 64 and m.groups(1, 5000) == 1 and m.rounds[0]["bucket"] == 2500 and m.rounds[1]["bucket"] == 1
        g5000 = [g for g in m.rounds[0]["large"] if len(g) == 5000]
        assert [np.unique(g, return_counts=True)[1].tolist() for g in g5000] == [[2500, 2500]]
        assert S.msd_round(g5000, S.bitlen(m.bs), False)["eq"] == 2  # the two buckets of 2500
        assert L["k_finalize_eq"] == 1 and all(L[k] == 2 * lvl for k in MSD) and MED not in L
    elif name == "equal_runs_over_medium_nb3":
        assert nb == 3 and m.groups(1, 18000) == 1 and m.rounds[0]["bucket"] == 9000 > S.MED_T
        g18000 = [g for g in m.rounds[0]["large"] if len(g) == 18000]
        assert [np.unique(g, return_counts=True)[1].tolist() for g in g18000] == [[9000, 9000]]
        assert S.msd_round(g18000, S.bitlen(m.bs), True)["eq"] == 2  # the two buckets of 9000
        assert L["k_finalize_eq"] == 1 and L[MED] == 6 and all(L[k] == 6 for k in MSD)
    elif name == "u64_words":
        assert m.bs == (1 << 20) + 1 and S.bitlen(m.bs - 1) == 21  # 21 + 11 > 31 >= 21 + 10
        assert [m.groups(r, 1500) for r in (1, 2, 3, 4)] == [33, 25, 9, 0]
        assert [m.groups(r, 700) for r in (1, 2, 3, 4)] == [33, 25, 9, 0]
        assert S.size_class(1500) == 11 and S.size_class(700) == 10 and not any(m.dense(r) for r in (1, 2, 3))
        assert L["k_small_sort_all<u64>"] == 3 and L["k_small_sort_all<u32>"] == 3
    elif name in ("early_gather_nb20", "early_gather_nb64", "early_off_repair_nb20"):
        _claim_early(m, L, int(name.split("nb")[1]), 4)
        assert case.mask == (S.DEFAULT if "repair" in name else S.HOT)
        assert L["k_classify"] == 7 and L["k_keygen_large"] == 6
    elif name == "early_off_nb3":
        _claim_early(m, L, 3, 3)
        assert case.blocks() == tuple(S.CASES["early_gather_nb20"].blocks()[i] for i in (0, 6, 13))
    elif name == "retire_nb20":
        assert nb == 20
        for i, b in enumerate(m.blocks):
            if i % 2 == 0:  # periodic: 300 groups of its 20 copies, which round 1 cannot split
                assert b.last_split == 0 and len(b.rounds) == 1 and b.rounds[0]["sizes"] == {20: 300}
                assert b.rounds[0]["active"] == b.n == 6000
            else:
                assert b.last_split == 6 and len(b.rounds) == 6
        assert m.groups(1, 20) == 3000 and m.groups(2, 20) == 0 and m.groups(6, 40) == 450
        assert m.rounds_sum == 10 * 1 + 10 * 7 and m.cyc_rounds == 7
        assert m.rounds[0]["active"] - m.rounds[1]["active"] > 60000  # the retired blocks' slots leave
    else:
        raise AssertionError(f"no claims for row {name}")


@pytest.mark.parametrize("name", list(S.CASES))
def test_row_is_what_it_claims(name):
    case = S.CASES[name]
    m = case.model()
    assert m.fixed_8bit  # KOLM_R0_CODE=0 gives 8-bit codes: round 0 holds exactly 8 characters
    assert m.nb == len(case.blocks()) and m.N == sum(len(b) for b in case.blocks()) < 1 << 21
    L = m.launches()
    assert L["k_classify"] == m.cyc_rounds == 1 + len(m.rounds)
    assert m.cyc_active == m.N + sum(x["active"] for x in m.rounds)
    _claims(name, case, m, L)


def test_multi_factor_rows_have_many_factors():
    for name, nfam in (("multi_factor_tiny_nb3", (7, 7, 7)), ("multi_factor_small_nb3", (11, 3))):
        for b, k in zip(S.CASES[name].blocks(), nfam):
            lens = np.diff(O.duval_starts(b) + [len(b)]).tolist()
            # every family a factor of its own (so every h wraps near the factors' ends), then three
            # factors of one byte (every key wraps several times)
            assert len(lens) == k + 3 and lens[-3:] == [1, 1, 1] and min(lens[:-3]) > 64, name
    for name in ("tiny_dense_nb3", "small_dense_nb3", "medium_nb3", "u64_words"):
        assert all(O.duval_starts(b) == [0] for b in S.CASES[name].blocks()), name  # one Lyndon word


def test_matrix_batch_shapes():
    """The three batch shapes of sort_pass, and the rows the issue's matrix asks for."""
    nbs = {n: len(c.blocks()) for n, c in S.CASES.items()}
    assert {3, 20, 64} <= set(nbs.values())
    for row in ("tiny_dense", "small_dense"):
        assert {nbs[f"{row}_nb{k}"] for k in (3, 20, 64)} == {3, 20, 64}
    assert all(b < 16 for n, b in nbs.items() if n.endswith("nb3")) and all(16 <= nbs[n] < 64 for n in nbs if n.endswith("nb20"))


# ------------------------------------------------------------------ 3. BBWT is a bijection on the case blocks

def _distinct_blocks():
    seen = {}
    for name, c in S.CASES.items():
        for i, b in enumerate(c.blocks()):
            seen.setdefault(b, f"{name}[{i}]")
    return sorted(seen.items(), key=lambda kv: len(kv[0]))


def test_bbwt_bijection_on_case_blocks():
    """decode.bbwt_inverse(bbwt(block)) == block for every distinct block of the matrix: the host
    decode is an exact check of the sorted order.  bbwt: the oracle's for blocks up to 200 KB, where
    the model's final order must give the same bytes, and the model's alone for the longer ones
    (the oracle takes 2..10 s on each of them).  model_payload, which stands in for the oracle's
    candidate 2 on those blocks in the GPU tests, is that candidate on the blocks up to 64 KiB."""
    for b, where in _distinct_blocks():
        bw = S.block_model(b).bbwt()
        if len(b) <= S.ORACLE_MAX:
            assert O.bbwt_forward(b) == bw, where
        if len(b) <= 65537:
            assert O.candidate(2, b) == S.model_payload(b), where
        assert H.bbwt_inverse(bw) == b, where
