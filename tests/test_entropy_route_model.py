"""The route matrix of tests/entropy_routes.py on the CPU: (1) the numpy model of the MTF / size /
MDL / emission stage against the oracle on every block of the matrix, (2) every row's input takes
every route the row claims, by the predictor, and every route of the stage is claimed by some row -
so that no row of tests/test_gpu_entropy_routes.py can pass vacuously - and (3) the predictor's
restatement of the selection rules on geometries worked out by hand."""
import numpy as np
import pytest

import entropy_routes as E
import oracle as O
from kolm import decode as H

ORACLE_MAX = 1 << 16  # blocks up to this size are compared with the oracle


def _distinct_blocks():
    seen = {}
    for name, c in E.CASES.items():
        for i, b in enumerate(c.blks()):
            seen.setdefault(b.block, (f"{name}[{i}]", b))
    return sorted(seen.values(), key=lambda kv: kv[1].n)


def _all_255(b):
    """The 16 KiB block of index 255: highly periodic, the oracle's BBWT needs seconds on it."""
    return b.n >= 1 << 14 and bool((b.m == 255).all())


# ------------------------------------------------------------------ 1. the model against the oracle

def test_model_against_oracle():
    """On every distinct block of at most 64 KiB (the all-255 one excepted, and without the oracle's
    BBWT on it): the oracle's BBWT gives the L the block was derived from, its MTF the chosen
    indices, its candidates 1..6 and 8 the model's payloads and sizes, and its Rice coder the
    model's code of the indices for every k in 0..15."""
    checked = 0
    for where, b in _distinct_blocks():
        assert H.mtf_decode(b.m) == b.L and O.mtf_encode(b.L) == b.m.tobytes(), where
        if b.n > ORACLE_MAX:
            assert H.bbwt_inverse(b.L) == b.block, where
            continue
        for k in range(16):
            assert E.rice_code(b.m, k) == O.rice_encode(b.m.tobytes(), k), (where, k)
        if _all_255(b):
            continue
        assert O.bbwt_forward(b.block) == b.L, where
        sz = E.block_sizes(b.block, b.m)
        for mid in (1, 2, 3, 4, 5, 6, 8):
            want = O.candidate(mid, b.block)
            assert E.payload(b.block, b.m, mid) == want, (where, mid)
            assert sz[mid] == len(want), (where, mid)
        assert sz[0] == b.n and sz[7] is None
        checked += 1
    assert checked >= 250


def test_model_payloads_decode():
    """The host decoder returns the block from the model's payload of methods 0..6 and 8 (the second
    check of the GPU test), on the emission rows' blocks."""
    for name in ("rice_slow_k2", "rice_edge_64", "winner_each", "ties", "simple_tiles"):
        for i, b in enumerate(E.CASES[name].blks()):
            for mid in (0, 1, 2, 3, 4, 5, 6, 8):
                assert H.decode_block(mid, E.payload(b.block, b.m, mid), b.n) == b.block, (name, i, mid)


def test_maps_by_hand():
    m = np.array([0x80, 0x01, 0xFF, 0, 0, 0, 0, 0x10, 0x35], np.uint8)
    # plane 0 collects bit 7 of bytes 0..7 at bits 7..0; the second group is zero padded
    assert E.bitplane(m).tolist() == [0b10100000, 0b00100000, 0b00100000, 0b00100001, 0b00100000, 0b00100000,
                                      0b00100000, 0b01100000, 0, 0, 0x80, 0x80, 0, 0x80, 0, 0x80]
    assert E.mapped(m, 4).tolist()[:3] == [0x08, 0x10, 0xFF] and E.mapped(m, 4)[8] == 0x53
    assert E.mapped(m, 5).tolist()[:2] == [0x01, 0x80] and E.mapped(m, 5)[8] == 0xAC
    assert E.mapped(m, 6).tolist()[:3] == [0xC0, 0x01, 0x80] and E.mapped(m, 6)[8] == 0x35 ^ 0x1A
    assert E.rice_bits([0, 3, 4, 255], 2).tolist() == [3, 3, 4, 66] and E.rice_bits([255], 0).tolist() == [256]
    assert E.rice_bits([255], 15).tolist() == [16]
    assert E.rice_code([5, 0], 2) == bytes([0b10010000]) and E.rice_code([2], 0) == bytes([0b11000000])
    assert E.uleb([0, 127, 128, 255]) == bytes([0, 127, 0x80, 1, 0xFF, 1])
    lf = E.lfsr_table()
    assert lf[:4].tolist() == [1, 2, 5, 11] and len(lf) == 255  # taps 0x96: bits 1, 2, 4, 7


def test_mdl_against_argmin():
    """Strict <, ties to the lowest id, disabled ids read 0xFFFFFFFF, nothing enabled -> raw, force
    overrides: against np.argmin (which returns the first minimum) over the enabled ids."""
    r = np.random.default_rng(5)
    for _ in range(2000):
        sizes = r.integers(1, 6, E.NCAND).tolist()  # small range: many ties
        mask = int(r.integers(0, 1 << E.NCAND))
        force = int(r.integers(-1, E.NCAND)) if r.random() < 0.3 else -1
        rep, win = E.mdl(sizes, mask, force)
        en = [i for i in range(E.NCAND) if (mask >> i) & 1]
        assert rep == [s if i in en else E.OFF for i, s in enumerate(sizes)]
        want = en[int(np.argmin([sizes[i] for i in en]))] if en else 0
        assert win == (force if force >= 0 else want)
    assert E.mdl([9, 9, 5, 5, 5, 5, 5, None, 9, None, None], 0x7C)[1] == 2
    assert E.mdl([9, 9, 5, 5, 5, 5, 5, None, 9, None, None], 0x70)[1] == 4
    assert E.mdl([9, 9, 5, 5, 5, 5, 5, None, 9, None, None], 0)[1] == 0


# ------------------------------------------------------------------ 2. every row is what it claims

@pytest.mark.parametrize("name", list(E.CASES))
def test_row_takes_the_routes_it_claims(name):
    case = E.CASES[name]
    got = E.predicted_routes(case)
    assert not [r for r in case.claims if r not in got], name
    assert sum(b.n for b in case.blks()) <= 2 << 20  # no batch over 2 MiB
    if case.mtf:
        sw = E.opposite_switch(case)
        run = case.runs()[0]
        a, b = case.predict(run), case.predict(run, sw)
        assert {a.kernel, b.kernel} == {"k_mtf_wave", "k_mtf_replay"}, name
        assert not [r for r in case.opposite if r not in b.routes], name
    else:
        assert not case.opposite


def test_every_route_is_claimed():
    """A route of ROUTES that no row claims fails here: the matrix must reach all of them."""
    claimed = set()
    for c in E.CASES.values():
        claimed |= set(c.claims) | set(c.opposite)
    assert not sorted(claimed - set(E.ROUTES)), "claims that are not routes"
    assert not [r for r in E.ROUTES if r not in claimed]


def test_rows_are_the_shapes_of_the_matrix():
    """The rows' shapes, written out: what the device evidence of the GPU test will be."""
    def ev(name, switch=None):
        c = E.CASES[name]
        p = c.predict(c.runs()[0], switch)
        return p.kernel, p.csz, p.cpb
    assert ev("wave_one_block") == ("k_mtf_wave", 1024, 5) and E.CASES["wave_one_block"].blks()[0].n == 4415
    assert ev("wave_63_blocks") == ("k_mtf_wave", 1024, 1) and ev("replay_64_blocks") == ("k_mtf_replay", 128, 8)
    assert E.CASES["wave_63_blocks"].blocks() == E.CASES["replay_64_blocks"].blocks()[:63]
    assert ev("replay_128_wholewg") == ("k_mtf_replay", 128, 256) and ev("replay_128_ragged") == ("k_mtf_replay", 128, 256)
    assert ev("replay_256") == ("k_mtf_replay", 256, 128) and ev("replay_512") == ("k_mtf_replay", 512, 128)
    assert ev("replay_1024") == ("k_mtf_replay", 1024, 128)
    for name in ("replay_256", "replay_512", "replay_1024"):
        lens = [b.n for b in E.CASES[name].blks()]
        assert len(lens) == 128 and all(x % 2 for x in lens[1:]) and lens.count(1) == 8 and max(lens[1:]) < 1500
    assert ev("deep_indices", 0) == ("k_mtf_replay", 128, 64) and ev("odd_base_var") == ("k_mtf_wave", 1024, 5)
    bases = np.cumsum([0] + [b.n for b in E.CASES["odd_base_var"].blks()])[1:4]
    assert (bases % 16).tolist() == [1, 7, 15]
    # the whole-workgroup row: every launch group of k_mtf_summary is one block's 256 full chunks
    R = E.predicted_routes(E.CASES["replay_128_wholewg"])
    assert not R & {"summary.16", "summary.byte", "summary.past_end", "replay.16", "replay.byte", "acc.add"}
    # winner_each: methods 2..6 in turn, each the unique minimum; ties: all five sizes equal
    c = E.CASES["winner_each"]
    sizes, win, _ = c.model(c.runs()[0])
    assert win == [2, 3, 4, 5, 6]
    for row, w in zip(sizes.tolist(), win):
        assert sorted(row[2:7])[0] == row[w] < sorted(row[2:7])[1]
    c = E.CASES["ties"]
    assert len(c.runs()) == 32 and sorted(r.mask for r in c.runs()) == [s << 2 for s in range(32)]
    for b in c.blks():
        assert len(set(E.block_sizes(b.block, b.m)[2:7])) == 1 and b.n % 8 == 0
    for run in c.runs():
        low = next((i for i in range(2, 7) if (run.mask >> i) & 1), 0)
        assert c.model(run)[1] == [low] * 3
    # mosaic: the nine methods in turn; the Rice blocks start at every byte residue modulo 4
    c = E.CASES["mosaic"]
    _, win, pays = c.model(c.runs()[0])
    assert len(win) >= 36 and win == [E.MOSAIC_ORDER[i % 9] for i in range(len(win))]
    off = np.cumsum([0] + [len(p) for p in pays])
    assert {int(off[i]) % 4 for i, w in enumerate(win) if w in E.RICE_IDS} == {0, 1, 2, 3}
    # rice_slow_k2: the largest payload there is, 66 bits a symbol
    b = E.CASES["rice_slow_k2"].blks()[0]
    assert E.block_sizes(b.block, b.m)[2] == (66 * (1 << 14) + 7) // 8


# ------------------------------------------------------------------ 3. the predictor by hand

def test_chunk_bytes_by_hand():
    """mtf_chunk_bytes: halved while ceil(bs / csz) * nb < 16384, down to 128; 1 KiB in the wave form."""
    assert [E.chunk_bytes(bs << 10, 128, False) for bs in (128, 64, 32, 16)] == [1024, 512, 256, 128]
    assert E.chunk_bytes((128 << 10) - 1024, 128, False) == 512 and E.chunk_bytes(1, 1 << 14, False) == 1024
    assert E.chunk_bytes(1, 16383, False) == 128 and E.chunk_bytes(1 << 15, 64, False) == 128
    # the inputs of test_gpu_switches.py under KOLM_MTF_WAVE=0: all 128
    assert {E.chunk_bytes(bs, nb, False) for bs, nb in ((65536, 6), (16384, 4), (1 << 17, 1), (16384, 20))} == {128}
    assert E.chunk_bytes(1 << 15, 64, True) == 1024
    assert [E.wave_mode(nb) for nb in (1, 63, 64)] == [True, True, False]
    assert E.wave_mode(1, 0) is False and E.wave_mode(100, 1) is True


def test_predict_by_hand():
    """Two fixed blocks of 40 bytes under the per-thread replay: chunks of 128 bytes, one per block;
    block 0 is [0, 40): not a multiple of 16 -> byte paths; a 40-byte block has a full last group."""
    blks = [E.from_m(np.arange(40, dtype=np.uint8)), E.from_m(np.full(40, 3, np.uint8))]
    p = E.predict(blks, [2, 0], [len(E.payload(blks[0].block, blks[0].m, 2)), 40], mask_used=E.NO_LZ, switch=0,
                  ties=[False, False])
    assert (p.kernel, p.csz, p.cpb, p.summary_bytes) == ("k_mtf_replay", 128, 1, 80 + 512)
    assert {"summary.byte", "replay.byte", "acc.add", "replay.reg0", "replay.reg1", "replay.lds", "cp.empty_range",
            "mdl.win2", "emit.fast", "emit.blockstart.lead0", "cheap.aligned", "cheap.tail", "cheap.unaligned",
            # indices 0..39 at k = 2: the thread of symbols 32..39 has 4 * 11 + 4 * 12 = 92 bits, that of 24..31 has
            # 76: slow; 16..23 has 60: fast.  300 bits in all: 38 bytes, so the raw block starts inside a word
            "emit.slow", "emit.edge_next.raw"} <= p.routes
    assert not p.routes & {"bp.pad", "summary.wholewg", "replay.64", "replay.16", "emit.q32_loop", "mtf.wave",
                           "cp.multi_chunk_range", "emit.edge_prev.raw", "emit.ns_lt8"}
    p = E.predict(blks[:1], [2], [1], mask_used=E.NO_LZ, switch=1, ties=[False])
    assert p.kernel == "k_mtf_wave" and {"wave.partial_step", "acc.lane"} <= p.routes
    assert "wave.short_group" not in p.routes
