"""The fast Lyndon route's integer core (kolmogorovlike-datacompressor_amd/csrc/lyndon_core.h) on the
CPU through tools/lyn_emu.cpp, which compiles the header the kernels use and walks their structure
serially: tiles of 256 lanes, the per-block prefix-min of the tile minima, live tiles only, an
unordered append (the tiles are taken forwards and backwards), rank sort, the Hillis-Steele
min-scan in suffix order, compaction.  Every factor-start list is compared with oracle.duval_starts.
The emulation records every text index it loads: one outside the block's [base, end), or a wide
load at a misaligned (virtual) address, fails the case.  Blocks are embedded between canary
neighbours at every address alignment.  The stand-alone program (its own main) is also built with
-fsanitize=address,undefined and run once on heap buffers of exactly the blocks' sizes.  Nothing is
preloaded into Python."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import oracle as O
from kolm import datagen as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "lyn_emu.cpp")
CANARY = 0xEE


class Info(ctypes.Structure):
    _fields_ = [("ncand", ctypes.c_uint32), ("live_tiles", ctypes.c_uint32), ("ncmp", ctypes.c_uint32),
                ("max_lcp", ctypes.c_uint32), ("lcp_sum", ctypes.c_uint64), ("bad", ctypes.c_uint64),
                ("loads", ctypes.c_uint64)]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lyn") / "lyn_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-DLYN_EMU_NO_MAIN", SRC, "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    U32, P = ctypes.c_uint32, ctypes.c_void_p
    lib.lyn_emu_block.argtypes = [P, U32, U32, U32, U32, U32, U32, P, P, P, ctypes.POINTER(Info)]
    lib.lyn_emu_block.restype = ctypes.c_int
    lib.lyn_emu_cands.argtypes = [P, U32, U32, U32, P, U32]
    lib.lyn_emu_cands.restype = ctypes.c_longlong
    lib.lyn_emu_consts.argtypes = [P]
    c = (U32 * 3)()
    lib.lyn_emu_consts(c)
    lib.TILE, lib.CAND_MAX, lib.LCP_MAX = int(c[0]), int(c[1]), int(c[2])
    return lib


def run(emu, s: bytes, base=0, amod=0, cap=None, lcp_cap=None, order=0, tail=0):
    """s as a block at offset `base` of a buffer with canary neighbours.  Returns (route, starts
    relative to the block or None, Info); checks that nothing outside the contract was loaded and
    that a fallback wrote nothing."""
    n = len(s)
    buf = np.full(base + n + tail, CANARY, np.uint8)
    buf[base:base + n] = np.frombuffer(s, np.uint8)
    starts = np.full(n + 1, 0xFFFFFFFF, np.uint32)
    ns = np.full(1, 0xFFFFFFFF, np.uint32)
    flag = np.zeros(base + n + tail, np.uint8)
    inf = Info()
    r = emu.lyn_emu_block(buf.ctypes.data, base, base + n, amod, emu.CAND_MAX if cap is None else cap,
                          emu.LCP_MAX if lcp_cap is None else lcp_cap, order, starts.ctypes.data, ns.ctypes.data,
                          flag.ctypes.data, ctypes.byref(inf))
    assert inf.bad == 0, f"{inf.bad} loads outside the block or misaligned"
    assert r in (0, 1)
    if r == 1:
        assert ns[0] == 0xFFFFFFFF and not flag.any() and (starts == 0xFFFFFFFF).all()
        return r, None, inf
    got = starts[:int(ns[0])].astype(np.int64) - base
    assert (starts[int(ns[0]):] == 0xFFFFFFFF).all()
    assert sorted(np.flatnonzero(flag) - base) == list(got)
    return r, list(map(int, got)), inf


def cands(emu, s: bytes, base=0, amod=0):
    n = len(s)
    buf = np.full(base + n, CANARY, np.uint8)
    buf[base:] = np.frombuffer(s, np.uint8)
    out = np.zeros(n, np.uint32)
    c = emu.lyn_emu_cands(buf.ctypes.data, base, base + n, amod, out.ctypes.data, n)
    assert c >= 0
    return [int(x) - base for x in out[:c]]


def accepted_equals_duval(emu, s: bytes, k=0, **kw):
    r, got, _ = run(emu, s, base=k % 7, amod=(5 * k) % 16, order=k & 1, tail=k % 3, **kw)
    assert r == 0, s[:32]
    assert got == O.duval_starts(s), s[:32]


@pytest.mark.parametrize("alphabet,maxlen", [((0, 1, 2), 10), ((0, 1), 14)])
def test_every_small_string(emu, alphabet, maxlen):
    """Zero bytes, tails shorter than 8 and equal words: all strings over the alphabet."""
    k = 0
    for n in range(1, maxlen + 1):
        for t in itertools.product(alphabet, repeat=n):
            accepted_equals_duval(emu, bytes(t), k)
            k += 1


def test_strings_over_0_and_255(emu):
    k = 0
    for n in range(1, 18):
        for t in itertools.product((0, 255), repeat=n) if n <= 10 else \
                (tuple(255 * ((c >> i) & 1) for i in range(n)) for c in range(0, 1 << n, 37)):
            accepted_equals_duval(emu, bytes(t), k)
            k += 1


@pytest.mark.parametrize("n", [4095, 4096, 4097, 8191, 8192, 8193])
def test_random_small_alphabet_at_tile_edges(emu, n):
    rng = np.random.default_rng(n)
    for k, alpha in enumerate((2, 3, 4, 7, 26)):
        s = (255 - rng.integers(0, alpha, n)).astype(np.uint8).tobytes()
        r, got, inf = run(emu, s, base=k, amod=3 * k, order=k & 1, lcp_cap=1 << 16)
        assert inf.ncand <= emu.CAND_MAX and r == 0
        assert got == O.duval_starts(s)


def test_every_start_is_a_candidate(emu):
    """Completeness on its own, also for inputs the resolver gives up on."""
    rng = np.random.default_rng(5)
    cases = [bytes(3000), b"ab" * 2500, bytes(range(96)) * 60, D.enwik_like(20000, seed=3),
             bytes([1]) + D.enwik_like(5000, seed=4) + bytes(700)]
    cases += [rng.integers(0, a, n).astype(np.uint8).tobytes() for a in (2, 3, 256) for n in (1, 9, 500, 5000)]
    for k, s in enumerate(cases):
        c = cands(emu, s, base=k % 5, amod=k)
        assert c == sorted(set(c)) and c[0] == 0
        assert set(O.duval_starts(s)) <= set(c)


def staircase(k: int, n: int, step: int) -> bytes:
    """Exactly k candidates, all of them factor starts: k strictly falling bytes, `step` apart, in a
    filler of larger bytes."""
    assert k <= 1600 and step >= 2 and (k - 1) * step + 2 <= n
    s = bytearray(b"\xf0" * n)
    for i in range(k):
        # two-byte values, strictly falling; the second byte (>= 40) is above every first byte (<= 8),
        # so it never begins a candidate itself
        s[i * step], s[i * step + 1] = 8 - i // 200, 239 - i % 200
    return bytes(s)


def lcp_pair(L: int) -> bytes:
    """Three candidates; the first two share exactly L bytes, no other pair shares any."""
    return b"b" + b"z" * (L - 1) + b"c" + b"b" + b"z" * (L - 1) + b"a"


def test_candidate_cap(emu):
    cap = emu.CAND_MAX
    s = staircase(cap, 9 * cap + 50, 9)
    assert len(cands(emu, s)) == cap
    for order in (0, 1):
        r, got, inf = run(emu, s, order=order)
        assert (r, inf.ncand) == (0, cap) and got == O.duval_starts(s) and len(got) == cap
    s = staircase(cap + 1, 9 * cap + 50, 9)
    for order in (0, 1):
        r, got, inf = run(emu, s, order=order, base=3)
        assert (r, inf.ncand) == (1, cap + 1)
    for k in (15, 16, 17):
        s = staircase(k, 9000, 500)
        r, got, inf = run(emu, s, cap=16, order=k & 1)
        assert inf.ncand == k and r == (0 if k <= 16 else 1)
        assert got is None or got == O.duval_starts(s)


def test_lcp_cap(emu):
    for cap, L in ((emu.LCP_MAX, emu.LCP_MAX), (16, 16), (8, 8), (300, 300), (1000, 1000)):
        s = lcp_pair(L)
        r, got, inf = run(emu, s, lcp_cap=cap, base=1, amod=7)
        assert (r, inf.max_lcp) == (0, L) and got == O.duval_starts(s)
        s = lcp_pair(L + 1)
        r, got, inf = run(emu, s, lcp_cap=cap, base=2, amod=9)
        assert r == 1 and inf.max_lcp > cap


def test_periodic_inputs_fall_back(emu):
    for s in (bytes(65536), b"ab" * 4000, bytes(range(96)) * 700):
        r, _, _ = run(emu, s)
        assert r == 1
    # short periodic inputs stay inside the budgets and must still be exact
    for s in (bytes(200), b"ab" * 100, bytes(range(96)) * 2 + bytes(range(50))):
        r, got, _ = run(emu, s)
        assert r == 0 and got == O.duval_starts(s)


def test_bench_stream_first_blocks_accepted(emu):
    """Blocks 0..7 of the benchmark's rank-0 stream: accepted with 4x headroom under both caps."""
    bs = 1 << 20
    data = D.enwik_like(8 * bs, seed=D.ENWIK_SEED)
    for b in range(8):
        s = data[b * bs:(b + 1) * bs]
        r, got, inf = run(emu, s, order=b & 1)
        assert r == 0 and got == O.duval_starts(s)
        assert 4 * inf.ncand <= emu.CAND_MAX and 4 * inf.max_lcp <= emu.LCP_MAX


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lyn_emu_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
