"""The search kernels' integer core (kolmogorovlike-datacompressor_amd/csrc/find_core.h) checked on
the CPU through tools/find_emu.cpp, which compiles the header k_find_count / k_find_emit use and
walks the kernels' tiles, threads and positions serially: the windows formed from aligned 16-byte
words, the masked prefix compare, the tail verify, the bounds rule, the per-tile counts, their scan
and the emit launches cut at scanned tile boundaries.  Every load is checked against the contract
(an aligned 16-byte word that holds a byte of [buf, buf + n)) and the violations are counted; the
buffer handed to the emulation is exactly the aligned words around the data.  Expected matches
come from `ref` (repeated bytes.find).  The stand-alone program (its own main) is also built with
-fsanitize=address,undefined and run once over the same sweeps on heap buffers of exactly those
sizes.  Nothing is preloaded into Python."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "find_emu.cpp")
TILE = 4096
NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8193)
LENS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 255, 256)
NO_LIMIT = (1 << 64) - 1
P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64


def ref(data, pats, lo=0, hi=None):
    """Every (offset, pattern index) with lo <= offset and offset + len <= hi, sorted."""
    hi = len(data) if hi is None else hi
    d, out = data[lo:hi], []
    for i, p in enumerate(pats):
        o = d.find(p)
        while o >= 0:
            out.append((lo + o, i))
            o = d.find(p, o + 1)
    return sorted(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fnd") / "find_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.fnd_emu_find.restype = U64
    lib.fnd_emu_find.argtypes = [P, U32, U32, P, P, U32, U64, U64, P, P, P, U64, P, P]
    lib.fnd_emu_find_grouped.restype = U64
    lib.fnd_emu_find_grouped.argtypes = [P, P, U32, U64, U64, P, P, U32, U64, U64, P, P, P, U64, P, P]
    lib.fnd_emu_groups.restype = None
    lib.fnd_emu_groups.argtypes = [P, U32, U64, U64, U32, P, P]
    lib.fnd_emu_tile_bytes.restype = U32
    assert lib.fnd_emu_tile_bytes() == TILE
    return lib


def pattern_arrays(pats):
    flat = np.frombuffer(b"".join(pats) + b"\0", np.uint8)
    off = np.zeros(len(pats) + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in pats])
    return flat, off


def find(emu, data, mis, pats, lo=0, stage=64 << 20, limit=NO_LIMIT):
    """The emulation over data placed `mis` bytes past a 16-byte boundary in a buffer that ends
    with the aligned word holding the last byte.  Returns (pairs, counts, emit launches); the
    contract violations must be 0."""
    n = len(data)
    size = (mis + n + 15) // 16 * 16
    raw = np.full(size + 32, 0xEE, np.uint8)
    base = (-raw.ctypes.data) % 16
    raw[base + mis:base + mis + n] = np.frombuffer(data, np.uint8)
    flat, off = pattern_arrays(pats)
    cap = (n + 1) * len(pats)
    counts, offs, which = np.zeros(len(pats), np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8)
    nfound, launches = U64(0), U32(0)
    bad = emu.fnd_emu_find(raw.ctypes.data + base + mis, n, lo, flat.ctypes.data, off.ctypes.data, len(pats), stage, limit,
                           counts.ctypes.data, offs.ctypes.data, which.ctypes.data, cap, ctypes.byref(nfound),
                           ctypes.byref(launches))
    assert bad == 0, (bad, n, mis, [len(p) for p in pats])
    k = nfound.value
    return list(zip(offs[:k].tolist(), which[:k].tolist())), counts.tolist(), launches.value


def haystack(kind, n, ln, seed):
    """(data, patterns): all zeros; period-3 abc; seeded two-letter noise; seeded random bytes with
    the pattern planted at 0, at n - ln, across the 4 KiB tile boundaries and across 16-byte lane
    boundaries at every phase, plus a pattern whose prefix ends the buffer while its last byte
    would lie past n."""
    rng = np.random.default_rng(seed)
    if kind == 0:
        return bytes(n), [bytes(ln)]
    if kind == 1:
        return (b"abc" * (n // 3 + 1))[:n], [(b"bca" * 86)[:ln]]
    if kind == 2:
        d = rng.integers(97, 99, n, dtype=np.uint8).tobytes()
        return d, [(d[:ln] + b"a" * ln)[:ln], b"a" * min(ln, 3)]
    d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    pat = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
    spots = [0, TILE - (ln + 1) // 2, 2 * TILE - 1, n - ln]
    if ln < 64:
        spots += [512 + k * 271 for k in range(1, 17)]
    for o in spots:
        if 0 <= o and o + ln <= n:
            d[o:o + ln] = pat
    pats = [pat]
    if ln < 256:
        pats.append(pat + bytes([pat[-1] ^ 0x55]))
    return bytes(d), pats


@pytest.mark.parametrize("kind", range(4))
def test_length_sweep(emu, kind):
    for mis in range(16):
        for n in NS:
            for ln in LENS:
                data, pats = haystack(kind, n, ln, 100 * mis + ln)
                want = ref(data, pats)
                got, counts, _ = find(emu, data, mis, pats)
                assert got == want, (kind, mis, n, ln)
                assert counts == [sum(1 for _, i in want if i == j) for j in range(len(pats))]


def test_planted_matches_are_where_they_were_put(emu):
    """The planted haystack does hold what the sweep relies on: a match at 0, at n - ln, one that
    straddles the 4 KiB tile boundary, one that begins at every phase of a 16-byte lane; and the
    truncated pattern, whose prefix ends the buffer, is not reported there."""
    for ln in LENS:
        data, pats = haystack(3, 8193, ln, ln)
        hits = [o for o, i in ref(data, pats) if i == 0]
        assert 0 in hits and 8193 - ln in hits
        assert any(o < TILE < o + ln or (ln == 1 and o == TILE - 1) for o in hits)
        if ln < 64:
            assert {o % 16 for o in hits} >= set(range(16))
        for mis in (0, 7, 15):
            got, counts, _ = find(emu, data, mis, pats)
            assert [o for o, i in got if i == 0] == hits
            if len(pats) == 2:
                assert (8193 - ln, 1) not in got and data.endswith(pats[1][:-1])


def test_overlaps_duplicates_and_order(emu):
    assert find(emu, b"aaaa", 3, [b"aa"])[0] == [(0, 0), (1, 0), (2, 0)]
    data = b"abcabcabc" * 500
    pats = [b"abc", b"abcabc", b"abc", b"c", b"zz"]
    got, counts, _ = find(emu, data, 5, pats)
    assert got == ref(data, pats) and counts[0] == counts[2] == 1500 and counts[4] == 0
    assert got[:4] == [(0, 0), (0, 1), (0, 2), (2, 3)]
    # lo: matches that begin before it are not reported
    assert find(emu, data, 9, pats, lo=4000)[0] == ref(data, pats, 4000)


def test_limit_and_small_stage(emu):
    data = bytes(5 * TILE + 3)
    pats = [b"\0", b"\0\0"]
    want = ref(data, pats)
    full, counts, launches = find(emu, data, 2, pats)
    assert full == want and launches == 1 and counts == [len(data), len(data) - 1]
    # the least staging the kernels accept is one tile's records: a launch per tile
    got, c2, launches = find(emu, data, 2, pats, stage=1)
    assert got == want and c2 == counts and launches == 6
    got, _, launches = find(emu, data, 2, pats, stage=5 * 3 * 2 * TILE)
    assert got == want and launches == 2
    for limit in (0, 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, len(want), len(want) + 1):
        got, c3, launches = find(emu, data, 11, pats, stage=5 * 2 * TILE, limit=limit)
        assert got == want[:limit] and c3 == counts
        assert launches == (0 if limit == 0 else min(-(-limit // (2 * TILE)), 6))


def groups(emu, bounds, lo, hi, L):
    b = np.asarray(bounds, np.uint64)
    S, carry = np.zeros(len(bounds), np.uint64), np.zeros(len(bounds) - 1, np.uint32)
    emu.fnd_emu_groups(b.ctypes.data, len(bounds) - 1, lo, hi, L, S.ctypes.data, carry.ctypes.data)
    return S.tolist(), carry.tolist()


def test_hold_back_bookkeeping(emu):
    """S_0 = lo, S_g+1 = max(S_g, b_g - (L - 1)), S_end = hi; the carry in front of group g + 1 is
    [S_g+1, b_g): fewer than L bytes, also over groups shorter than L - 1."""
    assert groups(emu, [0, 1000, 2000, 3000], 10, 2900, 256) == ([10, 745, 1745, 2900], [0, 255, 255])
    assert groups(emu, [0, 1000, 2000], 990, 2000, 4) == ([990, 997, 2000], [0, 3])
    assert groups(emu, [0, 1000, 2000], 999, 1500, 256) == ([999, 999, 1500], [0, 1])
    assert groups(emu, [0, 100, 200], 0, 200, 1) == ([0, 100, 200], [0, 0])
    # tiny groups: the start stays put and the carry grows over several of them
    S, carry = groups(emu, [500, 600, 610, 620, 700, 1000], 590, 1000, 101)
    assert S == [590, 590, 590, 590, 600, 1000] and carry == [0, 10, 20, 30, 100]
    rng = np.random.default_rng(2)
    for _ in range(300):
        ng = int(rng.integers(1, 9))
        cuts = np.cumsum(rng.integers(1, 300, ng + 1)).tolist()
        L = int(rng.integers(1, 257))
        lo = int(rng.integers(cuts[0], cuts[1]))
        hi = int(rng.integers(max(lo, cuts[-2]) + 1, cuts[-1] + 1))
        S, carry = groups(emu, cuts, lo, hi, L)
        assert S[0] == lo and S[-1] == hi and all(x <= y for x, y in zip(S, S[1:]))
        for g in range(ng - 1):
            assert S[g + 1] == max(S[g], cuts[g + 1] - (L - 1))
            assert carry[g + 1] == cuts[g + 1] - S[g + 1] < L


def grouped(emu, data, bounds, lo, hi, pats, stage=64 << 20, limit=NO_LIMIT):
    buf = np.frombuffer(data + b"\0", np.uint8)
    b = np.asarray(bounds, np.uint64)
    flat, off = pattern_arrays(pats)
    cap = (len(data) + 1) * len(pats)
    counts, offs, which = np.zeros(len(pats), np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8)
    nfound, launches = U64(0), U32(0)
    bad = emu.fnd_emu_find_grouped(buf.ctypes.data, b.ctypes.data, len(bounds) - 1, lo, hi, flat.ctypes.data,
                                   off.ctypes.data, len(pats), stage, limit, counts.ctypes.data, offs.ctypes.data,
                                   which.ctypes.data, cap, ctypes.byref(nfound), ctypes.byref(launches))
    assert bad == 0
    k = nfound.value
    return list(zip(offs[:k].tolist(), which[:k].tolist())), counts.tolist()


def test_grouped_search_over_synthetic_groups(emu):
    """The grouped search as the reader runs it (scan buffer = carry + the group's bytes): the
    same matches however the stream is cut, matches that span many groups included."""
    rng = np.random.default_rng(8)
    d = bytearray(rng.integers(97, 100, 6000, dtype=np.uint8).tobytes())
    long = rng.integers(0, 256, 256, dtype=np.uint8).tobytes()
    for o in (90, 1000, 4095 - 100, 6000 - 256):
        d[o:o + 256] = long
    data = bytes(d)
    pats = [long, b"ab", long[:9], b"abca", b"ab"]
    cuts = [list(range(0, 6001, 100)), [0, 6000], [0, 1, 2, 3, 50, 51, 300, 4096, 4097, 6000],
            [0] + sorted(set(rng.integers(1, 6000, 40).tolist())) + [6000]]
    for lo, hi in ((0, 6000), (91, 5999), (1000, 1256), (1001, 1256), (3000, 3000)):
        want = ref(data, pats, lo, hi)
        for bounds in cuts:
            # the groups a reader would decode: those that hold a byte of [lo, hi)
            sel = [i for i in range(len(bounds) - 1) if bounds[i] < hi and bounds[i + 1] > lo] if hi > lo else []
            if not sel:
                continue
            b = bounds[sel[0]:sel[-1] + 2]
            got, counts = grouped(emu, data, b, lo, hi, pats)
            assert got == want, (lo, hi, b[:5])
            assert counts == [sum(1 for _, i in want if i == j) for j in range(len(pats))]
            assert grouped(emu, data, b, lo, hi, pats, stage=1, limit=7)[0] == want[:7]


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "find_emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout and "runtime error" not in r.stderr
