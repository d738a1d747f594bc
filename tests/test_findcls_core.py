"""The class-pattern kernels' integer core (kolmogorovlike-datacompressor_amd/csrc/findcls_core.h)
checked on the CPU through tools/findcls_emu.cpp, which compiles the header k_findcls_count /
k_findcls_emit use and walks the kernels' tiles, threads and positions serially.  Every load is
checked against the contract (an aligned 16-byte word that holds a byte of [buf, buf + n)) and the
violations are counted; the buffer handed to the emulation is exactly the aligned words around the
data, and what those words hold outside the data is 0x00 (a class may hold it).  Expected matches
come from Python's re: a lookahead over an expression of \\xHH classes generated from the sets.
The stand-alone program (its own main) is also built with -fsanitize=address,undefined and run
once over its sweeps on heap buffers of exactly those sizes.  Nothing is preloaded into Python."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "findcls_emu.cpp")
TILE = 4096
NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8193)
MS = (1, 2, 7, 8, 9, 16, 17, 255, 256)
NO_LIMIT = (1 << 64) - 1
P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
ANY = frozenset(range(256))
DIGIT = frozenset(range(48, 58))


def expr_of(pat):
    """A pattern (a set per position) as an expression of \\xHH classes."""
    return b"".join(b"[" + b"".join(b"\\x%02x" % b for b in sorted(c)) + b"]" if c else b"[^\\x00-\\xff]" for c in pat)


def ref(data, pats, lo=0, hi=None):
    """Every (offset, pattern index) with lo <= offset and offset + m <= hi, sorted."""
    hi = len(data) if hi is None else hi
    out = []
    for i, p in enumerate(pats):
        rx = re.compile(b"(?=(" + expr_of(p) + b"))", re.DOTALL)
        out += [(lo + m.start(), i) for m in rx.finditer(data[lo:hi])]
    return sorted(out)


def counts_of(want, np_):
    return [sum(1 for _, i in want if i == j) for j in range(np_)]


def fold(c):
    return frozenset(b for b in range(256) if bytes([b]).lower() in {bytes([x]).lower() for x in c})


def literal(b, ignore_case=False):
    return [fold({x}) if ignore_case else frozenset({x}) for x in b]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fcl") / "findcls_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.fcl_emu_find.restype = U64
    lib.fcl_emu_find.argtypes = [P, U32, U32, P, P, U32, U64, U64, P, P, P, U64, P, P]
    lib.fcl_emu_find_grouped.restype = U64
    lib.fcl_emu_find_grouped.argtypes = [P, P, U32, U64, U64, P, P, U32, U64, U64, P, P, P, U64, P, P]
    lib.fcl_emu_classify.restype = U32
    lib.fcl_emu_classify.argtypes = [P, P, P]
    lib.fcl_emu_tile_bytes.restype = U32
    assert lib.fcl_emu_tile_bytes() == TILE
    return lib


@pytest.fixture(scope="module")
def lit_emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fnd") / "find_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(REPO, "tools", "find_emu.cpp"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.fnd_emu_find.restype = U64
    lib.fnd_emu_find.argtypes = [P, U32, U32, P, P, U32, U64, U64, P, P, P, U64, P, P]
    return lib


def class_arrays(pats):
    bm = np.zeros((sum(len(p) for p in pats) + 1, 32), np.uint8)
    k = 0
    for p in pats:
        for c in p:
            for b in c:
                bm[k, b >> 3] |= 1 << (b & 7)
            k += 1
    off = np.zeros(len(pats) + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in pats])
    return bm, off


def placed(data, mis):
    """data `mis` bytes past a 16-byte boundary, zeros around it: (array kept alive, address)."""
    size = (mis + len(data) + 15) // 16 * 16
    raw = np.zeros(size + 32, np.uint8)
    base = (-raw.ctypes.data) % 16
    raw[base + mis:base + mis + len(data)] = np.frombuffer(data, np.uint8)
    return raw, raw.ctypes.data + base + mis


def find(emu, data, mis, pats, lo=0, stage=64 << 20, limit=NO_LIMIT, refuse=False):
    """The emulation: (pairs, counts, emit launches); the contract violations must be 0."""
    n = len(data)
    raw, addr = placed(data, mis)
    bm, off = class_arrays(pats)
    cap = (n + 1) * len(pats)
    counts, offs, which = np.zeros(len(pats) + 1, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8)
    nfound, launches = U64(0), U32(0)
    bad = emu.fcl_emu_find(addr, n, lo, bm.ctypes.data, off.ctypes.data, len(pats), stage, limit, counts.ctypes.data,
                           offs.ctypes.data, which.ctypes.data, cap, ctypes.byref(nfound), ctypes.byref(launches))
    if refuse:
        return bad
    assert bad == 0, (bad, n, mis, [len(p) for p in pats])
    k = nfound.value
    return list(zip(offs[:k].tolist(), which[:k].tolist())), counts[:len(pats)].tolist(), launches.value


def check(emu, data, mis, pats, **kw):
    want = ref(data, pats, kw.get("lo", 0))
    got, counts, _ = find(emu, data, mis, pats, **kw)
    assert got == want, (len(data), mis, [len(p) for p in pats], got[:5], want[:5])
    assert counts == counts_of(want, len(pats))
    return want


def test_classifier_of_the_library(emu):
    """findcls_core.h's classify on every masked equality and on seeded random classes."""
    every = {frozenset(b for b in range(256) if b & mask == value): (mask, value)
             for mask in range(256) for value in range(256) if not value & ~mask}
    rng = np.random.default_rng(5)
    cases = list(every)[::13] + [frozenset(rng.integers(0, 256, int(rng.integers(1, 12))).tolist()) for _ in range(300)]
    cases += [frozenset(), DIGIT, ANY, frozenset({0x41, 0x61}), frozenset({0x40, 0x60}), frozenset(range(1, 256))]
    for c in cases:
        bm, _ = class_arrays([[c]])
        mask, value = ctypes.c_uint8(0), ctypes.c_uint8(0)
        kind = emu.fcl_emu_classify(bm.ctypes.data, ctypes.byref(mask), ctypes.byref(value))
        if not c:
            assert kind == 0
        elif c in every:
            assert (kind, mask.value, value.value) == (1,) + every[c], sorted(c)
        else:  # a table class: the hull still holds every member
            assert kind == 2 and all(b & mask.value == value.value for b in c)


def test_a_ignore_case_single_positions(emu):
    """(a) each byte under ignore_case over a buffer of all 256 bytes: exactly b and swapcase(b)."""
    data = bytes(range(256))
    for b0 in range(0, 256, 16):  # 16 patterns a call, the misalignment moving along
        pats = [literal(bytes([b]), True) for b in range(b0, b0 + 16)]
        got, counts, _ = find(emu, data, b0 // 16, pats)
        for i, b in enumerate(range(b0, b0 + 16)):
            want = sorted({b, ord(bytes([b]).swapcase())})
            assert [o for o, j in got if j == i] == want and counts[i] == len(want)
    assert len(literal(b"@", True)[0]) == 1 and len(literal(b"`", True)[0]) == 1 and len(literal(b"k", True)[0]) == 2


def test_b_classes_that_hold_zero_past_the_end(emu):
    """(b) trailing classes hold 0x00 and the data, zeros themselves, end 1..m-1 bytes before a
    full match would complete: nothing past n is a match."""
    zero_or = frozenset({0, 0x7A})        # a table class that holds 0x00
    low = frozenset(range(8))             # a masked equality that holds 0x00
    for m in MS:
        pats = [[frozenset({0x41})] + [zero_or] * (m - 1), [frozenset({0x41})] + [low] * (m - 1), [ANY] * (m - 1) + [low]]
        for short in sorted({1, 2, m // 2, m - 1} - {0}):
            if short >= m:
                continue
            for n in (m - short, 16 + m - short, TILE - 3, TILE + m - short):
                d = bytearray(n)
                if n >= m - short:
                    d[n - (m - short)] = 0x41  # the match would end `short` bytes past n
                for mis in (0, 5, 15):
                    want = check(emu, bytes(d), mis, pats)
                    assert all(o + len(pats[i]) <= n for o, i in want)
                    assert not any(o == n - (m - short) and i < 2 for o, i in want)


def test_c_wildcards_only(emu):
    """(c) all-wildcard patterns: exactly max(0, hi - lo - m + 1) matches."""
    rng = np.random.default_rng(3)
    for n in NS:
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for m in MS:
            for mis, lo in ((0, 0), (9, min(n, 5))):
                got, counts, _ = find(emu, data, mis, [[ANY] * m], lo=lo)
                k = max(0, n - lo - m + 1)
                assert counts == [k] and got == [(lo + o, 0) for o in range(k)]


def test_d_table_classes_first_or_late(emu):
    """(d) table classes only in the first 8 positions (the filter has hulls alone), and only
    after position 8 (the filter is exact, the tables are read in the tail)."""
    rng = np.random.default_rng(4)
    vowel, odd = frozenset(b"aeiou"), frozenset(b"bdfhjlnprtvxz")
    for n in (17, 4097, 8193):
        d = rng.integers(97, 123, n, dtype=np.uint8).tobytes()
        for m in (8, 9, 17, 40):
            if m > n:
                continue
            src = d[n // 2:n // 2 + m]
            first = [vowel if chr(b) in "aeiou" else frozenset(range(97, 123)) - vowel for b in src[:8]] + literal(src[8:])
            late = literal(src[:8]) + [odd if b in odd else frozenset(range(97, 123)) - odd for b in src[8:]]
            digits_first = [DIGIT] * 4 + literal(b"-") + [DIGIT] * 2
            for mis in (0, 3, 12):
                want = check(emu, d, mis, [first, late, digits_first])
                assert (n // 2, 0) in want and (n // 2, 1) in want


def planted(n, m, seed):
    """Random bytes with a digit string planted at 0, at n - m, across the tile boundaries and at
    every phase of a 16-byte lane; (data, the digits)."""
    rng = np.random.default_rng(seed)
    d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    s = rng.integers(48, 58, m, dtype=np.uint8).tobytes()
    spots = [0, TILE - (m + 1) // 2, 2 * TILE - 1, n - m]
    if m < 64:
        spots += [512 + k * 271 for k in range(1, 17)]
    for o in spots:
        if 0 <= o and o + m <= n:
            d[o:o + m] = s
    return bytes(d), s


def test_e_sweep_with_planted_matches(emu):
    """(e) the shapes of the issue: n x misalignment x m, one pattern and 16, matches planted across
    tile and lane boundaries at every phase."""
    for mis in range(16):
        for n in NS:
            for m in MS:
                data, s = planted(n, m, 100 * mis + m)
                one = [[DIGIT] * m]
                check(emu, data, mis, one)
                if (mis + m) % 4 == 0:  # 16 patterns: classes, case pairs, singletons and wildcards mixed
                    sixteen = [[DIGIT if (k + i) % 3 else frozenset({s[k]}) if i % 2 else ANY for k in range(m)]
                               for i in range(14)] + [literal(s[:m]), [DIGIT] * (m - 1) + [frozenset({0, 0x30})]]
                    check(emu, data, mis, sixteen)
    data, s = planted(8193, 9, 9)
    hits = [o for o, _ in ref(data, [[DIGIT] * 9])]
    assert 0 in hits and 8193 - 9 in hits and any(o < TILE < o + 9 for o in hits) and {o % 16 for o in hits} >= set(range(16))


def test_f_g_identical_and_empty(emu):
    """(f) two identical patterns are both reported; (g) an empty class: no match."""
    data = b"ab12cd34" * 700
    p = [DIGIT, DIGIT]
    got, counts, _ = find(emu, data, 7, [p, [frozenset(b"abcd")], p, [DIGIT, frozenset(), DIGIT], [frozenset()]])
    assert counts == [1400, 2800, 1400, 0, 0]
    assert got[:4] == [(0, 1), (1, 1), (2, 0), (2, 2)]
    assert got == ref(data, [p, [frozenset(b"abcd")], p, [DIGIT, frozenset(), DIGIT], [frozenset()]])
    assert find(emu, b"aaaa", 3, [literal(b"aa")])[0] == [(0, 0), (1, 0), (2, 0)]


def test_h_singletons_equal_the_literal_search(emu, lit_emu):
    """(h) all-singleton patterns give what find_emu gives for the same literals."""
    rng = np.random.default_rng(6)
    for n, mis in ((8193, 0), (4097, 11), (17, 6)):
        d = rng.integers(97, 100, n, dtype=np.uint8).tobytes()
        lits = [d[5:6], d[3:5], d[1:9], d[0:10], d[2:17], b"ab", b"ab"]
        raw, addr = placed(d, mis)
        flat = np.frombuffer(b"".join(lits) + b"\0", np.uint8)
        off = np.zeros(len(lits) + 1, np.uint32)
        off[1:] = np.cumsum([len(p) for p in lits])
        cap = (n + 1) * len(lits)
        counts, offs, which = np.zeros(len(lits), np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8)
        nfound, launches = U64(0), U32(0)
        assert lit_emu.fnd_emu_find(addr, n, 0, flat.ctypes.data, off.ctypes.data, len(lits), 64 << 20, NO_LIMIT,
                                    counts.ctypes.data, offs.ctypes.data, which.ctypes.data, cap, ctypes.byref(nfound),
                                    ctypes.byref(launches)) == 0
        k = nfound.value
        got, c2, _ = find(emu, d, mis, [literal(p) for p in lits])
        assert got == list(zip(offs[:k].tolist(), which[:k].tolist())) and c2 == counts.tolist() and k > 0


def test_i_limit_and_small_stage(emu):
    """(i) a small staging buffer: several emit launches; limit at, before and after a cut."""
    data = bytes(5 * TILE + 3)
    pats = [[frozenset(range(10))], [ANY, frozenset({0, 9})]]
    want = ref(data, pats)
    full, counts, launches = find(emu, data, 2, pats)
    assert full == want and launches == 1 and counts == [len(data), len(data) - 1]
    got, c2, launches = find(emu, data, 2, pats, stage=1)  # the least staging: a launch per tile
    assert got == want and c2 == counts and launches == 6
    got, _, launches = find(emu, data, 2, pats, stage=5 * 3 * 2 * TILE)
    assert got == want and launches == 2
    for limit in (0, 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, len(want), len(want) + 1):
        got, c3, launches = find(emu, data, 11, pats, stage=5 * 2 * TILE, limit=limit)
        assert got == want[:limit] and c3 == counts
        assert launches == (0 if limit == 0 else min(-(-limit // (2 * TILE)), 6))


def grouped(emu, data, bounds, lo, hi, pats, stage=64 << 20, limit=NO_LIMIT):
    buf = np.frombuffer(data + b"\0", np.uint8)
    b = np.asarray(bounds, np.uint64)
    bm, off = class_arrays(pats)
    cap = (len(data) + 1) * len(pats)
    counts, offs, which = np.zeros(len(pats), np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8)
    nfound, launches = U64(0), U32(0)
    bad = emu.fcl_emu_find_grouped(buf.ctypes.data, b.ctypes.data, len(bounds) - 1, lo, hi, bm.ctypes.data, off.ctypes.data,
                                   len(pats), stage, limit, counts.ctypes.data, offs.ctypes.data, which.ctypes.data, cap,
                                   ctypes.byref(nfound), ctypes.byref(launches))
    assert bad == 0
    k = nfound.value
    return list(zip(offs[:k].tolist(), which[:k].tolist())), counts.tolist()


def test_j_grouped_search_with_groups_smaller_than_the_pattern(emu):
    """(j) the grouped walk as the reader runs it (scan buffer = carry + the group's bytes): the
    same matches however the stream is cut, groups shorter than L included; the last pattern's
    final class holds 0x00, which the zeros behind a group's bytes must not satisfy."""
    rng = np.random.default_rng(8)
    d = bytearray(rng.integers(97, 100, 6000, dtype=np.uint8).tobytes())
    long = rng.integers(48, 58, 256, dtype=np.uint8).tobytes()
    for o in (90, 1000, 4095 - 100, 6000 - 256):
        d[o:o + 256] = long
    data = bytes(d)
    pats = [[DIGIT] * 256, literal(b"ab", True), [DIGIT] * 8 + [frozenset({long[8]})], [frozenset(b"ab"), ANY, frozenset(b"c")],
            literal(b"ab", True), [DIGIT] * 100 + [frozenset({0, 0x61})]]
    cuts = [list(range(0, 6001, 100)), [0, 6000], [0, 1, 2, 3, 50, 51, 300, 4096, 4097, 6000],
            [0] + sorted(set(rng.integers(1, 6000, 40).tolist())) + [6000]]
    for lo, hi in ((0, 6000), (91, 5999), (1000, 1256), (1001, 1256), (3000, 3000)):
        want = ref(data, pats, lo, hi)
        for bounds in cuts:
            sel = [i for i in range(len(bounds) - 1) if bounds[i] < hi and bounds[i + 1] > lo] if hi > lo else []
            if not sel:
                continue
            b = bounds[sel[0]:sel[-1] + 2]
            got, counts = grouped(emu, data, b, lo, hi, pats)
            assert got == want, (lo, hi, b[:5])
            assert counts == counts_of(want, len(pats))
            assert grouped(emu, data, b, lo, hi, pats, stage=1, limit=7)[0] == want[:7]


def test_limits_of_a_call(emu):
    """64 distinct table classes work, the 65th is refused; masked equalities count against nothing;
    17 patterns, 257 positions and an empty pattern are refused."""
    every = {frozenset(b for b in range(256) if b & mask == value) for mask in range(256) for value in range(256)
             if not value & ~mask}
    tables = [t for t in (frozenset({k, 255 - k, 7}) for k in range(8, 120)) if t not in every][:65]
    assert len(set(tables)) == 65
    data = bytes(range(256)) * 2
    ok = [tables[16 * i:16 * i + 16] * 2 + literal(b"xY", True) + [ANY] for i in range(4)]
    check(emu, data, 3, ok)
    assert find(emu, data, 3, ok + [[tables[64]]], refuse=True) == NO_LIMIT
    assert find(emu, data, 3, [[DIGIT]] * 17, refuse=True) == NO_LIMIT
    assert find(emu, data, 3, [[DIGIT] * 257], refuse=True) == NO_LIMIT
    assert find(emu, data, 3, [[DIGIT], []], refuse=True) == NO_LIMIT


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "findcls_emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout and "runtime error" not in r.stderr
