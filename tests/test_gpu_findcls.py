"""Class patterns on the device: kolm_find_classes_device, Reader.find_classes / count_classes, the
ignore_case searches and grep.

Expected results never come from the code under test: `ref` below is Python's re on the CPU, a
lookahead (every overlapping start) over the expression itself, or over an expression of \\xHH
classes generated here from a pattern's sets.  The small matrix of kolm_find_classes_device is also
compared with the CPU emulation of the kernels (tools/findcls_emu.cpp, built here with g++)."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from kolm import datagen as D

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TILE = 4096
NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8193)
MS = (1, 2, 7, 8, 9, 16, 17, 255, 256)
ANY = frozenset(range(256))
DIGIT = frozenset(range(48, 58))


def expr_of(pat):
    """A pattern (a set per position) as an expression of \\xHH classes."""
    return b"".join(b"[" + b"".join(b"\\x%02x" % b for b in sorted(c)) + b"]" if c else b"[^\\x00-\\xff]" for c in pat)


def ref(data, exprs, lo=0, hi=None, flags=0):
    """Every (offset, pattern index) with lo <= offset and offset + m <= hi, sorted.  exprs:
    expressions (bytes) or patterns given as sets."""
    hi = len(data) if hi is None else hi
    out = []
    for i, e in enumerate(exprs):
        e = e if isinstance(e, bytes) else expr_of(e)
        rx = re.compile(b"(?=(" + e + b"))", re.DOTALL | flags)
        out += [(lo + m.start(), i) for m in rx.finditer(data[lo:hi])]
    return sorted(out)


def counts_of(want, np_):
    return [sum(1 for _, i in want if i == j) for j in range(np_)]


def bitmaps(pat):
    bm = np.zeros((len(pat), 32), np.uint8)
    for k, c in enumerate(pat):
        for b in c:
            bm[k, b >> 3] |= 1 << (b & 7)
    return bm.tobytes()


@pytest.fixture(scope="module")
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fcl") / "findcls_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(REPO, "tools", "findcls_emu.cpp"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.fcl_emu_find.restype = ctypes.c_uint64
    lib.fcl_emu_find.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def emu_find(emu, data, mis, pats):
    """The emulation over data placed `mis` bytes past a 16-byte boundary: (pairs, violations, counts)."""
    raw = np.zeros(len(data) + 64, np.uint8)
    at = 16 + (mis - (raw.ctypes.data + 16)) % 16
    raw[at:at + len(data)] = np.frombuffer(data, np.uint8)
    flat = np.frombuffer(b"".join(bitmaps(p) for p in pats) + bytes(32), np.uint8)
    off = np.zeros(len(pats) + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in pats])
    cap = (len(data) + 1) * len(pats)
    counts, offs, which = np.zeros(len(pats), np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8)
    nfound, launches = ctypes.c_uint64(0), ctypes.c_uint32(0)
    bad = emu.fcl_emu_find(raw.ctypes.data + at, len(data), 0, flat.ctypes.data, off.ctypes.data, len(pats), 64 << 20,
                           (1 << 64) - 1, counts.ctypes.data, offs.ctypes.data, which.ctypes.data, cap,
                           ctypes.byref(nfound), ctypes.byref(launches))
    k = nfound.value
    return list(zip(offs[:k].tolist(), which[:k].tolist())), bad, counts.tolist()


def haystack(kind, n, m, seed):
    """(data, patterns as sets).  0: zeros under classes that hold 0x00 (a table class, a masked
    equality, wildcards): every position verifies the whole pattern; 1: random bytes under
    wildcards; 2: two-letter noise under case pairs with a table class last; 3: random bytes with
    a digit string planted at 0, at n - m, across the tile boundaries and at every phase of a lane,
    under digit classes, a mix with singletons, and a pattern one longer whose last class holds
    0x00 (its would-be match at n - m ends one byte past n)."""
    rng = np.random.default_rng(seed)
    if kind == 0:
        return bytes(n), [[frozenset(range(10))] * m, [frozenset(range(8))] * m, [ANY] * (m - 1) + [frozenset({0, 0x7A})]]
    if kind == 1:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes(), [[ANY] * m]
    if kind == 2:
        d = rng.integers(97, 99, n, dtype=np.uint8).tobytes()
        src = (d[:m] + b"a" * m)[:m]
        pair = [frozenset({b, b ^ 0x20}) for b in src]
        return d, [pair, pair[:-1] + [frozenset(b"abc")], [frozenset(b"ab")] * min(m, 3)]
    d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    s = rng.integers(48, 58, m, dtype=np.uint8).tobytes()
    spots = [0, TILE - (m + 1) // 2, 2 * TILE - 1, n - m]
    if m < 64:
        spots += [512 + k * 271 for k in range(1, 17)]
    for o in spots:
        if 0 <= o and o + m <= n:
            d[o:o + m] = s
    pats = [[DIGIT] * m, [DIGIT if k % 3 else frozenset({s[k]}) for k in range(m)]]
    if m < 256:
        pats.append([DIGIT] * m + [frozenset({0, 0x7A})])
    return bytes(d), pats


# ------------------------------------------------------------------ 1. kolm_find_classes_device

def test_find_classes_device_small_matrix(kolm_gpu, lib, emu):
    """Every misalignment with every pattern length: the planted haystack at n = 8193 and one of
    the other kinds at a length that cycles through the list; against re and the emulation."""
    cases = 0
    for mis in range(16):
        for k, m in enumerate(MS):
            for kind, n in ((3, 8193), ((mis + k) % 3, NS[(mis + 2 * k) % len(NS)])):
                data, pats = haystack(kind, n, m, 1000 * mis + k)
                want = ref(data, pats)
                offs, which, counts, _ = lib.find_classes_bytes(data, [bitmaps(p) for p in pats], data_offset=mis)
                assert list(zip(offs, which)) == want, (mis, m, kind, n)
                assert counts == counts_of(want, len(pats))
                got_emu, bad, emu_counts = emu_find(emu, data, mis, pats)
                assert bad == 0 and got_emu == want and emu_counts == counts, (mis, m, kind, n)
                cases += 1
    assert cases == 2 * 16 * len(MS)
    data, pats = haystack(3, 8193, 9, 5)
    assert ref(data, pats[:1])[-1] == (8193 - 9, 0) and (8193 - 9, 2) not in ref(data, pats)


def test_find_classes_device_sixteen_patterns_limit_and_capacity(kolm_gpu, lib, emu):
    data, base = haystack(3, 8193, 9, 77)
    s = data[:9]
    pats = [[DIGIT if (k + i) % 3 else frozenset({s[k]}) if i % 2 else ANY for k in range(9)] for i in range(13)]
    pats += [base[0], base[0], [DIGIT, frozenset(), DIGIT]]  # two identical patterns; an empty class
    want = ref(data, pats)
    assert counts_of(want, 16)[13] == counts_of(want, 16)[14] > 16 and counts_of(want, 16)[15] == 0
    for mis in (0, 7):
        offs, which, counts, _ = lib.find_classes_bytes(data, [bitmaps(p) for p in pats], data_offset=mis)
        assert list(zip(offs, which)) == want and counts == counts_of(want, 16)
        assert emu_find(emu, data, mis, pats) == (want, 0, counts)
    data = bytes(3 * TILE + 5)
    two = [[frozenset(range(10))] * 2, [frozenset({0, 9})]]
    want = ref(data, two)
    for limit in (0, 1, 7, len(want) - 1, len(want), len(want) + 1):
        offs, which, counts, _ = lib.find_classes_bytes(data, [bitmaps(p) for p in two], limit=limit, data_offset=3)
        assert list(zip(offs, which)) == want[:limit]
        assert counts == [len(data) - 1, len(data)]


# ------------------------------------------------------------------ 2. readers over containers made here

DATES = [b"2024-01-15", b"1999-12-31", b"2031-07-04", b"0000-00-00"]


@pytest.fixture(scope="module")
def text():
    """Text with dates, ERROR codes and words in odd case planted, some across the 4096-byte block
    boundaries; one date ends the data."""
    d = bytearray(D.enwik_like(200_000, seed=31))
    for k, o in enumerate(list(range(900, 190_000, 7001)) + [4096 * 3 - 4, 4096 * 7 - 9, 4096 * 11 - 1, 65536 - 5]):
        d[o:o + 10] = DATES[k % 4]
    for k, o in enumerate(range(2500, 180_000, 9973)):
        d[o:o + 9] = b"ERROR %03d" % (k * 37 % 1000)
        d[o + 40:o + 48] = (b"Compress", b"COMPRESS", b"cOmPrEsS", b"compress")[k % 4]
    d[-10:] = DATES[0]
    return bytes(d)


@pytest.fixture(scope="module")
def containers(kolm_gpu, text):
    """[(name, container, data)]: fixed blocks of 100 and 4096 bytes, and one CDC container."""
    kolm = kolm_gpu
    return [("fixed100", kolm.compress_blocks_fixed(text[:20_000], 100, hot_path=True), text[:20_000]),
            ("fixed4096", kolm.compress_blocks_fixed(text, 4096, hot_path=True), text),
            ("cdc", kolm.compress_blocks_cdc(text, hot_path=True), text)]


def expression_sets(data):
    word = data[1000:1005]
    return [[rb"\d{4}-\d{2}-\d{2}"], [rb"ERROR [0-9]{3}"], [rb".he"], [rb"t.e"], [rb"th."],  # a wildcard first, middle, last
            [rb"[a-c][^a-z]", rb"\s\S\s"], [rb"\d\d", rb"\d\d"],                             # identical: both reported
            [rb"\x00\xff[\x01-\x03]", re.escape(word)],                                     # an absent pattern
            [rb"\d{4}-\d{2}-\d{2}", rb"ERROR \d", rb"[Cc]ompress", rb".{5}RR", rb"\w\W\w", rb"[^\x00-\x7f]", rb"e[rs] ",
             rb"[A-Z][a-z]{3}", rb"\s[aeiou]", rb"-\d\d-", re.escape(word), rb"[\d_][\d_]", rb"\S{12}", rb"q.", rb"[.,;] ",
             rb"the"]]                                                                      # 16 mixed patterns


def test_reader_find_classes(kolm_gpu, containers):
    kolm = kolm_gpu
    for name, blob, data in containers:
        with kolm.open_container(blob) as rd:
            for exprs in expression_sets(data):
                want = ref(data, exprs)
                assert rd.find_classes(exprs) == want, (name, exprs)
                st = kolm.last_find()
                assert st["matches"] == len(want) == st["returned"] and st["patterns"] == len(exprs)
                assert st["blocks_decoded"] == len([b for b in rd.blocks if b[1]])
                assert rd.count_classes(exprs) == counts_of(want, len(exprs))
                assert kolm.last_find()["emit_launches"] == 0
            # one expression, one ClassPattern, patterns given as sets
            assert rd.find_classes(rb"\d{4}-\d{2}-\d{2}") == ref(data, [rb"\d{4}-\d{2}-\d{2}"])
            p = kolm.ClassPattern.of([DIGIT, {ord("-")}, DIGIT])
            assert rd.find_classes(p) == rd.find_classes([kolm.classes.compile(rb"\d-\d")]) == ref(data, [[DIGIT, {45}, DIGIT]])
    dates = ref(containers[1][2], [rb"\d{4}-\d{2}-\d{2}"])
    assert len(dates) >= 30 and (len(containers[1][2]) - 10, 0) in dates and (4096 * 3 - 4, 0) in dates


def test_ignore_case_words(kolm_gpu, containers):
    kolm = kolm_gpu
    for name, blob, data in containers:
        words = [b"compress", b"The", b"e", data[1000:1012], b"@`[{"]
        want = ref(data, [re.escape(w) for w in words], flags=re.IGNORECASE)
        with kolm.open_container(blob) as rd:
            assert rd.find_many(words, ignore_case=True) == want, name
            assert rd.count_many(words, ignore_case=True) == counts_of(want, len(words))
            assert rd.find_classes([kolm.classes.compile(re.escape(w), True) for w in words]) == want
            for i, w in enumerate(words[:3]):
                mine = [o for o, j in want if j == i]
                # find(p, ignore_case=True) is find_classes(literal(p, True)); find(p) is unchanged
                assert rd.find(w, ignore_case=True) == mine == [o for o, _ in rd.find_classes(kolm.ClassPattern.literal(w, True))]
                assert rd.count(w, ignore_case=True) == len(mine)
                exact = [o for o, _ in ref(data, [re.escape(w)])]
                assert rd.find(w) == exact == [o for o, _ in rd.find_classes(kolm.ClassPattern.literal(w))]
            assert rd.find(b"COMPRESS", 100, 150_000, limit=3, ignore_case=True) == \
                [o for o, _ in ref(data, [b"compress"], 100, 150_000, re.IGNORECASE)][:3]
        assert kolm.find(blob, b"compRESS", 500, 90_000, ignore_case=True) == \
            [o for o, _ in ref(data, [b"compress"], 500, 90_000, re.IGNORECASE)]
        assert kolm.find(blob, b"Compress", 500, 90_000) == [o for o, _ in ref(data, [b"Compress"], 500, 90_000)]
    want = ref(containers[1][2], [b"compress"], flags=re.IGNORECASE)
    assert len(want) > len(ref(containers[1][2], [b"compress"])) + 5


# ------------------------------------------------------------------ 3. group independence

def test_group_independence(kolm_gpu, containers, monkeypatch):
    """The same lists whatever KOLM_READ_BYTES and KOLM_FIND_STAGE are; zeros under a class that
    holds 0x00 make every position a match and every carry count."""
    kolm = kolm_gpu
    zeros = bytes(65536)
    zblob = kolm.compress_blocks_fixed(zeros, 4096, hot_path=True)
    _, blob, data = containers[1]
    exprs = expression_sets(data)[-1]
    results = []
    for env in ({}, {"KOLM_READ_BYTES": "4096"}, {"KOLM_FIND_STAGE": "65536"},
                {"KOLM_READ_BYTES": "4096", "KOLM_FIND_STAGE": "1"}, {"KOLM_READ_BYTES": "10000"}):
        monkeypatch.delenv("KOLM_READ_BYTES", raising=False)
        monkeypatch.delenv("KOLM_FIND_STAGE", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with kolm.open_container(zblob) as rd:
            z = rd.find_classes(rb"[\x00-\x09]{3}")
            zst = kolm.last_find()
        with kolm.open_container(blob) as rd:
            t = rd.find_classes(exprs)
            tst = kolm.last_find()
        results.append((z, t))
        assert zst["matches"] == 65534
        if env.get("KOLM_READ_BYTES") == "4096":
            assert zst["groups"] == 16 and tst["groups"] == tst["blocks_decoded"]
        elif not env.get("KOLM_READ_BYTES"):
            assert zst["groups"] == 1 and tst["groups"] == 1
        if env == {"KOLM_FIND_STAGE": "65536"}:  # 13107 records per launch, 4096 per tile: 3 tiles a launch
            assert zst["emit_launches"] == 6
        if env == {}:
            assert zst["emit_launches"] == 1
        if env.get("KOLM_FIND_STAGE") == "1":
            assert tst["emit_launches"] > tst["groups"] / 2
    assert results[0] == ([(o, 0) for o in range(65534)], ref(data, exprs))
    assert all(r == results[0] for r in results[1:])


def test_match_across_groups(kolm_gpu, text, monkeypatch):
    """A 256-position match spans three or four 100-byte blocks; with groups of one block the
    carries accumulate over several groups."""
    kolm = kolm_gpu
    rng = np.random.default_rng(4)
    s = rng.integers(48, 58, 256, dtype=np.uint8).tobytes()
    d = bytearray(text[:3000].replace(b"0", b"o"))
    for o in (150, 777, 1999, 3000 - 256):
        d[o:o + 256] = s
    data = bytes(d)
    blob = kolm.compress_blocks_fixed(data, 100, hot_path=True)
    exprs = [rb"\d{256}", rb"\d{8}" + s[8:9], rb"[a-z] [a-z]", rb"\d{100}[\x00a-z]"]
    for limit in ("100", "1", "250"):
        monkeypatch.setenv("KOLM_READ_BYTES", limit)
        with kolm.open_container(blob) as rd:
            assert rd.find_classes(exprs) == ref(data, exprs)
            assert kolm.last_find()["groups"] == (30 if limit != "250" else 15)
            assert [o for o, _ in rd.find_classes(exprs[0])] == [150, 777, 1999, 3000 - 256]
            assert [o for o, _ in rd.find_classes(exprs[0], 151, 2999)] == [777, 1999]
            assert rd.find_classes(exprs, 433, 2101) == ref(data, exprs, 433, 2101)


# ------------------------------------------------------------------ 4. window edges, limit

def test_window_edges(kolm_gpu, containers):
    kolm = kolm_gpu
    e = rb"\d{4}-\d{2}-\d{2}"
    for name, blob, data in containers:
        o = ref(data, [e])[2][0]
        with kolm.open_container(blob) as rd:
            f = lambda *a: [x for x, _ in rd.find_classes(e, *a)]  # noqa: E731
            assert f(o, o + 10) == [o]
            assert f(o + 1, o + 10) == [] and f(o, o + 9) == []
            assert f(o, o) == [] and f(o + 5, o) == [] and f(len(data), len(data) + 5) == []
            assert f(0, len(data)) == f() == f(0, len(data) + 99) == [x for x, _ in ref(data, [e])]
            assert rd.count_classes(e, o, o + 10) == [1] and rd.count_classes(e, o + 1) == [len(ref(data, [e], o + 1))]
            # the last date (in the whole text it ends the data), and a window that ends inside it
            last = ref(data, [e])[-1][0]
            assert f(last) == [last] and f(last, last + 9) == [] and f(last - 3, last + 10) == [last]
            assert name == "fixed100" or last == len(data) - 10


def test_limit_and_count(kolm_gpu, containers):
    kolm = kolm_gpu
    _, blob, data = containers[1]
    exprs = [rb"\d\d", rb"[Tt]h[ae]", rb"\d\d"]
    want = ref(data, exprs)
    assert len(want) > 100
    with kolm.open_container(blob) as rd:
        for k in (0, 1, len(want) - 1, len(want), len(want) + 1):
            assert rd.find_classes(exprs, limit=k) == want[:k]
            st = kolm.last_find()
            assert st["matches"] == len(want) and st["returned"] == min(k, len(want))
        assert rd.count_classes(exprs) == counts_of(want, 3)
        assert kolm.last_find()["emit_launches"] == 0 and kolm.last_find()["returned"] == 0
        assert rd.find_classes(rb"\xff[\xfe\xfd]\d") == [] and kolm.last_find()["emit_launches"] == 0
        assert rd.find_classes(kolm.ClassPattern.of([DIGIT, set()])) == []


# ------------------------------------------------------------------ 5. grep

def test_grep_ignore_case_and_classes(kolm_gpu, text):
    kolm = kolm_gpu
    data = text[:120_000]
    blob = kolm.compress_blocks_fixed(data, 4096, hot_path=True)
    lines = data.split(b"\n")
    starts = np.concatenate([[0], np.cumsum([len(ln) + 1 for ln in lines])[:-1]]).tolist()

    def host(exprs, flags=0, lo=0, hi=None):
        """The lines that hold the first byte of a match, from data.split."""
        own = sorted({int(np.searchsorted(starts, o, side="right")) - 1 for o, _ in ref(data, exprs, lo, hi, flags)})
        return [(k, lines[k]) for k in own]

    with kolm.open_container(blob, lines=True) as rd:
        assert rd.grep(b"compress", ignore_case=True) == host([b"compress"], re.IGNORECASE)
        assert rd.grep([b"ERROR", b"the end"], ignore_case=True, limit=5) == host([b"error", b"the end"], re.IGNORECASE)[:5]
        assert rd.grep(b"compress", 3000, 90_000, ignore_case=True) == host([b"compress"], re.IGNORECASE, 3000, 90_000)
        date = kolm.classes.compile(rb"\d{4}-\d{2}-\d{2}")
        assert rd.grep(date) == host([rb"\d{4}-\d{2}-\d{2}"])
        assert rd.grep([date, b"ERROR"]) == host([rb"\d{4}-\d{2}-\d{2}", b"ERROR"])
        assert rd.grep(b"compress") == host([b"compress"]) != rd.grep(b"compress", ignore_case=True)
        assert len(rd.grep(date)) >= 10
        with kolm.PatternSet([b"abc", b"abd"]) as ps:
            with pytest.raises(ValueError):
                rd.grep(ps, ignore_case=True)
        with pytest.raises(ValueError):
            rd.grep([b"w%d" % k for k in range(17)], ignore_case=True)
        with pytest.raises(ValueError):
            rd.grep([date] * 17)


# ------------------------------------------------------------------ 6. every method, host fallback

KEYS = {1: "xor", 2: "rice0", 3: "rice1", 4: "rice4", 5: "rice8", 6: "rice16", 7: "lz77", 8: "lfsr", 9: "repair"}


@pytest.fixture(scope="module")
def every_method_case(kolm_gpu, golden_kernels):
    """One block per method id 0..10 for two golden inputs, each the reference's own payload,
    under a TOC written here (as tests/test_gpu_find.py builds it)."""
    kolm = kolm_gpu
    z = np.load(os.path.join(GOLDEN, "v2new.npz"))
    mids, orig, pays, data = [], [], [], b""
    for name in ("grad4k", "text_hobbit"):
        inp = golden_kernels[f"{name}/input"].tobytes()
        for m in range(11):
            p = inp if m == 0 else z[f"{name}/v2new"].tobytes() if m == 10 else golden_kernels[f"{name}/{KEYS[m]}"].tobytes()
            mids.append(m), orig.append(len(inp)), pays.append(p)
            data += inp
    return kolm.write_container(kolm.MODE_CDC, 4096, len(data), mids, orig, pays), data


def test_every_method_container(kolm_gpu, every_method_case, monkeypatch):
    kolm = kolm_gpu
    blob, data = every_method_case
    exprs = [rb"[Tt]he\s", rb"\s[a-z]{4}\s", re.escape(data[4090:4094]) + rb".{4}", rb"[\x00-\x03][\x04-\x07]", rb"[.,;]\s[A-Z]"]
    assert min(counts_of(ref(data, exprs), 5)) > 0
    for env in (None, "5000"):
        if env:
            monkeypatch.setenv("KOLM_READ_BYTES", env)
        with kolm.open_container(blob) as rd:
            assert rd.find_classes(exprs) == ref(data, exprs)
            assert kolm.last_find()["blocks_decoded"] == 22
            assert rd.find_classes(exprs, 3000, len(data) - 3000) == ref(data, exprs, 3000, len(data) - 3000)


def test_host_fallback_gives_the_same(kolm_gpu, lib, monkeypatch):
    kolm = kolm_gpu
    z = np.load(os.path.join(GOLDEN, "v2new.npz"))
    with open(os.path.join(GOLDEN, "v2new.json")) as f:
        names = list(json.load(f)["containers"])
    for c in names:
        blob, data = z[f"C/{c}/full10"].tobytes(), z[f"C/{c}/input"].tobytes()
        mids = kolm.read_container(blob)[3]
        if 10 in mids and any(m != 10 for m in mids):
            break
    else:
        pytest.fail("no golden container mixes id 10 with other ids")
    mid = data[len(data) // 2:len(data) // 2 + 9]
    exprs = [re.escape(data[50:52]) + rb".", rb".[^\x00]" + re.escape(mid[2:]), rb"[\x00-\x40].[\x00-\x40]",
             kolm.ClassPattern.of([{data[50]}, set(), ANY])]
    rx = [e if isinstance(e, bytes) else e.regex() for e in exprs]

    def run(rd):
        return (rd.find_classes(exprs), rd.find_classes(exprs, 10, len(data) - 10, limit=5), rd.count_classes(exprs),
                rd.find_many([data[50:53], mid], ignore_case=True))

    with kolm.open_container(blob) as rd:
        dev = run(rd)
        assert "host" not in kolm.last_find()
    monkeypatch.setattr(lib, "KOLM_DECODE_MASK", lib.KOLM_DECODE_MASK & ~(1 << 10))
    with kolm.open_container(blob) as rd:
        assert rd._host_blocks
        host = run(rd)
        assert kolm.last_find().get("host") is True
    assert dev == host and dev[0] == ref(data, rx) and dev[1] == ref(data, rx, 10, len(data) - 10)[:5]
    assert dev[3] == ref(data, [re.escape(data[50:53]), re.escape(mid)], flags=re.IGNORECASE) and dev[2][1] >= 1


# ------------------------------------------------------------------ 7. checksums

def test_checksums(kolm_gpu, containers):
    from kolm.checksums import Checksums, KolmChecksumError
    kolm = kolm_gpu
    _, blob, data = containers[1]
    cs = kolm.checksums_of(blob)
    crcs = list(cs.crcs)
    crcs[3] ^= 0x00010000
    bad = Checksums(cs.mode, cs.size_field, cs.total_len, cs.lens, crcs)
    e = rb"[Tt]h[ae]"
    with kolm.open_container(blob, checksums=cs) as rd:
        assert rd.find_classes(e) == ref(data, [e])
    with kolm.open_container(blob, checksums=bad) as rd:
        assert rd.find_classes(e, 0, 3 * 4096) == ref(data, [e], 0, 3 * 4096)
        before = kolm.last_find()
        for lo, hi in ((0, len(data)), (3 * 4096, 4 * 4096), (4 * 4096 - 1, 5 * 4096)):
            with pytest.raises(KolmChecksumError) as ei:
                rd.find_classes(e, lo, hi)
            assert ei.value.block == 3 and ei.value.expected == crcs[3] and ei.value.got == cs.crcs[3]
            with pytest.raises(KolmChecksumError):
                rd.find(b"the", lo, hi, ignore_case=True)
        assert kolm.last_find() == before
        assert rd.find_classes(e, 4 * 4096) == ref(data, [e], 4 * 4096)


# ------------------------------------------------------------------ 8. argument errors

def test_argument_errors(kolm_gpu, lib, containers):
    kolm = kolm_gpu
    _, blob, data = containers[1]
    every = {frozenset(b for b in range(256) if b & mask == value) for mask in range(256) for value in range(256)
             if not value & ~mask}
    tables = [t for t in (frozenset({k, 255 - k, 7}) for k in range(8, 120)) if t not in every][:65]
    assert len(set(tables)) == 65
    rd = kolm.open_container(blob)
    assert rd.find_classes(re.escape(data[:4]), limit=1) == [(0, 0)]
    before = kolm.last_find()
    # 64 distinct table classes work (masked equalities beside them count against nothing)
    ok = [kolm.ClassPattern.of(tables[16 * i:16 * i + 16] + [{0x41, 0x61}, ANY, range(8)]) for i in range(4)]
    sets64 = [tables[16 * i:16 * i + 16] + [{0x41, 0x61}, ANY, set(range(8))] for i in range(4)]
    assert rd.find_classes(ok) == ref(data, sets64)
    before = kolm.last_find()
    for bad in ([kolm.ClassPattern.of([DIGIT])] * 17, [], ok + [kolm.ClassPattern.of([tables[64]])]):
        with pytest.raises(ValueError):
            rd.find_classes(bad)
        with pytest.raises(ValueError):
            rd.count_classes(bad)
    for bad in (rb"\d{257}", rb"", rb"a*", [rb"ok", rb""]):
        with pytest.raises(ValueError):
            rd.find_classes(bad)
    for bad in ([b""], [b"x" * 257], [b"a"] * 17, []):
        with pytest.raises(ValueError):
            rd.find_many(bad, ignore_case=True)
    for args in ((rb"\d", -1), (rb"\d", 0, -1)):
        with pytest.raises(ValueError):
            rd.find_classes(*args)
    with pytest.raises(ValueError):
        rd.find_classes(rb"\d", limit=-1)
    # the library's own checks, behind the binding's: the message names the pattern
    one = bitmaps([DIGIT])
    for bad, msg in (([one, b""], "pattern 1 is empty"), ([bitmaps([DIGIT] * 257)], "pattern 0 has 257 positions"),
                     ([one] * 17, "17 patterns"), ([], "0 patterns"),
                     ([p.bitmaps for p in ok] + [bitmaps([{0x41}]), bitmaps([ANY, ANY, tables[64]])],
                      "position 2 of pattern 5")):
        with pytest.raises(ValueError, match=msg):
            lib.reader_find_classes(rd._h, bad, 0, 10)
        with pytest.raises(ValueError, match=msg):
            lib.find_classes_bytes(b"some bytes", bad)
    for lo, hi in ((5, 4), (0, len(data) + 1)):
        with pytest.raises(ValueError, match="window"):
            lib.reader_find_classes(rd._h, [one], lo, hi)
    assert kolm.last_find() == before
    rd.close()
    with pytest.raises(ValueError, match="closed"):
        rd.find_classes(rb"\d")
    with pytest.raises(ValueError, match="closed"):
        rd.count(b"a", ignore_case=True)
    # a selected block the device does not decode: block and method named, before any launch
    odd = kolm.write_container(kolm.MODE_FIXED, 8, 16, [0, 11], [8, 8], [b"abcdefgh", b"12345678"])
    with kolm.open_container(odd) as r2:
        assert r2.find_classes(rb"[cC].", 0, 8) == [(2, 0)]
        with pytest.raises(ValueError, match=r"block 1 \(method 11"):
            lib.reader_find_classes(r2._h, [one], 0, 16)
    assert kolm.last_find()["bytes_scanned"] == 8
