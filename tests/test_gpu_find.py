"""Search on the device: kolm_find_device, Reader.find / find_many / count / count_many, kolm.find.

Expected results never come from the code under test: `ref` below is repeated bytes.find over
data[lo:hi], the pairs sorted.  The small matrix of kolm_find_device is also compared with the CPU
emulation of the kernels (tools/find_emu.cpp, built here with g++)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from kolm import datagen as D

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TILE = 4096
NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8193)
LENS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 255, 256)


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
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fnd") / "find_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(REPO, "tools", "find_emu.cpp"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.fnd_emu_find.restype = ctypes.c_uint64
    lib.fnd_emu_find.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def emu_find(emu, data, mis, pats):
    """The emulation over data placed `mis` bytes past a 16-byte boundary: (pairs, violations)."""
    raw = np.full(len(data) + 64, 0xEE, np.uint8)
    at = 16 + (mis - (raw.ctypes.data + 16)) % 16
    raw[at:at + len(data)] = np.frombuffer(data, np.uint8)
    flat = np.frombuffer(b"".join(pats) + b"\0", np.uint8)
    off = np.zeros(len(pats) + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in pats])
    cap = (len(data) + 1) * len(pats)
    counts, offs, which = np.zeros(len(pats), np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint8)
    nfound, launches = ctypes.c_uint64(0), ctypes.c_uint32(0)
    bad = emu.fnd_emu_find(raw.ctypes.data + at, len(data), 0, flat.ctypes.data, off.ctypes.data, len(pats), 64 << 20,
                           (1 << 64) - 1, counts.ctypes.data, offs.ctypes.data, which.ctypes.data, cap,
                           ctypes.byref(nfound), ctypes.byref(launches))
    k = nfound.value
    return list(zip(offs[:k].tolist(), which[:k].tolist())), bad, counts.tolist()


def haystack(kind, n, ln, seed):
    """(data, patterns) of the four kinds of the length sweep."""
    rng = np.random.default_rng(seed)
    if kind == 0:  # every position a candidate that verifies the whole pattern
        return bytes(n), [bytes(ln)]
    if kind == 1:
        return (b"abc" * (n // 3 + 1))[:n], [(b"bca" * 86)[:ln]]
    if kind == 2:
        d = rng.integers(97, 99, n, dtype=np.uint8).tobytes()
        return d, [(d[:ln] + b"a" * ln)[:ln], b"a" * min(ln, 3)]
    d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    pat = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
    spots = [0, TILE - (ln + 1) // 2, 2 * TILE - 1, n - ln]  # the start, across the tile boundaries, the very end
    if ln < 64:
        spots += [512 + k * 271 for k in range(1, 17)]     # across lane (16-byte) boundaries at every phase
    for o in spots:
        if 0 <= o and o + ln <= n:
            d[o:o + ln] = pat
    pats = [pat]
    if ln < 256:  # its prefix ends the buffer, its last byte would lie past the end: no match
        pats.append(pat + bytes([pat[-1] ^ 0x55]))
    return bytes(d), pats


# ------------------------------------------------------------------ 1. kolm_find_device

def test_find_device_small_matrix(kolm_gpu, lib, emu):
    """Every misalignment with every pattern length: the planted haystack at n = 8193 (tile
    boundaries, lane boundaries, the truncated pattern at the very end) and one of the other
    haystack kinds at a length that cycles through the list."""
    cases = 0
    for mis in range(16):
        for k, ln in enumerate(LENS):
            for kind, n in ((3, 8193), ((mis + k) % 3, NS[(mis + 2 * k) % len(NS)])):
                data, pats = haystack(kind, n, ln, 1000 * mis + k)
                want = ref(data, pats)
                offs, which, counts, _ = lib.find_bytes(data, pats, data_offset=mis)
                assert list(zip(offs, which)) == want, (mis, ln, kind, n)
                assert counts == [sum(1 for _, i in want if i == j) for j in range(len(pats))]
                got_emu, bad, emu_counts = emu_find(emu, data, mis, pats)
                assert bad == 0 and got_emu == want and emu_counts == counts, (mis, ln, kind, n)
                cases += 1
    assert cases == 2 * 16 * len(LENS)
    data, pats = haystack(3, 8193, 9, 5)
    assert ref(data, pats[:1])[-1] == (8193 - 9, 0) and data.endswith(pats[1][:-1])


def test_find_device_limit_and_capacity(kolm_gpu, lib):
    data = bytes(3 * TILE + 5)
    want = ref(data, [b"\0\0", b"\0"])
    for limit in (0, 1, 7, len(want) - 1, len(want), len(want) + 1):
        offs, which, counts, _ = lib.find_bytes(data, [b"\0\0", b"\0"], limit=limit, data_offset=3)
        assert list(zip(offs, which)) == want[:limit]
        assert counts == [len(data) - 1, len(data)]


# ------------------------------------------------------------------ 2. readers over containers made here

@pytest.fixture(scope="module")
def text():
    return D.enwik_like(200_000, seed=31)


@pytest.fixture(scope="module")
def containers(kolm_gpu, text):
    """[(name, container, data)]: fixed blocks of 100, 4096 and 65536 bytes, and one CDC container."""
    kolm = kolm_gpu
    return [("fixed100", kolm.compress_blocks_fixed(text[:20_000], 100, hot_path=True), text[:20_000]),
            ("fixed4096", kolm.compress_blocks_fixed(text, 4096, hot_path=True), text),
            ("fixed65536", kolm.compress_blocks_fixed(text, 65536, hot_path=True), text),
            ("cdc", kolm.compress_blocks_cdc(text, hot_path=True), text)]


def pattern_sets(data):
    word = data[1000:1004]
    return [[word], [b"e"], [word, data[1000:1012]],           # one a prefix of the other
            [word, data[5000:5007], word],                      # a duplicate: both reported
            [b"\xff\xfe not in the text \xfd", word, b"\x00\x01"],  # absent patterns
            [data[k:k + 1 + k % 23] for k in range(300, 300 + 16 * 97, 97)]]  # 16 patterns


def test_reader_find(kolm_gpu, containers):
    kolm = kolm_gpu
    for name, blob, data in containers:
        with kolm.open_container(blob) as rd:
            for pats in pattern_sets(data):
                want = ref(data, pats)
                assert rd.find_many(pats) == want, (name, pats)
                st = kolm.last_find()
                assert st["matches"] == len(want) == st["returned"] and st["patterns"] == len(pats)
                assert st["blocks_decoded"] == len([b for b in rd.blocks if b[1]])
                assert rd.count_many(pats) == [sum(1 for _, i in want if i == j) for j in range(len(pats))]
            assert rd.find(pats[0]) == [o for o, i in ref(data, pats[:1])]
        assert kolm.find(blob, data[1000:1004], 500, 9000) == [o for o, _ in ref(data, [data[1000:1004]], 500, 9000)]
    dup = ref(containers[1][2], pattern_sets(containers[1][2])[3])
    assert any(i == 2 for _, i in dup) and [o for o, i in dup if i == 0] == [o for o, i in dup if i == 2]


# ------------------------------------------------------------------ 3. group independence

def test_group_independence(kolm_gpu, containers, monkeypatch):
    kolm = kolm_gpu
    zeros = bytes(65536)
    zblob = kolm.compress_blocks_fixed(zeros, 4096, hot_path=True)
    _, blob, data = containers[1]
    pats = pattern_sets(data)[2]
    results = []
    for env in ({}, {"KOLM_READ_BYTES": "4096"}, {"KOLM_FIND_STAGE": "65536"},
                {"KOLM_READ_BYTES": "4096", "KOLM_FIND_STAGE": "1"}):
        monkeypatch.delenv("KOLM_READ_BYTES", raising=False)
        monkeypatch.delenv("KOLM_FIND_STAGE", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with kolm.open_container(zblob) as rd:
            z = rd.find(b"\0")
            zst = kolm.last_find()
        with kolm.open_container(blob) as rd:
            t = rd.find_many(pats)
            tst = kolm.last_find()
        results.append((z, t))
        assert zst["matches"] == 65536
        if "KOLM_READ_BYTES" in env:
            assert zst["groups"] == 16 and tst["groups"] == tst["blocks_decoded"]
        else:
            assert zst["groups"] == 1 and tst["groups"] == 1
        if env == {"KOLM_FIND_STAGE": "65536"}:  # 13107 records per launch, 4096 per tile: 3 tiles a launch
            assert zst["emit_launches"] == 6
        if env == {}:
            assert zst["emit_launches"] == 1
    assert results[0] == (list(range(65536)), ref(data, pats))
    assert all(r == results[0] for r in results[1:])


# ------------------------------------------------------------------ 4. a match across many groups

def test_match_across_groups(kolm_gpu, text, monkeypatch):
    kolm = kolm_gpu
    rng = np.random.default_rng(4)
    pat = rng.integers(0, 256, 256, dtype=np.uint8).tobytes()
    d = bytearray(text[:3000])
    for o in (150, 777, 1999, 3000 - 256):  # each spans three or four 100-byte blocks
        d[o:o + 256] = pat
    data = bytes(d)
    blob = kolm.compress_blocks_fixed(data, 100, hot_path=True)
    pats = [pat, pat[:9], data[40:43]]
    for limit in ("100", "1", "250"):
        monkeypatch.setenv("KOLM_READ_BYTES", limit)
        with kolm.open_container(blob) as rd:
            assert rd.find_many(pats) == ref(data, pats)
            assert kolm.last_find()["groups"] == (30 if limit != "250" else 15)
            assert rd.find(pat) == [150, 777, 1999, 3000 - 256]
            assert rd.find(pat, 151, 2999) == [777, 1999]
            assert rd.find_many(pats, 433, 2101) == ref(data, pats, 433, 2101)


# ------------------------------------------------------------------ 5. window edges, 6. limit

def test_window_edges(kolm_gpu, containers):
    kolm = kolm_gpu
    for name, blob, data in containers:
        pat = data[7000:7011]
        o = data.find(pat)
        with kolm.open_container(blob) as rd:
            assert rd.find(pat, o, o + len(pat)) == [o]
            assert rd.find(pat, o + 1, o + len(pat)) == [] and rd.find(pat, o, o + len(pat) - 1) == []
            assert rd.find(pat, o, o) == [] and rd.find(pat, len(data), len(data) + 5) == []
            assert rd.find(pat, 0, len(data)) == rd.find(pat) == rd.find(pat, 0, len(data) + 99) == \
                [x for x, _ in ref(data, [pat])]
            assert rd.count(pat, o, o + len(pat)) == 1 and rd.count(pat, o + 1) == len(ref(data, [pat], o + 1))


def test_limit_and_count(kolm_gpu, containers):
    kolm = kolm_gpu
    _, blob, data = containers[1]
    pats = pattern_sets(data)[2]
    want = ref(data, pats)
    assert len(want) > 3
    with kolm.open_container(blob) as rd:
        for k in (0, 1, len(want) - 1, len(want), len(want) + 1):
            assert rd.find_many(pats, limit=k) == want[:k]
            st = kolm.last_find()
            assert st["matches"] == len(want) and st["returned"] == min(k, len(want))
        assert rd.count(pats[0]) == len(rd.find(pats[0])) == len(ref(data, pats[:1]))
        rd.count(pats[0])
        assert kolm.last_find()["emit_launches"] == 0 and kolm.last_find()["returned"] == 0
        assert rd.find(b"\xff\xfe\xfd") == [] and kolm.last_find()["emit_launches"] == 0


# ------------------------------------------------------------------ 7. every method, host fallback

KEYS = {1: "xor", 2: "rice0", 3: "rice1", 4: "rice4", 5: "rice8", 6: "rice16", 7: "lz77", 8: "lfsr", 9: "repair"}


@pytest.fixture(scope="module")
def every_method_case(kolm_gpu, golden_kernels):
    """One block per method id 0..10 for two golden inputs, each the reference's own payload,
    under a TOC written here (as tests/test_gpu_range.py builds it)."""
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
    hob = data[11 * 4096:]
    pats = [hob[100:108], hob[5:6], data[4090:4100], hob[200:203]]
    for env in (None, "5000"):
        if env:
            monkeypatch.setenv("KOLM_READ_BYTES", env)
        with kolm.open_container(blob) as rd:
            assert rd.find_many(pats) == ref(data, pats)
            assert kolm.last_find()["blocks_decoded"] == 22
            assert rd.find_many(pats, 3000, len(data) - 3000) == ref(data, pats, 3000, len(data) - 3000)


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
    pats = [data[50:53], data[len(data) // 2:len(data) // 2 + 9], data[50:53]]
    with kolm.open_container(blob) as rd:
        dev = rd.find_many(pats), rd.find_many(pats, 10, len(data) - 10, limit=5), rd.count_many(pats)
        assert "host" not in kolm.last_find()
    monkeypatch.setattr(lib, "KOLM_DECODE_MASK", lib.KOLM_DECODE_MASK & ~(1 << 10))
    with kolm.open_container(blob) as rd:
        assert rd._host_blocks
        host = rd.find_many(pats), rd.find_many(pats, 10, len(data) - 10, limit=5), rd.count_many(pats)
        assert kolm.last_find().get("host") is True
    assert dev == host and dev[0] == ref(data, pats) and dev[1] == ref(data, pats, 10, len(data) - 10)[:5]


# ------------------------------------------------------------------ 8. checksums

def test_checksums(kolm_gpu, containers):
    from kolm.checksums import Checksums, KolmChecksumError
    kolm = kolm_gpu
    _, blob, data = containers[1]
    cs = kolm.checksums_of(blob)
    crcs = list(cs.crcs)
    crcs[3] ^= 0x00010000
    bad = Checksums(cs.mode, cs.size_field, cs.total_len, cs.lens, crcs)
    pat = data[1000:1004]
    with kolm.open_container(blob, checksums=cs) as rd:
        assert rd.find(pat) == [o for o, _ in ref(data, [pat])]
    with kolm.open_container(blob, checksums=bad) as rd:
        assert rd.find(pat, 0, 3 * 4096) == [o for o, _ in ref(data, [pat], 0, 3 * 4096)]
        before = kolm.last_find()
        for lo, hi in ((0, len(data)), (3 * 4096, 4 * 4096), (4 * 4096 - 1, 5 * 4096)):
            with pytest.raises(KolmChecksumError) as ei:
                rd.find(pat, lo, hi)
            assert ei.value.block == 3 and ei.value.expected == crcs[3] and ei.value.got == cs.crcs[3]
        assert kolm.last_find() == before
        assert rd.find(pat, 4 * 4096) == [o for o, _ in ref(data, [pat], 4 * 4096)]


# ------------------------------------------------------------------ 9. argument errors

def test_argument_errors(kolm_gpu, lib, containers):
    kolm = kolm_gpu
    _, blob, data = containers[1]
    rd = kolm.open_container(blob)
    assert rd.find(data[:4], limit=1) == [0]
    before = kolm.last_find()
    for bad in ([b""], [b"x" * 257], [b"a"] * 17, [], [b"ok", b""]):
        with pytest.raises(ValueError):
            rd.find_many(bad)
        with pytest.raises(ValueError):
            rd.count_many(bad)
    for args in ((b"a", -1), (b"a", 0, -1)):
        with pytest.raises(ValueError):
            rd.find(*args)
    with pytest.raises(ValueError):
        rd.find(b"a", limit=-1)
    # the library's own checks, behind the binding's: the message names the pattern
    for bad, text in (([b"ab", b""], "pattern 1 is empty"), ([b"x" * 257], "pattern 0 has 257 bytes"),
                      ([b"a"] * 17, "17 patterns"), ([], "0 patterns")):
        with pytest.raises(ValueError, match=text):
            lib.reader_find(rd._h, bad, 0, 10)
        with pytest.raises(ValueError, match=text):
            lib.find_bytes(b"some bytes", bad)
    for lo, hi in ((5, 4), (0, len(data) + 1)):
        with pytest.raises(ValueError, match="window"):
            lib.reader_find(rd._h, [b"a"], lo, hi)
    assert kolm.last_find() == before
    rd.close()
    with pytest.raises(ValueError, match="closed"):
        rd.find(b"a")
    with pytest.raises(ValueError, match="closed"):
        rd.count(b"a")
    # a selected block the device does not decode: block and method named, before any launch
    odd = kolm.write_container(kolm.MODE_FIXED, 8, 16, [0, 11], [8, 8], [b"abcdefgh", b"12345678"])
    with kolm.open_container(odd) as r2:
        assert r2.find(b"cd", 0, 8) == [2]
        with pytest.raises(ValueError, match=r"block 1 \(method 11"):
            lib.reader_find(r2._h, [b"cd"], 0, 16)
    assert kolm.last_find()["bytes_scanned"] == 8
