"""Pattern sets on the device: kolm.PatternSet, Reader.find_set / count_set, kolm_find_set_device.

Expected results never come from the code under test: `ref` is repeated bytes.find over
data[lo:hi], the pairs sorted; the large set uses `ref_dict` (a dictionary per pattern length, slid
over the data).  The small matrix of kolm_find_set_device is also compared with the CPU emulation
of the kernels (tools/findset_emu.cpp, built here with g++); sets of at most 16 patterns are
cross-checked against find_many / count_many."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from kolm import datagen as D

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096
NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8193)
LENS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 255, 256)
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


def ref_dict(data, pats, lo=0, hi=None):
    """The same for a large set of few distinct lengths: {len: {pattern: index}}, slid over the data."""
    hi = len(data) if hi is None else hi
    d, by_len, out = data[lo:hi], {}, []
    for i, p in enumerate(pats):
        by_len.setdefault(len(p), {})[p] = i
    for ln, table in by_len.items():
        for o in range(len(d) - ln + 1):
            i = table.get(d[o:o + ln])
            if i is not None:
                out.append((lo + o, i))
    return sorted(out)


def counts_of(want, npat):
    c = [0] * npat
    for _, i in want:
        c[i] += 1
    return c


@pytest.fixture(scope="module")
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fst") / "findset_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(REPO, "tools", "findset_emu.cpp"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.fst_emu_build.restype = P
    lib.fst_emu_build.argtypes = [P, P, U32, P, P]
    lib.fst_emu_free.restype = None
    lib.fst_emu_free.argtypes = [P]
    lib.fst_emu_find.restype = U64
    lib.fst_emu_find.argtypes = [P, P, U32, U32, U64, U64, P, P, P, U64, P, P]
    return lib


def emu_find(emu, data, mis, pats, cap=None):
    """The emulation over data placed `mis` bytes past a 16-byte boundary: (pairs, violations, counts)."""
    raw = np.full(len(data) + 64, 0xEE, np.uint8)
    at = 16 + (mis - (raw.ctypes.data + 16)) % 16
    raw[at:at + len(data)] = np.frombuffer(data, np.uint8)
    flat = np.frombuffer(b"".join(pats) + b"\0", np.uint8)
    off = np.zeros(len(pats) + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in pats])
    info, dup = np.zeros(7, np.uint32), np.zeros(2, np.uint32)
    h = emu.fst_emu_build(flat.ctypes.data, off.ctypes.data, len(pats), info.ctypes.data, dup.ctypes.data)
    assert h
    cap = (len(data) + 1) * min(len(pats), 256) if cap is None else cap
    counts, offs, which = np.zeros(len(pats), np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)
    nfound, launches = U64(0), U32(0)
    bad = emu.fst_emu_find(h, raw.ctypes.data + at, len(data), 0, 64 << 20, (1 << 64) - 1, counts.ctypes.data,
                           offs.ctypes.data, which.ctypes.data, cap, ctypes.byref(nfound), ctypes.byref(launches))
    emu.fst_emu_free(h)
    k = nfound.value
    return list(zip(offs[:k].tolist(), which[:k].tolist())), bad, counts.tolist()


def mixed_set(n, first, seed):
    """(data, patterns): lengths LENS[first], LENS[first + 2], .. (K = min(8, LENS[first])) over
    seeded random bytes; every pattern planted in a stretch of its own, across the 4 KiB tile
    boundaries, at several lane phases and at the very end (the longest first, so the shorter
    stay whole), each beside its truncation test: one more byte, so that its prefix ends the
    buffer and its last byte would lie past n."""
    rng = np.random.default_rng(seed)
    d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    ks = list(range(first, len(LENS), 2))
    made = {k: rng.integers(0, 256, LENS[k], dtype=np.uint8).tobytes() for k in ks}
    for k in reversed(ks):
        ln, pat = LENS[k], made[k]
        spots = [4200 + 300 * k, TILE - (ln + 1) // 2, 2 * TILE - 1, n - ln]
        if ln < 64:
            spots += [512 + k * 37 + j * 271 for j in range(1, 5)]
        for o in spots:
            if 0 <= o and o + ln <= n:
                d[o:o + ln] = pat
    pats = []
    for k in ks:
        pats.append(made[k])
        if LENS[k] < 256:
            pats.append(made[k] + bytes([made[k][-1] ^ 0x55]))
    return bytes(d), pats


# ------------------------------------------------------------------ 1. kolm_find_set_device

def test_find_set_device_small_matrix(kolm_gpu, lib, emu):
    """Every misalignment with every first length (K = 1, 2, 3, 7, 8): the planted haystack at
    n = 8193 and one at a length that cycles through NS, against `ref` and the emulation."""
    cases = 0
    for mis in range(16):
        for first in range(len(LENS)):
            for n in (8193, NS[(mis + 2 * first) % len(NS)]):
                data, pats = mixed_set(n, first, 1000 * mis + first)
                want = ref(data, pats)
                offs, which, counts, _ = lib.find_set_bytes(data, pats, data_offset=mis)
                assert list(zip(offs, which)) == want, (mis, first, n)
                assert counts == counts_of(want, len(pats))
                got_emu, bad, emu_counts = emu_find(emu, data, mis, pats)
                assert bad == 0 and got_emu == want and emu_counts == counts, (mis, first, n)
                cases += 1
    assert cases == 2 * 16 * len(LENS)
    # a zero pattern one byte longer than the data's zero tail
    data = b"\x01" * 4000 + bytes(97)
    offs, which, counts, _ = lib.find_set_bytes(data, [bytes(98), bytes(97)], data_offset=5)
    assert list(zip(offs, which)) == [(4000, 1)] and counts == [0, 1]


def test_find_set_device_limit_and_capacity(kolm_gpu, lib):
    data = bytes(3 * TILE + 5)
    pats = [b"\0\0", b"\0", b"\0\0\0"]
    want = ref(data, pats)
    k = len(want)
    for limit in (0, 1, k - 1, k, k + 1):
        offs, which, counts, _ = lib.find_set_bytes(data, pats, limit=limit, data_offset=3)
        assert list(zip(offs, which)) == want[:limit]
        assert counts == [len(data) - 1, len(data), len(data) - 2]
    # the two-call pattern: too small a capacity reports the need and emits nothing
    ctx = lib.device_ctx(lib.ensure_init())
    h, info = lib.patset_create(pats, ctx)
    dd = lib.DeviceBuffer(ctx, len(data) + 64)
    try:
        dd.upload(data, 0)
        counts = np.zeros(3, np.uint64)
        offs, which = np.full(8, 77, np.uint64), np.full(8, 77, np.uint32)
        nfound = U64(0)
        rc = lib.load().kolm_find_set_device(ctx, dd.ptr, len(data), h, lib.NO_LIMIT, counts.ctypes.data, offs.ctypes.data,
                                             which.ctypes.data, 8, ctypes.byref(nfound), None)
        assert rc == lib.KOLM_ECAP and nfound.value == k and counts.tolist() == [len(data) - 1, len(data), len(data) - 2]
        assert offs.tolist() == [77] * 8 and which.tolist() == [77] * 8
        rc = lib.load().kolm_find_set_device(ctx, dd.ptr, len(data), h, 8, None, offs.ctypes.data, which.ctypes.data, 8,
                                             ctypes.byref(nfound), None)
        assert rc == 0 and nfound.value == 8 and list(zip(offs.tolist(), which.tolist())) == want[:8]
        assert lib.find_set_device(ctx, dd.ptr, len(data), h, cap=k)[:2] == ([o for o, _ in want], [i for _, i in want])
    finally:
        dd.free()
        lib.patset_free(h)
    assert info["np"] == 3 and info["key_bytes"] == 1 and info["longest"] == 3 and info["longest_bucket"] == 3


def test_prefix_chain(kolm_gpu, lib, monkeypatch):
    """bytes(1) .. bytes(256) over zeros: 256 matches per position, the staging minimum; with a
    1-byte stage a launch per tile."""
    monkeypatch.setenv("KOLM_FIND_STAGE", "1")
    pats = [bytes(k) for k in range(1, 257)]
    n = TILE + 300
    offs, which, counts, _ = lib.find_set_bytes(bytes(n), pats, data_offset=9)
    assert counts == [n - k + 1 for k in range(1, 257)]
    want = [(o, i) for o in range(n) for i in range(min(256, n - o))]
    assert list(zip(offs, which)) == want


def test_every_key_of_a_small_filter(kolm_gpu, lib):
    """All 256 one-byte patterns (K = 1, 256 keys, the smallest filter, spans of two tiles) over
    seven tiles of random bytes: every position matches, so a filter word that does not hold
    what the set put there for the whole span shows as a lost match."""
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, 7 * TILE + 5, dtype=np.uint8).tobytes()
    pats = [bytes([b]) for b in range(256)]
    for mis in (0, 11):
        offs, which, counts, _ = lib.find_set_bytes(data, pats, data_offset=mis)
        assert offs == list(range(len(data))) and which == list(data)
        assert counts == [data.count(p) for p in pats]


def test_thousands_of_tiles(kolm_gpu, lib, emu):
    """32 MiB of text in one buffer (8192 tiles, thousands of workgroups) and 16 patterns of 6..14
    bytes drawn from it, several of them frequent and longer than 8 bytes, so that tens of
    thousands of candidates take the tail verify while other lanes count their matches.  The
    pairs and per-pattern totals must be those of repeated bytes.find on every one of three runs
    (a walk that wrote its counters between the loads of a verify lost about one match in a
    thousand of such patterns here, differently from run to run), and over the first 8 MiB those
    of the emulation."""
    n = 32 << 20
    data = D.enwik_like(n, seed=1)
    pats = list(dict.fromkeys(data[k:k + 6 + i % 9] for i, k in enumerate(range(7777, 7777 + 16 * 65537, 65537))))
    want = ref(data, pats)
    per = counts_of(want, len(pats))
    assert sum(1 for p, c in zip(pats, per) if len(p) > 8 and c > 2000) >= 1 and len(want) > 100_000
    for run in range(3):
        offs, which, counts, _ = lib.find_set_bytes(data, pats, data_offset=(0, 5, 11)[run])
        assert counts == per, (run, [(i, a - b) for i, (a, b) in enumerate(zip(counts, per)) if a != b])
        assert list(zip(offs, which)) == want, run
    part = data[:8 << 20]
    want8 = ref(part, pats)
    got_emu, bad, emu_counts = emu_find(emu, part, 5, pats, cap=len(want8) + 1)
    assert bad == 0 and got_emu == want8 and emu_counts == counts_of(want8, len(pats))
    offs, which, counts, _ = lib.find_set_bytes(part, pats, data_offset=5)
    assert list(zip(offs, which)) == got_emu and counts == emu_counts


# ------------------------------------------------------------------ 2. readers over containers made here

@pytest.fixture(scope="module")
def text():
    return D.enwik_like(60_000, seed=31)


@pytest.fixture(scope="module")
def containers(kolm_gpu, text):
    """[(name, container, data)]: hot-path candidates, blocks of 52 and 4096 bytes, and ids 0..9."""
    kolm = kolm_gpu
    return [("fixed52", kolm.compress_blocks_fixed(text[:6_000], 52, hot_path=True), text[:6_000]),
            ("fixed4096", kolm.compress_blocks_fixed(text, 4096, hot_path=True), text),
            ("ids0to9", kolm.compress_blocks_fixed(text[:20_000], 4096, hot_path=False), text[:20_000])]


def pattern_sets(data):
    word = data[1000:1004]
    big = sorted({data[k:k + 3 + k % 11] for k in range(0, 3000, 13)} | {word, b"e", b"\xff\xfe not there"})
    return [[word], [b"e"], [word, data[1000:1012], data[1000:1256]],   # prefixes of one another, one of 256 bytes
            [b"\xff\xfe not in the text \xfd", word, b"\x00\x01"],
            [data[k:k + 1 + k % 23] for k in range(300, 300 + 16 * 97, 97)],  # 16 patterns, K = 1
            big]


def test_reader_find_set(kolm_gpu, containers):
    kolm = kolm_gpu
    for name, blob, data in containers:
        with kolm.open_container(blob) as rd:
            for pats in pattern_sets(data):
                pats = list(dict.fromkeys(pats))
                want = ref(data, pats)
                with kolm.PatternSet(pats) as ps:
                    assert len(ps) == len(pats) and ps.patterns == tuple(pats) and ps.info["np"] == len(pats)
                    assert rd.find_set(ps) == want, (name, len(pats))
                    st = kolm.last_find()
                    assert st["matches"] == len(want) == st["returned"] and st["patterns"] == len(pats)
                    assert st["blocks_decoded"] == len([b for b in rd.blocks if b[1]])
                    assert rd.count_set(ps) == counts_of(want, len(pats))
                    assert kolm.last_find()["emit_launches"] == 0 and kolm.last_find()["matches"] == len(want)
                    lo, hi = 1003, len(data) - 777   # a window that starts and ends inside blocks
                    assert rd.find_set(ps, lo, hi) == ref(data, pats, lo, hi)
                if len(pats) <= 16:   # a cross-check with the 16-pattern route, not the oracle
                    assert rd.find_many(pats) == want and rd.count_many(pats) == counts_of(want, len(pats))
                assert rd.find_set(pats, 10, 5000, limit=9) == ref(data, pats, 10, 5000)[:9]   # a plain sequence
                assert rd.count_set(pats, 10, 5000) == counts_of(ref(data, pats, 10, 5000), len(pats))


def test_group_and_stage_independence(kolm_gpu, containers, monkeypatch):
    """KOLM_READ_BYTES so small that matches of up to 256 bytes straddle many groups, and
    KOLM_FIND_STAGE=1: the same pairs."""
    kolm = kolm_gpu
    rng = np.random.default_rng(4)
    pat = rng.integers(0, 256, 256, dtype=np.uint8).tobytes()
    d = bytearray(containers[0][2][:3000])
    for o in (150, 777, 1999, 3000 - 256):  # each spans five or six 52-byte blocks
        d[o:o + 256] = pat
    data = bytes(d)
    blob = kolm.compress_blocks_fixed(data, 52, hot_path=True)
    pats = [pat, pat[:9], data[40:43], pat[:200], b"e", pat[5:14]]
    want = ref(data, pats)
    assert [o for o, i in want if i == 0] == [150, 777, 1999, 3000 - 256]
    with kolm.PatternSet(pats) as ps:
        for env in ({}, {"KOLM_READ_BYTES": "52"}, {"KOLM_READ_BYTES": "1"}, {"KOLM_FIND_STAGE": "1"},
                    {"KOLM_READ_BYTES": "130", "KOLM_FIND_STAGE": "1"}):
            monkeypatch.delenv("KOLM_READ_BYTES", raising=False)
            monkeypatch.delenv("KOLM_FIND_STAGE", raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            with kolm.open_container(blob) as rd:
                assert rd.find_set(ps) == want, env
                st = kolm.last_find()
                assert st["groups"] == (1 if "KOLM_READ_BYTES" not in env else 29 if env["KOLM_READ_BYTES"] == "130" else 58)
                assert rd.count_set(ps) == counts_of(want, len(pats))
                assert rd.find_set(ps, 433, 2101) == ref(data, pats, 433, 2101)
                assert rd.find_set(ps, 151, 2999, limit=5) == ref(data, pats, 151, 2999)[:5]
                assert rd.find_many(pats) == want
    _, blob, data = containers[1]
    pats = list(dict.fromkeys(pattern_sets(data)[5]))
    want = ref(data, pats)
    monkeypatch.delenv("KOLM_READ_BYTES", raising=False)
    monkeypatch.setenv("KOLM_FIND_STAGE", "1")
    with kolm.open_container(blob) as rd:
        for k in (0, 1, len(want) - 1, len(want), len(want) + 1):
            assert rd.find_set(pats, limit=k) == want[:k]
            st = kolm.last_find()
            assert st["matches"] == len(want) and st["returned"] == min(k, len(want))
    monkeypatch.setenv("KOLM_READ_BYTES", "4096")
    with kolm.open_container(blob) as rd:
        assert rd.find_set(pats) == want and kolm.last_find()["groups"] == kolm.last_find()["blocks_decoded"]


def test_large_set_one_decode(kolm_gpu):
    """65 536 patterns of five lengths over 65 x 4096 + 7 bytes of four-letter noise in 64 KiB
    blocks: exactly the reference's pairs from one decode of each touched block."""
    kolm = kolm_gpu
    rng = np.random.default_rng(65536)
    n = 65 * TILE + 7
    d = rng.integers(97, 101, n, dtype=np.uint8).tobytes()
    lens = (8, 9, 10, 12, 14)
    seen, pats = set(), []
    while len(pats) < 65536:
        ln = lens[len(pats) % 5]
        if len(pats) % 2:
            p = rng.integers(97, 101, ln, dtype=np.uint8).tobytes()
        else:
            o = int(rng.integers(0, n - ln))
            p = d[o:o + ln]
        if p not in seen:
            seen.add(p)
            pats.append(p)
    want = ref_dict(d, pats)
    assert len(want) > 30000
    blob = kolm.compress_blocks_fixed(d, 65536, hot_path=True)
    with kolm.open_container(blob) as rd, kolm.PatternSet(pats) as ps:
        assert ps.info["np"] == 65536 and ps.info["key_bytes"] == 8 and ps.info["filter_bits"] == 1 << 18
        assert ps.info["slots"] >= 2 * ps.info["keys"] and ps.info["longest"] == 14
        rd.count(b"x")
        one = kolm.last_find()
        assert rd.find_set(ps) == want
        st = kolm.last_find()
        assert st["patterns"] == 65536 and st["matches"] == len(want)
        # one decode for the whole set
        assert (st["blocks_decoded"], st["groups"], st["bytes_decoded"]) == \
            (one["blocks_decoded"], one["groups"], one["bytes_decoded"]) == (5, one["groups"], n)
        assert rd.count_set(ps) == counts_of(want, 65536) and kolm.last_find()["emit_launches"] == 0
        lo, hi = 70_001, 200_003
        assert rd.find_set(ps, lo, hi, limit=1000) == ref_dict(d, pats, lo, hi)[:1000]
        rd.count(b"x", lo, hi)
        one = kolm.last_find()
        rd.find_set(ps, lo, hi, limit=1000)
        st = kolm.last_find()
        assert (st["blocks_decoded"], st["groups"], st["bytes_decoded"]) == \
            (one["blocks_decoded"], one["groups"], one["bytes_decoded"])


# ------------------------------------------------------------------ 3. checksums, host fallback, arguments

def test_checksums(kolm_gpu, containers):
    from kolm.checksums import Checksums, KolmChecksumError
    kolm = kolm_gpu
    _, blob, data = containers[1]
    cs = kolm.checksums_of(blob)
    crcs = list(cs.crcs)
    crcs[3] ^= 0x00010000
    bad = Checksums(cs.mode, cs.size_field, cs.total_len, cs.lens, crcs)
    pats = [data[1000:1004], b"e", data[5000:5009]]
    with kolm.PatternSet(pats) as ps:
        with kolm.open_container(blob, checksums=cs) as rd:
            assert rd.find_set(ps) == ref(data, pats)
        with kolm.open_container(blob, checksums=bad) as rd:
            assert rd.find_set(ps, 0, 3 * 4096) == ref(data, pats, 0, 3 * 4096)
            before = kolm.last_find()
            for lo, hi in ((0, len(data)), (3 * 4096, 4 * 4096), (4 * 4096 - 1, 5 * 4096)):
                with pytest.raises(KolmChecksumError) as ei:
                    rd.find_set(ps, lo, hi)
                assert ei.value.block == 3 and ei.value.expected == crcs[3] and ei.value.got == cs.crcs[3]
                with pytest.raises(KolmChecksumError):
                    rd.count_set(ps, lo, hi)
            assert kolm.last_find() == before
            assert rd.find_set(ps, 4 * 4096) == ref(data, pats, 4 * 4096)


def test_host_fallback_gives_the_same(kolm_gpu, lib, containers, monkeypatch):
    kolm = kolm_gpu
    _, blob, data = containers[2]
    pats = [data[50:53], data[9000:9009], b"e", data[50:58]]
    with kolm.open_container(blob) as rd:
        dev = rd.find_set(pats), rd.find_set(pats, 10, len(data) - 10, limit=5), rd.count_set(pats)
        assert "host" not in kolm.last_find()
    mids = {m for _, n, m in kolm.open_container(blob).blocks if n}
    monkeypatch.setattr(lib, "KOLM_DECODE_MASK", lib.KOLM_DECODE_MASK & ~(1 << max(mids)))
    with kolm.open_container(blob) as rd:
        assert rd._host_blocks
        host = rd.find_set(pats), rd.find_set(pats, 10, len(data) - 10, limit=5), rd.count_set(pats)
        assert kolm.last_find().get("host") is True and kolm.last_find()["patterns"] == 4
    assert dev == host and dev[0] == ref(data, pats) and dev[1] == ref(data, pats, 10, len(data) - 10)[:5]


def test_argument_errors(kolm_gpu, lib, containers):
    kolm = kolm_gpu
    _, blob, data = containers[1]
    rd = kolm.open_container(blob)
    assert rd.find_set([data[:4]], limit=1) == [(0, 0)]
    before = kolm.last_find()
    for bad, text in (([], "0 patterns"), ([b"a"] * 65537, "65537 patterns"), ([b"ok", b""], "pattern 1 is empty"),
                      ([b"x" * 257], "pattern 0 has 257 bytes"), ([b"ab", b"c", b"ab"], "patterns 0 and 2 are equal")):
        with pytest.raises(ValueError, match=text):
            kolm.PatternSet(bad)
        with pytest.raises(ValueError, match=text):
            rd.find_set(bad)
        with pytest.raises(ValueError, match=text):
            rd.count_set(bad)
    # the library's own checks, behind the binding's: the message names the patterns
    for bad, text in (([], "0 patterns"), ([b"ok", b""], "pattern 1 is empty"), ([b"x" * 257], "pattern 0 has 257 bytes"),
                      ([b"ab", b"c", b"ab"], "patterns 0 and 2 are equal"),
                      ([b"12345678x", b"q2345678", b"12345678y", b"12345678x"], "patterns 0 and 3 are equal")):
        with pytest.raises(ValueError, match=text):
            lib.patset_create(bad)
    with pytest.raises(TypeError):
        kolm.PatternSet(b"abc")
    ps = kolm.PatternSet([b"a", b"the"])
    for args in ((-1,), (0, -1)):
        with pytest.raises(ValueError):
            rd.find_set(ps, *args)
    with pytest.raises(ValueError):
        rd.find_set(ps, limit=-1)
    for lo, hi in ((5, 4), (0, len(data) + 1)):   # a window outside the data, behind the binding's clipping
        with pytest.raises(ValueError, match="window"):
            lib.reader_find_set(rd._h, ps._h, 2, lo, hi)
    # a set of another context than the reader's
    other = kolm.PatternSet([b"a"], ctx=lib.device_ctx(lib.ensure_init()))
    with pytest.raises(ValueError, match="context"):
        rd.find_set(other)
    other.close()
    assert kolm.last_find() == before
    # a plain sequence becomes a set of the reader's own context
    with kolm.open_container(blob, lib.device_ctx(lib.ensure_init())) as r4:
        assert r4.find_set([data[:4]], limit=1) == [(0, 0)] and r4.count_set([b"\xff\xfe"]) == [0]
    rd.find_set([data[:4]], limit=1)
    before = kolm.last_find()
    # a closed set, a closed reader
    assert rd.count_set(ps) == [data.count(b"a"), len(ref(data, [b"the"]))]
    ps.close()
    ps.close()
    with pytest.raises(ValueError, match="closed pattern set"):
        rd.find_set(ps)
    with pytest.raises(ValueError, match="closed pattern set"):
        rd.count_set(ps)
    rd.close()
    with kolm.PatternSet([b"a"]) as ps2:
        with pytest.raises(ValueError, match="closed"):
            rd.find_set(ps2)
        with pytest.raises(ValueError, match="closed"):
            rd.count_set(ps2)
        # a selected block the device does not decode: block and method named, before any launch
        odd = kolm.write_container(kolm.MODE_FIXED, 8, 16, [0, 11], [8, 8], [b"abcdefgh", b"12345678"])
        with kolm.open_container(odd) as r2, kolm.PatternSet([b"cd", b"h"]) as p2:
            assert r2.find_set(p2, 0, 8) == [(2, 0), (7, 1)]
            with pytest.raises(ValueError, match=r"block 1 \(method 11"):
                lib.reader_find_set(r2._h, p2._h, 2, 0, 16)
        assert kolm.last_find()["bytes_scanned"] == 8
    # the 16-pattern route keeps its limit
    with kolm.open_container(blob) as r3:
        with pytest.raises(ValueError):
            r3.find_many([b"a"] * 17)
