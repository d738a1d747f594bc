"""Regular expressions on the device: kolm_find_dfa_device, Reader.find_regex / count_regex,
kolm.find_regex and grep with Regex objects.

Expected results never come from the code under test: `ref` below is the rule of include/kolm.h
on the CPU, Python's re asked at every offset,
    re.compile(b"(?:" + expr + b")", re.DOTALL [| re.IGNORECASE]).match(data, o, min(hi, o + 256)) is not None,
and for the 8 MiB case a lookahead re.finditer over an expression whose matches are at most 6
bytes long (where the two agree: every start with a match inside the window)."""
import json
import os
import re

import numpy as np
import pytest

from kolm import datagen as D

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TILE = 4096


def ref(data, exprs, lo=0, hi=None, flags=0):
    """Every (offset, expression index) of the window [lo, hi), sorted."""
    hi = len(data) if hi is None else min(hi, len(data))
    out = []
    for i, e in enumerate(exprs):
        m = re.compile(b"(?:" + e + b")", re.DOTALL | flags).match
        out += [(o, i) for o in range(lo, hi) if m(data, o, min(hi, o + 256)) is not None]
    return sorted(out)


def counts_of(want, np_):
    return [sum(1 for _, i in want if i == j) for j in range(np_)]


@pytest.fixture(scope="module")
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


NAMED = [rb"ERROR|WARN(ING)?", rb"https?://[^ ]+", rb"\d{1,3}(\.\d{1,3}){3}", rb"[a-z0-9._]+@[a-z]+\.(com|org)"]
SIXTEEN = NAMED + [rb"[A-Z][a-z]+ [A-Z][a-z]+", rb"ab*c", rb"\n", rb"t(he|o) ", rb"(?:in|on|at)\s\w+", rb"\d+", rb"[.,;]+ ?\n?[A-Z]",
                   rb"e{2,}|o{2,}", rb"ERROR|WARN(ING)?", rb"q?u", rb"\w+ing", rb"[^a-z ]{3,}?"]


@pytest.fixture(scope="module")
def text():
    """Text with log words, URLs, addresses and mail names planted, some across the 4096-byte block
    boundaries, and runs a b* c of 256 and 257 bytes; a WARNING ends the data."""
    d = bytearray(D.enwik_like(60_000, seed=41))
    plants = [b"ERROR", b"WARNING", b"WARN ", b"http://a.example/x?y=1 ", b"https://kolm.org ", b"10.0.12.255", b"1.22.333.4444",
              b"joe.r_1@mail.com", b"x@y.org", b"Hello World", b"a@b.net"]
    spots = list(range(700, 58_000, 1531)) + [4096 * 3 - 4, 4096 * 7 - 2, 4096 * 11 - 1, 8192 - 7]
    for k, o in enumerate(spots):
        p = plants[k % len(plants)]
        d[o:o + len(p)] = p
    d[20_000:20_256] = b"a" + b"b" * 254 + b"c"   # a witness of exactly 256 bytes
    d[30_000:30_257] = b"a" + b"b" * 255 + b"c"   # 257: no match at 30 000
    d[-7:] = b"WARNING"
    return bytes(d)


def raw_container(kolm, data, bs):
    """Blocks of bs bytes stored as they are (method 0) under a TOC written here."""
    blocks = [data[o:o + bs] for o in range(0, len(data), bs)]
    return kolm.write_container(kolm.MODE_FIXED, bs, len(data), [0] * len(blocks), [len(b) for b in blocks], blocks)


@pytest.fixture(scope="module")
def containers(kolm_gpu, text):
    """[(name, container, data)]: blocks of 1, 7, 255, 256 and 4096 bytes, and one CDC container."""
    kolm = kolm_gpu
    part = text[19_800:19_800 + 700]  # holds the 256-byte run
    return [("raw1", raw_container(kolm, part, 1), part),
            ("raw7", raw_container(kolm, text[19_000:19_000 + 7 * 400], 7), text[19_000:19_000 + 7 * 400]),
            ("raw255", raw_container(kolm, text[:255 * 130], 255), text[:255 * 130]),
            ("raw256", raw_container(kolm, text[:256 * 130], 256), text[:256 * 130]),
            ("fixed4096", kolm.compress_blocks_fixed(text, 4096, hot_path=True), text),
            ("cdc", kolm.compress_blocks_cdc(text, hot_path=True), text)]


ENVS = ({}, {"KOLM_READ_BYTES": "8192"}, {"KOLM_FIND_STAGE": "1"}, {"KOLM_READ_BYTES": "8192", "KOLM_FIND_STAGE": "4096"})


def set_env(monkeypatch, env):
    monkeypatch.delenv("KOLM_READ_BYTES", raising=False)
    monkeypatch.delenv("KOLM_FIND_STAGE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------ 1. kolm_find_dfa_device

def test_find_dfa_device_every_data_offset(kolm_gpu, lib, text):
    """The same buffer at every misalignment 0..15, lengths around the tile size: against re."""
    from kolm import regex
    exprs = NAMED + [rb"ab*c", rb"[A-Z][a-z]+ [A-Z][a-z]+", rb"\n"]
    table = regex.table([regex.compile(e) for e in exprs])
    cases = {n: (text[19_900:19_900 + n], None) for n in (0, 1, 15, 17, 4095, 4097)}
    cases[8193] = (text[4096 * 3 - 100:4096 * 3 - 100 + 8193], None)
    for n, (data, _) in cases.items():
        cases[n] = (data, ref(data, exprs))
    assert len(cases[8193][1]) > 50 and (100, 4) in cases[4095][1]  # the 256-byte run
    for mis in range(16):
        for n, (data, want) in cases.items():
            offs, which, counts, _ = lib.find_dfa_bytes(data, table, data_offset=mis)
            assert list(zip(offs, which)) == want, (mis, n)
            assert counts == counts_of(want, len(exprs))
    data, want = cases[8193]
    for limit in (0, 1, 7, len(want) - 1, len(want), len(want) + 1):
        offs, which, counts, _ = lib.find_dfa_bytes(data, table, limit=limit, data_offset=3)
        assert list(zip(offs, which)) == want[:limit] and counts == counts_of(want, len(exprs))


def test_eight_mib_two_thousand_tiles(kolm_gpu, lib):
    """8 MiB, 2 048 tiles, a frequent expression of bounded length: every tile's count and every
    record's slot, against a lookahead finditer."""
    from kolm import regex
    rng = np.random.default_rng(7)
    base = np.frombuffer(D.enwik_like(1 << 18, seed=5), np.uint8)
    d = np.tile(base, 32)
    at = rng.integers(0, d.size, 200_000)
    d[at] = rng.integers(97, 123, at.size, dtype=np.uint8)  # no two copies alike
    data = d.tobytes()
    assert len(data) == 2048 * TILE
    e = rb"[aeiou][a-z]{1,3}[ ,.]\n?"
    want = np.fromiter((m.start() for m in re.finditer(b"(?=(" + e + b"))", data, re.DOTALL)), np.int64)
    assert want.size > 300_000
    table = regex.compile(e).table
    offs, which, counts, _ = lib.find_dfa_bytes(data, table, data_offset=5)
    assert counts == [want.size] and np.array_equal(np.asarray(offs, np.int64), want) and not any(which)
    offs, _, counts, _ = lib.find_dfa_bytes(data, table, limit=1000)
    assert counts == [want.size] and offs == want[:1000].tolist()


# ------------------------------------------------------------------ 2. readers over containers made here

def test_reader_find_regex(kolm_gpu, containers, monkeypatch):
    """Blocks of 1, 7, 255, 256, 4096 bytes and CDC blocks, each also in groups of 8 KiB and with a
    small staging buffer: the named expressions, 16 at once (two identical), counts and limits."""
    kolm = kolm_gpu
    for name, blob, data in containers:
        wants = [(exprs, ref(data, exprs)) for exprs in (NAMED[:1], NAMED, SIXTEEN)]
        for env in ENVS:
            set_env(monkeypatch, env)
            with kolm.open_container(blob) as rd:
                for exprs, want in wants:
                    assert rd.find_regex(exprs) == want, (name, env, exprs[-1])
                    st = kolm.last_find()
                    assert st["matches"] == len(want) == st["returned"] and st["patterns"] == len(exprs)
                    assert "host" not in st and st["blocks_decoded"] == len([b for b in rd.blocks if b[1]])
                    assert rd.count_regex(exprs) == counts_of(want, len(exprs))
                    assert kolm.last_find()["emit_launches"] == 0
                exprs, want = wants[2]
                for k in (0, 1, len(want) - 1, len(want) + 1):
                    assert rd.find_regex(exprs, limit=k) == want[:k]
                    assert kolm.last_find()["matches"] == len(want) and kolm.last_find()["returned"] == min(k, len(want))
                lo, hi = len(data) // 5, len(data) - 3
                assert rd.find_regex(NAMED, lo, hi) == ref(data, NAMED, lo, hi)
                if env.get("KOLM_READ_BYTES") and len(data) > 20_000:
                    assert kolm.last_find()["groups"] > 1
        c = counts_of(wants[2][1], 16)
        assert c[0] == c[12] and (name in ("raw1", "raw7") or min(c[:5]) > 0)
    data = containers[4][2]
    want = ref(data, SIXTEEN)
    assert (len(data) - 7, 0) in want and (20_000, 5) in want and (30_000, 5) not in want and (30_001, 5) not in want
    assert (4096 * 3 - 4, 0) in want or (4096 * 3 - 4, 1) in want or (4096 * 3 - 4, 2) in want or (4096 * 3 - 4, 3) in want


def test_match_spans_many_blocks(kolm_gpu, containers, monkeypatch):
    """The 256-byte witness lies in 256 blocks of one byte, 37 of seven and two or three of 255; a
    window that ends one byte short of it, or begins one byte late, loses the match."""
    kolm = kolm_gpu
    for name, o in (("raw1", 200), ("raw7", 1000), ("raw255", 20_000), ("raw256", 20_000), ("cdc", 20_000)):
        blob, data = next((b, d) for n, b, d in containers if n == name)
        assert data[o:o + 256] == b"a" + b"b" * 254 + b"c"
        for env in ENVS[:2] + ({"KOLM_READ_BYTES": "1"},):
            set_env(monkeypatch, env)
            with kolm.open_container(blob) as rd:
                f = lambda *a: [x for x, _ in rd.find_regex(rb"ab*c", *a)]  # noqa: E731
                assert o in f() and f(o, o + 256) == [o] and f(o, o + 255) == [] and f(o + 1, o + 256) == []
                assert f(o - 3, o + 400) == [x for x, _ in ref(data, [rb"ab*c"], o - 3, o + 400)]
                assert rd.count_regex([rb"ab*c", rb"b{250}"], o, o + 256) == [1, 5]


def test_ignore_case_and_the_public_function(kolm_gpu, containers):
    kolm = kolm_gpu
    _, blob, data = containers[4]
    exprs = [rb"error|warn(ing)?", rb"[a-z]+ world", rb"HTTPS?://[^ ]+"]
    want = ref(data, exprs, flags=re.IGNORECASE)
    assert len(want) > len(ref(data, exprs)) + 10
    with kolm.open_container(blob) as rd:
        assert rd.find_regex(exprs, ignore_case=True) == want
        assert rd.count_regex(exprs, ignore_case=True) == counts_of(want, 3)
        assert rd.find_regex([kolm.regex.compile(e, True) for e in exprs]) == want
        assert rd.find_regex(kolm.regex.compile(exprs[0]), ignore_case=True) == [(o, 0) for o, i in want if i == 0]
    assert kolm.find_regex(blob, exprs[0], 100, 50_000, ignore_case=True) == \
        [o for o, _ in ref(data, exprs[:1], 100, 50_000, re.IGNORECASE)]
    assert kolm.find_regex(blob, NAMED[0], limit=4) == [o for o, _ in ref(data, NAMED[:1])][:4]


# ------------------------------------------------------------------ 3. the three kinds of pattern agree

def test_literals_and_class_patterns_as_regex(kolm_gpu, containers):
    """A literal as Regex gives what find gives, a class pattern as Regex what find_classes gives."""
    kolm = kolm_gpu
    Regex = kolm.Regex
    for name, blob, data in containers[2:]:
        lits = [b"the", b"WARN", data[1000:1009], b"e", b"\n"]
        cps = [kolm.classes.compile(e) for e in (rb"\d\.\d", rb"[Tt]h[ae]", rb"ERROR", rb".\n.", rb"\w\W\w")]
        with kolm.open_container(blob) as rd:
            assert rd.find_regex([Regex.literal(p) for p in lits]) == rd.find_many(lits)
            assert rd.find_regex([Regex.literal(p, True) for p in lits]) == rd.find_many(lits, ignore_case=True)
            assert rd.find_regex(cps) == rd.find_classes(cps) == rd.find_regex([Regex.of_classes(p) for p in cps])
            assert len(rd.find_many(lits)) > 100 and len(rd.find_classes(cps)) > 100
            assert [o for o, _ in rd.find_regex(Regex.literal(b"the"), 50, 9000, 5)] == rd.find(b"the", 50, 9000, 5)


# ------------------------------------------------------------------ 4. grep

def test_grep_with_regex(kolm_gpu, text):
    kolm = kolm_gpu
    data = text
    blob = kolm.compress_blocks_fixed(data, 4096, hot_path=True)
    lines = data.split(b"\n")
    starts = np.concatenate([[0], np.cumsum([len(ln) + 1 for ln in lines])[:-1]]).tolist()

    def host(exprs, flags=0, lo=0, hi=None):
        """The lines that hold the first byte of a match, from data.split."""
        own = sorted({int(np.searchsorted(starts, o, side="right")) - 1 for o, _ in ref(data, exprs, lo, hi, flags)})
        return [(k, lines[k]) for k in own]

    with kolm.open_container(blob, lines=True) as rd:
        rx = kolm.regex.compile(NAMED[0])
        assert rd.grep(rx) == host(NAMED[:1]) and len(rd.grep(rx)) >= 8
        assert rd.grep([rx, kolm.regex.compile(NAMED[1])], limit=5) == host(NAMED[:2])[:5]
        assert rd.grep(rx, 3000, 40_000) == host(NAMED[:1], 0, 3000, 40_000)
        assert rd.grep(rx, ignore_case=True) == host(NAMED[:1], re.IGNORECASE)
        # literals and class patterns next to a Regex are converted
        mixed = [rx, b"Hello", kolm.classes.compile(rb"\d\d\.\d")]
        assert rd.grep(mixed) == host([NAMED[0], rb"Hello", rb"\d\d\.\d"])
        assert rd.grep(b"WARN") == host([b"WARN"])  # the literal path is what it was
        with kolm.PatternSet([b"abc", b"abd"]) as ps:
            with pytest.raises(ValueError):
                rd.grep([rx, ps])
        with pytest.raises(ValueError):
            rd.grep([rx] * 17)


# ------------------------------------------------------------------ 5. checksums, host fallback

def test_flipped_payload_byte_raises(kolm_gpu, containers):
    """Under checksums a flipped payload byte raises KolmChecksumError and no result leaves the call."""
    from kolm.checksums import KolmChecksumError
    kolm = kolm_gpu
    _, blob, data = containers[3]  # raw blocks of 256 bytes: a block's payload is its bytes
    cs = kolm.checksums_of(blob)
    at = blob.index(data[5 * 256:6 * 256])
    assert blob.count(data[5 * 256:6 * 256]) == 1
    bad = bytearray(blob)
    bad[at + 17] ^= 0x20
    e = [rb"[Tt]h[ae]", rb"\w+ing"]
    with kolm.open_container(blob, checksums=cs) as rd:
        assert rd.find_regex(e) == ref(data, e)
    with kolm.open_container(bytes(bad), checksums=cs) as rd:
        assert rd.find_regex(e, 0, 5 * 256) == ref(data, e, 0, 5 * 256)
        before = kolm.last_find()
        for lo, hi in ((0, len(data)), (5 * 256, 6 * 256), (6 * 256 - 1, 7 * 256)):
            with pytest.raises(KolmChecksumError) as ei:
                rd.find_regex(e, lo, hi)
            assert ei.value.block == 5 and ei.value.expected == cs.crcs[5]
            with pytest.raises(KolmChecksumError):
                rd.count_regex(e, lo, hi)
        assert kolm.last_find() == before
        assert rd.find_regex(e, 6 * 256) == ref(data, e, 6 * 256)


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
    exprs = [re.escape(data[50:52]) + rb".?", rb".[^\x00]+?" + re.escape(mid[2:]), rb"[\x00-\x40]{2,4}|" + re.escape(mid[:3])]

    def run(rd):
        return (rd.find_regex(exprs), rd.find_regex(exprs, 10, len(data) - 10, limit=5), rd.count_regex(exprs),
                rd.find_regex(exprs[:1], ignore_case=True))

    with kolm.open_container(blob) as rd:
        dev = run(rd)
        assert "host" not in kolm.last_find()
    monkeypatch.setattr(lib, "KOLM_DECODE_MASK", lib.KOLM_DECODE_MASK & ~(1 << 10))
    with kolm.open_container(blob) as rd:
        assert rd._host_blocks
        host = run(rd)
        assert kolm.last_find().get("host") is True
    assert dev == host and dev[0] == ref(data, exprs) and dev[1] == ref(data, exprs, 10, len(data) - 10)[:5]
    assert dev[3] == ref(data, exprs[:1], flags=re.IGNORECASE) and min(dev[2]) >= 1


# ------------------------------------------------------------------ 6. argument errors

class FakeTable:
    def __init__(self, t, **kw):
        self.cls_map, self.T, self.starts = t.cls_map, t.T.copy(), list(t.starts)
        self.__dict__.update(kw)


def test_argument_errors(kolm_gpu, lib, containers):
    kolm = kolm_gpu
    _, blob, data = containers[4]
    rd = kolm.open_container(blob)
    assert rd.find_regex(re.escape(data[:4]) + rb"+", limit=1) == [(0, 0)]
    before = kolm.last_find()
    for bad in ([rb"a"] * 17, [], rb"a*", rb"^a", [rb"ok", rb"(b"], rb"(a|b)*a(a|b){20}"):
        with pytest.raises(ValueError):
            rd.find_regex(bad)
        with pytest.raises(ValueError):
            rd.count_regex(bad)
    for args in ((rb"\d", -1), (rb"\d", 0, -1)):
        with pytest.raises(ValueError):
            rd.find_regex(*args)
    with pytest.raises(ValueError):
        rd.find_regex(rb"\d", limit=-1)
    # the library's own checks, behind the binding's: before any launch, the message names the fault
    t = kolm.regex.table([kolm.regex.compile(rb"ab+c"), kolm.regex.compile(rb"\d\d")])
    T_big, T_row, T_entry = t.T.copy(), t.T.copy(), t.T.copy()
    T_row[1, 0] = 2
    T_entry[2, 1] = t.nstates
    cls_bad = bytearray(t.cls_map)
    cls_bad[65] = t.ncls
    for fake, msg in ((FakeTable(t, starts=[2] * 17), "17 expressions"), (FakeTable(t, starts=[]), "0 expressions"),
                      (FakeTable(t, starts=[2, 1]), "expression 1 starts in state 1"),
                      (FakeTable(t, starts=[t.nstates, 2]), "expression 0 starts"),
                      (FakeTable(t, T=T_row), "rows 0 and 1 are zero"), (FakeTable(t, T=T_entry), "entry 1 of state 2"),
                      (FakeTable(t, cls_map=bytes(cls_bad)), "byte 65 has class"),
                      (FakeTable(t, T=np.zeros((lib.KOLM_RX_MAX_ENTRIES // 2 + 1, 2), np.uint16)), "at most 16384 entries")):
        with pytest.raises(ValueError, match=msg):
            lib.reader_find_dfa(rd._h, fake, 0, 10)
        with pytest.raises(ValueError, match=msg):
            lib.find_dfa_bytes(b"some bytes", fake)
    for lo, hi in ((5, 4), (0, len(data) + 1)):
        with pytest.raises(ValueError, match="window"):
            lib.reader_find_dfa(rd._h, t, lo, hi)
    assert kolm.last_find() == before
    rd.close()
    with pytest.raises(ValueError, match="closed"):
        rd.find_regex(rb"\d")
    # a selected block the device does not decode: block and method named, before any launch
    odd = kolm.write_container(kolm.MODE_FIXED, 8, 16, [0, 11], [8, 8], [b"abcdefgh", b"12345678"])
    with kolm.open_container(odd) as r2:
        assert r2.find_regex(rb"[cC].+?f", 0, 8) == [(2, 0)]
        with pytest.raises(ValueError, match=r"block 1 \(method 11"):
            lib.reader_find_dfa(r2._h, t, 0, 16)
    assert kolm.last_find()["bytes_scanned"] == 8
