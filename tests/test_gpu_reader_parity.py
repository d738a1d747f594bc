"""Every reader entry point decodes through one path (kolmogorovlike-datacompressor_amd/csrc/
kolm_reader.cpp: reader_check_blocks, reader_decode_group): read, find, find_set and the line
calls return the same bytes' answers and fail the same way -- same code, same text -- for a block
the device does not decode, a payload its decoder rejects and a decoded block whose CRC-32 is
wrong.  One container of 8 blocks of 4 KiB with five method ids; KOLM_READ_BYTES=8192 makes
several groups, and the blocks {0, 2, 3, 6} of the read and line queries give every group two
payload runs (a compaction).  Expected values come from the original bytes with plain Python."""
import bisect
import ctypes
import zlib

import numpy as np
import pytest

import decode_cases as DC

pytestmark = pytest.mark.gpu

BS = 4096
NB = 8
FORCE = [7, 0, 2, 1, 7, 8, 4, 0]  # the blocks' method ids
SEL = (0, 2, 3, 6)                # the blocks of the read and line queries
BAD = 3                           # the block the failing cases tamper with: second group of every plan below
REJECTED = "xor_short/too_few_values"  # a corpus payload of BAD's method that the decoders reject


def make_data():
    rng = np.random.default_rng(18)
    text = b"".join(b"row %d: the quick brown fox jumps\n" % i for i in range(700))
    assert len(text) >= 4 * BS
    noise = [bytes(rng.integers(0, 256, BS, dtype=np.uint8)) for _ in range(2)]
    rep = (b"abcabcabd" * 500)[:BS]
    ramp = bytes((i * 7) & 0xFF for i in range(BS))
    blocks = [text[:BS], noise[0], text[BS:2 * BS], text[2 * BS:3 * BS], rep, ramp, text[3 * BS:4 * BS], noise[1]]
    return b"".join(blocks)


class Ref:
    """Lines of the original bytes: delimiter positions, spans, line_of by bisect."""

    def __init__(self, data):
        self.pos = [i for i, v in enumerate(data) if v == 0x0A]
        self.counts = [data[b * BS:(b + 1) * BS].count(b"\n") for b in range(NB)]
        n = len(self.pos)
        self.spans = [((self.pos[k - 1] + 1) if k else 0, self.pos[k] if k < n else len(data)) for k in range(n + 1)]

    def line_of(self, o):
        return bisect.bisect_left(self.pos, o)


def find_all(data, pats):
    out = []
    for i, p in enumerate(pats):
        o = data.find(p)
        while o >= 0:
            out.append((o, i))
            o = data.find(p, o + 1)
    return sorted(out)


@pytest.fixture(scope="module")
def lib(kolm_gpu):
    from kolm import _lib
    return _lib


@pytest.fixture(scope="module")
def ctx(lib):
    return lib.device_ctx(lib.ensure_init())


@pytest.fixture(scope="module")
def made(kolm_gpu, lib, ctx):
    """The container, made and opened once (checksums and a line index attached)."""
    kolm = kolm_gpu
    data = make_data()
    _, method, payloads, _ = lib.encode_blocks(data, BS, cand_mask=lib.KOLM_HOTPATH_MASK, force=FORCE)
    mids = [int(m) for m in method]
    assert mids == FORCE and len(set(mids)) >= 3
    blob = kolm.write_container(kolm.MODE_FIXED, BS, len(data), mids, [BS] * NB, payloads)
    assert kolm.decompress(blob, device=False) == data
    cs = kolm.checksums_of(blob)
    assert cs.crcs == [zlib.crc32(data[b * BS:(b + 1) * BS]) for b in range(NB)]
    ref = Ref(data)
    # the lines the line queries ask for: one inside block 0, the one that starts in block 2 and ends
    # in block 3, one inside block 6 -- their delimiters lie in SEL's blocks and in no other
    k23 = ref.line_of(3 * BS)
    assert 2 * BS <= ref.spans[k23][0] < 3 * BS < ref.spans[k23][1] < 4 * BS
    k6 = ref.line_of(6 * BS + 2000)
    assert 6 * BS <= ref.pos[k6 - 1] and ref.pos[k6] < 7 * BS and ref.pos[1] < BS
    lines = [1, k23, k6]
    # the patterns: one across a block seam inside a group, one across a group seam
    pats = [data[BS - 3:BS + 3], data[2 * BS - 3:2 * BS + 3], b"fox jumps\nrow"]
    rd = kolm.open_container(blob, ctx, checksums=cs, lines=True)
    try:
        yield {"data": data, "blob": blob, "mids": mids, "payloads": payloads, "cs": cs, "ref": ref, "lines": lines,
               "pats": pats, "rd": rd}
    finally:
        rd.close()


def block_ranges(lens, blocks):
    starts = np.concatenate([[0], np.cumsum(lens)])
    return [(int(starts[b]), int(lens[b])) for b in blocks]


# ------------------------------------------------------------------ 1. same bytes

@pytest.mark.parametrize("limit", ("8192", None))
def test_same_bytes(kolm_gpu, ctx, made, monkeypatch, limit):
    kolm, rd, data, ref = kolm_gpu, made["rd"], made["data"], made["ref"]
    monkeypatch.delenv("KOLM_READ_BYTES", raising=False)
    if limit:
        monkeypatch.setenv("KOLM_READ_BYTES", limit)
    groups = {"sel": 2 if limit else 1, "all": 4 if limit else 1}
    assert rd.line_index.counts == ref.counts
    # read
    ranges = block_ranges([BS] * NB, SEL)
    assert rd.read_many(ranges) == [data[o:o + n] for o, n in ranges]
    st = kolm.last_read()
    assert (st["blocks_decoded"], st["groups"], st["compactions"]) == (4, groups["sel"], groups["sel"])
    # find, find_set: the whole window
    pats = made["pats"]
    want = find_all(data, pats)
    assert (BS - 3, 0) in want and (2 * BS - 3, 1) in want
    assert rd.find_many(pats) == want
    st = kolm.last_find()
    assert (st["blocks_decoded"], st["groups"], st["matches"]) == (NB, groups["all"], len(want))
    with kolm.PatternSet(pats, ctx) as ps:
        assert rd.find_set(ps) == want
        assert rd.count_set(ps) == [sum(1 for _, i in want if i == k) for k in range(len(pats))]
    assert kolm.last_find()["groups"] == groups["all"]
    # lines
    assert rd.line_spans(made["lines"]) == [ref.spans[k] for k in made["lines"]]
    st = kolm.last_lines()
    assert (st["blocks_decoded"], st["groups"]) == (4, groups["sel"])
    offs = [100, 2 * BS + 7, 3 * BS + 1, 6 * BS + 4000]
    assert rd.line_of(offs) == [ref.line_of(o) for o in offs]
    st = kolm.last_lines()
    assert (st["blocks_decoded"], st["groups"]) == (4, groups["sel"])


# ------------------------------------------------------------------ the four families on a raw handle

def families(kolm, lib, ctx, h, lens, lines, pats):
    """name -> call, each selecting block BAD: the library's entry points on the handle h (the
    Reader class would serve a block outside KOLM_DECODE_MASK on the host)."""
    total = int(sum(lens))
    ranges = block_ranges(lens, SEL)
    ps = kolm.PatternSet(pats, ctx)
    return ps, {
        "read": lambda: lib.reader_read(h, ranges),
        "find": lambda: lib.reader_find(h, pats, 0, total),
        "find_set": lambda: lib.reader_find_set(h, ps._handle(), len(pats), 0, total),
        "index_lines": lambda: lib.reader_index_lines(h, 0x0A, NB),
        "line_spans": lambda: lib.reader_line_spans(h, lines),
    }


def raw_find(lib, h, pat, lo, hi):
    """kolm_reader_find itself: (return code, nfound, message)."""
    flat, off = lib._pattern_arrays([pat])
    counts = np.zeros(1, np.uint64)
    nfound = ctypes.c_uint64(77)
    st = lib.FindStats()
    rc = lib.load().kolm_reader_find(h, flat.ctypes.data, off.ctypes.data, 1, lo, hi, lib.NO_LIMIT, counts.ctypes.data,
                                     ctypes.byref(nfound), ctypes.byref(st))
    return rc, int(nfound.value), lib.load().kolm_last_error().decode()


# ------------------------------------------------------------------ 2. a block the device does not decode

def test_same_refusal_for_an_undecodable_block(kolm_gpu, lib, ctx, made, monkeypatch):
    kolm = kolm_gpu
    monkeypatch.setenv("KOLM_READ_BYTES", "8192")
    other = 11
    assert other < 32 and not (lib.KOLM_DECODE_MASK >> other) & 1
    mids = list(made["mids"])
    mids[BAD] = other
    blob = kolm.write_container(kolm.MODE_FIXED, BS, NB * BS, mids, [BS] * NB, made["payloads"])
    assert [int(m) for m in kolm.read_toc(blob)[3]] == mids
    h, _ = lib.reader_open(blob, ctx)
    ps = None
    try:
        lib.reader_set_lines(h, 0x0A, made["ref"].counts)
        ps, calls = families(kolm, lib, ctx, h, [BS] * NB, made["lines"], made["pats"])
        lib.check(lib.load().kolm_ctx_set_timing(ctx, 1))
        before = lib.kernel_times(ctx)
        for name, call in calls.items():
            with pytest.raises(ValueError) as ei:  # the binding raises ValueError for KOLM_EARG alone
                call()
            assert str(ei.value) == f"block {BAD} (method {other}, {BS} bytes) is not decoded on the device", name
        assert lib.kernel_times(ctx) == before  # the check precedes the first launch
        assert raw_find(lib, h, b"fox", 0, NB * BS)[:2] == (-1, 0)
        # a call that does not select the block is served
        assert lib.reader_read(h, [(0, BS)]) == made["data"][:BS]
    finally:
        lib.load().kolm_ctx_set_timing(ctx, 0)
        if ps is not None:
            ps.close()
        lib.reader_close(h)


# ------------------------------------------------------------------ 3. a payload the decoder rejects

def test_same_rejection_for_a_malformed_payload(kolm_gpu, lib, ctx, made, monkeypatch):
    """Block BAD becomes the corpus case REJECTED as it stands: its payload and its length n (the
    corpus pins the rejection of that pair; the blocks behind it move up)."""
    from kolm import decode as H
    kolm = kolm_gpu
    monkeypatch.setenv("KOLM_READ_BYTES", "8192")
    c = next(c for c in DC.load() if c["name"] == REJECTED)
    assert c["mid"] == made["mids"][BAD] and c["n"] > 0
    with pytest.raises((ValueError, RuntimeError)):
        H.decode_block(c["mid"], c["payload"], c["n"])
    lens = [BS] * NB
    lens[BAD] = c["n"]
    payloads = list(made["payloads"])
    payloads[BAD] = c["payload"]
    blob = kolm.write_container(kolm.MODE_CDC, BS, sum(lens), made["mids"], lens, payloads)  # CDC: every length is stored
    counts = list(made["ref"].counts)
    counts[BAD] = 1  # the index says block BAD ends a line: line `line` starts in block 2 and ends there
    line = sum(counts[:BAD])
    h, _ = lib.reader_open(blob, ctx)
    ps = None
    try:
        lib.reader_set_lines(h, 0x0A, counts)
        ps, calls = families(kolm, lib, ctx, h, lens, [1, line], made["pats"])
        # an earlier search leaves results behind
        rc, nfound, _ = raw_find(lib, h, b"fox", 0, BS)
        assert rc == 0 and nfound == made["data"][:BS].count(b"fox") > 0
        texts = {}
        for name, call in calls.items():
            with pytest.raises(ValueError) as ei:
                call()
            texts[name] = str(ei.value)
        head = f"block {BAD} (method {c['mid']}): "
        assert texts["read"] in (head + "malformed payload", head + "decoded length mismatch")
        assert set(texts.values()) == {texts["read"]}, texts
        # find: no results leave the failed call, and the earlier ones are gone
        rc, nfound, msg = raw_find(lib, h, b"fox", 0, sum(lens))
        assert (rc, nfound, msg) == (-1, 0, texts["read"])
        one = np.zeros(1, np.uint64)
        assert lib.load().kolm_reader_find_copy(h, 0, 0, one.ctypes.data, None) == 0
        assert lib.load().kolm_reader_find_copy(h, 0, 1, one.ctypes.data, None) == -1
        assert lib.reader_read(h, [(0, BS)]) == made["data"][:BS]
    finally:
        if ps is not None:
            ps.close()
        lib.reader_close(h)


# ------------------------------------------------------------------ 4. a wrong checksum in the second group

def test_same_checksum_failure(kolm_gpu, lib, ctx, made, monkeypatch):
    from kolm.checksums import KolmChecksumError
    kolm, rd, data, cs = kolm_gpu, made["rd"], made["data"], made["cs"]
    monkeypatch.setenv("KOLM_READ_BYTES", "8192")
    wrong = list(cs.crcs)
    wrong[BAD] ^= 0x00010000
    h = rd._h
    ps = None
    lib.reader_set_checksums(h, wrong)
    try:
        ps, calls = families(kolm, lib, ctx, h, [BS] * NB, made["lines"], made["pats"])
        for name, call in calls.items():
            with pytest.raises(KolmChecksumError) as ei:
                call()
            e = ei.value
            assert (e.block, e.method, e.expected, e.got) == (BAD, made["mids"][BAD], wrong[BAD], cs.crcs[BAD]), name
        # a device read into the caller's buffer: several groups, the bad block in the second -- nothing is written
        ranges = block_ranges([BS] * NB, SEL)
        buf = lib.DeviceBuffer(ctx, 4 * BS + 128)
        try:
            buf.upload(bytes([0xA5]) * (4 * BS + 128))
            with pytest.raises(KolmChecksumError):
                lib.reader_read_device(h, ranges, buf.ptr + 64, 4 * BS)
            assert buf.download() == bytes([0xA5]) * (4 * BS + 128)
            lib.reader_set_checksums(h, cs.crcs)
            lib.reader_read_device(h, ranges, buf.ptr + 64, 4 * BS)
            assert lib.last_read()["groups"] == 2
            assert buf.download() == bytes([0xA5]) * 64 + b"".join(data[o:o + n] for o, n in ranges) + bytes([0xA5]) * 64
        finally:
            buf.free()
    finally:
        lib.reader_set_checksums(h, cs.crcs)
        if ps is not None:
            ps.close()
