"""The gather kernel's integer core (kolmogorovlike-datacompressor_amd/csrc/range_core.h) checked on
the CPU through tools/range_emu.cpp, which compiles the header k_range_gather uses and walks the
kernel's items, waves, lanes and head / body / tail split, checking every load and store against
the kernel's contract (loads: aligned 16-byte words of the source buffer that hold a byte of the
segment; stores: bytes of [dst, dst + len) only) and counting the violations.  The copies are
compared with numpy slices; canary bytes surround the destination; the source buffer handed to the
emulation is exactly as large as the padding contract allows.  The stand-alone program (its own
main) is also built with -fsanitize=address,undefined and run once over the same sweeps on heap
buffers of exactly those sizes.  Nothing is preloaded into Python."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "range_emu.cpp")
CANARY = 0xCC
PAD = 64


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("rng") / "range_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.rng_emu_gather.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                   ctypes.c_uint32, ctypes.c_uint32]
    lib.rng_emu_gather.restype = ctypes.c_uint64
    lib.rng_emu_item_bytes.restype = ctypes.c_uint32
    return lib


def aligned(nbytes, fill):
    """(array, offset): array[offset] lies at a 16-byte aligned address, nbytes follow it."""
    raw = np.full(nbytes + 2 * PAD + 16, fill, np.uint8)
    return raw, PAD + (-(raw.ctypes.data + PAD)) % 16


SRC_BYTES = ((np.arange(1 << 16, dtype=np.uint64) * 131 + (np.arange(1 << 16, dtype=np.uint64) >> 8) + 7) & 0xFF) \
    .astype(np.uint8)


def gather(emu, segs, waves=0, order=0):
    """segs: [(src, dst, len)], offsets from 16-byte aligned bases.  The source buffer the
    emulation may touch: the aligned words up to the last segment's end, nothing more.  Checks
    the contract count, the copied bytes and the canaries."""
    src_span = max((s + n for s, _, n in segs), default=0)
    dst_size = max((d + n for _, d, n in segs), default=0)
    src_size = (src_span + 15) // 16 * 16
    sraw, so = aligned(src_size, 0x5A)
    sraw[so:so + src_size] = SRC_BYTES[:src_size]
    draw, do = aligned(dst_size, CANARY)
    want = draw.copy()
    for s, d, n in segs:
        want[do + d:do + d + n] = SRC_BYTES[s:s + n]
    tab = np.ascontiguousarray(np.asarray(segs, dtype=np.uint64).reshape(-1, 3))
    bad = emu.rng_emu_gather(sraw.ctypes.data + so, src_size, draw.ctypes.data + do, tab.ctypes.data, len(segs), waves,
                             order)
    assert bad == 0, (bad, segs[:3], waves, order)
    diff = np.flatnonzero(draw != want)
    assert diff.size == 0, (int(diff[0]) - do, segs[:3], waves, order)


def test_one_segment_every_alignment_and_length(emu):
    cases = 0
    for sm in range(16):
        for dm in range(16):
            for n in range(81):
                gather(emu, [(sm, dm, n)])
                cases += 1
    assert cases == 16 * 16 * 81


def test_one_segment_around_the_item_size(emu):
    item = emu.rng_emu_item_bytes()
    assert item % 16 == 0 and 1024 <= item <= 16384  # "a few KiB"
    for n in (item - 1, item, item + 1, 2 * item + 17):
        for sm, dm in ((0, 0), (3, 9), (15, 1)):
            for order, waves in ((0, 0), (1, 2), (2, 2)):
                gather(emu, [(sm, dm, n)], waves, order)


def packed(lens, dm):
    segs, so, d = [], 3, dm
    for i, n in enumerate(lens):
        segs.append((so, d, n))
        so += n + (i * 7) % 23
        d += n
    return segs


def test_many_short_segments_share_destination_words(emu):
    """Segments of 0..33 bytes back to back in dst: neighbours share 16-byte words.  The items are
    walked forward, in reverse and in an interleaved wave order: a store wider than a segment's own
    bytes would overwrite what a neighbour wrote before."""
    lens = [(n * 5 + rep) % 34 for rep in range(3) for n in range(34)]
    assert set(lens) == set(range(34))
    for dm in (0, 5, 15):
        for order, waves in ((0, 0), (1, 3), (2, 0), (2, 5)):
            gather(emu, packed(lens, dm), waves, order)
    rng = np.random.default_rng(11)
    for _ in range(20):
        lens = rng.integers(0, 34, 60).tolist()
        gather(emu, packed(lens, int(rng.integers(0, 16))), int(rng.integers(0, 7)), int(rng.integers(0, 3)))


def test_several_items_under_a_grid_stride(emu):
    item = emu.rng_emu_item_bytes()
    lens = [1, 3 * item + 5, 0, 17, item, 2 * item - 1, 33, 16, item + 16]
    for waves in (1, 2, 5):
        for order in range(3):
            gather(emu, packed(lens, 7), waves, order)


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "range_emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout and "runtime error" not in r.stderr
