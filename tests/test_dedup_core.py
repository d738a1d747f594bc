"""The integer core of duplicate-block detection (kolmogorovlike-datacompressor_amd/csrc/dedup_core.h)
checked on the CPU through tools/dedup_emu.cpp, which compiles the header k_block_fp and k_dedup_cmp
use and walks the kernels' items, waves and lanes, checking every load against the kernels'
contract (aligned 16-byte words that lie inside the batch whole; single bytes of the block at hand)
and counting the violations: the emulation is told the batch's exact extent and counts every
load that leaves it.  The stand-alone program (its own main) is also built with
-fsanitize=address,undefined and run once over the same sweep on heap buffers of exactly the
batches' sizes.  Nothing is preloaded into Python."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "dedup_emu.cpp")
LENS = (1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8193)
ORDERS = ((0, 0), (1, 2), (2, 3), (2, 0))  # (order, waves): the kernel's grid, reversed, interleaved


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ddp") / "dedup_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.ddp_emu_fp.argtypes = [P, U64, P, U32, U32, U32, P]
    lib.ddp_emu_fp.restype = U64
    lib.ddp_emu_cmp.argtypes = [P, U64, P, P, U32, U32, U32, P]
    lib.ddp_emu_cmp.restype = U64
    lib.ddp_ref_fp.argtypes = [P, U64, P]
    lib.ddp_ref_fp.restype = None
    lib.ddp_emu_item_bytes.restype = U32
    return lib


def content(n, seed=0):
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed * 977)
    return ((i * 131 + (i >> 8) * 7 + 3) & 0xFF).astype(np.uint8)


_libc = ctypes.CDLL(None)
_libc.malloc.restype = ctypes.c_void_p
_libc.malloc.argtypes = [ctypes.c_size_t]
_libc.free.argtypes = [ctypes.c_void_p]


class place:
    """The batch in a heap block of exactly lead + len(batch) bytes: malloc's blocks begin on a
    16-byte boundary, so the batch begins `lead` bytes past one and ends where the allocation
    ends; the `lead` bytes in front are not part of it.  .addr is the batch's address.  The
    emulation is told the batch's extent and counts every load outside it (the kernels'
    wave-uniform item test implies the per-word test it walks, which it checks too)."""

    def __init__(self, batch: bytes, lead: int):
        self.raw = _libc.malloc(max(lead + len(batch), 1))
        assert self.raw and self.raw % 16 == 0
        ctypes.memset(self.raw, 0xEE, lead)
        ctypes.memmove(self.raw + lead, batch, len(batch))
        self.addr = self.raw + lead

    def __del__(self):
        _libc.free(self.raw)


def fingerprints(emu, batch: bytes, bounds, lead=0, order=0, waves=0):
    """[(f0, f1)] of the batch's blocks as the kernel computes them; contract count must be 0."""
    buf = place(batch, lead)
    b = np.ascontiguousarray(np.asarray(bounds, np.uint64))
    fp = np.zeros(2 * (len(b) - 1), np.uint64)
    bad = emu.ddp_emu_fp(buf.addr, len(batch), b.ctypes.data, len(b) - 1, waves, order, fp.ctypes.data)
    assert bad == 0, (bad, lead, bounds[:4], order, waves)
    return [(int(fp[2 * i]), int(fp[2 * i + 1])) for i in range(len(b) - 1)]


def compare(emu, batch: bytes, bounds, pairs, lead=0, order=0, waves=0):
    buf = place(batch, lead)
    b = np.ascontiguousarray(np.asarray(bounds, np.uint64))
    pr = np.ascontiguousarray(np.asarray(pairs, np.uint32).reshape(-1))
    differ = np.full(len(pairs), 7, np.uint32)
    bad = emu.ddp_emu_cmp(buf.addr, len(batch), b.ctypes.data, pr.ctypes.data, len(pairs), waves, order, differ.ctypes.data)
    assert bad == 0, (bad, lead, bounds[:4], pairs[:4])
    return [int(x) for x in differ]


def ref(emu, block: bytes):
    fp = np.zeros(2, np.uint64)
    buf = np.frombuffer(block, np.uint8)
    emu.ddp_ref_fp(buf.ctypes.data, len(block), fp.ctypes.data)
    return int(fp[0]), int(fp[1])


def test_same_content_same_fingerprint_at_every_alignment_and_order(emu):
    assert emu.ddp_emu_item_bytes() == 4096
    for n in LENS:
        blk = content(n).tobytes()
        want = ref(emu, blk)  # the definition restated byte by byte
        for a in range(16):
            # behind a prefix of a bytes (the block starts a bytes past a boundary), alone in the
            # batch at that alignment, and followed by other bytes
            assert fingerprints(emu, bytes(a) + blk, [0, a, a + n] if a else [0, n])[-1] == want, (n, a)
            assert fingerprints(emu, blk, [0, n], lead=a)[0] == want, (n, a)
            order, waves = ORDERS[a % len(ORDERS)]
            got = fingerprints(emu, blk + b"\x55" * 21, [0, n, n + 21], lead=a, order=order, waves=waves)
            assert got[0] == want, (n, a, order, waves)


def test_a_changed_byte_or_an_appended_zero_changes_it(emu):
    for n in LENS:
        blk = bytearray(content(n).tobytes())
        want = ref(emu, bytes(blk))
        for pos in sorted({0, n // 2, n - 1}):
            mod = bytearray(blk)
            mod[pos] ^= 0x01
            assert fingerprints(emu, bytes(mod), [0, n], lead=5)[0] != want, (n, pos)
        assert fingerprints(emu, bytes(blk) + b"\0", [0, n + 1], lead=5)[0] != want, n
    assert ref(emu, b"x") != ref(emu, b"x\0")


def test_zero_blocks_have_nonzero_pairwise_different_fingerprints(emu):
    fps = [fingerprints(emu, bytes(n), [0, n], lead=n % 16)[0] for n in LENS]
    assert all(f != (0, 0) and f[0] != 0 and f[1] != 0 for f in fps)
    assert len(set(fps)) == len(LENS)
    # and a zero word does not vanish from the sum: words of zeros at different indices differ
    assert ref(emu, bytes(16)) != ref(emu, bytes(32))


def test_blocks_of_one_batch_do_not_see_their_neighbours(emu):
    """Several blocks back to back (every piece count, shared aligned words at the edges): each
    fingerprint equals the block's own, in every item order."""
    lens = [1, 4097, 15, 16, 8193, 33, 4096, 17, 4095, 31, 32, 8 * 4096 + 7, 5, 17 * 4096, 16 * 4096]  # 1..3 runs
    blocks = [content(n, seed=i + 1).tobytes() for i, n in enumerate(lens)]
    bounds = np.concatenate(([0], np.cumsum(lens))).tolist()
    want = [ref(emu, b) for b in blocks]
    for lead in (0, 3, 15):
        for order, waves in ORDERS + ((0, 1), (1, 5)):
            assert fingerprints(emu, b"".join(blocks), bounds, lead, order, waves) == want, (lead, order, waves)


def test_compare_finds_a_difference_in_head_body_and_tail(emu):
    for n in (1, 15, 16, 17, 33, 4095, 4096, 4097, 8193, 3 * 4096 + 5):
        blk = content(n).tobytes()
        spots = sorted({0, min(5, n - 1), n // 2, max(n - 3, 0), n - 1})  # head, body word, tail bytes
        for gap in (0, 1, 7, 13):  # the copies' alignments differ from the block's by gap mod 16
            copies = []
            for pos in spots:
                c = bytearray(blk)
                c[pos] ^= 0x80
                copies.append(bytes(c))
            batch = blk + bytes(gap) + blk + b"".join(copies)
            bounds = [0, n] + ([n + gap] if gap else []) + [n + gap + n]
            first = len(bounds) - 2  # the equal copy's block number
            for c in copies:
                bounds.append(bounds[-1] + n)
            pairs = [(first + k, 0) for k in range(len(copies) + 1)]
            for lead, (order, waves) in ((0, (0, 0)), (9, (1, 2)), (15, (2, 3))):
                assert compare(emu, batch, bounds, pairs, lead, order, waves) == [0] + [1] * len(copies), (n, gap, lead)


def test_compare_ignores_the_bytes_around_the_blocks(emu):
    """Equal blocks whose neighbours differ: the bytes an aligned load drags in beyond a block's
    ends must not count."""
    for n in (1, 15, 17, 4097):
        blk = content(n).tobytes()
        batch = b"\x11" * 3 + blk + b"\x22" * 6 + blk + b"\x33" * 9
        bounds = [0, 3, 3 + n, 9 + n, 9 + 2 * n, 18 + 2 * n]
        for lead in range(0, 16, 5):
            assert compare(emu, batch, bounds, [(3, 1)], lead) == [0], (n, lead)
            fp = fingerprints(emu, batch, bounds, lead)
            assert fp[1] == fp[3] == ref(emu, blk)


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "dedup_emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout and "runtime error" not in r.stderr
