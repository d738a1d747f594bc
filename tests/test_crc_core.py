"""The integer core of the block CRC-32 (kolmogorovlike-datacompressor_amd/csrc/crc_core.h) checked
on the CPU through tools/crc_emu.cpp, which compiles the header k_crc32 uses and walks the kernel's
runs, waves and lanes (the loads are those of the fingerprint kernel: tools/dedup_emu.cpp's Emu),
checking every load against the kernel's contract (aligned 16-byte words that lie inside the batch
whole; single bytes of the block at hand) and counting the violations.  zlib.crc32 is the oracle.
The stand-alone program (its own main) is also built with -fsanitize=address,undefined and run once
over the same sweep on heap buffers of exactly the batches' sizes.  Nothing is preloaded into
Python."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "crc_emu.cpp")
# every word / piece / run edge (a run is 8 pieces of 4 KiB), and 4 runs
LENS = (1, 3, 4, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 32767, 32768, 32769, 100000)
ORDERS = ((0, 0), (1, 2), (2, 3), (2, 0))  # (order, waves): the kernel's grid, reversed, interleaved


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("crc") / "crc_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    P, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.crc_emu_blocks.argtypes = [P, U64, P, U32, U32, U32, P]
    lib.crc_emu_blocks.restype = U64
    lib.crc_emu_combine.argtypes = [U32, U32, U64]
    lib.crc_emu_combine.restype = U32
    lib.crc_emu_xpow.argtypes = [U32]
    lib.crc_emu_xpow.restype = U32
    lib.crc_ref.argtypes = [P, U64]
    lib.crc_ref.restype = U32
    return lib


def content(n, seed=0):
    i = np.arange(n, dtype=np.uint64) + np.uint64(seed * 977)
    return ((i * 131 + (i >> 8) * 7 + 3) & 0xFF).astype(np.uint8)


def fills(n):
    return bytes(n), b"\xff" * n, content(n).tobytes()


_libc = ctypes.CDLL(None)
_libc.malloc.restype = ctypes.c_void_p
_libc.malloc.argtypes = [ctypes.c_size_t]
_libc.free.argtypes = [ctypes.c_void_p]


class place:
    """The batch in a heap block of exactly lead + len(batch) bytes: malloc's blocks begin on a
    16-byte boundary, so the batch begins `lead` bytes past one and ends where the allocation
    ends; the `lead` bytes in front are not part of it.  .addr is the batch's address."""

    def __init__(self, batch: bytes, lead: int):
        self.raw = _libc.malloc(max(lead + len(batch), 1))
        assert self.raw and self.raw % 16 == 0
        ctypes.memset(self.raw, 0xEE, lead)
        ctypes.memmove(self.raw + lead, batch, len(batch))
        self.addr = self.raw + lead

    def __del__(self):
        _libc.free(self.raw)


def crcs(emu, batch: bytes, bounds, lead=0, order=0, waves=0):
    """The blocks' CRC-32 as the kernel computes them; the contract count must be 0."""
    buf = place(batch, lead)
    b = np.ascontiguousarray(np.asarray(bounds, np.uint64))
    out = np.full(len(b) - 1, 0xDEADBEEF, np.uint32)
    bad = emu.crc_emu_blocks(buf.addr, len(batch), b.ctypes.data, len(b) - 1, waves, order, out.ctypes.data)
    assert bad == 0, (bad, lead, list(bounds)[:4], order, waves)
    return [int(x) for x in out]


def test_known_answers(emu):
    for msg, want in ((b"123456789", 0xCBF43926), (b"", 0), (bytes(1), 0xD202EF8D), (bytes(2), 0x41D912FF)):
        assert zlib.crc32(msg) == want
        assert crcs(emu, msg, [0, len(msg)]) == [want]
        buf = np.frombuffer(msg, np.uint8) if msg else np.zeros(1, np.uint8)
        assert emu.crc_ref(buf.ctypes.data, len(msg)) == want
    # x^(2^32 - 1) = 1: what the negative powers of the run weights rest on
    assert emu.crc_emu_xpow(0xFFFFFFFF) == 0x80000000 == emu.crc_emu_xpow(0)


@pytest.mark.parametrize("n", LENS)
def test_every_length_content_lead_and_order(emu, n):
    """Each block alone at every misalignment (both batch-end byte paths occur), and packed with
    others as a variable-geometry batch (a prefix, an empty block, a tail), in the four walks."""
    for blk in fills(n):
        want = zlib.crc32(blk)
        for lead in range(16):
            pre = bytes([0xE0 + lead]) * ((lead * 7 + 3) & 15)
            batch = pre + blk + b"\x55" * 21
            bounds = [0, len(pre), len(pre) + n, len(pre) + n, len(batch)]
            packed = [zlib.crc32(pre), want, 0, zlib.crc32(b"\x55" * 21)]
            for order, waves in ORDERS:
                assert crcs(emu, blk, [0, n], lead, order, waves) == [want], (n, lead, order, waves)
                assert crcs(emu, batch, bounds, lead, order, waves) == packed, (n, lead, order, waves)


def test_blocks_of_one_batch_do_not_see_their_neighbours(emu):
    lens = list(LENS) + [0, 5, 8 * 4096 + 7, 0, 17 * 4096]
    blocks = [content(n, seed=i + 1).tobytes() for i, n in enumerate(lens)]
    bounds = np.concatenate(([0], np.cumsum(lens))).tolist()
    want = [zlib.crc32(b) for b in blocks]
    for lead in (0, 3, 15):
        for order, waves in ORDERS + ((0, 1), (1, 5)):
            assert crcs(emu, b"".join(blocks), bounds, lead, order, waves) == want, (lead, order, waves)


def test_combine(emu):
    a, b = content(12345, 1).tobytes(), content(1 << 16, 2).tobytes()
    for lb in (0, 1, 1 << 16):
        assert emu.crc_emu_combine(zlib.crc32(a), zlib.crc32(b[:lb]), lb) == zlib.crc32(a + b[:lb]), lb
    # len_b = 2^31 + 5 without allocating it: B = b1 + b2, in one step and in two
    ca, c1, c2 = zlib.crc32(a), 0x12345678, 0x9ABCDEF0  # any words: combine is a function of the three numbers
    l1, l2 = (1 << 31) - 100, 105
    cb = emu.crc_emu_combine(c1, c2, l2)
    assert emu.crc_emu_combine(ca, cb, l1 + l2) == emu.crc_emu_combine(emu.crc_emu_combine(ca, c1, l1), c2, l2)
    # the same split at a length zlib can check: the two paths and zlib agree
    b1, b2 = b[:40000], b[40000:]
    two = emu.crc_emu_combine(emu.crc_emu_combine(ca, zlib.crc32(b1), len(b1)), zlib.crc32(b2), len(b2))
    assert two == emu.crc_emu_combine(ca, zlib.crc32(b), len(b)) == zlib.crc32(a + b)


def test_the_python_combine_is_the_same_function(emu):
    from kolm.checksums import crc32_combine
    rng = np.random.default_rng(5)
    for lb in (0, 1, 2, 1 << 16, (1 << 31) + 5, (1 << 32) - 1, 1 << 40):
        x, y = (int(v) for v in rng.integers(0, 1 << 32, 2))
        assert crc32_combine(x, y, lb) == emu.crc_emu_combine(x, y, lb), lb


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "crc_emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout and "runtime error" not in r.stderr
