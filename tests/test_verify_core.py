"""The verify compare kernel's integer core (kolmogorovlike-datacompressor_amd/csrc/verify_core.h)
checked on the CPU through tools/verify_emu.cpp, which compiles the header k_verify_cmp uses and
walks the kernel's grid, tiles, waves and head / body / tail split: an exhaustive small sweep
(base misalignment 0..15, total 0..48, every single differing byte, three block layouts) against
per-block first offsets computed here, the everything-differs and nothing-differs cases, bytes
planted just outside the compared range, and several tiles under a grid stride.  The stand-alone
program (its own main) is also built with -fsanitize=address,undefined and run once over the
same sweep on buffers of exactly `total` bytes.  Nothing is preloaded into Python.  Second: the
layout of kolm_verify_report against the ctypes struct (CPU)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from kolm import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "verify_emu.cpp")
HEADER = os.path.join(REPO, "include", "kolm.h")
EQUAL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vfy") / "verify_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.vfy_emu_compare.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                    ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    lib.vfy_emu_compare.restype = ctypes.c_uint64
    return lib


def layout(kind, total):
    if kind == "ones":
        return list(range(total + 1))
    if kind == "mixed":
        b, lens, i = [0], [1, 2, 3, 15, 16, 17], 0
        while b[-1] < total:
            b.append(min(total, b[-1] + lens[i % 6]))
            i += 1
        return b
    return [0, total] if total else [0]


def expected(a, b, bounds):
    diff = np.flatnonzero(a != b)
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        d = diff[(diff >= lo) & (diff < hi)]
        out.append(int(d[0]) - lo if len(d) else EQUAL)
    return out


def ops_bound(total, nb):
    """Minimum operations of the slow path at the most: one per byte of the head and of the tail
    (< 16 each) and one per (word, block the word touches) — the words plus the nb - 1 block
    edges that can fall inside a word.  Bounded by the data size, not by the differing bytes."""
    return 30 + total // 16 + nb


def compare(emu, a, b, mis, bounds, grid=0, pad=32):
    """a, b: uint8 arrays of the compared range; the emulator gets them inside larger buffers
    (pad bytes on each side, the range's first byte at an address congruent to mis mod 16).
    Returns (first_bad list, minimum operations)."""
    total = len(a)
    bufs = []
    for x, fill in ((a, 0x11), (b, 0xEE)):  # the bytes around the range differ between the buffers
        raw = np.full(total + 2 * pad + 32, fill, np.uint8)
        o = pad + ((mis - (raw.ctypes.data + pad)) % 16)
        raw[o:o + total] = x
        bufs.append((raw, o))
    bd = np.asarray(bounds, np.uint32)
    fb = np.zeros(max(len(bounds) - 1, 1), np.uint32)
    (ra, oa), (rb, ob) = bufs
    ops = emu.vfy_emu_compare(ra.ctypes.data + oa, rb.ctypes.data + ob, total, mis, bd.ctypes.data, len(bounds) - 1,
                              fb.ctypes.data, grid)
    return fb[:len(bounds) - 1].tolist(), ops


def test_small_sweep_every_single_byte(emu):
    cases = 0
    for mis in range(16):
        for total in range(49):
            a = ((np.arange(total) * 7 + 3) & 0xFF).astype(np.uint8)
            for kind in ("ones", "mixed", "one"):
                bounds = layout(kind, total)
                for p in range(total):
                    b = a.copy()
                    b[p] ^= 0x80
                    got, ops = compare(emu, a, b, mis, bounds)
                    assert got == expected(a, b, bounds), (mis, total, kind, p)
                    assert ops == 1
                    cases += 1
    assert cases == 16 * 3 * sum(range(49))


def test_everything_and_nothing_differs(emu):
    for mis in range(16):
        for total in range(49):
            a = ((np.arange(total) * 7 + 3) & 0xFF).astype(np.uint8)
            for kind in ("ones", "mixed", "one"):
                bounds = layout(kind, total)
                nb = len(bounds) - 1
                got, ops = compare(emu, a, a.copy(), mis, bounds)
                assert got == [EQUAL] * nb and ops == 0  # the equal path: no lookup, no minimum
                got, ops = compare(emu, a, ~a, mis, bounds)
                assert got == [0] * nb, (mis, total, kind)
                assert ops <= ops_bound(total, nb)


def test_bytes_outside_the_range_are_not_reported(emu):
    # compare() surrounds both ranges with bytes that differ between the buffers
    for mis in (0, 1, 15):
        for total in (0, 1, 15, 16, 17, 48):
            a = np.arange(total, dtype=np.uint8)
            bounds = layout("mixed", total)
            got, ops = compare(emu, a, a.copy(), mis, bounds, pad=1)
            assert got == [EQUAL] * (len(bounds) - 1) and ops == 0


def test_tiles_and_grid_stride(emu):
    tile = 16 * 1024  # bytes of one workgroup iteration
    rng = np.random.default_rng(5)
    for mis, total in ((0, tile), (5, 3 * tile + 37), (15, 2 * tile - 1)):
        a = rng.integers(0, 256, total, dtype=np.uint8)
        bounds = [0, 1, 4097, total - 3, total]
        for p in (0, 1, 4096, 4097, tile - 1, total - 4, total - 3, total - 1):
            b = a.copy()
            b[p] ^= 1
            for grid in (0, 1, 2):
                assert compare(emu, a, b, mis, bounds, grid)[0] == expected(a, b, bounds), (mis, total, p, grid)
        b = a.copy()
        b[rng.integers(0, total, 200)] ^= 0x40
        assert compare(emu, a, b, mis, bounds, 2)[0] == expected(a, b, bounds)
        got, ops = compare(emu, a, ~a, mis, bounds)
        assert got == [0, 0, 0, 0] and ops <= ops_bound(total, 4)


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "verify_emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cases ok" in r.stdout and "runtime error" not in r.stderr


def test_verify_report_layout_matches_header(tmp_path):
    assert ctypes.sizeof(_lib.VerifyReport) == 6 * 4 + 8 + 2 * 8
    fields = [f for f, _ in _lib.VerifyReport._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kolm.h"\nint main(void){printf("%zu'
                   + "".join(" %zu" for _ in fields) + '\\n", sizeof(kolm_verify_report)'
                   + "".join(f", offsetof(kolm_verify_report, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.VerifyReport)
    assert got[1:] == [getattr(_lib.VerifyReport, f).offset for f in fields]
    text = open(HEADER).read()
    assert "#define KOLM_EVERIFY (-8)" in text and _lib.KOLM_EVERIFY == -8
    assert _lib.KOLM_VERIFY_EQUAL == 0xFFFFFFFF and _lib.KOLM_VERIFY_REJECTED == 0xFFFFFFFE
