"""The LZ77 decoder's token parse (kolmogorovlike-datacompressor_amd/csrc/lz_parse_core.h, the
body of k_dec_lz_parse) checked on the CPU through tools/lz_parse_emu.cpp, which compiles the
header the kernel compiles and drives it as the kernel does: a batch of blocks whose token
records go into per-block slices of two shared slot arrays, here of exactly `total` entries
between poisoned guard words.  The emulator reports any write outside a block's own slots,
more records than output bytes, and record positions that do not strictly increase, and
resolves the records serially to bytes.  Checked: every LZ77 case of the conformance corpus
against PY's recorded verdict, and every token string of up to 4 tokens over {literal, copy
len 0/1/2/5 x dist 1/2/over} at n = 0..6 against kolm.decode.decode_lz77.  The stand-alone
program (its own main) is also built with -fsanitize=address,undefined and run over the same
sweep and the same corpus cases.  Nothing is preloaded into Python."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import decode_cases as DC
from kolm import decode as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "lz_parse_emu.cpp")
LZ = [c for c in DC.load() if c["mid"] == 7]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lzp") / "lz_parse_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.lzp_emu_decode.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + [ctypes.c_void_p] * 3
    lib.lzp_emu_decode.restype = ctypes.c_uint32
    return lib


def decode_batch(emu, pays, lens):
    """One batch through the emulator: [bytes or None per block]; the parse's contract holds."""
    nb = len(pays)
    off = np.zeros(nb + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in pays])
    arena = np.frombuffer(b"".join(pays) + b"\0", np.uint8)
    ln = np.asarray(lens, np.uint32)
    ob = np.concatenate([[0], np.cumsum(ln, dtype=np.int64)])
    out = np.full(int(ob[-1]) + 1, 0xA5, np.uint8)
    st = np.full(nb, 99, np.uint32)
    nt = np.full(nb, 99, np.uint32)
    viol = emu.lzp_emu_decode(arena.ctypes.data, off.ctypes.data, ln.ctypes.data, nb, out.ctypes.data,
                              st.ctypes.data, nt.ctypes.data)
    assert viol == 0, f"parse contract violated: {viol}"
    assert out[-1] == 0xA5 and (nt <= ln).all()
    return [out[ob[b]:ob[b + 1]].tobytes() if st[b] == 0 else None for b in range(nb)]


def host(pay, n):
    try:
        return H.decode_lz77(pay, n)
    except ValueError:
        return None


def test_corpus_cases_one_batch_and_alone(emu):
    """Back to back in one batch (a block that overran its slots would corrupt the next one's
    records, or the guard behind the last) and each alone: PY's bytes, or a rejection where
    the corpus rule allows one; the host decoder gives the same verdict."""
    got = decode_batch(emu, [c["payload"] for c in LZ], [c["n"] for c in LZ])
    for c, g in zip(LZ, got):
        DC.check_against_py(c, g)
        assert g == host(c["payload"], c["n"]), c["name"]
        assert decode_batch(emu, [c["payload"]], [c["n"]]) == [g], c["name"]
    assert sum(g is not None for g in got) >= 0.6 * len(LZ)


def test_zero_length_copies_take_no_slot(emu):
    """More tokens than output bytes: every block between two plain ones, the last block of
    the batch included; ULEB values past 32 bits saturate instead of wrapping to 0."""
    z = b"\x01\x00\x01"
    plain = (b"\x00x\x00y\x00z", 3, b"xyz")
    pays, lens, want = [], [], []
    for rep in (1, 2, 3, 50, 5000):
        for p, n, w in (plain, (b"\x00A" + z * rep + b"\x00B", 2, b"AB")):
            pays.append(p), lens.append(n), want.append(w)
    assert decode_batch(emu, pays, lens) == want
    wide = [(b"\x00A\x01\x80\x80\x80\x80\x10\x01", 9, b"A" * 9),        # length 2^32
            (b"\x00A\x01\x83\x80\x80\x80\x80\x00\x01", 4, b"AAAA"),     # 6-byte overlong 3
            (b"\x00A\x01\x03\x81\x80\x80\x80\x80\x00", 4, b"AAAA"),     # 6-byte overlong distance 1
            (b"\x00A\x01\x03\x81\x80\x80\x80\x10", 4, None),            # distance 2^32 + 1
            (b"\x00A\x01\x03\x81\x80\x80\x80\x80\x01", 4, None)]        # distance 2^35 + 1
    assert decode_batch(emu, [p for p, _, _ in wide], [n for _, n, _ in wide]) == [w for _, _, w in wide]
    for p, n, w in wide:
        assert host(p, n) == w


TOKENS = [b"\x00"] + [bytes((1, ln, d)) for ln in (0, 1, 2, 5) for d in (1, 2, 7)]  # 7: past every output here


def test_exhaustive_small_sweep(emu):
    """Every string of up to 4 tokens, n = 0..6, each n one batch of 30941 blocks, against the
    host decoder (itself pinned to PY by the corpus)."""
    strings = []
    for k in range(5):
        for combo in itertools.product(range(len(TOKENS)), repeat=k):
            strings.append(b"".join(TOKENS[t] + (bytes((65 + i,)) if t == 0 else b"") for i, t in enumerate(combo)))
    assert len(strings) == sum(13 ** k for k in range(5))
    accepted = 0
    for n in range(7):
        got = decode_batch(emu, strings, [n] * len(strings))
        want = [host(p, n) for p in strings]
        bad = [i for i in range(len(strings)) if got[i] != want[i]]
        assert not bad, (n, strings[bad[0]].hex(), got[bad[0]], want[bad[0]])
        accepted += sum(g is not None for g in got)
    assert accepted > 10000


def test_standalone_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lz_parse_emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    SRC, "-o", exe], check=True)
    cases = tmp_path / "cases.txt"
    cases.write_text("".join(f"{c['n']} {c['payload'].hex() or '-'}\n" for c in LZ))
    r = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{216601 + len(LZ)} cases ok" in r.stdout and "runtime error" not in r.stderr
