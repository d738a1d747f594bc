"""The v2_new (id 10) decoder's integer core (kolmogorovlike-datacompressor_amd/csrc/v2_decode_core.h)
checked on the CPU through tools/v2_decode_emu.cpp, which compiles the header the kernels use and
drives it with the kernels' tiling: the 85 PY payloads of tests/golden/v2new.npz and the
hand-made payloads of tests/v2_payloads.py (every automaton mode over raw planes, Rice planes
with k = 0..15, codewords laid across the parse tile's edges) against the host decoder
kolm.decode.decode_new_pipeline, and the malformed payloads rejected.  The stand-alone program
(its own main) is also built with -fsanitize=address,undefined and run once over the same cases."""
import ctypes
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import v2_payloads as V
from kolm import decode as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "v2_decode_emu.cpp")
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("v2d") / "v2_decode_emu.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.v2d_emu_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p]
    lib.v2d_emu_decode.restype = ctypes.c_uint32
    return lib


def decode(emu, payload, n):
    out = ctypes.create_string_buffer(max(n, 1))
    st = emu.v2d_emu_decode(payload, len(payload), n, out)
    return st, out.raw[:n]


def goldens():
    z = np.load(os.path.join(GOLDEN, "v2new.npz"))
    with open(os.path.join(GOLDEN, "v2new.json")) as f:
        names = json.load(f)["kernels"]
    return [(n, z[f"{n}/v2new"].tobytes(), z[f"{n}/input"].tobytes()) for n in names]


def good_cases():
    junk = [(n + "+junk", p + b"\xde\xad\xbe\xef", d) for n, p, d in V.automaton_cases()]
    return goldens() + list(V.automaton_cases()) + junk + list(V.rice_cases()) + \
        [("neighbour", V.VALID_NEIGHBOUR, bytes(4)), ("empty", b"", b""), ("empty_junk", b"\xff", b"")]


def bad_cases():
    return [(p, V.MALFORMED_N) for p in V.MALFORMED] + [(V.k16_block()[0], 4)]


def test_golden_payloads(emu):
    cases = goldens()
    assert len(cases) == 85
    for name, pay, data in cases:
        assert H.decode_new_pipeline(pay, len(data)) == data, name
        assert decode(emu, pay, len(data)) == (0, data), name


def test_automaton_modes_raw_planes(emu):
    cases = V.automaton_cases()
    assert len(cases) == 196
    for name, pay, data in cases:
        if len(data) <= 257:
            assert H.decode_new_pipeline(pay, len(data)) == data, name  # the forward models invert
        assert decode(emu, pay, len(data)) == (0, data), name
        assert decode(emu, pay + b"\xde\xad\xbe\xef", len(data)) == (0, data), name


def test_rice_planes(emu):
    for name, pay, data in V.rice_cases():
        assert H.decode_new_pipeline(pay, len(data)) == data, name
        assert decode(emu, pay, len(data)) == (0, data), name


def test_k16_is_host_only(emu):
    pay, data = V.k16_block()
    assert H.decode_new_pipeline(pay, len(data)) == data  # PY decodes any k byte
    assert decode(emu, pay, len(data))[0] != 0             # the device core stops at 15


def test_malformed_rejected(emu):
    for pay in V.MALFORMED:
        with pytest.raises(ValueError):
            H.decode_new_pipeline(pay, V.MALFORMED_N)
        assert decode(emu, pay, V.MALFORMED_N)[0] != 0, pay
        assert decode(emu, pay, 0) == (0, b"")  # n == 0: nothing to decode, whatever the payload
    assert decode(emu, V.VALID_NEIGHBOUR, 4) == (0, bytes(4))
    assert H.decode_new_pipeline(V.VALID_NEIGHBOUR, 4) == bytes(4)


def test_truncations_never_decode_wrong(emu):
    """Every proper prefix of a valid payload is rejected or decodes to the same bytes as on the
    host decoder (which raises where the emulation rejects)."""
    name, pay, data = V.rice_cases()[1]
    for cut in range(len(pay)):
        st, got = decode(emu, pay[:cut], len(data))
        try:
            want = H.decode_new_pipeline(pay[:cut], len(data))
        except ValueError:
            want = None
        assert (None if st else got) == want, cut


def test_standalone_sanitized(tmp_path):
    exe = str(tmp_path / "v2_decode_emu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    good, bad = good_cases(), bad_cases()
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(good) + len(bad)))
        for _, pay, data in good:
            f.write(struct.pack("<III", len(data), len(pay), 1) + pay + data)
        for pay, n in bad:
            f.write(struct.pack("<III", n, len(pay), 0) + pay)
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"v2_decode_emu: {len(good) + len(bad)} file cases" in r.stdout
    assert "v2_decode_emu: ok" in r.stdout
