"""The decoder conformance corpus (tests/golden/decode_cases.json, written from the Python
reference by tests/golden/make_golden_decode_cases.py) and the one rule both decoders are held
to, shared by test_decode_conformance.py (host), test_gpu_decode_conformance.py (device) and
test_lz_parse_core.py (the LZ77 parse core on the CPU)."""
import base64
import json
import os
import zlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The only classes in which a decoder of this project may reject a payload PY decodes.
PINNED_REJECTS = {
    "xor_trailing": "exactly n values must fill the payload; PY stops reading after the n-th value",
    "lfsr_trailing": "exactly n values must fill the payload; PY stops reading after the n-th value",
    "lz_zero_copy_far": "a copy's distance is checked once per copy, zero-length ones included; "
                        "PY checks it once per copied byte, so never for such a copy",
}


def load():
    with open(os.path.join(GOLDEN, "decode_cases.json")) as f:
        cases = json.load(f)
    for c in cases:
        c["payload"] = bytes.fromhex(c["payload"])
    return cases


def py_bytes(c):
    """The bytes PY decodes the case to; None where it raises or does not return."""
    py = c["py"]
    if not isinstance(py, dict):
        return None
    if "ok" in py:
        return bytes.fromhex(py["ok"])
    if "ok_zlib" in py:
        return zlib.decompress(base64.b64decode(py["ok_zlib"]))
    return None


def check_against_py(c, got):
    """got: the bytes a decoder of this project returned for case c, or None for a rejection.
    Where PY returns bytes, ours return the same bytes — or reject, in the classes of
    PINNED_REJECTS only; never other bytes.  Where PY raises ValueError (its own verdict on a
    malformed stream), ours reject.  A PY hang or a crash of another type (AssertionError,
    IndexError, ...) pins nothing here: the device and the host then only have to agree."""
    want = py_bytes(c)
    if want is not None:
        assert len(want) == c["n"]
        if got is None:
            assert c["class"] in PINNED_REJECTS, f"{c['name']}: rejected, PY decodes it"
        else:
            assert got == want, f"{c['name']}: bytes differ from PY's"
    elif isinstance(c["py"], dict) and c["py"]["error"] == "ValueError":
        assert got is None, f"{c['name']}: accepted, PY raises {c['py']['message']!r}"
