"""Host decoders (kolm/decode.py) against the decoder conformance corpus: payloads no encoder
of this project writes, with what the Python reference makes of each recorded beside them
(tests/golden/decode_cases.json, make_golden_decode_cases.py).  Byte-exact: where PY returns
bytes the host returns the same bytes, or rejects in the few pinned classes of
decode_cases.PINNED_REJECTS; where PY raises ValueError the host rejects.  The device decoders
are held to the same rule, and to the host, by test_gpu_decode_conformance.py."""
import pytest

import decode_cases as DC
from kolm import decode as H

CASES = DC.load()


def host_verdict(c):
    try:
        return H.decode_block(c["mid"], c["payload"], c["n"])
    except (ValueError, RuntimeError):  # RuntimeError: Re-Pair's length mismatch, as in PY
        return None


def test_corpus_shape():
    """What the generator asserted still holds for the committed file: PY decodes at least 60 %
    of every method's cases and at least one case of every class; payloads are small; the
    pinned classes exist."""
    assert len({c["name"] for c in CASES}) == len(CASES) > 150
    for mid in {c["mid"] for c in CASES}:
        mine = [c for c in CASES if c["mid"] == mid]
        assert sum(DC.py_bytes(c) is not None for c in mine) >= 0.6 * len(mine), mid
    for cls in {c["class"] for c in CASES}:
        assert any(DC.py_bytes(c) is not None for c in CASES if c["class"] == cls), cls
    assert all(len(c["payload"]) <= 8192 for c in CASES)
    assert set(DC.PINNED_REJECTS) <= {c["class"] for c in CASES}
    assert {c["mid"] for c in CASES} == set(range(10))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_host_decoder_matches_py(c):
    DC.check_against_py(c, host_verdict(c))


def test_pinned_rejections_are_rejections():
    """The pinned classes are real divergences, not slack: every case of them that is not the
    class's plain sibling is rejected by the host although PY decodes it."""
    seen = set()
    for c in CASES:
        if c["class"] in DC.PINNED_REJECTS and c["name"].split("/")[1] != "none":
            assert DC.py_bytes(c) is not None and host_verdict(c) is None, c["name"]
            seen.add(c["class"])
    assert seen == set(DC.PINNED_REJECTS)
