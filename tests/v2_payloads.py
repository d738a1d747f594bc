"""Hand-made v2_new (id 10) payloads for tests/test_v2_decode_core.py and
tests/test_gpu_v2_decode.py: the automaton's forward models (PY:664-900, written out here, not
taken from the code under test), the slim header (PY:1558-1576), raw planes and Rice-coded run
lengths of the planes' BBWT (the oracle's bbwt_forward).  Every case is (name, payload, data)."""
import functools

import numpy as np

AUTOMATA = [(0, 0), (1, 1), (1, 2), (1, 3), (1, 4), (1, 7), (1, 300), (1, 70000), (2, 0), (2, 1), (2, 2), (2, 3),
            (2, 0x1F7), (3, 0), (4, 0), (5, 0), (5, 1), (6, 0), (7, 9)]
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 257, 4097]
PARSE_TILE_BITS = 256 * 64  # one parse tile of the decoder: 256 words of 64 bits
AUTO_TILE = 4096            # one automaton tile of the decoder

MALFORMED = [
    b"\x00\xff",                              # shorter than 3 bytes
    b"\x05" + bytes(12),                      # plen 5
    b"\x24\x01\x02\x03",                      # plen 4, param truncated
    b"\x00\x00\x00" + b"\x04" * 7,            # k list past the end
    b"\x00\xff\x00" + bytes(7),               # raw plane truncated
    b"\x00\xfe\x00\x00\xff",                  # no unary terminator
    b"\x00\xfe\x00\x00\x00" + bytes(7),       # zero run
    b"\x00\xfe\x00\x00\xfc" + bytes(7),       # run 6 > 4
]
MALFORMED_N = 4
VALID_NEIGHBOUR = b"\x00\xfe\x00\x00\xf0" + bytes(7)  # decodes to four zero bytes


def _dil(x):
    return ((x << 1) | x | (x >> 1)) & 0xFF


def _ero(x):
    return ~_dil(~x & 0xFF) & 0xFF


def predictor(mode, param, i, r):
    """The model's prediction of byte i from the original bytes r[:i]."""
    if mode == 1:
        return 0 if param == 0 or i < param else r[i - param]
    if mode in (2, 3):
        if i == 0:
            return 0
        if i == 1:
            return r[0]
        a, b = r[i - 1], r[i - 2]
        if mode == 3:
            return (a & 0xF0) | (b & 0x0F)
        x = (a, b, a ^ b, a | b)[param & 3]
        return x ^ (x >> 1)
    if mode == 4:
        if i == 0:
            return 0
        if i < 3:
            return r[i - 1]
        a, b, c = r[i - 1], r[i - 2], r[i - 3]
        return (a & b) | (a & c) | (b & c)
    if mode == 5:
        if i == 0:
            return 0
        d = r[i - 1]
        m = _ero(_dil(d)) if (param & 1) == 0 else _dil(_ero(d))
        e = _dil(d) ^ _ero(d)
        return (m & e) | (d & ~e & 0xFF)
    return 0


def forward(mode, param, data):
    return bytes(data[i] ^ predictor(mode, param, i, data) for i in range(len(data)))


def header(mode, param, raw_mask, b1_mask, ks):
    pb = b"" if param == 0 else param.to_bytes((param.bit_length() + 7) // 8, "little")
    return bytes([(mode << 5) | len(pb)]) + pb + bytes([raw_mask, b1_mask]) + bytes(ks)


def planes_of(mapped):
    """[8][n] 0/1 arrays: plane j = bit 7 - j of every mapped byte."""
    a = np.frombuffer(mapped, dtype=np.uint8)
    return [((a >> (7 - j)) & 1).astype(np.uint8) for j in range(8)]


def raw_plane(bits):
    return np.packbits(bits).tobytes()


def runs_of(L):
    """(first bit, run lengths) of a 0/1 array."""
    L = np.asarray(L, dtype=np.uint8)
    cut = np.flatnonzero(np.diff(L)) + 1
    edges = np.concatenate([[0], cut, [L.size]])
    return int(L[0]), [int(x) for x in np.diff(edges)]


def rice_bits(runs, k):
    out = []
    for v in runs:
        out.append("1" * (v >> k) + "0")
        if k:
            out.append(format(v & ((1 << k) - 1), "b").zfill(k))
    return "".join(out)


def bits_to_bytes(s):
    s += "0" * (-len(s) % 8)
    return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


def raw_payload(mode, param, data):
    """All eight planes raw: only the automaton inverse is left to the decoder."""
    return header(mode, param, 0xFF, 0x00, []) + b"".join(raw_plane(p) for p in planes_of(forward(mode, param, data)))


def rice_payload(mode, param, data, ks, raw_mask=0):
    """Planes with raw_mask bit clear: runs of the oracle's BBWT of the plane, Rice coded with
    the next k of ks."""
    import oracle
    body, b1, used = b"", 0, []
    ks = list(ks)
    for j, p in enumerate(planes_of(forward(mode, param, data))):
        if (raw_mask >> j) & 1:
            body += raw_plane(p)
            continue
        L = np.frombuffer(oracle.bbwt_forward(p.tobytes()), dtype=np.uint8)
        first, runs = runs_of(L)
        b1 |= first << j
        k = ks.pop(0)
        used.append(k)
        body += bits_to_bytes(rice_bits(runs, k))
    return header(mode, param, raw_mask, b1, used) + body


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def automaton_cases():
    """190 all-raw blocks: every (mode, param) x every size, and six whose length passes the
    automaton kernel's tile lengths by one."""
    cases = []
    for mi, (mode, param) in enumerate(AUTOMATA):
        for n in SIZES:
            data = _rand(n, 1000 * mi + n)
            cases.append((f"m{mode}p{param}n{n}", raw_payload(mode, param, data), data))
    # lengths one past the automaton kernel's tiles: 256 threads x 16 bytes (15 for stride 3, 14
    # for stride 7) in the scan modes, 4096 bytes for long strides and the serial modes
    for mode, param, n in ((1, 1, 4097), (1, 3, 2 * 3840 + 1), (1, 7, 3584 + 1), (1, 300, 2 * AUTO_TILE + 1),
                           (3, 0, 2 * AUTO_TILE + 1), (4, 0, 2 * AUTO_TILE + 1)):
        data = _rand(n, 77 + mode + param)
        cases.append((f"m{mode}p{param}tile{n}", raw_payload(mode, param, data), data))
    return cases


def tile_case():
    """Plane 0 (k = 3) laid out against the parse tile: a unary run over the first tile
    boundary, a remainder field over the second, and the plane's padded end exactly on the
    third, where plane 1 (k = 0: one unary run of n ones, several tiles long) starts; plane 2
    is one k = 15 codeword, planes 3..7 raw.  The run lengths are chosen, not derived from data:
    returns (payload, n) and the expected bytes are the host decoder's."""
    T = PARSE_TILE_BITS
    runs = [1] * ((T - 8) // 4)                    # 4-bit codewords up to bit T - 8
    runs.append((10 << 3) | 2)                     # ones at T - 8 .. T + 1
    assert len(rice_bits(runs, 3)) == T + 6
    runs += [1] * ((T - 8) // 4)                   # to bit 2T - 2
    runs.append(5)                                 # its zero at 2T - 2, remainder at 2T - 1 .. 2T + 1
    assert len(rice_bits(runs, 3)) == 2 * T + 2
    runs += [1] * ((T - 4) // 4)                   # to bit 3T - 2: padded to 3T
    p0 = bits_to_bytes(rice_bits(runs, 3))
    assert len(p0) * 8 == 3 * T
    n = sum(runs)
    p1 = bits_to_bytes(rice_bits([n], 0))
    p2 = bits_to_bytes(rice_bits([n], 15))
    rng = np.random.default_rng(5)
    raws = b"".join(raw_plane(rng.integers(0, 2, n, dtype=np.uint8)) for _ in range(5))
    return header(2, 2, 0xF8, 0b101, [3, 0, 15]) + p0 + p1 + p2 + raws, n


@functools.lru_cache(maxsize=None)
def rice_cases():
    """Rice planes by hand: (name, payload, data)."""
    from kolm import decode as H
    rng = np.random.default_rng(11)
    small = rng.integers(0, 4, 5000, dtype=np.uint8).tobytes()
    cases = [
        ("n1_k0", rice_payload(0, 0, b"\x5a", [0] * 8), b"\x5a"),
        ("zeros700", rice_payload(0, 0, bytes(700), [0, 15, 1, 2, 3, 7, 11, 4]), bytes(700)),
        ("small5000", rice_payload(1, 1, small, [0, 0, 0, 0, 15, 15, 9, 5]), small),
        ("mixed_raw", rice_payload(4, 0, small[:1234], [2, 6, 1], raw_mask=0b01011011), small[:1234]),
    ]
    pay, n = tile_case()
    cases.append(("tile_edges", pay, H.decode_new_pipeline(pay, n)))
    return cases


def k16_block():
    """(payload, data): plane 0 is one run of 4 coded with k = 16, planes 1..7 raw zeros."""
    return b"\x00\xfe\x00\x10" + bits_to_bytes(rice_bits([4], 16)) + bytes(7), bytes(4)
