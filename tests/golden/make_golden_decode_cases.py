#!/usr/bin/env python3
"""Decoder conformance corpus: hand-structured payloads and what the Python reference makes of them.

PY = /root/reference/final_researched/kolm_final_researched_v2-2.py (read-only), run ONLY in
the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_decode_cases.py

Writes tests/golden/decode_cases.json (data only): a list of cases, each

    {"name", "class", "mid", "n", "payload": hex,
     "py": {"ok": hex} | {"ok_zlib": base64 of zlib, outputs past 64 bytes} | {"error", "message"} | "hang"}

where "py" is what PY's own block decoder (_select_decoders()[mid], PY:2194-2207) returns or
raises for (payload, n), or "hang" when it has not returned within the wall-clock guard below.
The payloads are streams the encoders never write: built here by hand and with the oracle's
rice_encode / mtf_encode / uleb128, never by a device encoder.  They aim at the edges of the
device decoders (csrc/k_decode.hip): ULEB widths, the 8-byte and 2048-byte steps of the xor /
lfsr kernel, LZ77 tokens that produce nothing, the Rice word walk at every bit offset, MTF
chunk and inverse-BBWT tile edges.  Every payload is at most 8 KiB.

The corpus must be mostly streams PY decodes: at least 60 % of every method's cases, and at
least one case of every class.  tests/test_decode_conformance.py and
tests/test_gpu_decode_conformance.py read the JSON.
"""
from __future__ import annotations

import base64
import json
import os
import random
import signal
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.dont_write_bytecode = True

from make_golden import load_reference  # noqa: E402
import oracle as O  # noqa: E402

GUARD_S = 1.0          # PY has this long per case
MAX_PAYLOAD = 8 << 10
HANGS = {"repair/used_cycle"}  # the only cases PY may not finish

CASES = []


def add(cls, name, mid, n, payload):
    payload = bytes(payload)
    assert len(payload) <= MAX_PAYLOAD, (name, len(payload))
    full = f"{cls}/{name}"
    assert all(c["name"] != full for c in CASES), full
    CASES.append({"name": full, "class": cls, "mid": mid, "n": n, "payload": payload})


U = O.uleb128


def uw(v, width):
    """v as a ULEB128 of exactly `width` bytes (overlong when v needs fewer)."""
    out = bytearray(((v >> (7 * i)) & 0x7F) | 0x80 for i in range(width))
    out[-1] &= 0x7F
    assert v >> (7 * width) == 0
    return bytes(out)


# ------------------------------------------------------------------ raw
def raw_cases():
    for n in (0, 1, 7, 300):
        add("raw_length", f"exact_{n}", 0, n, bytes((i * 37 + 1) & 0xFF for i in range(n)))
    add("raw_length", "one_short", 0, 5, b"abcd")
    add("raw_length", "one_long", 0, 5, b"abcdef")


# ------------------------------------------------------------------ xor / lfsr
def value_stream(vals, widths=None):
    return b"".join(uw(v, widths[i]) if widths and widths[i] else U(v) for i, v in enumerate(vals))


def uleb_cases(mid, tag):
    rnd = random.Random(100 + mid)
    edge = [0, 127, 128, 255, 256, 383, 1 << 14]
    add(f"{tag}_values", "edge_values", mid, len(edge), value_stream(edge))
    add(f"{tag}_values", "edge_values_twice", mid, 2 * len(edge), value_stream(edge + edge[::-1]))
    add(f"{tag}_values", "overlong_80_00", mid, 3, b"\x05" + b"\x80\x00" + b"\x07")
    add(f"{tag}_values", "three_byte", mid, 3, b"\x05" + uw(0x1234, 3) + b"\x81\x01")
    add(f"{tag}_values", "six_byte", mid, 3, uw(200, 6) + b"\x09" + uw((1 << 41) + 77, 6))
    add(f"{tag}_values", "ten_byte_2_pow_63", mid, 2, uw((1 << 63) + 5, 10) + b"\x01")
    add(f"{tag}_values", "80_02_05", mid, 2, b"\x80\x02\x05")
    # a two-byte value across the 8-bytes-per-thread edge and across the 2048-byte step edge:
    # one-byte values up to payload offset 7 (2047), then the two bytes at 7/8 (2047/2048)
    for at in (7, 2047):
        # (the one-byte values repeat with period 24 so that PY's long output compresses)
        vals = [(i % 24) * 5 for i in range(at)] + [128 + rnd.randrange(128)] + [rnd.randrange(128) for _ in range(9)]
        pay = value_stream(vals)
        assert pay[at] >= 128 and pay[at + 1] < 128 and all(b < 128 for b in pay[:at])
        add(f"{tag}_edges", f"straddle_{at}", mid, len(vals), pay)
        if at == 7:  # and a three-byte value with its middle byte on the edge
            vals3 = vals[:at - 1] + [vals[at]] + vals[at + 1:]
            w = [0] * len(vals3)
            w[at - 1] = 3
            add(f"{tag}_edges", f"straddle3_{at}", mid, len(vals3), value_stream(vals3, w))
    ns = [0, 1, 255, 256, 2049] + ([254, 511] if mid == 8 else [])
    for n in ns:
        vals = [rnd.randrange(256) for _ in range(n)]
        add(f"{tag}_lengths", f"n_{n}", mid, n, value_stream(vals))
    vals = [rnd.randrange(256) for _ in range(20)]
    good = value_stream(vals)
    add(f"{tag}_trailing", "one_byte", mid, 20, good + b"\x00")
    add(f"{tag}_trailing", "a_value_more", mid, 19, good)
    add(f"{tag}_trailing", "unfinished_value", mid, 20, good + b"\x85")
    add(f"{tag}_trailing", "none", mid, 20, good)
    add(f"{tag}_trailing", "n_0_with_payload", mid, 0, b"\x05")
    add(f"{tag}_short", "too_few_values", mid, 21, good)
    add(f"{tag}_short", "last_byte_128", mid, 21, good + b"\x80")
    add(f"{tag}_short", "last_value_wide_unfinished", mid, 21, good + b"\x81\x80\x80")
    add(f"{tag}_short", "empty_payload", mid, 1, b"")
    add(f"{tag}_short", "complete", mid, 21, good + b"\x81\x80\x00")
    add(f"{tag}_short", "complete_2", mid, 22, good + b"\x81\x01\x7f")
    add(f"{tag}_short", "complete_3", mid, 1, b"\xff\x01")


# ------------------------------------------------------------------ lz77
def lit(b):
    return bytes((0, b))


def cp(length, dist):
    return b"\x01" + U(length) + U(dist)


def lits(rnd, k):
    return b"".join(lit(rnd.randrange(256)) for _ in range(k))


def lz_cases():
    rnd = random.Random(7)
    A, B = lit(0x41), lit(0x42)
    z = cp(0, 1)
    add("lz_zero_copy", "mid_stream", 7, 2, A + z + B)
    add("lz_zero_copy", "fifty_in_n2", 7, 2, A + z * 50 + B)
    add("lz_zero_copy", "two_hundred_in_n3", 7, 3, A + z * 200 + B + cp(1, 2))
    add("lz_zero_copy", "before_literal", 7, 3, A + B + z + lit(0x43))
    add("lz_zero_copy", "before_final_cut_copy", 7, 6, A + B + cp(0, 2) + cp(100, 2))
    add("lz_zero_copy", "after_output_full", 7, 2, A + B + z)
    add("lz_zero_copy", "between_copies", 7, 9, A + B + cp(3, 2) + cp(0, 5) + cp(4, 1))
    add("lz_zero_copy", "dist_0", 7, 2, A + cp(0, 0) + B)
    add("lz_zero_copy_far", "at_output_0", 7, 1, z + A)
    add("lz_zero_copy_far", "dist_past_output", 7, 3, A + B + cp(0, 3) + A)
    add("lz_zero_copy_far", "dist_4097_at_5000", 7, 5001, A + cp(4999, 1) + cp(0, 4097) + B)
    add("lz_wide_uleb", "length_2_pow_32", 7, 9, A + b"\x01\x80\x80\x80\x80\x10\x01")
    add("lz_wide_uleb", "length_2_pow_32_plus_3", 7, 9, A + b"\x01\x83\x80\x80\x80\x10\x01")
    add("lz_wide_uleb", "length_2_pow_70", 7, 9, A + b"\x01" + uw(1 << 70, 11) + b"\x01")
    add("lz_wide_uleb", "overlong_length_6_bytes", 7, 4, A + b"\x01" + uw(3, 6) + b"\x01")
    add("lz_wide_uleb", "overlong_distance_6_bytes", 7, 4, A + b"\x01\x03" + uw(1, 6))
    add("lz_wide_uleb", "distance_2_pow_35_plus_1", 7, 4, A + b"\x01\x03" + uw((1 << 35) + 1, 6))
    add("lz_wide_uleb", "distance_2_pow_32_plus_1", 7, 4, A + b"\x01\x03" + uw((1 << 32) + 1, 5))
    add("lz_wide_uleb", "length_2_pow_32_mid_stream", 7, 3, A + cp(1 << 32, 1))
    add("lz_ends", "copy_cut_at_orig_len", 7, 5, A + B + cp(1000, 2))
    add("lz_ends", "trailing_tokens", 7, 2, A + B + lit(0x43) + cp(5, 1))
    add("lz_ends", "trailing_garbage", 7, 2, A + B + b"\x07\xff\x80")
    add("lz_ends", "short_output", 7, 3, A + B)
    add("lz_ends", "n_0_empty", 7, 0, b"")
    add("lz_ends", "n_0_with_payload", 7, 0, b"\x02\x02")
    add("lz_ends", "exact", 7, 4, A + B + cp(2, 2))
    head = lits(rnd, 40)
    for o in (4096, 5000):
        fill = head + cp(o - 40, 40)
        add("lz_window", f"dist_4096_at_{o}", 7, o + 3, fill + cp(3, 4096))
        add("lz_window", f"dist_4097_at_{o}", 7, o + 3, fill + cp(3, 4097))
    add("lz_window", "dist_o_at_4095", 7, 4100, head + cp(4055, 40) + cp(5, 4095))
    add("lz_window", "dist_o_plus_1_at_100", 7, 110, head + cp(60, 40) + cp(10, 101))
    for n in (1025, 4097):
        for d in (1, 2, 3):
            add("lz_runs", f"dist_{d}_n_{n}", 7, n, lits(rnd, d) + cp(n - d, d))
    # runs in pieces: every copy sources the copy before it (pointer-jumping depth)
    pay, o = lits(rnd, 3), 3
    while o < 1200:
        step = 1 + (o * 7) % 5
        pay += cp(step, min(o, 1 + (o * 3) % 4))
        o += step
    add("lz_chain", "copies_of_copies", 7, o, pay)
    pay, o = lits(rnd, 16), 16
    for _ in range(100):
        pay += cp(16, 16)
        o += 16
    add("lz_chain", "chain_of_100", 7, o, pay)
    pay, o = lits(rnd, 1), 1
    while o < 2048:  # doubling: each copy sources everything before it
        pay += cp(o, o)
        o *= 2
    add("lz_chain", "doubling", 7, o, pay)
    add("lz_malformed", "copy_first", 7, 3, cp(3, 1))
    add("lz_malformed", "unknown_flag", 7, 2, A + b"\x02\x41")
    add("lz_malformed", "unknown_flag_ff", 7, 2, A + b"\xff")
    add("lz_malformed", "truncated_literal", 7, 2, A + b"\x00")
    add("lz_malformed", "truncated_length", 7, 3, A + b"\x01\x80")
    add("lz_malformed", "truncated_distance", 7, 3, A + b"\x01\x02\x81")
    add("lz_malformed", "no_distance", 7, 3, A + b"\x01\x02")
    add("lz_malformed", "flag_only", 7, 3, A + b"\x01")
    for name, pay, n in (("well_formed", A + cp(2, 1), 3), ("well_formed_2", A + B + cp(1, 2) + B, 4),
                         ("well_formed_3", lits(rnd, 9), 9), ("well_formed_4", A + cp(7, 1) + B, 9),
                         ("well_formed_5", A + B + cp(4, 1) + cp(2, 6), 8)):
        add("lz_malformed", name, 7, n, pay)


# ------------------------------------------------------------------ Rice family (ids 2..6)
def code(v):
    return "1" * (v >> 2) + "0" + f"{v & 3:02b}"


def pack(bits, pad="0"):
    bits += pad * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def rice(vals):
    return pack("".join(code(v) for v in vals))


def filler(nbits):
    """Codewords of 3 and 4 bits (values 0..7) filling exactly nbits (not 1, 2 or 5)."""
    b = 0
    while (nbits - 4 * b) % 3:
        b += 1
    a = (nbits - 4 * b) // 3
    assert a >= 0
    return [i & 3 for i in range(a)] + [4 + (i & 3) for i in range(b)]


def interleave(seq):
    seq = bytes(seq) + bytes(-len(seq) % 8)
    out = bytearray()
    for g in range(0, len(seq), 8):
        for bit in range(8):
            out.append(sum(((seq[g + i] >> (7 - bit)) & 1) << (7 - i) for i in range(8)))
    return bytes(out)


def rice_cases():
    rnd = random.Random(11)
    every = list(range(256))
    rnd.shuffle(every)
    assert rice(every) == O.rice_encode(bytes(every), 2)
    add("rice_all_values", "shuffled_256", 2, 256, rice(every))
    add("rice_all_values", "low_ranks_descending", 2, 40, rice(range(39, -1, -1)))
    for mid in (4, 5, 6):
        add("rice_inverse_maps", f"every_byte_id{mid}", mid, 256, rice(every))
        add("rice_inverse_maps", f"short_id{mid}", mid, 5, rice([0x80, 0x01, 0x0F, 0xF0, 0x55]))
        add("rice_inverse_maps", f"nibbles_id{mid}", mid, 16, rice([(i * 0x11) ^ (i >> 1) for i in range(16)]))
    # q = 62 / 63 codewords starting at every bit offset of a 64-bit word: one stream per value,
    # 64 codewords of 65 bits back to back (q = 62: the start moves by 1 mod 64), or of 66 bits
    # with a 3-bit value between them (q = 63: by 69 = 5 mod 64); then a few alone
    for v in range(248, 256):
        bits, starts, vals = "", set(), []
        for i in range(64):
            starts.add(len(bits) % 64)
            bits += code(v)
            vals.append(v)
            if v >= 252:
                bits += code(i & 3)
                vals.append(i & 3)
        assert starts == set(range(64)) and bits == "".join(map(code, vals))
        add("rice_long_unary", f"value_{v}_at_every_bit_offset", 2, len(vals), pack(bits))
    for s in (0, 1, 7, 31, 32, 61, 62, 63):
        pre = filler(s if s not in (1, 2, 5) else s + 64)
        vals = pre + [248 + (s * 3) % 8, 1, 6]
        add("rice_long_unary", f"value_{vals[-3]}_alone_at_bit_{s}", 2, len(vals), rice(vals))
    add("rice_long_unary", "two_words_of_255", 2, 9, rice([255] * 8 + [3]))
    add("rice_long_unary", "ends_the_payload", 2, 3, pack(code(2) + code(5) + code(255), pad="1"))
    for s in (0, 1, 13, 63):  # a 64-ones run: value 256, no byte
        pre = filler(s if s not in (1, 2, 5) else s + 64)
        add("rice_long_unary", f"run_of_64_at_bit_{s}", 2, len(pre) + 2, pack("".join(map(code, pre)) + "1" * 64 + "000" + code(1)))
    add("rice_long_unary", "run_of_130", 2, 2, pack("1" * 130 + "000" + code(1)))
    add("rice_long_unary", "all_ones_16_bytes", 2, 4, b"\xff" * 16)
    # payloads of 1..17 bytes (the aligned 16-byte load of the word reader needs 16 bytes past B)
    for nbytes in range(1, 18):
        vals, used = [], 0
        while True:
            v = rnd.choice([0, 1, 2, 3, 5, 6, 9, 14, 21])
            if used + len(code(v)) > 8 * nbytes:
                break
            vals.append(v)
            used += len(code(v))
        add("rice_payload_lengths", f"bytes_{nbytes}", 2, len(vals), rice(vals)[:nbytes] + bytes(nbytes - len(rice(vals))))
    vals = [rnd.choice([0, 1, 2, 3, 4, 9, 33]) for _ in range(41)]
    bits = "".join(map(code, vals))
    add("rice_padding", "zeros", 2, 41, pack(bits))
    add("rice_padding", "ones", 2, 41, pack(bits, pad="1"))
    add("rice_padding", "more_codewords", 2, 41, pack(bits + code(7) + code(0) + code(200)))
    add("rice_padding", "garbage_bytes", 2, 41, pack(bits) + bytes(rnd.randrange(256) for _ in range(40)))
    add("rice_padding", "ones_run_after_last_value", 2, 41, pack(bits) + b"\xff" * 24)
    add("rice_padding", "n_0_with_payload", 2, 0, b"\xff\x00")
    add("rice_padding", "n_0_empty", 2, 0, b"")
    # the stream ends inside the last codeword: 1 remainder bit short, 2 short, inside the unary run
    body = filler(3 * 8 - 6) + [1]
    full = "".join(map(code, body))           # 21 bits
    last = code(9)                              # 110 01 -> bits 21..25
    assert len(full + last) == 26
    add("rice_truncated", "complete", 2, len(body) + 1, pack(full + last))
    assert len(full + last[:3]) == 24
    add("rice_truncated", "both_remainder_bits_short", 2, len(body) + 1, pack(full + last[:3]))
    body2 = filler(3 * 8 - 4 - 3) + [1]
    add("rice_truncated", "one_remainder_bit_short", 2, len(body2) + 1, pack("".join(map(code, body2)) + code(9)[:4]))
    add("rice_truncated", "inside_unary", 2, len(body) + 1, pack(full + "111"))
    add("rice_truncated", "a_value_missing", 2, len(body) + 2, pack(full + last))
    add("rice_truncated", "empty_payload", 2, 1, b"")
    add("rice_truncated", "complete_2", 2, len(body2) + 1, pack("".join(map(code, body2)) + code(9)))
    add("rice_truncated", "complete_3", 2, 1, pack(code(0)))
    add("rice_truncated", "complete_4", 2, 2, pack(code(255) + code(255)))
    # id 3: n % 8 = 0, 1, 7 (the encoder writes 8 * ceil(n / 8) values)
    for n in (8, 16, 24, 32, 40, 48, 64, 256, 1024, 1, 7, 9, 15, 1025):
        ranks = [rnd.choice([0, 0, 0, 1, 2, 3, 7, 40]) for _ in range(n)]
        add("rice_bitplane", f"n_{n}", 3, n, rice(interleave(ranks)))
    add("rice_bitplane", "n_8_unpadded_count", 3, 9, rice(interleave([1, 2, 3, 0, 0, 1, 0, 2])))
    # MTF ranks at the replay's table-word edges (entries 0..3 / 4..7 in registers, 8.. in LDS),
    # repeated (runs of 12) and alternated with the next rank (6 pairs), across MTF chunk edges
    # (1024); the second order puts other runs on the edges.  Rank 255 costs 66 bits: its runs are
    # 3 long and its alternations 2 pairs, so that the payloads stay small.
    for tag, order in (("a", [3, 4, 7, 8, 11, 12, 255]), ("b", [12, 255, 8, 3, 11, 4, 7])):
        unit = []
        for r, nxt in zip(order, order[1:] + order[:1]):
            unit += [r] * (3 if r == 255 else 12) + [r, nxt] * (2 if 255 in (r, nxt) else 6)
        for n in (1023, 1024, 1025, 2049):
            add("rice_mtf_ranks", f"runs_and_pairs_{tag}_n_{n}", 2, n, rice((unit * (n // len(unit) + 1))[:n]))
    add("rice_mtf_ranks", "rep_255_n_100", 2, 100, rice([255] * 100))
    # BBWT strings no forward transform produces, at the inverse's tile edge (4096)
    for n in (4095, 4096, 4097):
        L = bytes(rnd.choice(b"abcd") for _ in range(n))
        add("rice_bbwt_strings", f"random_4_symbols_n_{n}", 2, n, O.rice_encode(O.mtf_encode(L), 2))
    for n in (1000, 4097):
        # the stable sort of L is the permutation x -> x + 1 mod n: one n-cycle
        L = bytearray(n)
        L[0] = 1
        add("rice_bbwt_strings", f"single_cycle_n_{n}", 2, n, O.rice_encode(O.mtf_encode(bytes(L)), 2))
        L = bytes(sorted(rnd.choice(b"\x00\x07\x80\xff") for _ in range(n)))  # sorted: every slot a fixed point
        add("rice_bbwt_strings", f"fixed_points_n_{n}", 2, n, O.rice_encode(O.mtf_encode(L), 2))


# ------------------------------------------------------------------ repair
def rp(rules, seq):
    body = b"".join(U(x) + U(y) for x, y in rules)
    return b"RP" + U(256) + U(len(rules)) + body + U(len(seq)) + b"".join(U(s) for s in seq)


def repair_cases():
    add("repair_forward", "reference", 9, 5, rp([(257, 67), (65, 66)], [256, 257]))
    add("repair_forward", "chain", 9, 7, rp([(258, 257), (65, 66), (259, 67), (68, 69)], [256, 257]))
    add("repair_cycles", "unused_undefined_symbol", 9, 2, rp([(65, 66), (999, 65)], [256]))
    add("repair_cycles", "unused_cycle", 9, 4, rp([(65, 66), (258, 65), (257, 66)], [256, 256]))
    add("repair", "used_cycle", 9, 4, rp([(257, 65), (256, 66)], [256]))
    CASES[-1]["class"] = "repair_cycles"


# ------------------------------------------------------------------ PY's verdict
class Hang(Exception):
    pass


def verdict(dec, c):
    def on_alarm(signum, frame):
        raise Hang()
    signal.signal(signal.SIGALRM, on_alarm)
    signal.setitimer(signal.ITIMER_REAL, GUARD_S)
    try:
        out = bytes(dec[c["mid"]](c["payload"], c["n"], None))
        if len(out) <= 64:
            return {"ok": out.hex()}
        return {"ok_zlib": base64.b64encode(zlib.compress(out, 9)).decode()}  # long outputs: zlib, base64
    except Hang:
        return "hang"
    except Exception as e:  # noqa: BLE001 — the fixture records whatever PY raises
        return {"error": type(e).__name__, "message": str(e)}
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)


def main():
    py = load_reference()
    dec = py._select_decoders()
    raw_cases()
    uleb_cases(1, "xor")
    uleb_cases(8, "lfsr")
    lz_cases()
    rice_cases()
    repair_cases()
    for c in CASES:
        c["py"] = verdict(dec, c)
        c["payload"] = c["payload"].hex()
    ok = lambda c: isinstance(c["py"], dict) and ("ok" in c["py"] or "ok_zlib" in c["py"])  # noqa: E731
    assert {c["name"] for c in CASES if c["py"] == "hang"} == HANGS
    for mid in sorted({c["mid"] for c in CASES}):
        mine = [c for c in CASES if c["mid"] == mid]
        good = sum(map(ok, mine))
        print(f"method {mid}: {len(mine)} cases, PY decodes {good}")
        assert good >= 0.6 * len(mine), mid
    for cls in sorted({c["class"] for c in CASES}):
        assert any(ok(c) for c in CASES if c["class"] == cls), cls
    path = os.path.join(HERE, "decode_cases.json")
    with open(path, "w") as f:  # one case per line
        f.write("[\n" + ",\n".join(json.dumps(c, sort_keys=True) for c in CASES) + "\n]\n")
    print(len(CASES), "cases,", os.path.getsize(path), "bytes")
    for c in CASES:
        if not ok(c):
            print(c["name"], c["mid"], c["py"])


if __name__ == "__main__":
    main()
