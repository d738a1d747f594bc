#!/usr/bin/env python3
"""CPU model of the round-0 key forms of the cyclic sort: the share of a block's
positions still tied (active) when each prefix-doubling round starts, for
  fixed : C fixed-width rank codes + the partial next character (k_keypos_r0), h0 = C
  code  : 64 bits of the order-preserving prefix-code stream (alpha_code.h, k_keypos_r0c), h0 = 8
The text is treated as linear (no Lyndon-factor wrap; past the end the stream is zero bits), and
the code builder below restates alpha_code.h (same sample, same split rule, same clip and padding).

  python tools/r0_code_model.py [--kib 1024] [--seed 20251212] [--maxlen 8] [--keybits 64]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kolmogorovlike-datacompressor_amd"))
from kolm import datagen  # noqa: E402


def build_code(present, wts, maxlen=8, minlen=2):
    """bits[256], len[256] of the weight-balanced alphabetic code (alpha_code.h)."""
    syms = [c for c in range(256) if present[c]]
    cum = [0]
    for c in syms:
        cum.append(cum[-1] + (int(wts[c]) or 1))
    bits, lens = [0] * 256, [0] * 256
    nodes = {1: (0, len(syms))}
    for d in range(maxlen + 1):
        for nid in range(1 << d, 2 << d):
            if nid not in nodes:
                continue
            lo, hi = nodes[nid]
            if hi - lo == 1:
                ln = max(d, minlen)
                lens[syms[lo]] = ln
                bits[syms[lo]] = (nid - (1 << d)) << (ln - d)
                continue
            cap = 1 << (maxlen - d - 1)
            tot = cum[hi] - cum[lo]
            s = next(k for k in range(lo + 1, hi + 1) if 2 * (cum[k] - cum[lo]) >= tot)
            if s > lo + 1 and tot - 2 * (cum[s - 1] - cum[lo]) <= 2 * (cum[s] - cum[lo]) - tot:
                s -= 1
            s = min(max(s, hi - cap, lo + 1), lo + cap, hi - 1)
            nodes[2 * nid], nodes[2 * nid + 1] = (lo, s), (s, hi)
    return np.array(bits, np.uint64), np.array(lens, np.uint64)


def sample_weights(t):
    """Every 16th 16-byte chunk from the block's base (k_alpha_weights)."""
    idx = np.arange(len(t))
    return np.bincount(t[(idx & 0xF0) == 0], minlength=256)


def keys_code(t, maxlen, keybits):
    present = np.bincount(t, minlength=256) > 0
    bits, lens = build_code(present, sample_weights(t), maxlen)
    ln = lens[t].astype(np.int64)
    off = np.concatenate(([0], np.cumsum(ln)))
    total = int(off[-1])
    stream = np.zeros(total + 128, np.uint8)
    for k in range(maxlen):  # bit k (from the top) of every code that has one
        m = ln > k
        stream[off[:-1][m] + k] = ((bits[t][m] >> (lens[t][m] - np.uint64(k + 1))) & np.uint64(1)).astype(np.uint8)
    by = np.packbits(stream)
    o = off[:-1]
    b0, s = o >> 3, (o & 7).astype(np.uint64)
    hi = np.zeros(len(t), np.uint64)
    for k in range(8):
        hi = (hi << np.uint64(8)) | by[b0 + k].astype(np.uint64)
    key = (hi << s) | (by[b0 + 8].astype(np.uint64) >> (np.uint64(8) - s))
    if keybits < 64:
        key >>= np.uint64(64 - keybits)
    return key, float(ln.mean())


def keys_fixed(t):
    present = np.bincount(t, minlength=256) > 0
    rank = (np.cumsum(present) - 1).astype(np.uint64)
    sigma = int(present.sum())
    w = max(1, (sigma - 1).bit_length())
    C = max(1, min(32, 64 // w))
    part = min(64 - C * w, w)
    c = np.concatenate((rank[t], np.zeros(C + 1, np.uint64)))
    key = np.zeros(len(t), np.uint64)
    for k in range(C):
        key = (key << np.uint64(w)) | c[k:k + len(t)]
    if part:
        key = (key << np.uint64(part)) | (c[C:C + len(t)] >> np.uint64(w - part))
    return key, C


def shares(key, h0, rounds=3):
    """Share of the positions in groups of two or more when the round of each h starts."""
    n = len(key)
    _, g = np.unique(key, return_inverse=True)
    out = []
    h = h0
    for _ in range(rounds):
        cnt = np.bincount(g)
        out.append(float((cnt[g] > 1).sum()) / n)
        g2 = np.concatenate((g[h:] + 1, np.zeros(min(h, n), np.int64)))[:n]
        _, g = np.unique(g.astype(np.int64) * (n + 2) + g2, return_inverse=True)
        h *= 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kib", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=20251212)
    ap.add_argument("--maxlen", type=int, default=8)
    ap.add_argument("--keybits", type=int, default=64)
    a = ap.parse_args()
    t = np.frombuffer(datagen.enwik_like(a.kib << 10, seed=a.seed), np.uint8)
    kf, C = keys_fixed(t)
    sf = shares(kf, C)
    kc, avg = keys_code(t, a.maxlen, a.keybits)
    h0 = a.keybits // a.maxlen
    sc = shares(kc, h0)
    print(f"block {a.kib} KiB, seed {a.seed}: {int((np.bincount(t, minlength=256) > 0).sum())} symbols, "
          f"mean code length {avg:.2f} bits ({a.keybits / avg:.1f} characters per key)")
    print(f"fixed  h0={C:2d}: " + " ".join(f"{x:.3f}" for x in sf) + f"  sum {sum(sf):.3f}")
    print(f"code   h0={h0:2d}: " + " ".join(f"{x:.3f}" for x in sc) + f"  sum {sum(sc):.3f}")


if __name__ == "__main__":
    main()
