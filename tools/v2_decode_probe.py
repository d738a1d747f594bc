#!/usr/bin/env python3
"""Device time of the v2_new (id 10) decoder against the id-2 decoder on the same blocks.

One process: 32 x 1 MiB enwik_like blocks, encoded forced to id 10 and forced to id 2, decoded
with kolm_decode_blocks_device (its `ms`: HIP events around the decode kernels), 3 warm-ups and
10 timed runs of each, alternating.  The id-2 decode is the yardstick.  For each of the 13
automaton kinds the encoder can select, an all-raw payload of the same blocks is timed too: no
Rice parse and no inverse BBWT, so what is left is the plane pack and the automaton inverse.
Writes min / median / max ms, MB/s and the ratios to profiles/r08/v2_decode.json (--out).

    python tools/v2_decode_probe.py [--blocks 32] [--block-size 1048576] [--runs 10] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "kolmogorovlike-datacompressor_amd"))

from kolm import _lib, datagen  # noqa: E402

KINDS = [(0, 0), (1, 1), (1, 2), (1, 3), (1, 4), (2, 0), (2, 1), (2, 2), (2, 3), (3, 0), (4, 0), (5, 0), (5, 1)]


def _dil(x):
    return (x << 1) | x | (x >> 1)


def forward(mode, param, r):
    """The automaton's forward map of one block (uint8 array), vectorised: every model is
    y[i] = r[i] ^ predictor(r[i-1], r[i-2], r[i-3])."""
    n = r.size
    a = np.concatenate([[0], r[:-1]]).astype(np.uint8)
    b = np.concatenate([[0, 0], r[:-2]]).astype(np.uint8)[:n]
    c = np.concatenate([[0, 0, 0], r[:-3]]).astype(np.uint8)[:n]
    if mode == 0:
        p = np.zeros(n, np.uint8)
    elif mode == 1:
        p = np.concatenate([np.zeros(param, np.uint8), r[:-param]])[:n]
    elif mode == 2:
        x = (a, b, a ^ b, a | b)[param & 3]
        p = x ^ (x >> 1)
        p[:2] = a[:2]
    elif mode == 3:
        p = (a & 0xF0) | (b & 0x0F)
        p[:2] = a[:2]
    elif mode == 4:
        p = (a & b) | (a & c) | (b & c)
        p[:3] = a[:3]
    else:
        dil, ero = _dil(a), ~_dil(~a)
        m = ~_dil(~dil) if (param & 1) == 0 else _dil(ero)
        e = dil ^ ero
        p = (m & e) | (a & ~e)
    return r ^ p.astype(np.uint8)


def raw_payload(mode, param, blk):
    y = forward(mode, param, np.frombuffer(blk, dtype=np.uint8))
    pb = b"" if param == 0 else param.to_bytes((param.bit_length() + 7) // 8, "little")
    planes = b"".join(np.packbits((y >> (7 - j)) & 1).tobytes() for j in range(8))
    return bytes([(mode << 5) | len(pb)]) + pb + b"\xff\x00" + planes


class DeviceDecode:
    def __init__(self, ctx, L, payloads, mids, lens):
        self.ctx, self.L = ctx, L
        arena = b"".join(payloads)
        self.off = np.zeros(len(payloads) + 1, np.uint64)
        self.off[1:] = np.cumsum([len(p) for p in payloads])
        self.meth = np.asarray(mids, np.uint32)
        self.lens = np.asarray(lens, np.uint32)
        self.total = int(self.lens.sum())
        self.dp, self.do = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.kolm_dev_alloc(ctx, len(arena) + 64, ctypes.byref(self.dp)))
        _lib.check(L.kolm_dev_alloc(ctx, self.total + 64, ctypes.byref(self.do)))
        _lib.check(L.kolm_memcpy_h2d(ctx, self.dp, arena, len(arena)))

    def run(self):
        ms = ctypes.c_double(0.0)
        _lib.check(self.L.kolm_decode_blocks_device(self.ctx, self.dp, self.off.ctypes.data, self.meth.ctypes.data,
                                                    self.lens.ctypes.data, len(self.lens), self.do, self.total,
                                                    ctypes.byref(ms)))
        return ms.value

    def output(self):
        out = ctypes.create_string_buffer(self.total)
        _lib.check(self.L.kolm_memcpy_d2h(self.ctx, out, self.do, self.total))
        return out.raw

    def free(self):
        self.L.kolm_dev_free(self.ctx, self.dp)
        self.L.kolm_dev_free(self.ctx, self.do)


def stats(ms, nbytes):
    ms = sorted(ms)
    med = float(np.median(ms))
    return {"min_ms": ms[0], "median_ms": med, "max_ms": ms[-1], "mb_per_s": nbytes / 1e6 / (med / 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=32)
    ap.add_argument("--block-size", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r08", "v2_decode.json"))
    args = ap.parse_args()
    nb, bs = args.blocks, args.block_size
    data = datagen.enwik_like(nb * bs)
    blocks = [data[i * bs:(i + 1) * bs] for i in range(nb)]
    _lib.ensure_init(0)
    L = _lib.load()
    pays = {}
    for mid in (10, 2):
        _, meth, p, _ = _lib.encode_blocks(data, bs, cand_mask=1 << mid, force=[mid] * nb)
        assert all(int(m) == mid for m in meth)
        pays[mid] = p
    ctx = ctypes.c_void_p()
    _lib.check(L.kolm_ctx_create(0, ctypes.byref(ctx)))
    res = {"blocks": nb, "block_size": bs, "runs": args.runs, "warmup": args.warmup,
           "payload_bytes": {str(m): sum(len(x) for x in pays[m]) for m in pays}}
    try:
        lens = [bs] * nb
        d10 = DeviceDecode(ctx, L, pays[10], [10] * nb, lens)
        d2 = DeviceDecode(ctx, L, pays[2], [2] * nb, lens)
        for _ in range(args.warmup):
            d10.run()
            d2.run()
        t10, t2 = [], []
        for _ in range(args.runs):
            t10.append(d10.run())
            t2.append(d2.run())
        assert d10.output() == data and d2.output() == data
        res["v2_new"] = stats(t10, nb * bs)
        res["id2"] = stats(t2, nb * bs)
        res["v2_over_id2"] = res["v2_new"]["median_ms"] / res["id2"]["median_ms"]
        print(json.dumps({k: res[k] for k in ("v2_new", "id2", "v2_over_id2")}))
        d10.free()
        res["automaton_raw"] = {}
        for mode, param in KINDS:
            dr = DeviceDecode(ctx, L, [raw_payload(mode, param, b) for b in blocks], [10] * nb, lens)
            for _ in range(args.warmup):
                dr.run()
            tr, ty = [], []
            for _ in range(args.runs):
                tr.append(dr.run())
                ty.append(d2.run())
            assert dr.output() == data, (mode, param)
            st = stats(tr, nb * bs)
            st["over_id2"] = st["median_ms"] / float(np.median(ty))
            res["automaton_raw"][f"{mode},{param}"] = st
            print(json.dumps({f"raw {mode},{param}": st}))
            dr.free()
        d2.free()
    finally:
        L.kolm_ctx_destroy(ctx)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
