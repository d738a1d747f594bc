#!/usr/bin/env python3
"""Cost of verify-after-encode against a device-to-device copy of the same bytes.

One process: 32 x 1 MiB and 256 x 1 MiB enwik_like blocks, resident on the device, encoded with
the hot-path candidates (kolm_encode_blocks_device), 3 warm-ups and 10 timed rounds; each round
runs, in turn, the encode call with verify off, the same call with verify on, and a
hipMemcpyAsync device-to-device copy of the same `total` bytes (HIP events on the null stream).
Measured: the wall time of the encode call off and on, the check's own device times (ms_decode,
ms_compare of the verify report), and the copy — the yardstick for the compare kernel, which
moves the same 2 x total bytes.  Writes min / median / max to profiles/r09/verify.json (--out).

    python tools/verify_probe.py [--blocks 32,256] [--block-size 1048576] [--runs 10] [--out PATH]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "kolmogorovlike-datacompressor_amd"))

from kolm import _lib, datagen  # noqa: E402


class HipCopy:
    """hipMemcpyAsync(device to device) of n bytes between two buffers, timed with HIP events."""

    def __init__(self, src: int, dst: int, n: int):
        self.hip = ctypes.CDLL("libamdhip64.so")  # the runtime libkolm_hip.so already loaded
        self.src, self.dst, self.n = ctypes.c_void_p(src), ctypes.c_void_p(dst), ctypes.c_size_t(n)
        self.ev = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.ev:
            self.ok(self.hip.hipEventCreate(ctypes.byref(e)))

    @staticmethod
    def ok(rc):
        if rc:
            raise RuntimeError(f"HIP error {rc}")

    def run(self) -> float:
        self.ok(self.hip.hipEventRecord(self.ev[0], None))
        self.ok(self.hip.hipMemcpyAsync(self.dst, self.src, self.n, 3, None))  # hipMemcpyDeviceToDevice
        self.ok(self.hip.hipEventRecord(self.ev[1], None))
        self.ok(self.hip.hipEventSynchronize(self.ev[1]))
        ms = ctypes.c_float(0.0)
        self.ok(self.hip.hipEventElapsedTime(ctypes.byref(ms), self.ev[0], self.ev[1]))
        return ms.value

    def free(self):
        for e in self.ev:
            self.hip.hipEventDestroy(e)


def stats(ms):
    ms = sorted(ms)
    return {"min_ms": ms[0], "median_ms": float(np.median(ms)), "max_ms": ms[-1]}


def probe(ctx, nb, bs, runs, warmup):
    n = nb * bs
    data = b"".join(datagen.enwik_like(min(32 << 20, n - o), seed=1 + o // (32 << 20)) for o in range(0, n, 32 << 20))
    mask = _lib.KOLM_HOTPATH_MASK
    d_in = _lib.input_buffer(ctx, data)
    arena = _lib.DeviceBuffer(ctx, _lib.arena_capacity(n, nb, mask))
    d_cp = _lib.DeviceBuffer(ctx, n + 64)
    copy = HipCopy(d_in.ptr, d_cp.ptr, n)
    t = {"encode_off": [], "encode_on": [], "decode": [], "compare": [], "copy": [], "device_off": [], "device_on": []}
    try:
        for it in range(warmup + runs):
            row = {}
            for key, on in (("off", False), ("on", True)):
                t0 = time.perf_counter()
                _, meth, off, st = _lib.encode_blocks_device(ctx, d_in.ptr, n, bs, arena.ptr, arena.nbytes, mask,
                                                             verify=on)
                row["encode_" + key] = 1e3 * (time.perf_counter() - t0)
                row["device_" + key] = st["ms_total"]
            rep = _lib.verify_report(ctx)
            assert rep["blocks"] == nb and rep["bad_blocks"] == 0 and rep["bytes"] == n
            row["decode"], row["compare"] = rep["ms_decode"], rep["ms_compare"]
            row["copy"] = copy.run()
            if it >= warmup:
                for k, v in row.items():
                    t[k].append(v)
        assert d_cp.download(4096) == data[:4096]
        hist = np.bincount(meth, minlength=_lib.KOLM_NCAND).tolist()
    finally:
        copy.free()
        for b in (d_in, arena, d_cp):
            b.free()
    res = {k: stats(v) for k, v in t.items()}
    res["methods"] = hist
    res["payload_bytes"] = int(off[-1])
    res["compare_over_copy"] = res["compare"]["median_ms"] / res["copy"]["median_ms"]
    res["verify_over_encode"] = (res["encode_on"]["median_ms"] - res["encode_off"]["median_ms"]) / \
        res["encode_off"]["median_ms"]
    res["compare_gb_per_s"] = 2 * n / 1e9 / (res["compare"]["median_ms"] / 1e3)
    res["copy_gb_per_s"] = 2 * n / 1e9 / (res["copy"]["median_ms"] / 1e3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", default="32,256")
    ap.add_argument("--block-size", type=int, default=1 << 20)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r09", "verify.json"))
    args = ap.parse_args()
    ctx = _lib.device_ctx(_lib.ensure_init(0))
    res = {"block_size": args.block_size, "runs": args.runs, "warmup": args.warmup, "hot_path": True, "cases": {}}
    for nb in (int(x) for x in args.blocks.split(",")):
        r = probe(ctx, nb, args.block_size, args.runs, args.warmup)
        res["cases"][str(nb)] = r
        print(json.dumps({str(nb): {k: r[k] for k in ("encode_off", "encode_on", "decode", "compare", "copy",
                                                      "compare_over_copy", "verify_over_encode")}}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
