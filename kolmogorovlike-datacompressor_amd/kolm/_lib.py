"""ctypes binding of libkolm_hip.so (C ABI declared in include/kolm.h).

The product path has no CPU fallback: if the HIP library is missing or no HIP device is
visible, every GPU entry point raises ``KolmUnavailable`` (an ``ImportError`` subclass
for the loader, ``RuntimeError`` for device problems).

Note on HIP runtimes: PyTorch-ROCm ships its own ``libamdhip64.so.7``.  A process that
uses both torch and this library must import torch first, so that both share torch's
already-loaded runtime (same SONAME) — see ``kolm.parallel``.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import re
import sys
import threading
import time

import numpy as np

from .checksums import KolmChecksumError
from .lines import KolmLineIndexError

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KOLM_LIB") or os.path.join(HERE, "libkolm_hip.so")  # KOLM_LIB: A/B builds

KOLM_NCAND = 11
KOLM_DEFAULT_MASK = 0x3FF   # the reference's candidates 0..9 as shipped (kolm.h)
KOLM_FULL_MASK = 0x7FF      # + v2_new (id 10), automaton evaluated serially (opt-in)
KOLM_HOTPATH_MASK = 0x1FF  # BBWT / MTF+Rice / LZ77 path, ids 0..8
KOLM_REPAIR_MAX_BLOCK = 1 << 22
KOLM_EFORMAT = -6
KOLM_ERANGE = -7
KOLM_EVERIFY = -8
KOLM_ECHECKSUM = -9
KOLM_ELINES = -10
ERRORS = {-1: "bad argument", -2: "capacity too small", -3: "HIP error", -4: "collective error",
          -5: "not initialised", -6: "malformed container", -7: "field overflow",
          -8: "payload does not decode to its input", -9: "decoded bytes do not match their CRC-32",
          -10: "the line index does not describe the decoded bytes"}
KOLM_VERIFY_EQUAL = 0xFFFFFFFF     # per-block word of the verify entry points: the block is equal
KOLM_VERIFY_REJECTED = 0xFFFFFFFE  # the decoder rejected the payload
VR_NONE, VR_DIFFER, VR_REJECTED, VR_LENGTH = 0, 1, 2, 3  # kolm_verify_report.first_bad_reason
CR_NONE, CR_MISMATCH, CR_REJECTED = 0, 1, 2  # kolm_check_report.first_bad_reason


class KolmUnavailable(ImportError):
    pass


class KolmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"kolm error {code} ({ERRORS.get(code, '?')}): {msg}")
        self.code = code


KT_NAMES = ["classify", "keygen", "msd", "small_sort", "lsd", "lz_parse", "mtf", "sizes", "emit",
            "lyndon_gather", "repair", "cdc"]


class KolmVerifyError(KolmError):
    """An encode call with verify on produced a payload that does not decode to its input
    (KOLM_EVERIFY): .block / .method / .offset / .reason describe the lowest-numbered bad
    block (reason 1 bytes differ, 2 the decoder rejected the payload), .report the whole
    kolm_verify_report as a dict."""

    def __init__(self, msg: str, report: dict):
        super().__init__(KOLM_EVERIFY, msg)
        self.report = report
        self.block = report["first_bad_block"]
        self.method = report["first_bad_method"]
        self.offset = report["first_bad_offset"]
        self.reason = report["first_bad_reason"]


class KTime(ctypes.Structure):
    _fields_ = [("ms", ctypes.c_double), ("launches", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


class Stats(ctypes.Structure):
    _fields_ = [
        ("lin_rounds", ctypes.c_uint32),
        ("cyc_rounds", ctypes.c_uint32),
        ("lin_active", ctypes.c_uint64),
        ("cyc_active", ctypes.c_uint64),
        ("lz_tokens", ctypes.c_uint64),
        ("lz_long", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("ms_sa", ctypes.c_double),
        ("ms_lz", ctypes.c_double),
        ("ms_entropy", ctypes.c_double),
        ("ms_emit", ctypes.c_double),
        ("kt", KTime * len(KT_NAMES)),
        ("ms_repair", ctypes.c_double),
        ("rp_rules", ctypes.c_uint64),
        ("rp_batches", ctypes.c_uint64),
        ("rp_final", ctypes.c_uint64),
        ("lz_fix", ctypes.c_uint64),
        ("cyc_rounds_sum", ctypes.c_uint64),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "kt"}
        d["kernels"] = {KT_NAMES[i]: {"ms": self.kt[i].ms, "launches": self.kt[i].launches,
                                      "bytes": self.kt[i].bytes} for i in range(len(KT_NAMES))
                        if self.kt[i].launches}
        return d


class VerifyReport(ctypes.Structure):
    _fields_ = [
        ("blocks", ctypes.c_uint32),
        ("bad_blocks", ctypes.c_uint32),
        ("first_bad_block", ctypes.c_uint32),
        ("first_bad_method", ctypes.c_uint32),
        ("first_bad_offset", ctypes.c_uint32),
        ("first_bad_reason", ctypes.c_uint32),
        ("bytes", ctypes.c_uint64),
        ("ms_decode", ctypes.c_double),
        ("ms_compare", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CheckReport(ctypes.Structure):
    _fields_ = [
        ("blocks", ctypes.c_uint32),
        ("bad_blocks", ctypes.c_uint32),
        ("first_bad_block", ctypes.c_uint32),
        ("first_bad_method", ctypes.c_uint32),
        ("first_bad_expected", ctypes.c_uint32),
        ("first_bad_got", ctypes.c_uint32),
        ("first_bad_reason", ctypes.c_uint32),
        ("stream_crc", ctypes.c_uint32),
        ("bytes", ctypes.c_uint64),
        ("ms_decode", ctypes.c_double),
        ("ms_crc", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ReadStats(ctypes.Structure):
    _fields_ = [
        ("ranges", ctypes.c_uint32),
        ("blocks_decoded", ctypes.c_uint32),
        ("groups", ctypes.c_uint32),
        ("compactions", ctypes.c_uint32),
        ("bytes_returned", ctypes.c_uint64),
        ("bytes_decoded", ctypes.c_uint64),
        ("ms_decode", ctypes.c_double),
        ("ms_gather", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FindStats(ctypes.Structure):
    _fields_ = [
        ("patterns", ctypes.c_uint32),
        ("blocks_decoded", ctypes.c_uint32),
        ("groups", ctypes.c_uint32),
        ("emit_launches", ctypes.c_uint32),
        ("matches", ctypes.c_uint64),
        ("returned", ctypes.c_uint64),
        ("bytes_decoded", ctypes.c_uint64),
        ("bytes_scanned", ctypes.c_uint64),
        ("ms_decode", ctypes.c_double),
        ("ms_find", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LinesStats(ctypes.Structure):
    _fields_ = [
        ("queries", ctypes.c_uint32),
        ("blocks_decoded", ctypes.c_uint32),
        ("groups", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("bytes_decoded", ctypes.c_uint64),
        ("ms_decode", ctypes.c_double),
        ("ms_lines", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class PatsetInfo(ctypes.Structure):
    _fields_ = [
        ("np", ctypes.c_uint32),
        ("key_bytes", ctypes.c_uint32),
        ("keys", ctypes.c_uint32),
        ("slots", ctypes.c_uint32),
        ("filter_bits", ctypes.c_uint32),
        ("longest", ctypes.c_uint32),
        ("longest_bucket", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RangeSeg(ctypes.Structure):
    _fields_ = [("src", ctypes.c_uint64), ("dst", ctypes.c_uint64), ("len", ctypes.c_uint64)]


class DedupReport(ctypes.Structure):
    _fields_ = [
        ("blocks", ctypes.c_uint32),
        ("blocks_encoded", ctypes.c_uint32),
        ("candidate_pairs", ctypes.c_uint32),
        ("collisions", ctypes.c_uint32),
        ("bytes", ctypes.c_uint64),
        ("bytes_encoded", ctypes.c_uint64),
        ("ms_hash", ctypes.c_double),
        ("ms_compare", ctypes.c_double),
        ("ms_compact", ctypes.c_double),
        ("ms_expand", ctypes.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None
_lock = threading.Lock()
_result_lock = threading.Lock()  # kolm_compress_fixed's result buffer (see compress_fixed)
_inited_device = None

# (name, restype, argtypes) of every symbol declared in include/kolm.h
P = ctypes.c_void_p
U8P = ctypes.c_char_p
SZ = ctypes.c_size_t
U32 = ctypes.c_uint32
U64 = ctypes.c_uint64
I32 = ctypes.c_int
SIGNATURES = [
    ("kolm_init", I32, [I32]),
    ("kolm_shutdown", I32, []),
    ("kolm_last_error", ctypes.c_char_p, []),
    ("kolm_device_count", I32, [ctypes.POINTER(I32)]),
    ("kolm_bbwt_forward", I32, [U8P, SZ, P]),
    ("kolm_mtf_encode", I32, [U8P, SZ, P]),
    ("kolm_rice_encode", I32, [U8P, SZ, I32, P, SZ, ctypes.POINTER(SZ)]),
    ("kolm_lz77_encode", I32, [U8P, SZ, P, SZ, ctypes.POINTER(SZ)]),
    ("kolm_bbwt_mtf_rice", I32, [U8P, SZ, I32, I32, P, SZ, ctypes.POINTER(SZ)]),
    ("kolm_encode_blocks", I32, [U8P, P, P, U32, U32, P, P, P, P, U64, P, P]),
    ("kolm_encode_blocks_multi", I32, [I32, U8P, U64, U32, U32, P, P, P, P, U64, P, P]),
    ("kolm_ctx_create", I32, [I32, ctypes.POINTER(P)]),
    ("kolm_ctx_destroy", I32, [P]),
    ("kolm_ctx_reserve", I32, [P, U64, U32]),
    ("kolm_dev_alloc", I32, [P, U64, ctypes.POINTER(P)]),
    ("kolm_dev_free", I32, [P, P]),
    ("kolm_memcpy_h2d", I32, [P, P, P, U64]),
    ("kolm_memcpy_d2h", I32, [P, P, P, U64]),
    ("kolm_ctx_sync", I32, [P]),
    ("kolm_ctx_set_timing", I32, [P, I32]),
    ("kolm_ctx_set_serial", I32, [P, I32]),
    ("kolm_ctx_kernel_times", I32, [P, P, SZ, ctypes.POINTER(SZ)]),
    ("kolm_encode_blocks_device", I32, [P, P, U64, U32, U32, P, P, U64, P, P, P, P]),
    ("kolm_encode_blocks_device_var", I32, [P, P, P, U32, U32, P, P, U64, P, P, P, P]),
    ("kolm_cdc_boundaries", I32, [U8P, U64, U32, U32, U32, I32, P, U64, ctypes.POINTER(U64)]),
    ("kolm_cdc_boundaries_device", I32, [P, P, U64, U32, U32, U32, I32, P, U64, ctypes.POINTER(U64)]),
    ("kolm_decode_blocks", I32, [P, P, P, P, U32, P, U64]),
    ("kolm_decode_blocks_device", I32, [P, P, P, P, P, U32, P, U64, ctypes.POINTER(ctypes.c_double)]),
    ("kolm_compress_fixed", I32, [P, U64, U32, U32, ctypes.POINTER(P), ctypes.POINTER(U64), P]),
    ("kolm_result_copy", I32, [P, U64]),
    ("kolm_toc_write", I32, [I32, U32, U64, U32, P, P, P, P, U64, ctypes.POINTER(U64)]),
    ("kolm_toc_read", I32, [U8P, U64, P, ctypes.POINTER(U64), P, P, P, U32]),
    ("kolm_comm_unique_id", I32, [P]),
    ("kolm_comm_init", I32, [P, I32, I32, U8P, ctypes.POINTER(P)]),
    ("kolm_comm_destroy", I32, [P]),
    ("kolm_comm_rank", I32, [P, ctypes.POINTER(I32), ctypes.POINTER(I32)]),
    ("kolm_comm_allreduce", I32, [P, P, U32, I32, I32]),
    ("kolm_comm_barrier", I32, [P]),
    ("kolm_gather_payloads", I32, [P, P, U64, P, P, U32, I32, P, U64, U32, P, P, P, P, I32]),
    ("kolm_comm_wait", I32, [P]),
    ("kolm_verify_blocks_device", I32, [P, P, P, U32, P, P, P, P, ctypes.POINTER(VerifyReport)]),
    ("kolm_verify_container", I32, [P, U64, P, U64, P, U32, ctypes.POINTER(VerifyReport)]),
    ("kolm_ctx_set_verify", I32, [P, I32]),
    ("kolm_set_verify", I32, [I32]),
    ("kolm_ctx_verify_report", I32, [P, ctypes.POINTER(VerifyReport)]),
    ("kolm_range_plan", I32, [P, U32, P, P, U32, U64, P, P, P, P, P, P, P]),
    ("kolm_reader_open", I32, [P, P, U64, ctypes.POINTER(P)]),
    ("kolm_reader_close", I32, [P]),
    ("kolm_reader_info", I32, [P, P, P, P, U32]),
    ("kolm_reader_read", I32, [P, P, P, U32, P, U64, ctypes.POINTER(ReadStats)]),
    ("kolm_reader_read_device", I32, [P, P, P, U32, P, U64, ctypes.POINTER(ReadStats)]),
    ("kolm_ctx_set_dedup", I32, [P, I32]),
    ("kolm_set_dedup", I32, [I32]),
    ("kolm_ctx_dedup_report", I32, [P, ctypes.POINTER(DedupReport)]),
    ("kolm_ctx_lyndon_report", I32, [P, ctypes.POINTER(U32), ctypes.POINTER(U32)]),
    ("kolm_block_fingerprints_device", I32, [P, P, P, U32, P]),
    ("kolm_find_duplicates_device", I32, [P, P, P, U32, P, ctypes.POINTER(DedupReport)]),
    ("kolm_dedup_plan", I32, [P, P, P, U32, U32, P, P, P, P, P, P, P, P, P]),
    ("kolm_crc32_blocks_device", I32, [P, P, P, U32, P, ctypes.POINTER(ctypes.c_double)]),
    ("kolm_crc32_combine", U32, [U32, U32, U64]),
    ("kolm_ctx_set_checksums", I32, [P, I32]),
    ("kolm_set_checksums", I32, [I32]),
    ("kolm_ctx_checksums", I32, [P, P, U32, ctypes.POINTER(U32)]),
    ("kolm_decode_blocks_crc", I32, [P, P, P, P, U32, P, U64, P, P]),
    ("kolm_check_container", I32, [U8P, U64, P, P, U32, ctypes.POINTER(CheckReport)]),
    ("kolm_reader_set_checksums", I32, [P, P, U32]),
    ("kolm_find_device", I32, [P, P, U64, P, P, U32, U64, P, P, P, U64, ctypes.POINTER(U64),
                               ctypes.POINTER(ctypes.c_double)]),
    ("kolm_reader_find", I32, [P, P, P, U32, U64, U64, U64, P, ctypes.POINTER(U64), ctypes.POINTER(FindStats)]),
    ("kolm_reader_find_copy", I32, [P, U64, U64, P, P]),
    ("kolm_find_classes_device", I32, [P, P, U64, P, P, U32, U64, P, P, P, U64, ctypes.POINTER(U64),
                                       ctypes.POINTER(ctypes.c_double)]),
    ("kolm_reader_find_classes", I32, [P, P, P, U32, U64, U64, U64, P, ctypes.POINTER(U64), ctypes.POINTER(FindStats)]),
    ("kolm_find_dfa_device", I32, [P, P, U64, P, P, U32, U32, P, U32, U64, P, P, P, U64, ctypes.POINTER(U64),
                                   ctypes.POINTER(ctypes.c_double)]),
    ("kolm_reader_find_dfa", I32, [P, P, P, U32, U32, P, U32, U64, U64, U64, P, ctypes.POINTER(U64),
                                   ctypes.POINTER(FindStats)]),
    ("kolm_patset_create", I32, [P, P, P, U32, ctypes.POINTER(P)]),
    ("kolm_patset_free", None, [P]),
    ("kolm_patset_info", I32, [P, ctypes.POINTER(PatsetInfo)]),
    ("kolm_find_set_device", I32, [P, P, U64, P, U64, P, P, P, U64, ctypes.POINTER(U64),
                                   ctypes.POINTER(ctypes.c_double)]),
    ("kolm_reader_find_set", I32, [P, P, U64, U64, U64, P, ctypes.POINTER(U64), ctypes.POINTER(FindStats)]),
    ("kolm_reader_find_copy32", I32, [P, U64, U64, P, P]),
    ("kolm_delim_count_device", I32, [P, P, P, U32, U32, P, ctypes.POINTER(ctypes.c_double)]),
    ("kolm_delim_count_pieces_device", I32, [P, P, P, U32, U32, P, P, U64, ctypes.POINTER(ctypes.c_double)]),
    ("kolm_lines_locate", I32, [P, U32, P, U32, P, P]),
    ("kolm_lines_locate_offsets", I32, [P, P, U32, P, U32, P, P, P]),
    ("kolm_reader_set_lines", I32, [P, U32, P, U32]),
    ("kolm_reader_index_lines", I32, [P, U32, P, U32, ctypes.POINTER(LinesStats)]),
    ("kolm_reader_line_spans", I32, [P, P, U32, P, P, ctypes.POINTER(LinesStats)]),
    ("kolm_reader_line_of", I32, [P, P, U32, P, ctypes.POINTER(LinesStats)]),
    ("kolm_ctx_set_lines", I32, [P, I32, U32]),
    ("kolm_set_lines", I32, [I32, U32]),
    ("kolm_ctx_lines", I32, [P, P, U32, ctypes.POINTER(U32), ctypes.POINTER(U32)]),
]
KOLM_FIND_MAX_PATTERNS = 16
KOLM_FIND_MAX_LEN = 256
KOLM_FIND_SET_MAX_PATTERNS = 65536
KOLM_RX_MAX_ENTRIES = 16384
KOLM_COMM_ID_BYTES = 128
KOLM_ECAP = -2
KOLM_ERCCL = -4
KOLM_DECODE_MASK = 0x7FF  # methods decoded on the device: every id 0..10 (kolm.h)


def decode_blocks(payloads, methods, orig_lens, expect=None) -> bytes:
    """Decode the given blocks on the device (kolm_decode_blocks); every method must be in
    KOLM_DECODE_MASK.  Returns the concatenated decoded bytes.  expect (optional, one CRC-32
    per block): kolm_decode_blocks_crc checks the decoded bytes on the device; a mismatch
    raises KolmChecksumError for the lowest-numbered such block (numbered within this call)
    and nothing is returned."""
    ensure_init()
    nb = len(payloads)
    if nb == 0:
        return b""
    off = np.zeros(nb + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in payloads])
    arena = np.frombuffer(b"".join(payloads) + b"\0", dtype=np.uint8)
    meth = np.ascontiguousarray(np.asarray(methods, dtype=np.uint32))
    lens = np.ascontiguousarray(np.asarray(orig_lens, dtype=np.uint32))
    total = int(lens.astype(np.uint64).sum())
    out = np.zeros(max(total, 1), dtype=np.uint8)
    if expect is None:
        check(load().kolm_decode_blocks(arena.ctypes.data, off.ctypes.data, meth.ctypes.data, lens.ctypes.data, nb,
                                        out.ctypes.data, total))
        return out[:total].tobytes()
    exp = np.ascontiguousarray(np.asarray(expect, dtype=np.uint32))
    if exp.shape != (nb,):
        raise ValueError("expect must have one CRC-32 per block")
    got = np.zeros(nb, dtype=np.uint32)
    rc = load().kolm_decode_blocks_crc(arena.ctypes.data, off.ctypes.data, meth.ctypes.data, lens.ctypes.data, nb,
                                       out.ctypes.data, total, exp.ctypes.data, got.ctypes.data)
    if rc == KOLM_ECHECKSUM:
        i = int((got != exp).nonzero()[0][0])
        raise KolmChecksumError(i, int(meth[i]), int(exp[i]), int(got[i]))
    check(rc)
    return out[:total].tobytes()


def load():
    """Load libkolm_hip.so (raises KolmUnavailable when it is not built)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise KolmUnavailable(
                    f"{LIB_PATH} not built: run `make -C kolmogorovlike-datacompressor_amd` "
                    "or __graft_entry__.build() (there is no CPU fallback)")
            lib = ctypes.CDLL(LIB_PATH)
            for name, res, args in SIGNATURES:
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def check(rc: int, ctx=None):
    if rc != 0:
        msg = load().kolm_last_error()
        text = msg.decode() if msg else ""
        if rc == KOLM_EVERIFY:
            raise KolmVerifyError(text, verify_report(ctx))
        raise KolmError(rc, text)


def verify_report(ctx=None) -> dict:
    """The verify report of ctx's (None: the default context's) last encode call that ran
    with verify on (kolm_ctx_verify_report)."""
    rep = VerifyReport()
    rc = load().kolm_ctx_verify_report(ctx, ctypes.byref(rep))
    if rc:
        raise KolmError(rc, "kolm_ctx_verify_report")
    return rep.as_dict()


_last_verify: dict = {}
_ENV_VERIFY = os.environ.get("KOLM_VERIFY", "0").strip() not in ("", "0")  # the contexts' own default


class _verify_scope:
    """Runs one native encode call with verify on, on ctx (None: the default context): the
    switch is set and restored under _result_lock (the lock compress_fixed holds around its
    call: every verified call of this binding is serialised by it), and the call's report is
    kept for last_verify().  The switch goes back to what KOLM_VERIFY gave the context.
    verify false: no lock, no call — the path as it was."""

    def __init__(self, verify: bool, locked: bool = False, ctx=None):
        self.verify, self.locked, self.ctx = bool(verify), locked, ctx

    def _set(self, on: int) -> int:
        L = load()
        return L.kolm_set_verify(on) if self.ctx is None else L.kolm_ctx_set_verify(self.ctx, on)

    def __enter__(self):
        if self.verify:
            if not self.locked:
                _result_lock.acquire()
            rc = self._set(1)
            if rc:
                if not self.locked:
                    _result_lock.release()
                check(rc)
        return self

    def __exit__(self, et, ev, tb):
        global _last_verify
        if self.verify:
            try:
                if et is None or isinstance(ev, KolmVerifyError):
                    _last_verify = verify_report(self.ctx)
                self._set(1 if _ENV_VERIFY else 0)
            finally:
                if not self.locked:
                    _result_lock.release()
        return False


def last_verify() -> dict:
    """Report of the last verified encode call made through this binding."""
    return dict(_last_verify)


def dedup_report(ctx=None) -> dict:
    """The dedup report of ctx's (None: the default context's) last encode call
    (kolm_ctx_dedup_report): all zero when that call ran with dedup off."""
    rep = DedupReport()
    rc = load().kolm_ctx_dedup_report(ctx, ctypes.byref(rep))
    if rc:
        raise KolmError(rc, "kolm_ctx_dedup_report")
    return rep.as_dict()


def lyndon_report(ctx=None) -> dict:
    """Routes of the Lyndon factorisation of ctx's (None: the default context's) last batch
    (kolm_ctx_lyndon_report): blocks resolved from prefix-minimum candidates (accepted) and blocks
    left to the Duval kernels (fallback)."""
    acc, fb = U32(0), U32(0)
    rc = load().kolm_ctx_lyndon_report(ctx, ctypes.byref(acc), ctypes.byref(fb))
    if rc:
        raise KolmError(rc, "kolm_ctx_lyndon_report")
    return {"accepted": int(acc.value), "fallback": int(fb.value)}


_last_dedup: dict = {}
_ENV_DEDUP = os.environ.get("KOLM_DEDUP", "0").strip() not in ("", "0")  # the contexts' own default


class _dedup_scope:
    """Runs one native encode call with dedup on, on ctx (None: the default context), as
    _verify_scope does for verify: the switch is set before and goes back to what KOLM_DEDUP
    gave the context afterwards, and the call's report is kept for last_dedup().  The caller
    holds _result_lock (_encode_scope)."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def _set(self, on: int) -> int:
        L = load()
        return L.kolm_set_dedup(on) if self.ctx is None else L.kolm_ctx_set_dedup(self.ctx, on)

    def __enter__(self):
        check(self._set(1))
        return self

    def __exit__(self, et, ev, tb):
        global _last_dedup
        if et is None or isinstance(ev, KolmVerifyError):
            _last_dedup = dedup_report(self.ctx)
        self._set(1 if _ENV_DEDUP else 0)
        return False


_last_crcs = None
_ENV_CHECKSUMS = os.environ.get("KOLM_CHECKSUMS", "0").strip() not in ("", "0")  # the contexts' own default


def ctx_checksums(ctx=None):
    """The CRC-32 words of ctx's (None: the default context's) last encode call, container
    block order (kolm_ctx_checksums): empty when that call ran with checksums off."""
    n = U32(0)
    check(load().kolm_ctx_checksums(ctx, None, 0, ctypes.byref(n)))
    crc = np.zeros(max(n.value, 1), dtype=np.uint32)
    check(load().kolm_ctx_checksums(ctx, crc.ctypes.data, len(crc), ctypes.byref(n)))
    return [int(c) for c in crc[:n.value]]


class _checksums_scope:
    """Runs one native encode call with checksums on, on ctx (None: the default context), as
    _dedup_scope does for dedup: the call's words are kept for last_crcs().  The caller holds
    _result_lock (_encode_scope)."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def _set(self, on: int) -> int:
        L = load()
        return L.kolm_set_checksums(on) if self.ctx is None else L.kolm_ctx_set_checksums(self.ctx, on)

    def __enter__(self):
        check(self._set(1))
        return self

    def __exit__(self, et, ev, tb):
        global _last_crcs
        if et is None:
            _last_crcs = ctx_checksums(self.ctx)
        self._set(1 if _ENV_CHECKSUMS else 0)
        return False


def last_crcs():
    """The CRC-32 words of the last encode call made through this binding, or None when it ran
    with checksums off (or did not return a result)."""
    return None if _last_crcs is None else list(_last_crcs)


_last_lines = None
_ENV_LINES = os.environ.get("KOLM_LINES", "0").strip() not in ("", "0")  # the contexts' own default
_ENV_LINES_DELIM = int(os.environ.get("KOLM_LINES_DELIM", "10").strip() or "10") & 0xFF


def ctx_lines(ctx=None):
    """(delim, counts) of ctx's (None: the default context's) last encode call, container block
    order (kolm_ctx_lines): no counts when that call ran with the line index off."""
    n, d = U32(0), U32(0)
    check(load().kolm_ctx_lines(ctx, None, 0, ctypes.byref(n), ctypes.byref(d)))
    cnt = np.zeros(max(n.value, 1), dtype=np.uint32)
    check(load().kolm_ctx_lines(ctx, cnt.ctypes.data, len(cnt), ctypes.byref(n), ctypes.byref(d)))
    return int(d.value), [int(c) for c in cnt[:n.value]]


class _lines_scope:
    """Runs one native encode call with the line index on for the delimiter byte `delim`, on ctx
    (None: the default context), as _checksums_scope does for checksums: the call's counts are
    kept for last_lines_counts().  The caller holds _result_lock (_encode_scope)."""

    def __init__(self, delim: int, ctx=None):
        self.delim, self.ctx = delim, ctx

    def _set(self, on: int, delim: int) -> int:
        L = load()
        return L.kolm_set_lines(on, delim) if self.ctx is None else L.kolm_ctx_set_lines(self.ctx, on, delim)

    def __enter__(self):
        check(self._set(1, self.delim))
        return self

    def __exit__(self, et, ev, tb):
        global _last_lines
        if et is None:
            _last_lines = ctx_lines(self.ctx)
        self._set(1 if _ENV_LINES else 0, _ENV_LINES_DELIM)
        return False


def last_lines_counts():
    """(delim, counts) of the last encode call made through this binding, or None when it ran with
    the line index off (or did not return a result)."""
    return None if _last_lines is None else (_last_lines[0], list(_last_lines[1]))


@contextlib.contextmanager
def _encode_scope(verify: bool, dedup: bool, locked: bool = False, ctx=None, checksums: bool = False, lines=None):
    """The switches of one native encode call.  dedup and checksums false: _verify_scope alone,
    the path as it was (last_dedup() then reports nothing, last_crcs() None).  Otherwise
    _result_lock is taken once for all the switches (it is not reentrant), unless the caller holds
    it (locked).  With KOLM_DEDUP / KOLM_CHECKSUMS set in the environment the contexts do it
    whatever the argument says, so the call is treated as if the argument were true and
    last_dedup() / last_crcs() report it."""
    global _last_dedup, _last_crcs, _last_lines
    dedup = bool(dedup) or _ENV_DEDUP
    checksums = bool(checksums) or _ENV_CHECKSUMS
    if lines is None and _ENV_LINES:  # the contexts count whatever the argument says: report it
        lines = _ENV_LINES_DELIM
    _last_crcs = None
    _last_lines = None
    if not dedup:
        _last_dedup = {}
    if not dedup and not checksums and lines is None:
        with _verify_scope(verify, locked, ctx):
            yield
        return
    if not locked:
        _result_lock.acquire()
    try:
        with contextlib.ExitStack() as stack:
            if checksums:
                stack.enter_context(_checksums_scope(ctx))
            if lines is not None:
                stack.enter_context(_lines_scope(int(lines), ctx))
            if dedup:
                stack.enter_context(_dedup_scope(ctx))
            stack.enter_context(_verify_scope(verify, True, ctx))
            yield
    finally:
        if not locked:
            _result_lock.release()


def last_dedup() -> dict:
    """kolm_dedup_report of the last encode call made through this binding; empty when that
    call ran with dedup off."""
    return dict(_last_dedup)


def _bounds_array(n: int, block_size, bounds):
    """u64 block bounds [nb + 1] of n bytes in blocks of block_size, or the given bounds."""
    if bounds is None:
        if not block_size or block_size <= 0:
            raise ValueError("give a positive block_size or bounds")
        b = list(range(0, n, block_size)) + [n]
    else:
        b = [int(x) for x in bounds]
        if b[0] != 0 or b[-1] != n or any(y <= x for x, y in zip(b, b[1:])):
            raise ValueError("bounds must start at 0, increase strictly and end at len(data)")
    return np.ascontiguousarray(np.asarray(b, dtype=np.uint64))


def block_fingerprints_device(ctx, d_data: int, bounds):
    """kolm_block_fingerprints_device: u64[nb, 2].  Not a format: may change between versions."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    nb = len(b) - 1
    fp = np.zeros((max(nb, 1), 2), dtype=np.uint64)
    check(load().kolm_block_fingerprints_device(ctx, d_data, b.ctypes.data, nb, fp.ctypes.data))
    return fp[:nb]


def find_duplicates_device(ctx, d_data: int, bounds):
    """kolm_find_duplicates_device: (rep u32[nb], report dict)."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    nb = len(b) - 1
    rep = np.zeros(max(nb, 1), dtype=np.uint32)
    r = DedupReport()
    check(load().kolm_find_duplicates_device(ctx, d_data, b.ctypes.data, nb, rep.ctypes.data, ctypes.byref(r)))
    return rep[:nb], r.as_dict()


def _on_device(data, data_offset: int, device, fn):
    """fn(ctx, device address of data) with data uploaded data_offset (0..15) bytes into a buffer."""
    dev = ensure_init() if device is None else device
    ctx = device_ctx(dev)
    data = bytes(data)
    dd = DeviceBuffer(ctx, data_offset + len(data) + 64)
    try:
        dd.upload(data, data_offset)
        return fn(ctx, dd.ptr + data_offset)
    finally:
        dd.free()


def block_fingerprints(data, block_size=None, bounds=None, device: int = None, data_offset: int = 0):
    """Uploads data and returns its blocks' fingerprints, u64[nb, 2] (block_fingerprints_device)."""
    if len(data) == 0:
        return np.zeros((0, 2), dtype=np.uint64)
    b = _bounds_array(len(data), block_size, bounds)
    return _on_device(data, data_offset, device, lambda ctx, p: block_fingerprints_device(ctx, p, b))


def duplicate_blocks(data, block_size=None, bounds=None, device: int = None, data_offset: int = 0):
    """Uploads data and returns (rep, report): rep[i] = i for a distinct block, else the
    lowest-numbered block with the same bytes (find_duplicates_device)."""
    if len(data) == 0:
        return np.zeros(0, dtype=np.uint32), DedupReport().as_dict()
    b = _bounds_array(len(data), block_size, bounds)
    return _on_device(data, data_offset, device, lambda ctx, p: find_duplicates_device(ctx, p, b))


def crc32_blocks_device(ctx, d_data: int, bounds):
    """kolm_crc32_blocks_device: (the blocks' CRC-32 as a list, k_crc32's device ms)."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    nb = len(b) - 1
    crc = np.zeros(max(nb, 1), dtype=np.uint32)
    ms = ctypes.c_double(0.0)
    check(load().kolm_crc32_blocks_device(ctx, d_data, b.ctypes.data, nb, crc.ctypes.data, ctypes.byref(ms)))
    return [int(c) for c in crc[:nb]], ms.value


def crc32_blocks(data, block_size=None, bounds=None, device: int = None, data_offset: int = 0):
    """Uploads data and returns its blocks' CRC-32 (crc32_blocks_device).  bounds may hold
    empty blocks (equal neighbours): their CRC-32 is 0."""
    n = len(data)
    if bounds is None:
        if n == 0:
            return []
        b = _bounds_array(n, block_size, None)
    else:
        bl = [int(x) for x in bounds]
        if not bl or bl[0] != 0 or bl[-1] != n or any(y < x for x, y in zip(bl, bl[1:])):
            raise ValueError("bounds must start at 0, not decrease and end at len(data)")
        b = np.ascontiguousarray(np.asarray(bl, dtype=np.uint64))
    return _on_device(data, data_offset, device, lambda ctx, p: crc32_blocks_device(ctx, p, b))[0]


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """kolm_crc32_combine (host only, no device)."""
    return int(load().kolm_crc32_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, int(len_b)))


def check_container(container, expect=None):
    """kolm_check_container on the default context: (the blocks' CRC-32 as computed from the
    decoded bytes, report dict).  expect: one CRC-32 per block, or None to compute only.  A
    malformed container raises ValueError as decompress does."""
    ensure_init()
    container = bytes(container)
    got = np.zeros(65536, dtype=np.uint32)
    exp = None
    if expect is not None:  # a container holds at most 65535 blocks: the library never reads past the array
        exp = np.zeros(65536, dtype=np.uint32)
        exp[:len(expect)] = np.asarray(expect, dtype=np.uint32)[:65536]
    rep = CheckReport()
    rc = load().kolm_check_container(container, len(container), None if exp is None else exp.ctypes.data,
                                     got.ctypes.data, len(got), ctypes.byref(rep))
    if rc == KOLM_EFORMAT:
        raise ValueError(load().kolm_last_error().decode())
    check(rc)
    r = rep.as_dict()
    return [int(c) for c in got[:r["blocks"]]], r


def dedup_plan(lens, fps, force=None, fp_bits: int = 128, differ=None, distinct_off=None) -> dict:
    """kolm_dedup_plan (host only, no device).  differ None: {"pairs": [(member, rep), ...]} and,
    when there are no pairs, phase B's keys too.  Otherwise also "rep", "distinct",
    "collisions", "compact" [(src, dst, len)] and, given distinct_off (a function of the
    distinct block list -> their payload offsets, or None), "payload_off" and "expand"."""
    L = load()
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.uint32))
    nb = len(ln)
    fp = np.ascontiguousarray(np.asarray(fps, dtype=np.uint64).reshape(-1))
    if fp.size != 2 * nb:
        raise ValueError("fps must hold two words per block")
    fz = None if force is None else np.ascontiguousarray(np.asarray(force, dtype=np.int32))
    pairs = np.zeros(max(2 * nb, 1), dtype=np.uint32)
    counts = np.zeros(3, dtype=np.uint32)
    args = (ln.ctypes.data, fp.ctypes.data, fz.ctypes.data if fz is not None else None, nb, fp_bits)
    check(L.kolm_dedup_plan(*args, None, pairs.ctypes.data, None, None, None, None, None, None, counts.ctypes.data))
    npairs = int(counts[0])
    out = {"pairs": [(int(pairs[2 * p]), int(pairs[2 * p + 1])) for p in range(npairs)]}
    if differ is None and npairs:
        return out
    df = np.ascontiguousarray(np.asarray(differ if differ is not None else [], dtype=np.uint32))
    if df.size != npairs:
        raise ValueError("differ must hold one word per pair")
    rep = np.zeros(max(nb, 1), dtype=np.uint32)
    dist = np.zeros(max(nb, 1), dtype=np.uint32)
    comp = (RangeSeg * max(nb, 1))()
    check(L.kolm_dedup_plan(*args, df.ctypes.data if npairs else None, pairs.ctypes.data, rep.ctypes.data,
                            dist.ctypes.data, ctypes.addressof(comp), None, None, None, counts.ctypes.data))
    nd = int(counts[1])
    out.update(rep=[int(x) for x in rep[:nb]], distinct=[int(x) for x in dist[:nd]], collisions=int(counts[2]),
               compact=[(comp[i].src, comp[i].dst, comp[i].len) for i in range(nd)])
    if distinct_off is not None:
        doff = np.ascontiguousarray(np.asarray(distinct_off(out["distinct"]), dtype=np.uint64))
        if doff.size != nd + 1:
            raise ValueError("distinct_off must give one offset more than distinct blocks")
        poff = np.zeros(nb + 1, dtype=np.uint64)
        exp = (RangeSeg * max(nb, 1))()
        check(L.kolm_dedup_plan(*args, df.ctypes.data if npairs else None, None, None, None, None, doff.ctypes.data,
                                poff.ctypes.data, ctypes.addressof(exp), counts.ctypes.data))
        out.update(payload_off=[int(x) for x in poff], expand=[(exp[i].src, exp[i].dst, exp[i].len) for i in range(nb)])
    return out


def verify_blocks_device(ctx, d_data: int, bounds, d_payloads: int, payload_off, methods):
    """kolm_verify_blocks_device: original and payloads device-resident.  Returns (first_bad
    u32[nb]: offset of the block's first differing byte, KOLM_VERIFY_EQUAL or
    KOLM_VERIFY_REJECTED; report dict)."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    off = np.ascontiguousarray(np.asarray(payload_off, dtype=np.uint64))
    meth = np.ascontiguousarray(np.asarray(methods, dtype=np.uint32))
    nb = len(meth)
    if len(b) != nb + 1 or len(off) != nb + 1:
        raise ValueError("bounds and payload_off must have one entry more than methods")
    fb = np.zeros(max(nb, 1), dtype=np.uint32)
    rep = VerifyReport()
    check(load().kolm_verify_blocks_device(ctx, d_data, b.ctypes.data, nb, d_payloads, off.ctypes.data,
                                           meth.ctypes.data, fb.ctypes.data, ctypes.byref(rep)))
    return fb[:nb], rep.as_dict()


def verify_blocks(data, bounds, payloads, methods, device: int = None, data_offset: int = 0):
    """Uploads data (block i = data[bounds[i]:bounds[i+1]], bounds[0] = 0) and the blocks'
    payloads, then checks on the device that every payload decodes to its block
    (verify_blocks_device).  data_offset (0..15) places the data that many bytes into its
    device buffer (any alignment is accepted).  Returns (first_bad, report)."""
    dev = ensure_init() if device is None else device
    ctx = device_ctx(dev)
    data = bytes(data)
    pay = b"".join(payloads)
    off = np.zeros(len(payloads) + 1, dtype=np.uint64)
    if payloads:
        off[1:] = np.cumsum([len(p) for p in payloads])
    dd = DeviceBuffer(ctx, data_offset + len(data) + 64)
    dp = DeviceBuffer(ctx, len(pay) + 64)
    try:
        dd.upload(data, data_offset)
        dp.upload(pay)
        return verify_blocks_device(ctx, dd.ptr + data_offset, bounds, dp.ptr, off, methods)
    finally:
        dd.free()
        dp.free()


def verify_container(container, data):
    """kolm_verify_container on the default context: (first_bad u32[nb] or None when the
    lengths differ, report dict).  A malformed container raises ValueError as decompress does."""
    ensure_init()
    container, data = bytes(container), bytes(data)
    fb = np.zeros(65536, dtype=np.uint32)
    rep = VerifyReport()
    rc = load().kolm_verify_container(container, len(container), data, len(data), fb.ctypes.data, len(fb),
                                      ctypes.byref(rep))
    if rc == KOLM_EFORMAT:
        raise ValueError(load().kolm_last_error().decode())
    check(rc)
    r = rep.as_dict()
    return (None if r["first_bad_reason"] == VR_LENGTH else fb[:r["blocks"]].copy()), r


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = load().kolm_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def ensure_init(device: int = None):
    """Create the default context (device from $KOLM_DEVICE, else 0)."""
    global _inited_device
    if _inited_device is not None:
        return _inited_device
    if device is None:
        device = int(os.environ.get("KOLM_DEVICE", "0"))
    lib = load()
    if device_count() <= 0:
        raise KolmUnavailable("no HIP device visible: the kolm GPU path has no CPU fallback")
    check(lib.kolm_init(device))
    _inited_device = device
    return device


_dev_ctx = {}


def device_ctx(device: int):
    """A context of this process on `device` (kolm_ctx_create, cached) for the
    device-resident entry points (kolm_encode_blocks_device, ...)."""
    with _lock:
        ctx = _dev_ctx.get(device)
    if ctx is None:
        ctx = ctypes.c_void_p()
        check(load().kolm_ctx_create(int(device), ctypes.byref(ctx)))
        with _lock:
            _dev_ctx.setdefault(device, ctx)
            ctx = _dev_ctx[device]
    return ctx


def encode_blocks_device(ctx, d_data: int, n: int, block_size: int, d_arena: int, arena_cap: int,
                         cand_mask: int = KOLM_DEFAULT_MASK, verify: bool = False, dedup: bool = False,
                         checksums: bool = False, lines=None):
    """Batched MDL encode of fixed blocks of the device buffer d_data[0, n) into the
    device arena (kolm_encode_blocks_device).  Returns (sizes, method, offsets, stats).
    verify: the batch is checked on ctx before the call returns (KolmVerifyError).
    dedup: repeated blocks are encoded once (same outputs; last_dedup()).
    checksums: the blocks' CRC-32 are taken on the resident input (last_crcs())."""
    nb = (n + block_size - 1) // block_size if n else 0
    sizes = np.zeros((max(nb, 1), KOLM_NCAND), dtype=np.uint32)
    method = np.zeros(max(nb, 1), dtype=np.uint32)
    off = np.zeros(nb + 1, dtype=np.uint64)
    st = Stats()
    with _encode_scope(verify, dedup, ctx=ctx, checksums=checksums, lines=lines):
        check(load().kolm_encode_blocks_device(ctx, d_data, n, block_size, cand_mask, None, d_arena, arena_cap,
                                               sizes.ctypes.data, method.ctypes.data, off.ctypes.data,
                                               ctypes.byref(st)), ctx)
    return sizes[:nb], method[:nb], off, st.as_dict()


class DeviceBuffer:
    """Device memory of a context (kolm_dev_alloc): the input and payload arenas of the
    device-resident entry points, without any other framework.  ptr is the device address."""

    def __init__(self, ctx, nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        check(load().kolm_dev_alloc(ctx, max(self.nbytes, 1), ctypes.byref(p)))
        self.ptr = int(p.value)

    def upload(self, data, offset: int = 0):
        """Copies host bytes (bytes / bytearray / memoryview / numpy) to ptr + offset."""
        src = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8) if len(data) else None
        if src is None:
            return
        if offset + src.size > self.nbytes:
            raise ValueError("upload exceeds the buffer")
        check(load().kolm_memcpy_h2d(self.ctx, self.ptr + offset, src.ctypes.data, src.size))

    def download(self, n: int = None, offset: int = 0) -> bytes:
        n = self.nbytes - offset if n is None else int(n)
        if offset + n > self.nbytes:
            raise ValueError("download exceeds the buffer")
        if n <= 0:
            return b""
        out = _new_bytes(n)
        check(load().kolm_memcpy_d2h(self.ctx, ctypes.cast(ctypes.c_char_p(out), ctypes.c_void_p), self.ptr + offset,
                                     n))
        return out

    def zero_tail(self, start: int):
        """Zeroes [start, nbytes) (the 64-byte read-ahead padding behind an input)."""
        if start < self.nbytes:
            self.upload(bytes(self.nbytes - start), start)

    def free(self):
        if self.ptr:
            check(load().kolm_dev_free(self.ctx, self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            if self.ptr and _lib is not None:
                _lib.kolm_dev_free(self.ctx, self.ptr)
                self.ptr = 0
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def input_buffer(ctx, data) -> "DeviceBuffer":
    """The device copy of an input batch with its 64 bytes of zero read-ahead padding
    (the layout kolm_encode_blocks_device expects)."""
    n = len(data)
    buf = DeviceBuffer(ctx, n + 64)
    buf.upload(data)
    buf.zero_tail(n)
    return buf


def arena_capacity(n: int, nb: int, cand_mask: int) -> int:
    """Device arena bytes that always hold the payloads of n input bytes in nb blocks
    (raw in the mask bounds every winner by its block; kolm_api.cpp sizes it the same)."""
    return (n if cand_mask & 1 else 9 * n) + 64 * nb + 256


def kernel_times(ctx) -> dict:
    """Per-kernel HIP-event timing accumulated while timing was enabled on ctx."""
    import json
    n = ctypes.c_size_t(0)
    check(load().kolm_ctx_kernel_times(ctx, None, 0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(n.value + 1)
    check(load().kolm_ctx_kernel_times(ctx, buf, n.value + 1, ctypes.byref(n)))
    return json.loads(buf.value.decode())


def _buf(n):
    return ctypes.create_string_buffer(max(int(n), 1))


def bbwt_forward(data: bytes) -> bytes:
    ensure_init()
    n = len(data)
    out = _buf(n)
    check(load().kolm_bbwt_forward(data, n, out))
    return out.raw[:n]


def mtf_encode(data: bytes) -> bytes:
    ensure_init()
    n = len(data)
    out = _buf(n)
    check(load().kolm_mtf_encode(data, n, out))
    return out.raw[:n]


def rice_encode(seq: bytes, k: int) -> bytes:
    ensure_init()
    n = len(seq)
    cap = (n * ((255 >> k) + 1 + k) + 7) // 8 + 16
    out = _buf(cap)
    ln = ctypes.c_size_t(0)
    check(load().kolm_rice_encode(seq, n, k, out, cap, ctypes.byref(ln)))
    return out.raw[:ln.value]


def lz77_encode(data: bytes) -> bytes:
    ensure_init()
    n = len(data)
    cap = 2 * n + 16
    out = _buf(cap)
    ln = ctypes.c_size_t(0)
    check(load().kolm_lz77_encode(data, n, out, cap, ctypes.byref(ln)))
    return out.raw[:ln.value]


def bbwt_mtf_rice(data: bytes, flags: int, k: int = 2) -> bytes:
    ensure_init()
    n = len(data)
    cap = (n + 8) * ((255 >> k) + 1 + k) // 8 + 64
    out = _buf(cap)
    ln = ctypes.c_size_t(0)
    check(load().kolm_bbwt_mtf_rice(data, n, flags, k, out, cap, ctypes.byref(ln)))
    return out.raw[:ln.value]


def encode_blocks(data: bytes, block_size: int, cand_mask: int = KOLM_DEFAULT_MASK, force=None,
                  verify: bool = False, dedup: bool = False, checksums: bool = False, lines=None):
    """Batched MDL encode of fixed-size blocks.  Returns (sizes[nb,KOLM_NCAND], method[nb],
    payloads list, stats dict).  verify: check the payloads on the device before returning
    (KolmVerifyError on a bad block).  dedup: repeated blocks are encoded once.  checksums:
    the blocks' CRC-32 are taken on the resident input (last_crcs())."""
    ensure_init()
    n = len(data)
    nb = (n + block_size - 1) // block_size if n else 0
    starts = np.arange(nb, dtype=np.uint64) * np.uint64(block_size)
    lens = np.full(nb, block_size, dtype=np.uint32)
    if nb:
        lens[-1] = n - (nb - 1) * block_size
    sizes = np.zeros((max(nb, 1), KOLM_NCAND), dtype=np.uint32)
    method = np.zeros(max(nb, 1), dtype=np.uint32)
    off = np.zeros(nb + 1, dtype=np.uint64)
    cap = 9 * n + 64 * nb + 64
    arena = np.zeros(cap, dtype=np.uint8)
    fz = None
    if force is not None:
        fz = np.ascontiguousarray(np.asarray(force, dtype=np.int32))
        if fz.shape != (nb,):
            raise ValueError("force must have one entry per block")
    st = Stats()
    with _encode_scope(verify, dedup, checksums=checksums, lines=lines):
        check(load().kolm_encode_blocks(
            data, starts.ctypes.data, lens.ctypes.data, nb, cand_mask,
            fz.ctypes.data if fz is not None else None,
            sizes.ctypes.data, method.ctypes.data, arena.ctypes.data, cap, off.ctypes.data,
            ctypes.byref(st)))
    payloads = [arena[int(off[i]):int(off[i + 1])].tobytes() for i in range(nb)]
    return sizes[:nb], method[:nb], payloads, st.as_dict()


def compress_fixed(data, block_size: int, cand_mask: int = KOLM_DEFAULT_MASK, verify: bool = False,
                   dedup: bool = False, checksums: bool = False, lines=None):
    """The whole KOLR container of data in fixed blocks (kolm_compress_fixed): (bytes, stats).
    verify: every device batch is checked before its payloads count (KolmVerifyError, no
    container, on a bad block).  dedup: every device batch encodes its repeated blocks once.
    checksums: every device batch takes its blocks' CRC-32 on the resident input (last_crcs())."""
    ensure_init()
    n = len(data)
    src = np.frombuffer(memoryview(data).cast("B"), dtype=np.uint8) if n else np.zeros(1, np.uint8)
    out = ctypes.c_void_p()
    ln = ctypes.c_uint64(0)
    st = Stats()
    # the result lives in the context's pinned buffer until the next call: the call and the
    # copy out of it run under one lock (ctypes drops the GIL inside the call)
    with _result_lock:
        tc = time.perf_counter() if _HOST_PROF else 0.0
        with _encode_scope(verify, dedup, locked=True, checksums=checksums, lines=lines):
            rc = load().kolm_compress_fixed(src.ctypes.data, n, block_size, cand_mask, ctypes.byref(out),
                                            ctypes.byref(ln), ctypes.byref(st))
            if rc == KOLM_EVERIFY:
                check(rc)
        if rc == KOLM_ERANGE:
            import struct
            raise struct.error(load().kolm_last_error().decode())
        check(rc)
        # the result bytes object is allocated uninitialised and filled by the library's
        # copy threads (kolm_result_copy) instead of one single-threaded string_at copy
        t0 = time.perf_counter() if _HOST_PROF else 0.0
        if _HOST_PROF:
            print(f"[kolm] host: native call {1e3 * (t0 - tc):.2f} ms", file=sys.stderr)
        blob = _new_bytes(ln.value)
        t1 = time.perf_counter() if _HOST_PROF else 0.0
        if ln.value:
            check(load().kolm_result_copy(ctypes.cast(ctypes.c_char_p(blob), ctypes.c_void_p), ln.value))
        if _HOST_PROF:
            print(f"[kolm] host: bytes alloc {1e3 * (t1 - t0):.2f} ms, result copy "
                  f"{1e3 * (time.perf_counter() - t1):.2f} ms", file=sys.stderr)
    return blob, st.as_dict()


_HOST_PROF = os.environ.get("KOLM_HOST_PROF", "0") not in ("", "0")  # debug: phase times on stderr

_PyBytes_New = ctypes.pythonapi.PyBytes_FromStringAndSize
_PyBytes_New.restype = ctypes.py_object
_PyBytes_New.argtypes = [ctypes.c_void_p, ctypes.c_ssize_t]


def _new_bytes(n: int) -> bytes:
    """A fresh bytes object of n bytes, contents undefined until written (the C API's
    PyBytes_FromStringAndSize(NULL, n) idiom); it is filled before anyone else sees it."""
    return _PyBytes_New(None, n) if n else b""


def encode_blocks_var(data: bytes, bounds, cand_mask: int = KOLM_DEFAULT_MASK, force=None, verify: bool = False,
                      dedup: bool = False, checksums: bool = False, lines=None):
    """Batched MDL encode of content-defined blocks: block i = data[bounds[i]:bounds[i+1]]
    (bounds[0] = 0, strictly increasing, bounds[-1] = len(data)).  Same return value as
    encode_blocks."""
    ensure_init()
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    nb = max(len(b) - 1, 0)
    if nb and (b[0] != 0 or int(b[-1]) != len(data) or np.any(np.diff(b.astype(np.int64)) <= 0)):
        raise ValueError("bounds must start at 0, increase strictly and end at len(data)")
    starts = np.ascontiguousarray(b[:-1]) if nb else np.zeros(0, np.uint64)
    lens = np.ascontiguousarray(np.diff(b).astype(np.uint32)) if nb else np.zeros(0, np.uint32)
    n = len(data)
    sizes = np.zeros((max(nb, 1), KOLM_NCAND), dtype=np.uint32)
    method = np.zeros(max(nb, 1), dtype=np.uint32)
    off = np.zeros(nb + 1, dtype=np.uint64)
    cap = 9 * n + 64 * nb + 64
    arena = np.zeros(cap, dtype=np.uint8)
    fz = None
    if force is not None:
        fz = np.ascontiguousarray(np.asarray(force, dtype=np.int32))
        if fz.shape != (nb,):
            raise ValueError("force must have one entry per block")
    st = Stats()
    with _encode_scope(verify, dedup, checksums=checksums, lines=lines):
        check(load().kolm_encode_blocks(
            data, starts.ctypes.data, lens.ctypes.data, nb, cand_mask,
            fz.ctypes.data if fz is not None else None,
            sizes.ctypes.data, method.ctypes.data, arena.ctypes.data, cap, off.ctypes.data,
            ctypes.byref(st)))
    payloads = [arena[int(off[i]):int(off[i + 1])].tobytes() for i in range(nb)]
    return sizes[:nb], method[:nb], payloads, st.as_dict()


def cdc_boundaries(data: bytes, min_size: int, avg_size: int, max_size: int, merge_orphan_tail: bool = True):
    """FastCDC chunk starts followed by len(data) (kolm_cdc_boundaries, PY:210-309)."""
    ensure_init()
    n = len(data)
    cap = n // max(min_size, 1) + 3
    starts = np.zeros(cap, dtype=np.uint64)
    cnt = ctypes.c_uint64(0)
    check(load().kolm_cdc_boundaries(data, n, min_size, avg_size, max_size, 1 if merge_orphan_tail else 0,
                                     starts.ctypes.data, cap, ctypes.byref(cnt)))
    return starts[:cnt.value + 1] if cnt.value else starts[:0]


def encode_blocks_multi(data: bytes, block_size: int, ngpu: int, cand_mask: int = KOLM_DEFAULT_MASK,
                        verify: bool = False, dedup: bool = False):
    """encode_blocks over ngpu devices of this process (contiguous block shards, one host
    thread per device; kolm_encode_blocks_multi).  Same return value."""
    ensure_init()
    n = len(data)
    nb = (n + block_size - 1) // block_size if n else 0
    sizes = np.zeros((max(nb, 1), KOLM_NCAND), dtype=np.uint32)
    method = np.zeros(max(nb, 1), dtype=np.uint32)
    off = np.zeros(nb + 1, dtype=np.uint64)
    cap = 9 * n + 64 * nb + 64
    arena = np.zeros(cap, dtype=np.uint8)
    st = Stats()
    with _encode_scope(verify, dedup):
        check(load().kolm_encode_blocks_multi(
            int(ngpu), data, n, block_size, cand_mask, None, sizes.ctypes.data, method.ctypes.data,
            arena.ctypes.data, cap, off.ctypes.data, ctypes.byref(st)))
    payloads = [arena[int(off[i]):int(off[i + 1])].tobytes() for i in range(nb)]
    return sizes[:nb], method[:nb], payloads, st.as_dict()


# ---- random-access reads (kolm_range_plan, kolm_reader_*) ----------------------------------

def _ranges_arrays(ranges):
    """[(offset, length), ...] -> (offs u64[n], lens u64[n]); negative values raise ValueError."""
    offs = np.zeros(max(len(ranges), 1), dtype=np.uint64)
    lens = np.zeros(max(len(ranges), 1), dtype=np.uint64)
    for i, (o, n) in enumerate(ranges):
        if o < 0 or n < 0:
            raise ValueError(f"range {i}: negative offset or length")
        offs[i], lens[i] = o, n
    return offs, lens


def range_plan(orig_lens, ranges, group_limit: int = 0) -> dict:
    """kolm_range_plan (host only, no device): which blocks a read of `ranges` decodes and how
    the decoded bytes are packed.  Returns {"sel": [block, ...], "groups": [[block, ...], ...],
    "runs": [[block, ...], ...], "segs": [[(src, dst, len), ...] per group]}.  A range outside
    the data raises ValueError (the message names the range)."""
    L = load()
    ol = np.ascontiguousarray(np.asarray(orig_lens, dtype=np.uint32))
    offs, lens = _ranges_arrays(ranges)
    counts = np.zeros(4, dtype=np.uint64)
    rc = L.kolm_range_plan(ol.ctypes.data, len(ol), offs.ctypes.data, lens.ctypes.data, len(ranges), group_limit,
                           None, None, None, None, None, None, counts.ctypes.data)
    if rc == -1:
        raise ValueError(L.kolm_last_error().decode())
    if rc != KOLM_ECAP:
        check(rc)
    ns, ng, nr, nseg = (int(x) for x in counts)
    sel = np.zeros(max(ns, 1), dtype=np.uint32)
    gfirst = np.zeros(ng + 1, dtype=np.uint32)
    rfirst = np.zeros(nr + 1, dtype=np.uint32)
    gseg = np.zeros(ng + 1, dtype=np.uint32)
    segs = (RangeSeg * max(nseg, 1))()
    check(L.kolm_range_plan(ol.ctypes.data, len(ol), offs.ctypes.data, lens.ctypes.data, len(ranges), group_limit,
                            sel.ctypes.data, gfirst.ctypes.data, rfirst.ctypes.data, gseg.ctypes.data,
                            ctypes.addressof(segs), counts.ctypes.data, counts.ctypes.data))
    sel = [int(b) for b in sel[:ns]]
    return {"sel": sel,
            "groups": [sel[int(gfirst[g]):int(gfirst[g + 1])] for g in range(ng)],
            "runs": [sel[int(rfirst[r]):int(rfirst[r + 1])] for r in range(nr)],
            "segs": [[(segs[i].src, segs[i].dst, segs[i].len) for i in range(int(gseg[g]), int(gseg[g + 1]))]
                     for g in range(ng)]}


_last_read: dict = {}


def last_read() -> dict:
    """kolm_read_stats of the last reader call made through this binding."""
    return dict(_last_read)


def reader_open(container, ctx=None):
    """kolm_reader_open on ctx (None: the default context).  Returns (handle, info dict with
    mode, size_field, total_len, nblocks, payload_bytes, methods, orig_lens).  A malformed
    container raises ValueError / struct.error as decompress does."""
    ensure_init()
    blob = bytes(container)
    h = ctypes.c_void_p()
    rc = load().kolm_reader_open(ctx, blob, len(blob), ctypes.byref(h))
    if rc == KOLM_EFORMAT:
        raise ValueError(load().kolm_last_error().decode())
    if rc == KOLM_ERANGE:
        import struct
        raise struct.error(load().kolm_last_error().decode())
    check(rc)
    info = np.zeros(5, dtype=np.uint64)
    check(load().kolm_reader_info(h, info.ctypes.data, None, None, 0))
    nb = int(info[3])
    meth = np.zeros(max(nb, 1), dtype=np.uint32)
    lens = np.zeros(max(nb, 1), dtype=np.uint32)
    check(load().kolm_reader_info(h, info.ctypes.data, meth.ctypes.data, lens.ctypes.data, max(nb, 1)))
    return h, {"mode": int(info[0]), "size_field": int(info[1]), "total_len": int(info[2]), "nblocks": nb,
               "payload_bytes": int(info[4]), "methods": [int(m) for m in meth[:nb]],
               "orig_lens": [int(n) for n in lens[:nb]]}


def reader_close(h):
    check(load().kolm_reader_close(h))


def reader_set_checksums(h, crcs):
    """kolm_reader_set_checksums: the expected CRC-32 of every block (None clears)."""
    if crcs is None:
        check(load().kolm_reader_set_checksums(h, None, 0))
        return
    c = np.ascontiguousarray(np.asarray(crcs, dtype=np.uint32))
    rc = load().kolm_reader_set_checksums(h, c.ctypes.data, len(c))
    if rc == -1:
        raise ValueError(load().kolm_last_error().decode())
    check(rc)


_CHECKSUM_MSG = re.compile(r"block (\d+) \(method (\d+)\): expected CRC-32 ([0-9a-f]{8}), got ([0-9a-f]{8})")


def _read_check(rc):
    if rc == -1:  # KOLM_EARG: a range outside the data, or a selected block that does not decode
        raise ValueError(load().kolm_last_error().decode())
    if rc == KOLM_ECHECKSUM:  # the message names the block (kolm.h)
        m = _CHECKSUM_MSG.search(load().kolm_last_error().decode())
        if m:
            raise KolmChecksumError(int(m.group(1)), int(m.group(2)), int(m.group(3), 16), int(m.group(4), 16))
        raise KolmChecksumError(-1, -1, 0, 0)  # a text this binding does not know: still the checksum error
    check(rc)


def reader_read(h, ranges) -> bytes:
    """kolm_reader_read: the ranges' bytes packed back to back, as one bytes object."""
    global _last_read
    offs, lens = _ranges_arrays(ranges)
    total = int(lens[:len(ranges)].sum()) if ranges else 0
    out = _new_bytes(total)
    st = ReadStats()
    _read_check(load().kolm_reader_read(h, offs.ctypes.data, lens.ctypes.data, len(ranges),
                                        ctypes.cast(ctypes.c_char_p(out), ctypes.c_void_p) if total else None,
                                        total, ctypes.byref(st)))
    _last_read = st.as_dict()
    return out


# ---- search (kolm_find_device, kolm_reader_find) -------------------------------------------

NO_LIMIT = (1 << 64) - 1
_last_find: dict = {}


def last_find() -> dict:
    """kolm_find_stats of the last search made through this binding."""
    return dict(_last_find)


def find_patterns(patterns) -> list:
    """The patterns of a search as a list of bytes; ValueError for what the library refuses
    (no pattern or more than 16, an empty one, one of more than 256 bytes)."""
    if isinstance(patterns, (bytes, bytearray, memoryview, str)):
        raise TypeError("patterns must be a sequence of bytes-like objects")
    pats = [memoryview(p).tobytes() for p in patterns]
    if not 1 <= len(pats) <= KOLM_FIND_MAX_PATTERNS:
        raise ValueError(f"{len(pats)} patterns (1..{KOLM_FIND_MAX_PATTERNS} are allowed)")
    for i, p in enumerate(pats):
        if not p:
            raise ValueError(f"pattern {i} is empty")
        if len(p) > KOLM_FIND_MAX_LEN:
            raise ValueError(f"pattern {i} has {len(p)} bytes (at most {KOLM_FIND_MAX_LEN})")
    return pats


def _pattern_arrays(pats):
    off = np.zeros(len(pats) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(p) for p in pats])
    flat = np.frombuffer(b"".join(bytes(p) for p in pats) + b"\0", dtype=np.uint8)
    return flat, off


def _find_device_call(fn, lead, npat: int, which_dtype, limit, cap=0):
    """The two-call protocol of a kolm_find_*_device function fn, whose arguments begin with `lead`
    (the context, the buffer and the variant's patterns).  The first call has room for `cap` results
    (0: it only counts); KOLM_ECAP names the capacity, and the second call emits.  Returns (offsets,
    pattern indices as which_dtype, counts of the npat patterns, device ms); the library's argument
    errors raise ValueError."""
    counts = np.zeros(max(npat, 1), dtype=np.uint64)
    nfound, ms = U64(0), ctypes.c_double(0.0)
    lim = NO_LIMIT if limit is None else int(limit)

    def call(k):
        offs = np.zeros(max(k, 1), dtype=np.uint64)
        which = np.zeros(max(k, 1), dtype=which_dtype)
        rc = fn(*lead, lim, counts.ctypes.data, offs.ctypes.data, which.ctypes.data, k, ctypes.byref(nfound), ctypes.byref(ms))
        return rc, offs, which

    rc, offs, which = call(int(cap or 0))
    if rc == -1:
        raise ValueError(load().kolm_last_error().decode())
    if rc == KOLM_ECAP:  # the capacity is known now: the second call emits
        rc, offs, which = call(int(nfound.value))
    check(rc)
    k = int(nfound.value)
    return offs[:k].tolist(), which[:k].tolist(), [int(x) for x in counts[:npat]], ms.value


def _reader_find_call(fn, copy, h, lead, lo: int, hi: int, npat: int, which_dtype, limit):
    """A kolm_reader_find* function fn with the variant's arguments `lead` behind the reader, then
    its copy function (kolm_reader_find_copy / _copy32).  Returns (offsets, pattern indices, counts
    of the npat patterns); the stats go to last_find().  Argument errors raise ValueError, a
    checksum mismatch KolmChecksumError, and last_find() keeps what it held."""
    global _last_find
    counts = np.zeros(max(npat, 1), dtype=np.uint64)
    nfound = U64(0)
    st = FindStats()
    lim = NO_LIMIT if limit is None else int(limit)
    _read_check(fn(h, *lead, lo, hi, lim, counts.ctypes.data, ctypes.byref(nfound), ctypes.byref(st)))
    k = int(nfound.value)
    offs = np.zeros(max(k, 1), dtype=np.uint64)
    which = np.zeros(max(k, 1), dtype=which_dtype)
    check(copy(h, 0, k, offs.ctypes.data, which.ctypes.data))
    _last_find = st.as_dict()
    return offs[:k].tolist(), which[:k].tolist(), [int(x) for x in counts[:npat]]


def find_device(ctx, dptr: int, n: int, patterns, limit=None):
    """kolm_find_device over the n bytes at the device address dptr.  Returns (offsets,
    pattern indices, counts per pattern, device ms); the patterns are passed as given (the
    library's argument errors raise ValueError)."""
    pats = list(patterns)
    flat, off = _pattern_arrays(pats)
    lead = (ctx, dptr, n, flat.ctypes.data, off.ctypes.data, len(pats))
    return _find_device_call(load().kolm_find_device, lead, len(pats), np.uint8, limit)


def find_bytes(data, patterns, limit=None, device: int = None, data_offset: int = 0):
    """Uploads data data_offset (0..15) bytes into a buffer and searches it (find_device)."""
    return _on_device(data, data_offset, device, lambda ctx, p: find_device(ctx, p, len(data), patterns, limit))


def reader_find(h, patterns, lo: int, hi: int, limit=None):
    """kolm_reader_find + kolm_reader_find_copy.  Returns (offsets, pattern indices, counts per
    pattern); the stats go to last_find().  Argument errors raise ValueError, a checksum
    mismatch KolmChecksumError, and last_find() keeps what it held."""
    pats = list(patterns)
    flat, off = _pattern_arrays(pats)
    L = load()
    return _reader_find_call(L.kolm_reader_find, L.kolm_reader_find_copy, h, (flat.ctypes.data, off.ctypes.data, len(pats)),
                             lo, hi, len(pats), np.uint8, limit)


# ---- class patterns (kolm_find_classes_device, kolm_reader_find_classes) --------------------
# A pattern is passed as its positions' 32-byte bitmaps back to back (ClassPattern.bitmaps).

def _class_arrays(pats):
    off = np.zeros(len(pats) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(p) // 32 for p in pats])
    flat = np.frombuffer(b"".join(bytes(p) for p in pats) + bytes(32), dtype=np.uint8)
    return flat, off


def find_classes_device(ctx, dptr: int, n: int, bitmaps, limit=None):
    """kolm_find_classes_device over the n bytes at the device address dptr; returns what
    find_device returns.  The patterns are passed as given."""
    pats = list(bitmaps)
    flat, off = _class_arrays(pats)
    lead = (ctx, dptr, n, flat.ctypes.data, off.ctypes.data, len(pats))
    return _find_device_call(load().kolm_find_classes_device, lead, len(pats), np.uint8, limit)


def find_classes_bytes(data, bitmaps, limit=None, device: int = None, data_offset: int = 0):
    """Uploads data data_offset (0..15) bytes into a buffer and searches it (find_classes_device)."""
    return _on_device(data, data_offset, device, lambda ctx, p: find_classes_device(ctx, p, len(data), bitmaps, limit))


def reader_find_classes(h, bitmaps, lo: int, hi: int, limit=None):
    """kolm_reader_find_classes + kolm_reader_find_copy; returns and raises as reader_find."""
    pats = list(bitmaps)
    flat, off = _class_arrays(pats)
    L = load()
    return _reader_find_call(L.kolm_reader_find_classes, L.kolm_reader_find_copy, h,
                             (flat.ctypes.data, off.ctypes.data, len(pats)), lo, hi, len(pats), np.uint8, limit)


# ---- regular expressions (kolm_find_dfa_device, kolm_reader_find_dfa) -----------------------
# The expressions of a call are passed as one automaton: a kolm.regex.Table, or anything with its
# cls_map (256 bytes), T (a (nstates, ncls) uint16 array) and starts.

def _dfa_arrays(table):
    cls = np.frombuffer(bytes(table.cls_map), dtype=np.uint8)
    T = np.ascontiguousarray(table.T, dtype=np.uint16)
    starts = np.asarray(list(table.starts) + [0], dtype=np.uint16)
    if cls.size != 256 or T.ndim != 2:
        raise ValueError("an automaton has a class map of 256 bytes and a table of states x classes")
    return cls, T, starts, len(table.starts)


def find_dfa_device(ctx, dptr: int, n: int, table, limit=None):
    """kolm_find_dfa_device over the n bytes at the device address dptr; returns what find_device
    returns.  The automaton is passed as given."""
    cls, T, starts, ne = _dfa_arrays(table)
    lead = (ctx, dptr, n, cls.ctypes.data, T.ctypes.data, T.shape[0], T.shape[1], starts.ctypes.data, ne)
    return _find_device_call(load().kolm_find_dfa_device, lead, ne, np.uint8, limit)


def find_dfa_bytes(data, table, limit=None, device: int = None, data_offset: int = 0):
    """Uploads data data_offset (0..15) bytes into a buffer and searches it (find_dfa_device)."""
    return _on_device(data, data_offset, device, lambda ctx, p: find_dfa_device(ctx, p, len(data), table, limit))


def reader_find_dfa(h, table, lo: int, hi: int, limit=None):
    """kolm_reader_find_dfa + kolm_reader_find_copy; returns and raises as reader_find."""
    cls, T, starts, ne = _dfa_arrays(table)
    L = load()
    return _reader_find_call(L.kolm_reader_find_dfa, L.kolm_reader_find_copy, h,
                             (cls.ctypes.data, T.ctypes.data, T.shape[0], T.shape[1], starts.ctypes.data, ne), lo, hi, ne,
                             np.uint8, limit)


# ---- pattern sets (kolm_patset_create, kolm_find_set_device, kolm_reader_find_set) ---------

def set_patterns(patterns) -> list:
    """The patterns of a set as a list of bytes; ValueError for what the library refuses (no
    pattern or more than 65 536, an empty one, one of more than 256 bytes, two equal ones)."""
    if isinstance(patterns, (bytes, bytearray, memoryview, str)):
        raise TypeError("patterns must be a sequence of bytes-like objects")
    pats = [memoryview(p).tobytes() for p in patterns]
    if not 1 <= len(pats) <= KOLM_FIND_SET_MAX_PATTERNS:
        raise ValueError(f"{len(pats)} patterns (1..{KOLM_FIND_SET_MAX_PATTERNS} are allowed)")
    seen = {}
    for i, p in enumerate(pats):
        if not p:
            raise ValueError(f"pattern {i} is empty")
        if len(p) > KOLM_FIND_MAX_LEN:
            raise ValueError(f"pattern {i} has {len(p)} bytes (at most {KOLM_FIND_MAX_LEN})")
        if seen.setdefault(p, i) != i:
            raise ValueError(f"patterns {seen[p]} and {i} are equal (a set holds distinct patterns)")
    return pats


def patset_create(patterns, ctx=None):
    """kolm_patset_create on ctx (None: the default context) with the patterns as given: the
    library's argument errors raise ValueError.  Returns (handle, info dict)."""
    ensure_init()
    pats = list(patterns)
    flat, off = _pattern_arrays(pats)
    h = ctypes.c_void_p()
    L = load()
    rc = L.kolm_patset_create(ctx, flat.ctypes.data, off.ctypes.data, len(pats), ctypes.byref(h))
    if rc == -1:
        raise ValueError(L.kolm_last_error().decode())
    check(rc)
    info = PatsetInfo()
    check(L.kolm_patset_info(h, ctypes.byref(info)))
    return h, info.as_dict()


def patset_free(h):
    load().kolm_patset_free(h)


def find_set_device(ctx, dptr: int, n: int, pset, limit=None, cap=None):
    """kolm_find_set_device over the n bytes at the device address dptr with the set handle
    pset (np from its info).  Returns (offsets, pattern indices, counts per pattern, device ms).
    cap: the capacity of the first call (default 0: the two-call pattern always runs)."""
    L = load()
    info = PatsetInfo()
    check(L.kolm_patset_info(pset, ctypes.byref(info)))
    return _find_device_call(L.kolm_find_set_device, (ctx, dptr, n, pset), info.np, np.uint32, limit, cap)


def find_set_bytes(data, patterns, limit=None, data_offset: int = 0, device: int = None, cap=None):
    """Uploads data data_offset (0..15) bytes into a buffer, makes a set of the patterns in that
    buffer's context and searches (find_set_device)."""
    def run(ctx, p):
        h, _ = patset_create(patterns, ctx)
        try:
            return find_set_device(ctx, p, len(data), h, limit, cap)
        finally:
            patset_free(h)
    return _on_device(data, data_offset, device, run)


def reader_find_set(h, pset, np_: int, lo: int, hi: int, limit=None):
    """kolm_reader_find_set + kolm_reader_find_copy32.  Returns (offsets, pattern indices, counts
    per pattern); the stats go to last_find().  Errors as reader_find."""
    L = load()
    return _reader_find_call(L.kolm_reader_find_set, L.kolm_reader_find_copy32, h, (pset,), lo, hi, np_, np.uint32, limit)


def reader_read_device(h, ranges, dptr: int, cap: int):
    """kolm_reader_read_device: the packed bytes stay at the device address dptr (cap bytes)."""
    global _last_read
    offs, lens = _ranges_arrays(ranges)
    st = ReadStats()
    _read_check(load().kolm_reader_read_device(h, offs.ctypes.data, lens.ctypes.data, len(ranges), dptr, cap,
                                               ctypes.byref(st)))
    _last_read = st.as_dict()


# ---- line index (kolm_delim_count_device, kolm_reader_line_*) ------------------------------

_last_lines_stats: dict = {}
_LINES_MSG = re.compile(r"block (\d+): expected (\d+) delimiters, got (\d+)")


def last_lines() -> dict:
    """kolm_lines_stats of the last line call made through this binding."""
    return dict(_last_lines_stats)


def delim_count_device(ctx, d_data: int, bounds, delim: int):
    """kolm_delim_count_device: (the blocks' delimiter counts as a list, k_delim_count's device ms)."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    nb = len(b) - 1
    cnt = np.zeros(max(nb, 1), dtype=np.uint32)
    ms = ctypes.c_double(0.0)
    check(load().kolm_delim_count_device(ctx, d_data, b.ctypes.data, nb, delim, cnt.ctypes.data, ctypes.byref(ms)))
    return [int(c) for c in cnt[:nb]], ms.value


def delim_count_pieces_device(ctx, d_data: int, bounds, delim: int):
    """kolm_delim_count_pieces_device: (the blocks' counts, their 4 KiB pieces' counts block after
    block, device ms of k_delim_count and the scan of the piece counts)."""
    b = np.ascontiguousarray(np.asarray(bounds, dtype=np.uint64))
    nb = len(b) - 1
    npc = int(((np.diff(b) + np.uint64(4095)) // np.uint64(4096)).sum()) if nb else 0
    cnt, pc = np.zeros(max(nb, 1), dtype=np.uint32), np.zeros(max(npc, 1), dtype=np.uint32)
    ms = ctypes.c_double(0.0)
    check(load().kolm_delim_count_pieces_device(ctx, d_data, b.ctypes.data, nb, delim, cnt.ctypes.data, pc.ctypes.data, npc,
                                                ctypes.byref(ms)))
    return [int(c) for c in cnt[:nb]], [int(c) for c in pc[:npc]], ms.value


def delim_counts(data, delim: int, block_size=None, bounds=None, device: int = None, data_offset: int = 0):
    """Uploads data and returns its blocks' counts of the byte `delim` (delim_count_device).  bounds
    may hold empty blocks (equal neighbours): their count is 0."""
    n = len(data)
    if bounds is None:
        if n == 0:
            return []
        b = _bounds_array(n, block_size, None)
    else:
        bl = [int(x) for x in bounds]
        if not bl or bl[0] != 0 or bl[-1] != n or any(y < x for x, y in zip(bl, bl[1:])):
            raise ValueError("bounds must start at 0, not decrease and end at len(data)")
        b = np.ascontiguousarray(np.asarray(bl, dtype=np.uint64))
    return _on_device(data, data_offset, device, lambda ctx, p: delim_count_device(ctx, p, b, delim))[0]


def lines_locate(counts, idx):
    """kolm_lines_locate (host only): [(block, number inside the block)] of the delimiter numbers
    idx; ValueError for a number at or above the sum of counts."""
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.uint32))
    i = np.ascontiguousarray(np.asarray(idx, dtype=np.uint64))
    blk, j = np.zeros(max(len(i), 1), dtype=np.uint32), np.zeros(max(len(i), 1), dtype=np.uint32)
    rc = load().kolm_lines_locate(c.ctypes.data, len(c), i.ctypes.data, len(i), blk.ctypes.data, j.ctypes.data)
    if rc == -1:
        raise ValueError(load().kolm_last_error().decode())
    check(rc)
    return [(int(a), int(b)) for a, b in zip(blk[:len(i)], j[:len(i)])]


def lines_locate_offsets(orig_lens, counts, offs):
    """kolm_lines_locate_offsets (host only): [(block, offset inside it, delimiters before the
    block)] of the stream offsets offs; ValueError for an offset above the sum of orig_lens."""
    ln = np.ascontiguousarray(np.asarray(orig_lens, dtype=np.uint32))
    c = np.ascontiguousarray(np.asarray(counts, dtype=np.uint32))
    o = np.ascontiguousarray(np.asarray(offs, dtype=np.uint64))
    m = max(len(o), 1)
    blk, inb, bef = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint64)
    rc = load().kolm_lines_locate_offsets(ln.ctypes.data, c.ctypes.data, len(c), o.ctypes.data, len(o), blk.ctypes.data,
                                          inb.ctypes.data, bef.ctypes.data)
    if rc == -1:
        raise ValueError(load().kolm_last_error().decode())
    check(rc)
    return [(int(a), int(b), int(d)) for a, b, d in zip(blk[:len(o)], inb[:len(o)], bef[:len(o)])]


def _lines_check(rc):
    if rc == KOLM_ELINES:  # the message names the block (kolm.h)
        m = _LINES_MSG.search(load().kolm_last_error().decode())
        if m:
            raise KolmLineIndexError(int(m.group(1)), int(m.group(2)), int(m.group(3)))
        raise KolmLineIndexError(-1, 0, 0)  # a text this binding does not know: still the line index error
    _read_check(rc)


def reader_set_lines(h, delim: int, counts):
    """kolm_reader_set_lines: the delimiter count of every block (None detaches)."""
    if counts is None:
        check(load().kolm_reader_set_lines(h, 0, None, 0))
        return
    c = np.ascontiguousarray(np.asarray(list(counts) or [0], dtype=np.uint32))
    rc = load().kolm_reader_set_lines(h, delim, c.ctypes.data, len(counts))
    if rc == -1:
        raise ValueError(load().kolm_last_error().decode())
    check(rc)


def reader_index_lines(h, delim: int, nblocks: int):
    """kolm_reader_index_lines: builds and attaches the index; returns the counts."""
    global _last_lines_stats
    cnt = np.zeros(max(nblocks, 1), dtype=np.uint32)
    st = LinesStats()
    _lines_check(load().kolm_reader_index_lines(h, delim, cnt.ctypes.data, max(nblocks, 1), ctypes.byref(st)))
    _last_lines_stats = st.as_dict()
    return [int(c) for c in cnt[:nblocks]]


def reader_line_spans(h, lines):
    """kolm_reader_line_spans: [(start, end)] of the lines.  ValueError for what the library
    refuses, KolmChecksumError / KolmLineIndexError as it reports them; last_lines() then keeps
    what it held."""
    global _last_lines_stats
    k = np.ascontiguousarray(np.asarray(lines, dtype=np.uint64))
    m = max(len(k), 1)
    a, b = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
    st = LinesStats()
    _lines_check(load().kolm_reader_line_spans(h, k.ctypes.data, len(k), a.ctypes.data, b.ctypes.data, ctypes.byref(st)))
    _last_lines_stats = st.as_dict()
    return [(int(x), int(y)) for x, y in zip(a[:len(k)], b[:len(k)])]


def reader_line_of(h, offsets):
    """kolm_reader_line_of: the line number of every offset (errors as reader_line_spans)."""
    global _last_lines_stats
    o = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
    out = np.zeros(max(len(o), 1), dtype=np.uint64)
    st = LinesStats()
    _lines_check(load().kolm_reader_line_of(h, o.ctypes.data, len(o), out.ctypes.data, ctypes.byref(st)))
    _last_lines_stats = st.as_dict()
    return [int(x) for x in out[:len(o)]]
