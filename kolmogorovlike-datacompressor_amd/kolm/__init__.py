"""kolm — MI355X-native block-transform hot path of KolmogorovLike-DataCompressor v2-2.

Drop-in for the reference's block API (PY = final_researched/kolm_final_researched_v2-2.py):

    compress_blocks_fixed(data, block_size=8192) -> bytes      PY:2332-2445
    compress_blocks_cdc(data, min_size, avg_size, max_size)    PY:2213-2326
    cdc_fast_boundaries_strict(data, min, avg, max, merge)     PY:210-309
    decompress(container) -> bytes                             PY:2451-2550
    open_container(container) -> Reader                        (not in PY: byte ranges of a
                                                               container, only the touched
                                                               blocks decoded, on the device;
                                                               with lines=: lines of the data,
                                                               kolm.lines)
    _select_encoders() / _select_decoders()                    PY:2152-2207
    bbwt_forward, mtf_encode, rice_encode, encode_lz77,
    encode_bbwt_mtf_rice, encode_raw, encode_xor,
    encode_lfsr_predict, fixed_boundaries, uleb128_encode      (same names / meaning)

Every encode-side computation of candidates 0..9 runs as hand-written HIP kernels on
the GPU (libkolm_hip.so through ctypes, include/kolm.h); the per-block MDL loop of PY
is one batched device call for all blocks.  There is no CPU fallback: without the
library or a HIP device the encode functions raise ``KolmUnavailable``.

Candidate ids are the reference's (the list index is the on-disk method id):
0 raw, 1 xor, 2 bbwt, 3 bbwt_bp, 4 bbwt_nib, 5 bbwt_br, 6 bbwt_gray, 7 lz77,
8 lfsr_pred, 9 repair, 10 v2_new.  v2_new always raises in PY (NameError)
and is never selected, so by default the MDL argmin runs over ids 0..9 exactly as PY's
does and compress_blocks_fixed() returns PY's container byte for byte.  ``G_V2_NEW =
True`` (or ``v2_new=True``) enables id 10 as the pipeline defines it with its automaton
evaluated serially (PY:1033-1035): encode_new_pipeline on the GPU
(csrc/k_v2.hip), bit-exact against PY run that way.  Re-Pair (9) is the exact
batched device Re-Pair of csrc/repair_core.h (blocks up to 4 MiB).  ``hot_path=True``
restricts the candidates to ids 0..8 (the BBWT / MTF+Rice / LZ77 path of the north star;
ids unchanged, containers still decodable by the reference).
"""
from __future__ import annotations

import re
import struct
import sys
import zlib
from typing import Any, Callable, Dict, List, Optional, Tuple

from . import _lib, classes, regex
from .classes import ClassPattern
from .regex import Regex
from ._lib import KolmError, KolmUnavailable, KolmVerifyError  # noqa: F401
from .checksums import Checksums, KolmChecksumError, as_checksums
from .lines import KolmLineIndexError, LineIndex, as_line_index, delim_byte
from .container import (MODE_CDC, MODE_FIXED, read_container, read_toc, uleb128_decode_stream,  # noqa: F401
                        uleb128_encode, write_container)
from .decode import decode_block

__all__ = [
    "compress_blocks_fixed", "compress_blocks_cdc", "cdc_fast_boundaries_strict", "decompress",
    "fixed_boundaries", "bbwt_forward", "mtf_encode",
    "rice_encode", "encode_lz77", "encode_bbwt_mtf_rice", "encode_raw", "encode_xor",
    "encode_lfsr_predict", "repair_compress", "encode_new_pipeline", "decode_new_pipeline", "uleb128_encode", "uleb128_decode_stream", "CANDIDATE_NAMES",
    "KolmUnavailable", "KolmError", "last_stats", "KolmVerifyError", "last_verify", "verify",
    "open_container", "Reader", "PatternSet", "ClassPattern", "classes", "Regex", "regex", "find_regex", "last_read", "find", "last_find", "last_dedup", "duplicate_blocks", "block_fingerprints",
    "Checksums", "KolmChecksumError", "crc32_blocks", "crc32_combine", "last_checksums", "checksums_of", "check",
    "LineIndex", "KolmLineIndexError", "line_index", "line_index_of", "last_line_index", "last_lines",
]

CANDIDATE_NAMES = ["raw", "xor", "bbwt", "bbwt_bp", "bbwt_nib", "bbwt_br", "bbwt_gray", "lz77",
                   "lfsr_pred", "repair", "v2_new"]
GPU_CANDIDATES = 11

# CLI-style switches of the reference (PY:92-96); ids stay stable (CPP:3750-3775 semantics)
G_NO_LZ77: bool = False
G_ONLY_METHOD: Optional[str] = None
# candidate 10 (v2_new) with its automaton evaluated serially; PY as shipped raises instead
G_V2_NEW: bool = False
# verify-after-encode (not in PY): every encode batch is decoded on the device and compared
# with its input before the call returns; a bad block raises KolmVerifyError
G_VERIFY: bool = False
# dedup (not in PY): every device batch encodes its repeated blocks once and copies the payload
# to the repeats; the output is byte for byte the same, the saving is time
G_DEDUP: bool = False
# checksums (not in PY): every device batch takes the CRC-32 of its blocks on the resident input;
# the container's bytes do not change, the manifest is last_checksums() (kolm.checksums)
G_CHECKSUMS: bool = False
# line index (not in PY): every device batch counts the delimiter bytes of its blocks on the resident
# input; the container's bytes do not change, the index is last_line_index() (kolm.lines).  True
# (the delimiter b"\n") or a one-byte delimiter
G_LINES = False

_last_stats: Dict[str, Any] = {}


def last_stats() -> Dict[str, Any]:
    """Device statistics of the last batched call (rounds, active positions, ms per stage)."""
    return dict(_last_stats)


def last_verify() -> Dict[str, Any]:
    """Report of the last verified encode call (kolm_verify_report): blocks, bad_blocks,
    first_bad_block / _method / _offset / _reason, bytes, ms_decode, ms_compare."""
    return _lib.last_verify()


def _want_verify(verify: Optional[bool]) -> bool:
    return G_VERIFY if verify is None else bool(verify)


def last_dedup() -> Dict[str, Any]:
    """Report of the last encode call when it ran with dedup on (kolm_dedup_report): blocks,
    blocks_encoded, candidate_pairs, collisions, bytes, bytes_encoded, ms_hash, ms_compare,
    ms_compact, ms_expand, summed over the call's device batches; empty when it ran with dedup off."""
    return _lib.last_dedup()


def _want_dedup(dedup: Optional[bool]) -> bool:
    return G_DEDUP if dedup is None else bool(dedup)


def duplicate_blocks(data: bytes, block_size: Optional[int] = None, bounds=None) -> List[int]:
    """The duplicate map of data's blocks (fixed blocks of block_size, or bounds[i]..bounds[i+1]),
    found on the device without encoding anything: rep[i] = i for a block that would be encoded,
    else the lower-numbered block with the same bytes that the plan paired it with
    (kolm_dedup_plan: the first block of its length and fingerprint).  Fingerprints propose the
    candidates, a byte-for-byte compare settles them; with real fingerprints a duplicate's
    representative is the earliest block with its bytes, while a block whose fingerprint
    collides with a different block's ($KOLM_DEDUP_BITS makes that happen) is its own
    representative even when an identical block came before it."""
    rep, _ = _lib.duplicate_blocks(data, block_size, bounds)
    return [int(r) for r in rep]


def block_fingerprints(data: bytes, block_size: Optional[int] = None, bounds=None, data_offset: int = 0):
    """The device's 128-bit fingerprints of data's blocks, u64[nb, 2] (for tests: the function
    may change between versions and must not be persisted)."""
    return _lib.block_fingerprints(data, block_size, bounds, data_offset=data_offset)


def _want_checksums(checksums: Optional[bool]) -> bool:
    return G_CHECKSUMS if checksums is None else bool(checksums)


_last_checksums: Optional[Checksums] = None


def last_checksums() -> Optional[Checksums]:
    """The manifest (kolm.checksums.Checksums) of the last encode call of this module when it
    ran with checksums on: every block's CRC-32, taken on the device from the resident input,
    and their combination, the CRC-32 of the whole input.  None when it ran with checksums off."""
    return _last_checksums


def _keep_checksums(want: bool, mode: int, size_field: int, data, lens, multi_block_size: Optional[int] = None) -> None:
    """After an encode call: the manifest from the words the call left (kolm_ctx_checksums), or,
    for a multi-device call (its contexts ignore the switch), from one crc32_blocks pass."""
    global _last_checksums
    _last_checksums = None
    crcs = _lib.last_crcs()
    if multi_block_size is not None and (want or _lib._ENV_CHECKSUMS):
        crcs = crc32_blocks(data, multi_block_size)
    if crcs is not None:
        _last_checksums = Checksums(mode, size_field, len(data), lens, crcs)


def _keep_empty(want: bool, mode: int, size_field: int) -> None:
    """Empty input: nothing is launched; with checksums on the manifest is the empty one, not None."""
    global _last_checksums
    _last_checksums = Checksums(mode, size_field, 0, [], []) if want or _lib._ENV_CHECKSUMS else None


def _want_lines(lines) -> Optional[int]:
    """The delimiter byte of an encode call's `lines` argument (None: G_LINES), or None for off."""
    if lines is None:
        lines = G_LINES
    if lines is False:
        return None
    return 0x0A if lines is True else delim_byte(lines)


_last_line_index: Optional[LineIndex] = None


def last_line_index() -> Optional[LineIndex]:
    """The line index (kolm.lines.LineIndex) of the last encode call of this module when it ran
    with lines on: every block's delimiter count, taken on the device from the resident input.
    None when it ran with lines off."""
    return _last_line_index


def _keep_lines(delim: Optional[int], mode: int, size_field: int, data, lens, multi_block_size: Optional[int] = None) -> None:
    """After an encode call: the index from the counts the call left (kolm_ctx_lines), or, for a
    multi-device call (its contexts ignore the switch), from one line_index pass."""
    global _last_line_index
    _last_line_index = None
    got = _lib.last_lines_counts()
    if multi_block_size is not None and (delim is not None or _lib._ENV_LINES):
        d = _lib._ENV_LINES_DELIM if delim is None else delim
        got = (d, _lib.delim_counts(data, d, multi_block_size))
    if got is not None:
        _last_line_index = LineIndex(mode, size_field, len(data), lens, got[0], got[1])


def _keep_empty_lines(delim: Optional[int], mode: int, size_field: int) -> None:
    """Empty input: nothing is launched; with lines on the index is the empty one, not None."""
    global _last_line_index
    if delim is None and _lib._ENV_LINES:
        delim = _lib._ENV_LINES_DELIM
    _last_line_index = None if delim is None else LineIndex(mode, size_field, 0, [], delim, [])


def line_index(data: bytes, block_size: Optional[int] = None, bounds=None, delim=b"\n", data_offset: int = 0,
               size_field: int = 0) -> LineIndex:
    """The line index of data's blocks (fixed blocks of block_size: the index of
    compress_blocks_fixed(data, block_size); or bounds[i]..bounds[i+1], empty blocks allowed: a CDC
    index with the given size field, compress_blocks_cdc's avg_size), counted on the device in one
    streaming pass (k_delim_count).  data_offset (0..15) places the data that many bytes into its
    device buffer."""
    d = delim_byte(delim)
    n = len(data)
    counts = _lib.delim_counts(data, d, block_size, bounds, data_offset=data_offset)
    if bounds is None:
        if not block_size or block_size <= 0:
            raise ValueError("give a positive block_size or bounds")
        return LineIndex(MODE_FIXED, block_size, n, [min(block_size, n - i) for i in range(0, n, block_size)], d, counts)
    bl = [int(x) for x in bounds]
    return LineIndex(MODE_CDC, size_field, n, [y - x for x, y in zip(bl, bl[1:])], d, counts)


def line_index_of(container: bytes, delim=b"\n", checksums=None) -> LineIndex:
    """The line index of an existing container: every block is decoded on the device and its
    delimiters counted there (kolm_reader_index_lines); only the counts come back."""
    with Reader(container, checksums=checksums, lines=delim) as r:
        return r.line_index


def crc32_blocks(data: bytes, block_size: Optional[int] = None, bounds=None, data_offset: int = 0) -> List[int]:
    """The standard CRC-32 (zlib.crc32) of data's blocks (fixed blocks of block_size, or
    bounds[i]..bounds[i+1]; empty blocks are allowed and give 0), computed on the device
    (k_crc32).  data_offset (0..15) places the data that many bytes into its device buffer."""
    return _lib.crc32_blocks(data, block_size, bounds, data_offset=data_offset)


def crc32_combine(a: int, b: int, len_b: int) -> int:
    """CRC-32 of A + B from a = CRC-32(A), b = CRC-32(B) and len_b = len(B) (zlib's
    crc32_combine; host arithmetic of the library, no device)."""
    if len_b < 0:
        raise ValueError("len_b must not be negative")
    return _lib.crc32_combine(a, b, len_b)


# ---------------------------------------------------------------------------
# chunking
# ---------------------------------------------------------------------------

def fixed_boundaries(data: bytes, block_size: int = 8192) -> List[Tuple[int, int]]:
    """PY:314-320 (no tail merge — the reference Python does not merge)."""
    n = len(data)
    if n == 0:
        return []
    if block_size <= 0:
        raise ValueError("block_size must be positive")
    return [(i, min(n, i + block_size)) for i in range(0, n, block_size)]


_U31 = 0x7FFFFFFF


def cdc_fast_boundaries_strict(data: bytes, min_size: int = 4096, avg_size: int = 8192, max_size: int = 16384,
                               merge_orphan_tail: bool = True) -> List[Tuple[int, int]]:
    """FastCDC with normalized chunking (PY:210-309) on the GPU (k_cdc.hip), same chunks.

    Note (parity): PY's GEAR entries are all odd (PY:164), so the rolled fingerprint is
    always odd and no mask test ever passes: the reference cuts every chunk at
    min(remaining, max_size) and only the tail rule varies.  The device path evaluates the
    masks as the reference does and reproduces exactly that."""
    n = len(data)
    if n == 0:
        return []
    if not (min_size > 0 and min_size <= avg_size <= max_size):
        raise ValueError("Require 0 < min_size <= avg_size <= max_size")
    if avg_size < 64:
        raise ValueError("avg_size too small; use >= 64")
    # sizes past 2^31 act as 2^31 - 1 (n < 2^31; the mask bits clamp at 20 either way)
    mn, av, mx = min(min_size, _U31), min(avg_size, _U31), min(max_size, _U31)
    s = _lib.cdc_boundaries(bytes(data), mn, av, mx, merge_orphan_tail)
    return [(int(s[i]), int(s[i + 1])) for i in range(len(s) - 1)]


# ---------------------------------------------------------------------------
# kernel-level functions (GPU)
# ---------------------------------------------------------------------------

def bbwt_forward(s: bytes) -> bytes:
    """Bijective BWT (PY:351-423) on the GPU."""
    return _lib.bbwt_forward(bytes(s)) if s else b""


def mtf_encode(data: bytes) -> List[int]:
    """Move-to-front indices (PY:460-468) on the GPU."""
    return list(_lib.mtf_encode(bytes(data))) if data else []


def rice_encode(seq, k: int) -> bytes:
    """Rice code of byte values (PY:1413-1421), byte padded, on the GPU."""
    b = bytes(seq)
    if any(v > 255 for v in b):  # bytes() already guarantees < 256
        raise ValueError("rice_encode: values must be bytes")
    if not 0 <= k <= 15:
        raise ValueError("rice_encode: k must be in [0, 15]")
    return _lib.rice_encode(b, k) if b else b""


def encode_lz77(block: bytes) -> Tuple[bytes, Dict[str, Any]]:
    """LZ77, 4 KiB window, ULEB tokens (PY:1711-1763) on the GPU."""
    return (_lib.lz77_encode(bytes(block)) if block else b""), {}


def encode_bbwt_mtf_rice(block: bytes, use_bitplane: bool = False, use_lfsr: bool = False,
                         use_nibble: bool = False, use_bitrev: bool = False, use_gray: bool = False,
                         rice_param: int = 2) -> Tuple[bytes, Dict[str, Any]]:
    """BBWT -> MTF -> [one bitwise map] -> Rice (PY:2028-2073) on the GPU.

    The reference applies the maps in the order bitplane, lfsr, nibble, bitrev, gray; the
    candidates use at most one (PY:2156-2160), which is what the device path supports.
    """
    flags = (1 if use_bitplane else 0) | (2 if use_lfsr else 0) | (4 if use_nibble else 0) \
        | (8 if use_bitrev else 0) | (16 if use_gray else 0)
    if flags not in (0, 1, 4, 8, 16):
        raise NotImplementedError("only single bitwise maps (the reference candidates) are offloaded")
    n = len(block)
    payload = _lib.bbwt_mtf_rice(bytes(block), flags, rice_param) if n else b""
    length = 8 * ((n + 7) // 8) if flags & 1 else n
    return payload, {"flags": flags, "k": rice_param, "length": length, "orig_len": n}


def _batched_single(block: bytes, mid: int) -> bytes:
    if not block:
        return b""
    _, _, payloads, _ = _lib.encode_blocks(bytes(block), len(block), cand_mask=1 << mid, force=[mid])
    return payloads[0]


def encode_raw(block: bytes) -> Tuple[bytes, Dict[str, Any]]:  # PY:2098
    return bytes(block), {}


def encode_xor(block: bytes) -> Tuple[bytes, Dict[str, Any]]:  # PY:2105-2111 (GPU emit)
    return _batched_single(block, 1), {}


def encode_lfsr_predict(block: bytes) -> Tuple[bytes, Dict[str, Any]]:  # PY:1984-2003 (GPU emit)
    return _batched_single(block, 8), {}


def repair_compress(block: bytes) -> Tuple[bytes, Dict[str, Any]]:
    """Strict Re-Pair grammar, ULEB-serialised (PY:1841-1911), on the GPU.  The reference's
    meta dict carries its rule table for introspection; here it carries the counts."""
    block = bytes(block)
    if not block:
        from .container import uleb128_encode as _u
        return b"RP" + _u(256) + _u(0) + _u(0), {"rules": {}, "final_len": 0}
    if len(block) > _lib.KOLM_REPAIR_MAX_BLOCK:
        raise ValueError("repair: blocks up to 4 MiB are supported on the device")
    _, _, payloads, st = _lib.encode_blocks(block, len(block), cand_mask=1 << 9, force=[9])
    return payloads[0], {"nrules": st.get("rp_rules"), "final_len": st.get("rp_final"), "terminals": 256}


def encode_new_pipeline(block: bytes) -> bytes:
    """v2_new (PY:1498-1576) with the automaton evaluated serially, on the GPU."""
    return _batched_single(bytes(block), 10)


def decode_new_pipeline(payload: bytes, n: int) -> bytes:
    """Inverse of encode_new_pipeline (decode_new_pipeline PY:1578-1648, the automaton inverse
    PY:1056-1092) on the GPU (csrc/k_v2dec.hip): one kolm_decode_blocks call.  Rice parameters
    up to 15 (all an encoder writes); kolm.decode.decode_new_pipeline is the host decoder."""
    try:
        return _lib.decode_blocks([bytes(payload)], [10], [n])
    except _lib.KolmError as e:
        raise ValueError(str(e)) from None


_V2_DEVICE_MAX = 1 << 28  # kolm_decode_blocks refuses longer id-10 blocks (8 plane blocks index in 32 bits)


def _v2_k_above_15(payload: bytes) -> bool:
    """Header peek of an id-10 payload: does its k list hold a Rice parameter the device does
    not decode (> 15; PY's decoder accepts any byte, no encoder writes one)?"""
    if len(payload) < 3 or (payload[0] & 7) > 4 or len(payload) < 3 + (payload[0] & 7):
        return False
    pos = 1 + (payload[0] & 7)
    nenc = 8 - bin(payload[pos]).count("1")
    return any(k > 15 for k in payload[pos + 2:pos + 2 + nenc])


def _v2_new(block: bytes):
    if not G_V2_NEW:
        raise NameError("v2_new raises in the reference (PY:1037-1043); never selected")
    return encode_new_pipeline(block), {}


def _select_encoders() -> List[Tuple[Callable[[bytes], Tuple[bytes, Dict[str, Any]]], str]]:
    """Candidate registry (PY:2152-2178); list index = on-disk method id.  Unlike PY's
    --only/--no-lz77 (which renumber and produce undecodable containers),
    disabled candidates keep their ids (their entries raise and are skipped)."""
    encs = [
        (encode_raw, "raw"),
        (encode_xor, "xor"),
        (lambda b: encode_bbwt_mtf_rice(b, False, False, False, False, False, rice_param=2), "bbwt"),
        (lambda b: encode_bbwt_mtf_rice(b, True, False, False, False, False, rice_param=2), "bbwt_bp"),
        (lambda b: encode_bbwt_mtf_rice(b, False, False, True, False, False, rice_param=2), "bbwt_nib"),
        (lambda b: encode_bbwt_mtf_rice(b, False, False, False, True, False, rice_param=2), "bbwt_br"),
        (lambda b: encode_bbwt_mtf_rice(b, False, False, False, False, True, rice_param=2), "bbwt_gray"),
        (encode_lz77, "lz77"),
        (encode_lfsr_predict, "lfsr_pred"),
        (repair_compress, "repair"),
        (_v2_new, "v2_new"),
    ]
    mask = candidate_mask()

    def disabled(_b):
        raise RuntimeError("candidate disabled")

    return [(e if (mask >> i) & 1 or (i == 10 and not G_V2_NEW) else disabled, n) for i, (e, n) in enumerate(encs)]


def _select_decoders():
    """Decoder registry aligned with the encoder ids (PY:2194-2207)."""
    return [(lambda payload, n, meta=None, _m=m: decode_block(_m, payload, n)) for m in range(11)]


def candidate_mask(hot_path: bool = False, v2_new: Optional[bool] = None) -> int:
    mask = _lib.KOLM_HOTPATH_MASK if hot_path else _lib.KOLM_DEFAULT_MASK
    if (G_V2_NEW if v2_new is None else v2_new) and not hot_path:
        mask |= 1 << 10
    if G_NO_LZ77:
        mask &= ~(1 << 7)
    if G_ONLY_METHOD is not None:
        name = G_ONLY_METHOD.lower()
        if name not in CANDIDATE_NAMES:
            raise ValueError(f"--only={G_ONLY_METHOD} not found in candidates")
        idx = CANDIDATE_NAMES.index(name)
        if idx >= GPU_CANDIDATES:
            raise ValueError(f"--only={G_ONLY_METHOD}: candidate not offloaded")
        if idx == 10 and not (G_V2_NEW if v2_new is None else v2_new):
            # PY: the only candidate raises, and so does its raw fallback call (PY:2363-2364)
            raise NameError("v2_new raises in the reference (PY:1037-1043); enable G_V2_NEW to compute it")
        mask = 1 << idx
    return mask


# ---------------------------------------------------------------------------
# block API
# ---------------------------------------------------------------------------

def encode_blocks(data: bytes, block_size: int, cand_mask: Optional[int] = None, devices: int = 1,
                  hot_path: bool = False, v2_new: Optional[bool] = None, verify: Optional[bool] = None,
                  dedup: Optional[bool] = None, checksums: Optional[bool] = None, lines=None):
    """Batched device MDL over fixed blocks: (method_ids, orig_lens, payloads, sizes).
    devices > 1 shards the blocks over that many GPUs of this process.  `verify` (default
    G_VERIFY): the payloads are decoded and compared with the input on the device before the
    call returns (KolmVerifyError otherwise).  `dedup` (default G_DEDUP): repeated blocks are
    encoded once per device batch (same result; last_dedup()).  `checksums` (default
    G_CHECKSUMS): the blocks' CRC-32 are taken on the device from the resident input
    (last_checksums(); with devices > 1 from one separate crc32_blocks pass).  `lines` (default
    G_LINES; True or a one-byte delimiter): the blocks' delimiter counts are taken the same way
    (last_line_index())."""
    if block_size <= 0:
        raise ValueError("block_size must be positive")
    global _last_stats, _last_checksums, _last_line_index
    mask = candidate_mask(hot_path, v2_new) if cand_mask is None else cand_mask
    n = len(data)
    _last_checksums = None
    _last_line_index = None
    ld = _want_lines(lines)
    if n == 0:
        _keep_empty(_want_checksums(checksums), MODE_FIXED, block_size)
        _keep_empty_lines(ld, MODE_FIXED, block_size)
        return [], [], [], None
    if devices > 1:
        sizes, method, payloads, st = _lib.encode_blocks_multi(bytes(data), block_size, devices, mask,
                                                               verify=_want_verify(verify), dedup=_want_dedup(dedup))
    else:
        sizes, method, payloads, st = _lib.encode_blocks(bytes(data), block_size, mask, verify=_want_verify(verify),
                                                         dedup=_want_dedup(dedup), checksums=_want_checksums(checksums),
                                                         lines=ld)
    _last_stats = st
    orig = [min(block_size, n - i) for i in range(0, n, block_size)]
    _keep_checksums(_want_checksums(checksums), MODE_FIXED, block_size, data, orig, block_size if devices > 1 else None)
    _keep_lines(ld, MODE_FIXED, block_size, data, orig, block_size if devices > 1 else None)
    return [int(m) for m in method], orig, payloads, sizes


def compress_blocks_fixed(data: bytes, block_size: int = 8192, devices: int = 1, hot_path: bool = False,
                          v2_new: Optional[bool] = None, verify: Optional[bool] = None,
                          dedup: Optional[bool] = None, checksums: Optional[bool] = None, lines=None) -> bytes:
    """Fixed-size chunking + per-block MDL selection + KOLR container (PY:2332-2445).
    `devices` (not in PY) spreads the blocks over that many GPUs of this process;
    `hot_path` (not in PY) restricts the candidates to ids 0..8; `v2_new` (default
    G_V2_NEW) adds candidate 10 (see the module docstring); `verify` (not in PY, default
    G_VERIFY) checks on the device that every payload decodes to its block before the
    container is handed out (KolmVerifyError, and no container, otherwise; last_verify());
    `dedup` (not in PY, default G_DEDUP) encodes the repeated blocks of every device batch once
    and copies the payload to the repeats: the same container in less time (last_dedup());
    `checksums` (not in PY, default G_CHECKSUMS) takes the CRC-32 of every block on the device
    from the resident input: the same container, and last_checksums() is its manifest (with
    devices > 1 the manifest comes from one separate crc32_blocks pass over the data); `lines`
    (not in PY, default G_LINES; True for b"\n" or a one-byte delimiter) counts that byte in every
    block the same way: the same container, and last_line_index() is its line index."""
    if block_size <= 0:
        raise ValueError("block_size must be positive")
    global _last_stats, _last_checksums, _last_line_index
    _last_checksums = None
    _last_line_index = None
    ld = _want_lines(lines)
    n = len(data)
    nb = (n + block_size - 1) // block_size
    if nb > 0xFFFF:
        raise struct.error("'H' format requires 0 <= number <= 65535")
    if devices > 1:
        mids, orig, payloads, _ = encode_blocks(data, block_size, devices=devices, hot_path=hot_path, v2_new=v2_new,
                                                verify=verify, dedup=dedup, checksums=checksums,
                                                lines=False if ld is None else ld)
        return write_container(MODE_FIXED, block_size, n, mids, orig, payloads)
    if n == 0:
        _keep_empty(_want_checksums(checksums), MODE_FIXED, block_size)
        _keep_empty_lines(ld, MODE_FIXED, block_size)
        return write_container(MODE_FIXED, block_size, 0, [], [], [])
    # one native call: staged upload, batched encode, TOC, payloads into the container
    blob, st = _lib.compress_fixed(data, block_size, candidate_mask(hot_path, v2_new), verify=_want_verify(verify),
                                   dedup=_want_dedup(dedup), checksums=_want_checksums(checksums), lines=ld)
    _last_stats = st
    orig = [min(block_size, n - i) for i in range(0, n, block_size)]
    _keep_checksums(_want_checksums(checksums), MODE_FIXED, block_size, data, orig)
    _keep_lines(ld, MODE_FIXED, block_size, data, orig)
    return blob


def compress_blocks_cdc(data: bytes, min_size: int = 4096, avg_size: int = 8192, max_size: int = 16384,
                        hot_path: bool = False, v2_new: Optional[bool] = None, verify: Optional[bool] = None,
                        dedup: Optional[bool] = None, checksums: Optional[bool] = None, lines=None) -> bytes:
    """FastCDC chunking + per-block MDL selection + KOLR container in CDC mode
    (PY:2213-2326): boundaries and every candidate on the GPU, one batched device call for
    all chunks (variable block geometry), the TOC on the host.  `hot_path` (not in PY)
    restricts the candidates to ids 0..8; `verify`, `dedup`, `checksums` and `lines` as in
    compress_blocks_fixed (identical chunks are encoded once; this adds no shift resistance to
    the chunking)."""
    global _last_stats, _last_checksums, _last_line_index
    _last_checksums = None
    _last_line_index = None
    ld = _want_lines(lines)
    bounds = cdc_fast_boundaries_strict(data, min_size, avg_size, max_size)
    if len(bounds) > 0xFFFF:  # PY packs the block count as '<H' before encoding (PY:2222)
        raise struct.error("'H' format requires 0 <= number <= 65535")
    n = len(data)
    if n == 0:
        _keep_empty(_want_checksums(checksums), MODE_CDC, avg_size)
        _keep_empty_lines(ld, MODE_CDC, avg_size)
        return write_container(MODE_CDC, avg_size, 0, [], [], [])
    edges = [s for s, _ in bounds] + [n]
    _, method, payloads, st = _lib.encode_blocks_var(bytes(data), edges, candidate_mask(hot_path, v2_new),
                                                     verify=_want_verify(verify), dedup=_want_dedup(dedup),
                                                     checksums=_want_checksums(checksums), lines=ld)
    _last_stats = st
    _keep_checksums(_want_checksums(checksums), MODE_CDC, avg_size, data, [e - s for s, e in bounds])
    _keep_lines(ld, MODE_CDC, avg_size, data, [e - s for s, e in bounds])
    return write_container(MODE_CDC, avg_size, n, [int(m) for m in method], [e - s for s, e in bounds], payloads)


def _match_toc(cs: Checksums, mode: int, size_field: int, total_len: int, orig) -> None:
    """A manifest belongs to a container when mode, size_field, total_len and every block
    length agree with its TOC."""
    if (cs.mode, cs.size_field, cs.total_len) != (mode, size_field, total_len):
        raise ValueError(f"checksums: the manifest is of another container (mode {cs.mode}, size field {cs.size_field}, "
                         f"{cs.total_len} bytes; the container: mode {mode}, size field {size_field}, {total_len} bytes)")
    if cs.lens != [int(n) for n in orig]:
        raise ValueError("checksums: the manifest's block lengths differ from the container's")


def _match_toc_lines(li: LineIndex, mode: int, size_field: int, total_len: int, orig) -> None:
    """A line index belongs to a container when mode, size_field, total_len and every block length
    agree with its TOC."""
    if (li.mode, li.size_field, li.total_len) != (mode, size_field, total_len):
        raise ValueError(f"line index: the index is of another container (mode {li.mode}, size field {li.size_field}, "
                         f"{li.total_len} bytes; the container: mode {mode}, size field {size_field}, {total_len} bytes)")
    if li.lens != [int(n) for n in orig]:
        raise ValueError("line index: the index's block lengths differ from the container's")


def _host_check(i: int, mid: int, want: int, block: bytes) -> None:
    got = zlib.crc32(block)
    if got != want:
        raise KolmChecksumError(i, mid, want, got)


def decompress(container: bytes, device: bool = True, checksums=None) -> bytes:
    """Inverse of compress_blocks_fixed / compress_blocks_cdc / the reference's containers
    (PY:2451-2550).  The TOC is parsed on the host; every block (ids 0..10: raw, xor, the
    BBWT family, lz77, lfsr_pred, Re-Pair and v2_new — KOLM_DECODE_MASK) is decoded on the GPU
    in one kolm_decode_blocks batch (decode side: SURVEY §8f-4).  The host decoders of
    kolm/decode.py take an id outside the device mask and an id-10 block whose header lists a
    Rice parameter above 15 (PY decodes any k byte; the device decodes 0..15, all that an
    encoder writes) or that is 2^28 bytes or longer (the device's id-10 limit); `device=False`
    (not in PY) decodes everything on the host.

    `checksums` (not in PY): a kolm.checksums.Checksums manifest, or its sidecar bytes.  It must
    agree with the TOC (mode, size field, total length, block lengths: ValueError otherwise).
    The blocks decoded on the device are checked there, against their CRC-32, while the decoded
    bytes are still resident (kolm_decode_blocks_crc); blocks the host decoders take are checked
    with zlib.crc32.  A mismatch raises KolmChecksumError (a ValueError: .block .method
    .expected .got) and no data is returned."""
    mode, size_field, total_len, mids, orig, payloads = read_container(container)
    cs = None if checksums is None else as_checksums(checksums)
    if cs is not None:
        _match_toc(cs, mode, size_field, total_len, orig)
    parts: List[Optional[bytes]] = [None] * len(mids)
    if device:
        sel = [i for i, m in enumerate(mids)
               if (_lib.KOLM_DECODE_MASK >> m) & 1
               and not (m == 10 and orig[i] and (orig[i] >= _V2_DEVICE_MAX or _v2_k_above_15(payloads[i])))]
        if sel:
            try:
                dec = _lib.decode_blocks([payloads[i] for i in sel], [mids[i] for i in sel],
                                         [orig[i] for i in sel],
                                         None if cs is None else [cs.crcs[i] for i in sel])
            except KolmChecksumError as e:  # numbered within the call: the container's block number
                bad = sel[e.block]
                for i in range(bad):  # the lowest-numbered bad block is named: host-decoded ones before it first
                    if i not in sel:
                        _host_check(i, mids[i], cs.crcs[i], decode_block(mids[i], payloads[i], orig[i]))
                raise KolmChecksumError(bad, e.method, e.expected, e.got) from None
            except _lib.KolmError as e:
                raise ValueError(str(e)) from None
            pos = 0
            for i in sel:
                parts[i] = dec[pos:pos + orig[i]]
                pos += orig[i]
    out = bytearray()
    for i, (mid, n, p) in enumerate(zip(mids, orig, payloads)):
        if parts[i] is None:
            parts[i] = decode_block(mid, p, n)
            if cs is not None:
                _host_check(i, mid, cs.crcs[i], parts[i])
        out += parts[i]
    if len(out) != total_len:
        raise ValueError(f"Length mismatch: got {len(out)}, expect {total_len}")
    return bytes(out)


def last_read() -> Dict[str, Any]:
    """kolm_read_stats of the last Reader call: ranges, bytes_returned, blocks_decoded,
    bytes_decoded, groups, compactions, ms_decode, ms_gather (a call served by the host
    decoders reports its blocks and bytes with groups = 0 and "host": True)."""
    return dict(_last_read) if _last_read.get("host") else _lib.last_read()


_last_read: Dict[str, Any] = {}


class Reader:
    """Random-access reads of a KOLR container (not in PY): open_container() parses the TOC
    and keeps the payload area resident on the device; every read decodes only the blocks its
    ranges touch, packs the requested bytes on the device (k_range_gather) and brings back
    nothing else.  A context manager; close() frees the resident payloads.

    Blocks the device does not decode — a method id outside KOLM_DECODE_MASK, an id-10 block
    with a Rice parameter byte above 15 or of 2^28 bytes or more, the cases decompress() gives
    to the host decoders — are found at open; a call whose ranges touch one is served by
    kolm.decode.decode_block on the host, for that call (same bytes; no speed claimed).

    `checksums` (a kolm.checksums.Checksums or its sidecar bytes; it must agree with the TOC):
    every read then takes the CRC-32 of the blocks it decodes, on the device where they lie
    (kolm_reader_set_checksums) or with zlib.crc32 for host-decoded blocks, before any byte is
    handed out: a mismatch raises KolmChecksumError and the read returns nothing.

    `lines` (a kolm.lines.LineIndex or its sidecar bytes, which must agree with the TOC; or True /
    a one-byte delimiter to build the index at open: every block decoded once, on the device):
    the record view of the data.  line_count, line_spans, line_of, read_lines and grep then
    decode only the blocks that hold a delimiter they need (kolm_reader_line_spans /
    kolm_reader_line_of); an index that does not describe the decoded bytes raises
    KolmLineIndexError and the call returns nothing."""

    def __init__(self, container: bytes, ctx=None, checksums=None, lines=None):
        blob = bytes(container)
        self._cs = None if checksums is None else as_checksums(checksums)
        self._ctx = ctx
        self._h, info = _lib.reader_open(blob, ctx)
        self.mode, self.size_field = info["mode"], info["size_field"]
        self._total = info["total_len"]
        if self._cs is not None:
            try:
                _match_toc(self._cs, self.mode, self.size_field, self._total, info["orig_lens"])
                _lib.reader_set_checksums(self._h, self._cs.crcs)
            except Exception:
                self.close()
                raise
        starts, pos = [], 0
        for n in info["orig_lens"]:
            starts.append(pos)
            pos += n
        self._starts = starts + [pos]
        self.blocks: List[Tuple[int, int, int]] = list(zip(starts, info["orig_lens"], info["methods"]))
        # host-only blocks (the container's bytes are kept only when there is one)
        self._host_blocks: List[int] = []
        self._blob: Optional[bytes] = None
        need_payload = [i for i, (_, n, m) in enumerate(self.blocks) if m == 10 and n]
        if need_payload or any(not (_lib.KOLM_DECODE_MASK >> m) & 1 for _, _, m in self.blocks):
            payloads = read_container(blob)[5]
            self._host_blocks = [i for i, (_, n, m) in enumerate(self.blocks) if n and (
                not (_lib.KOLM_DECODE_MASK >> m) & 1
                or (m == 10 and (n >= _V2_DEVICE_MAX or _v2_k_above_15(payloads[i]))))]
            if self._host_blocks:
                self._blob = blob
        self._li: Optional[LineIndex] = None
        if lines is not None and lines is not False:
            try:
                self._attach_lines(lines, info["orig_lens"])
            except Exception:
                self.close()
                raise

    def _attach_lines(self, lines, orig) -> None:
        given = isinstance(lines, LineIndex) or (isinstance(lines, (bytes, bytearray, memoryview)) and len(lines) != 1)
        if given:
            li = as_line_index(lines)
            _match_toc_lines(li, self.mode, self.size_field, self._total, orig)
            _lib.reader_set_lines(self._h, li.delim, li.counts)
        else:
            d = 0x0A if lines is True else delim_byte(lines)
            if self._host_blocks:  # a block the device does not decode: the whole index on the host
                data = self._read_host([(0, self._total)])[0]
                li = LineIndex.of_blocks(self.mode, self.size_field, [data[s:s + n] for s, n, _ in self.blocks], d)
                _lib.reader_set_lines(self._h, d, li.counts)
            else:
                li = LineIndex(self.mode, self.size_field, self._total, orig, d,
                               _lib.reader_index_lines(self._h, d, len(self.blocks)))
        self._li = li

    @property
    def line_index(self) -> Optional[LineIndex]:
        """The attached kolm.lines.LineIndex, or None."""
        return self._li

    def __len__(self) -> int:
        return self._total

    def __enter__(self) -> "Reader":
        return self

    def __exit__(self, *exc) -> bool:
        self.close()
        return False

    def __del__(self):
        try:
            if not sys.is_finalizing():  # at interpreter exit the runtime goes down with the process
                self.close()
        except Exception:  # noqa: BLE001
            pass

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            _lib.reader_close(h)

    def _handle(self):
        if self._h is None:
            raise ValueError("I/O operation on closed reader")
        return self._h

    def _check(self, ranges) -> List[Tuple[int, int]]:
        out = []
        for i, (o, n) in enumerate(ranges):
            o, n = int(o), int(n)
            if o < 0 or n < 0 or o + n > self._total:
                raise ValueError(f"range {i}: [{o}, +{n}) is not inside the container's {self._total} bytes")
            out.append((o, n))
        return out

    def _touches_host_block(self, ranges) -> bool:
        for o, n in ranges:
            for b in self._host_blocks:
                s, ln, _ = self.blocks[b]
                if n and o < s + ln and o + n > s:
                    return True
        return False

    def _read_host(self, ranges) -> List[bytes]:
        """The ranges through the host decoders: every touched block decoded once."""
        import bisect
        global _last_read
        _, _, _, mids, orig, payloads = read_container(self._blob)
        dec: Dict[int, bytes] = {}
        out = []
        for o, n in ranges:
            piece = bytearray()
            if n:
                b = bisect.bisect_right(self._starts, o) - 1
                while b < len(mids) and self._starts[b] < o + n:
                    if orig[b]:
                        if b not in dec:
                            dec[b] = decode_block(mids[b], payloads[b], orig[b])
                            if self._cs is not None:
                                _host_check(b, mids[b], self._cs.crcs[b], dec[b])
                        lo, hi = max(o, self._starts[b]), min(o + n, self._starts[b + 1])
                        piece += dec[b][lo - self._starts[b]:hi - self._starts[b]]
                    b += 1
            out.append(bytes(piece))
        _last_read = {"host": True, "ranges": len(ranges), "bytes_returned": sum(n for _, n in ranges),
                      "blocks_decoded": len(dec), "bytes_decoded": sum(len(v) for v in dec.values()), "groups": 0,
                      "compactions": 0, "ms_decode": 0.0, "ms_gather": 0.0}
        return out

    def read_many(self, ranges) -> List[bytes]:
        """The bytes of every (offset, length) in `ranges`, as a list.  Strict: a range outside
        the data raises ValueError before anything is launched.  One device call serves the
        whole list; its packed result is sliced on the host."""
        global _last_read
        h = self._handle()
        ranges = self._check(ranges)
        if self._host_blocks and self._touches_host_block(ranges):
            return self._read_host(ranges)
        _last_read = {}
        packed = _lib.reader_read(h, ranges)
        out, pos = [], 0
        for _, n in ranges:
            out.append(packed[pos:pos + n])
            pos += n
        return out

    def read(self, offset: int = 0, size: int = -1) -> bytes:
        """Like a file's read at `offset`: at most `size` bytes (all the rest when negative),
        clipped at the end of the data."""
        self._handle()
        if offset < 0:
            raise ValueError("negative offset")
        offset = min(int(offset), self._total)
        n = self._total - offset if size is None or size < 0 else min(int(size), self._total - offset)
        return self.read_many([(offset, n)])[0]

    def _window(self, start, end, limit):
        """(lo, hi) of data[start:end]: clipped to the data as slice bounds are; a negative start,
        end or limit raises ValueError."""
        start, end = int(start), self._total if end is None else int(end)
        if start < 0 or end < 0 or (limit is not None and int(limit) < 0):
            raise ValueError("start, end and limit must not be negative")
        return min(start, self._total), min(end, self._total)

    def _search_host(self, lo, hi, limit, npat, hits_of):
        """A search of data[lo:hi] on the host, for a window with a block the device does not
        decode: hits_of(data) yields (offset in data, pattern index) of every match of the npat
        patterns, in any order.  Returns what the device path returns; the stats go to last_find()."""
        global _last_find
        data = self._read_host([(lo, hi - lo)])[0]
        hits, counts = [], [0] * npat
        for o, i in hits_of(data):
            hits.append((lo + o, i))
            counts[i] += 1
        hits.sort()
        if limit is not None:
            hits = hits[:int(limit)]
        rd = dict(_last_read)
        _last_find = {"host": True, "patterns": npat, "matches": sum(counts), "returned": len(hits),
                      "blocks_decoded": rd["blocks_decoded"], "groups": 0, "emit_launches": 0,
                      "bytes_decoded": rd["bytes_decoded"], "bytes_scanned": hi - lo, "ms_decode": 0.0,
                      "ms_find": 0.0}
        return [o for o, _ in hits], [i for _, i in hits], counts

    def _search(self, patterns, start, end, limit):
        """(offsets, pattern indices, counts) of the patterns in data[start:end]."""
        global _last_find
        h = self._handle()
        pats = _lib.find_patterns(patterns)
        lo, hi = self._window(start, end, limit)
        if lo >= hi:  # nothing to search: no device call
            return [], [], [0] * len(pats)
        if self._host_blocks and self._touches_host_block([(lo, hi - lo)]):
            def hits_of(data):
                for i, p in enumerate(pats):
                    o = data.find(p)
                    while o >= 0:
                        yield o, i
                        o = data.find(p, o + 1)
            return self._search_host(lo, hi, limit, len(pats), hits_of)
        offs, which, counts = _lib.reader_find(h, pats, lo, hi, limit)
        _last_find = {}
        return offs, which, counts

    def find(self, pattern, start: int = 0, end: Optional[int] = None, limit: Optional[int] = None,
             ignore_case: bool = False) -> List[int]:
        """Every offset o with start <= o, o + len(pattern) <= end and data[o:o + len] ==
        pattern, ascending, overlapping matches included; with `limit` the first `limit` of
        them.  Searched on the device where the decoded blocks lie (kolm_reader_find): only
        the offsets come back.  start / end are clipped to the data as slice bounds are
        (negative values raise ValueError); the pattern is bytes-like, 1..256 bytes.
        ignore_case: ASCII letters match either case (the class path: find_classes of
        ClassPattern.literal(pattern, True))."""
        if ignore_case:
            return self._search_classes(_folded([pattern]), start, end, limit)[0]
        return self._search([pattern], start, end, limit)[0]

    def find_many(self, patterns, start: int = 0, end: Optional[int] = None,
                  limit: Optional[int] = None, ignore_case: bool = False) -> List[Tuple[int, int]]:
        """(offset, pattern index) of every match of up to 16 patterns, sorted; identical
        patterns are both reported.  ignore_case as find."""
        if ignore_case:
            offs, which, _ = self._search_classes(_folded(patterns), start, end, limit)
            return list(zip(offs, which))
        offs, which, _ = self._search(patterns, start, end, limit)
        return list(zip(offs, which))

    def count(self, pattern, start: int = 0, end: Optional[int] = None, ignore_case: bool = False) -> int:
        """len(find(pattern, start, end)) without listing the matches (no emit launch)."""
        if ignore_case:
            return self._search_classes(_folded([pattern]), start, end, 0)[2][0]
        return self._search([pattern], start, end, 0)[2][0]

    def count_many(self, patterns, start: int = 0, end: Optional[int] = None, ignore_case: bool = False) -> List[int]:
        """The number of matches of every pattern."""
        if ignore_case:
            return self._search_classes(_folded(patterns), start, end, 0)[2]
        return self._search(patterns, start, end, 0)[2]

    def _search_classes(self, pats, start, end, limit):
        """(offsets, pattern indices, counts) of the ClassPatterns `pats` in data[start:end]."""
        global _last_find
        h = self._handle()
        if not 1 <= len(pats) <= _lib.KOLM_FIND_MAX_PATTERNS:
            raise ValueError(f"{len(pats)} patterns (1..{_lib.KOLM_FIND_MAX_PATTERNS} are allowed)")
        if classes.table_classes(pats) > classes.MAX_TABLE_CLASSES:
            raise ValueError(f"the patterns hold {classes.table_classes(pats)} distinct classes that are no masked "
                             f"equality (at most {classes.MAX_TABLE_CLASSES})")
        lo, hi = self._window(start, end, limit)
        if lo >= hi:  # nothing to search: no device call
            return [], [], [0] * len(pats)
        if self._host_blocks and self._touches_host_block([(lo, hi - lo)]):
            def hits_of(data):
                for i, p in enumerate(pats):  # the lookahead finds overlapping matches too
                    for m in re.finditer(b"(?=(" + p.regex() + b"))", data, re.DOTALL):
                        yield m.start(), i
            return self._search_host(lo, hi, limit, len(pats), hits_of)
        offs, which, counts = _lib.reader_find_classes(h, [p.bitmaps for p in pats], lo, hi, limit)
        _last_find = {}
        return offs, which, counts

    def find_classes(self, patterns, start: int = 0, end: Optional[int] = None,
                     limit: Optional[int] = None) -> List[Tuple[int, int]]:
        """(offset, pattern index) of every match of up to 16 class patterns in data[start:end],
        sorted: o matches when data[o + j] lies in the pattern's class j for every j.
        `patterns`: one ClassPattern or expression (bytes, compiled by kolm.classes.compile:
        b"ERROR [0-9]{3}", rb"\\d{4}-\\d{2}-\\d{2}") or a sequence of them.  Overlapping matches,
        identical patterns, start / end / limit as find_many; searched on the device
        (kolm_reader_find_classes).  A call holds at most 64 distinct classes that are no masked
        equality (kolm.classes)."""
        offs, which, _ = self._search_classes(_class_patterns(patterns), start, end, limit)
        return list(zip(offs, which))

    def count_classes(self, patterns, start: int = 0, end: Optional[int] = None) -> List[int]:
        """The number of matches of every class pattern (no emit launch)."""
        return self._search_classes(_class_patterns(patterns), start, end, 0)[2]

    def _search_regex(self, rxs, start, end, limit):
        """(offsets, expression indices, counts) of the Regex objects `rxs` in data[start:end]."""
        global _last_find
        h = self._handle()
        table = regex.table(rxs)  # ValueError: no expression, more than 16, too large an automaton
        lo, hi = self._window(start, end, limit)
        if lo >= hi:  # nothing to search: no device call
            return [], [], [0] * len(rxs)
        if self._host_blocks and self._touches_host_block([(lo, hi - lo)]):
            def hits_of(data):
                for i, r in enumerate(rxs):  # the rule of kolm.h, offset by offset
                    for o in range(len(data)):
                        if r.host.match(data, o, min(len(data), o + regex.MAX_WALK)) is not None:
                            yield o, i
            return self._search_host(lo, hi, limit, len(rxs), hits_of)
        offs, which, counts = _lib.reader_find_dfa(h, table, lo, hi, limit)
        _last_find = {}
        return offs, which, counts

    def find_regex(self, exprs, start: int = 0, end: Optional[int] = None, limit: Optional[int] = None,
                   ignore_case: bool = False) -> List[Tuple[int, int]]:
        """(offset, expression index) of every start of a match of up to 16 regular expressions in
        data[start:end], sorted: o is a match of expression i when some data[o:o + k], 1 <= k <= 256
        and o + k <= end, is matched by it exactly, which is
        re.compile(b"(?:" + expr + b")", re.DOTALL).match(data, o, min(end, o + 256)) is not None.
        `exprs`: one expression (bytes, compiled by kolm.regex.compile: rb"ERROR|WARN(ING)?",
        rb"https?://[^ ]+"), Regex or ClassPattern, or a sequence of them.  Overlapping matches,
        identical expressions, start / end / limit as find_many; only starts are reported, no
        lengths.  Searched on the device (kolm_reader_find_dfa): the expressions become one
        automaton of at most 16 384 transitions (kolm.regex)."""
        offs, which, _ = self._search_regex(regex.as_list(exprs, ignore_case), start, end, limit)
        return list(zip(offs, which))

    def count_regex(self, exprs, start: int = 0, end: Optional[int] = None, ignore_case: bool = False) -> List[int]:
        """The number of matching starts of every expression (no emit launch)."""
        return self._search_regex(regex.as_list(exprs, ignore_case), start, end, 0)[2]

    def _search_set(self, pset, start, end, limit):
        """(offsets, pattern indices, counts) of a PatternSet (or a sequence of patterns: a
        temporary set, closed before returning) in data[start:end]."""
        global _last_find
        h = self._handle()
        if not isinstance(pset, PatternSet):
            with PatternSet(pset, self._ctx) as tmp:
                return self._search_set(tmp, start, end, limit)
        ph = pset._handle()
        pats = pset.patterns
        lo, hi = self._window(start, end, limit)
        if lo >= hi:  # nothing to search: no device call
            return [], [], [0] * len(pats)
        if self._host_blocks and self._touches_host_block([(lo, hi - lo)]):
            def hits_of(data):
                by_len: Dict[int, Dict[bytes, int]] = {}
                for i, p in enumerate(pats):
                    by_len.setdefault(len(p), {})[p] = i
                for ln, table in by_len.items():
                    for o in range(len(data) - ln + 1):
                        i = table.get(data[o:o + ln])
                        if i is not None:
                            yield o, i
            return self._search_host(lo, hi, limit, len(pats), hits_of)
        offs, which, counts = _lib.reader_find_set(h, ph, len(pats), lo, hi, limit)
        _last_find = {}
        return offs, which, counts

    def find_set(self, pset, start: int = 0, end: Optional[int] = None,
                 limit: Optional[int] = None) -> List[Tuple[int, int]]:
        """(offset, pattern index) of every match of a PatternSet (up to 65 536 distinct
        patterns) in data[start:end], sorted: the shape of find_many, from one decode of the
        window and one pass over it (kolm_reader_find_set).  start / end / limit as find.  A
        plain sequence of patterns is accepted too: a temporary set."""
        offs, which, _ = self._search_set(pset, start, end, limit)
        return list(zip(offs, which))

    def count_set(self, pset, start: int = 0, end: Optional[int] = None) -> List[int]:
        """The number of matches of every pattern of the set (no emit launch)."""
        return self._search_set(pset, start, end, 0)[2]

    # ---- lines (kolm.lines) ----

    def _lines(self) -> LineIndex:
        self._handle()
        if self._li is None:
            raise ValueError("no line index is attached: open_container(container, lines=True) builds one, "
                             "lines=<a LineIndex or its sidecar bytes> attaches one")
        return self._li

    def line_count(self) -> int:
        """The number of lines: delimiters + 1 (an empty container has one empty line)."""
        return self._lines().nlines

    def _host_block_positions(self, b: int, cache: Dict[int, List[int]]) -> List[int]:
        """The delimiter positions of block b through the host decoders (checked against the index)."""
        if b not in cache:
            s, n, _ = self.blocks[b]
            data = self._read_host([(s, n)])[0]
            cache[b] = [i for i, v in enumerate(data) if v == self._li.delim]
            if len(cache[b]) != self._li.counts[b]:
                raise KolmLineIndexError(b, self._li.counts[b], len(cache[b]))
        return cache[b]

    def _host_lines_stats(self, queries: int, cache) -> None:
        global _last_lines
        _last_lines = {"host": True, "queries": queries, "blocks_decoded": len(cache), "groups": 0,
                       "bytes_decoded": sum(self.blocks[b][1] for b in cache), "ms_decode": 0.0, "ms_lines": 0.0}

    def line_spans(self, lines) -> List[Tuple[int, int]]:
        """(start, end) of every line number in `lines` (0 .. line_count() - 1; ValueError
        otherwise, before anything is launched): data[start:end] is the line, without its
        delimiter.  Only the blocks that hold a bounding delimiter are decoded: the blocks a long
        line merely passes through are not (kolm_reader_line_spans; last_lines())."""
        global _last_lines
        li, h = self._lines(), self._handle()
        ks = [int(k) for k in lines]
        D = li.delimiters
        for i, k in enumerate(ks):
            if k < 0 or k > D:
                raise ValueError(f"line {i}: {k} is not one of the container's {D + 1} lines")
        if self._host_blocks:
            need = sorted({k - 1 for k in ks if k > 0} | {k for k in ks if k < D})
            loc = _lib.lines_locate(li.counts, need)
            if any(b in self._host_blocks for b, _ in loc):
                cache: Dict[int, List[int]] = {}
                pos = {k: self._starts[b] + self._host_block_positions(b, cache)[j] for k, (b, j) in zip(need, loc)}
                self._host_lines_stats(len(need), cache)
                return [(pos[k - 1] + 1 if k else 0, pos[k] if k < D else self._total) for k in ks]
        _last_lines = {}
        return _lib.reader_line_spans(h, ks)

    def line_of(self, offsets) -> List[int]:
        """The line number of every offset (0 .. len(self)): the delimiters in data[:offset].  A
        delimiter's own offset belongs to the line it ends.  An offset at a block's start or at the
        end of the data is answered from the index alone (kolm_reader_line_of)."""
        global _last_lines
        li, h = self._lines(), self._handle()
        offs = [int(o) for o in offsets]
        for i, o in enumerate(offs):
            if o < 0 or o > self._total:
                raise ValueError(f"offset {i}: {o} is not inside the container's {self._total} bytes")
        if self._host_blocks:
            loc = _lib.lines_locate_offsets([n for _, n, _ in self.blocks], li.counts, offs)
            if any(b in self._host_blocks and inb for b, inb, _ in loc):
                import bisect
                cache: Dict[int, List[int]] = {}
                out = [before + (bisect.bisect_left(self._host_block_positions(b, cache), inb) if inb else 0)
                       for b, inb, before in loc]
                self._host_lines_stats(sum(1 for _, inb, _ in loc if inb), cache)
                return out
        _last_lines = {}
        return _lib.reader_line_of(h, offs)

    def read_lines(self, first: int, count: int = 1) -> List[bytes]:
        """Lines first .. first + count - 1 as a list of bytes (no delimiters), clipped at the last
        line the way read clips at the end of the data: one line_spans call for the two outer
        lines, then one read of the bytes between them."""
        li = self._lines()
        first, count = int(first), int(count)
        if first < 0 or count < 0:
            raise ValueError("first and count must not be negative")
        if first >= li.nlines or count == 0:
            return []
        last = min(first + count, li.nlines) - 1
        (start, _), (_, end) = self.line_spans([first, last])
        return self.read_many([(start, end - start)])[0].split(bytes([li.delim]))

    def grep(self, patterns, start: int = 0, end: Optional[int] = None,
             limit: Optional[int] = None, ignore_case: bool = False) -> List[Tuple[int, bytes]]:
        """(line number, line) of the distinct lines that own at least one match of the patterns in
        data[start:end], ascending; with `limit` the first `limit` lines.  A match belongs to the
        line its first byte lies in (also when the pattern contains the delimiter).  `patterns`: one
        bytes-like pattern, a sequence of them (more than 16: a temporary PatternSet) or a
        PatternSet.  Built from what exists: find_many / find_set, line_of on the match offsets,
        line_spans, read_many.  Up to 16 patterns may also be ClassPatterns (kolm.classes), or
        literals with ignore_case (ASCII letters match either case): the class path of
        find_classes; a PatternSet or more than 16 patterns with either raise ValueError.  Regex
        objects (kolm.regex.compile) among up to 16 patterns put the call on the path of
        find_regex, literals and ClassPatterns next to them converted; a PatternSet or more
        than 16 patterns with them raise ValueError too."""
        self._lines()
        if limit is not None and int(limit) < 0:
            raise ValueError("start, end and limit must not be negative")
        if isinstance(patterns, (bytes, bytearray, memoryview, ClassPattern, Regex)):
            patterns = [patterns]
        if not isinstance(patterns, PatternSet) and any(isinstance(p, Regex) for p in patterns):
            if len(patterns) > _lib.KOLM_FIND_MAX_PATTERNS or any(isinstance(p, PatternSet) for p in patterns):
                raise ValueError(f"regular expressions take at most {_lib.KOLM_FIND_MAX_PATTERNS} patterns and no "
                                 "PatternSet")
            rxs = [regex.as_regex(p, ignore_case) if isinstance(p, (Regex, ClassPattern))
                   else Regex.literal(p, ignore_case) for p in patterns]
            offs, which, _ = self._search_regex(rxs, start, end, None)
            hits = list(zip(offs, which))
        elif ignore_case or (not isinstance(patterns, PatternSet) and any(isinstance(p, ClassPattern) for p in patterns)):
            if isinstance(patterns, PatternSet) or len(patterns) > _lib.KOLM_FIND_MAX_PATTERNS:
                raise ValueError("ignore_case and class patterns take at most "
                                 f"{_lib.KOLM_FIND_MAX_PATTERNS} patterns and no PatternSet")
            pats = [classes.as_pattern(p, ignore_case) if isinstance(p, ClassPattern)
                    else ClassPattern.literal(p, ignore_case) for p in patterns]
            offs, which, _ = self._search_classes(pats, start, end, None)
            hits = list(zip(offs, which))
        elif isinstance(patterns, PatternSet) or len(patterns) > _lib.KOLM_FIND_MAX_PATTERNS:
            hits = self.find_set(patterns, start, end)
        else:
            hits = self.find_many(patterns, start, end)
        offs = sorted({o for o, _ in hits})
        owners = sorted(set(self.line_of(offs))) if offs else []
        if limit is not None:
            owners = owners[:int(limit)]
        if not owners:
            return []
        spans = self.line_spans(owners)
        return list(zip(owners, self.read_many([(s, e - s) for s, e in spans])))

    def read_many_device(self, ranges, dptr: int, cap: int) -> List[int]:
        """The ranges' bytes packed back to back at the device address dptr (cap bytes
        available), left on the device; returns every range's offset in that buffer.  Ranges
        that touch a host-only block raise ValueError here (there is no device result)."""
        global _last_read
        h = self._handle()
        ranges = self._check(ranges)
        if self._host_blocks and self._touches_host_block(ranges):
            raise ValueError("a range touches a block the device does not decode")
        if sum(n for _, n in ranges) > cap:
            raise ValueError("the ranges' bytes exceed the device buffer")
        _last_read = {}
        _lib.reader_read_device(h, ranges, dptr, cap)
        offs, pos = [], 0
        for _, n in ranges:
            offs.append(pos)
            pos += n
        return offs

class PatternSet:
    """Up to 65 536 pairwise distinct patterns of 1..256 bytes, prepared once for
    Reader.find_set / count_set (kolm_patset_create): the hashed tables of the set live on the
    device until close().  ctx (optional): a context of kolm._lib.device_ctx instead of the
    default one; a set serves the readers of its own context.  ValueError for no pattern, more
    than 65 536, an empty one, one of more than 256 bytes and two equal ones.  `.patterns` is
    the tuple of the patterns, `.info` the set's kolm_patset_info: np, key_bytes, keys, slots,
    filter_bits, longest, longest_bucket."""

    def __init__(self, patterns, ctx=None):
        self._h = None
        self.patterns: Tuple[bytes, ...] = tuple(_lib.set_patterns(patterns))
        self._h, self.info = _lib.patset_create(self.patterns, ctx)

    def __len__(self) -> int:
        return len(self.patterns)

    def __enter__(self) -> "PatternSet":
        return self

    def __exit__(self, *exc) -> bool:
        self.close()
        return False

    def __del__(self):
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:  # noqa: BLE001
            pass

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None:
            _lib.patset_free(h)

    def _handle(self):
        if self._h is None:
            raise ValueError("operation on closed pattern set")
        return self._h


def last_lines() -> Dict[str, Any]:
    """kolm_lines_stats of the last Reader.line_spans / line_of (read_lines and grep end with one):
    queries, blocks_decoded, groups, bytes_decoded, ms_decode, ms_lines (a call served on the host
    reports its blocks with groups = 0 and "host": True)."""
    return dict(_last_lines) if _last_lines.get("host") else _lib.last_lines()


_last_lines: Dict[str, Any] = {}


def last_find() -> Dict[str, Any]:
    """kolm_find_stats of the last Reader.find / find_many / count / count_many / find_set /
    count_set / find_classes / count_classes / find_regex / count_regex: patterns,
    matches (total, whatever the limit), returned, blocks_decoded, groups, emit_launches,
    bytes_decoded, bytes_scanned, ms_decode, ms_find (a call served on the host reports its
    blocks and matches with groups = 0 and "host": True)."""
    return dict(_last_find) if _last_find.get("host") else _lib.last_find()


_last_find: Dict[str, Any] = {}


def _folded(patterns) -> List[ClassPattern]:
    """The literals of an ignore_case search as class patterns."""
    return [ClassPattern.literal(p, True) for p in _lib.find_patterns(patterns)]


def _class_patterns(patterns) -> List[ClassPattern]:
    """One ClassPattern or expression, or a sequence of them, as a list of ClassPatterns."""
    if isinstance(patterns, (bytes, bytearray, memoryview, ClassPattern)):
        patterns = [patterns]
    return [classes.as_pattern(p) for p in patterns]


def find_regex(container: bytes, expr, start: int = 0, end: Optional[int] = None, limit: Optional[int] = None,
               checksums=None, ignore_case: bool = False) -> List[int]:
    """Reader.find_regex of one expression over `container`: opens, searches, closes; the offsets."""
    with Reader(container, checksums=checksums) as r:
        return [o for o, _ in r.find_regex([expr], start, end, limit, ignore_case)]


def find(container: bytes, pattern, start: int = 0, end: Optional[int] = None, limit: Optional[int] = None,
         checksums=None, ignore_case: bool = False) -> List[int]:
    """Reader.find over `container`: opens, searches, closes."""
    with Reader(container, checksums=checksums) as r:
        if ignore_case:
            return r.find(pattern, start, end, limit, ignore_case=True)
        return r.find(pattern, start, end, limit)


def open_container(container: bytes, ctx=None, checksums=None, lines=None) -> Reader:
    """A Reader over `container` (see Reader).  ctx (optional): a context of kolm._lib.device_ctx
    instead of the default one.  checksums (optional): the container's manifest; reads are then
    checked.  lines (optional): the container's line index (a LineIndex or its sidecar bytes), or
    True / a one-byte delimiter to build one at open.  A malformed container raises what
    decompress raises."""
    return Reader(container, ctx, checksums, lines)


def verify(container: bytes, data: bytes) -> Dict[str, Any]:
    """Does `container` hold `data`?  Checked on the device (kolm_verify_container): the
    payloads and the data go up, every block is decoded and compared there, and one word per
    block comes back.  Returns {"ok", "blocks", "bad": [(block, method, offset, reason), ...],
    "reason", "bytes", "ms_decode", "ms_compare"}: reason 1 bytes differ (offset = the block's
    first differing byte), 2 the decoder rejected the payload, 3 the container's total length
    is not len(data) (nothing decoded, "bad" empty).  A malformed container raises the
    ValueError decompress raises; every method id must be in KOLM_DECODE_MASK."""
    fb, rep = _lib.verify_container(container, data)
    bad: List[Tuple[int, int, int, int]] = []
    if fb is not None and rep["bad_blocks"]:
        _, _, _, mids, _, _, _ = read_toc(bytes(container))
        for i in (int(j) for j in (fb != _lib.KOLM_VERIFY_EQUAL).nonzero()[0]):
            rej = int(fb[i]) == _lib.KOLM_VERIFY_REJECTED
            bad.append((i, int(mids[i]), 0 if rej else int(fb[i]), _lib.VR_REJECTED if rej else _lib.VR_DIFFER))
    return {"ok": rep["bad_blocks"] == 0 and rep["first_bad_reason"] == _lib.VR_NONE, "blocks": rep["blocks"],
            "bad": bad, "reason": rep["first_bad_reason"], "bytes": rep["bytes"],
            "ms_decode": rep["ms_decode"], "ms_compare": rep["ms_compare"]}


def checksums_of(container: bytes) -> Checksums:
    """The manifest of an existing container (one the reference wrote, for example): every block
    is decoded on the device and its CRC-32 taken there (kolm_check_container without an
    expectation); only the words come back.  Every method id must be in KOLM_DECODE_MASK; a
    block the decoder rejects raises ValueError."""
    mode, size_field, total_len, mids, orig, _, _ = read_toc(bytes(container))
    got, rep = _lib.check_container(container, None)
    if rep["bad_blocks"]:
        raise ValueError(f"block {rep['first_bad_block']} (method {rep['first_bad_method']}): malformed payload")
    return Checksums(mode, size_field, total_len, [int(n) for n in orig], got, rep["stream_crc"])


def check(container: bytes, checksums) -> Dict[str, Any]:
    """Is `container` intact?  Checked on the device without the original data
    (kolm_check_container): the payloads go up, every block is decoded and its CRC-32 taken
    there, and one word per block comes back to be compared with the manifest (a
    kolm.checksums.Checksums or its sidecar bytes; ValueError when it is of another container).
    Returns {"ok", "blocks", "bad": [(block, method, expected, got, reason), ...], "reason",
    "stream_crc", "bytes", "ms_decode", "ms_crc"}: reason 1 the CRC-32 differs, 2 the decoder
    rejected the payload (the reason of the lowest-numbered bad block at the top level).  A
    malformed container raises the ValueError decompress raises; every method id must be in
    KOLM_DECODE_MASK."""
    cs = as_checksums(checksums)
    mode, size_field, total_len, mids, orig, _, _ = read_toc(bytes(container))
    _match_toc(cs, mode, size_field, total_len, orig)
    got, rep = _lib.check_container(container, cs.crcs)
    bad: List[Tuple[int, int, int, int, int]] = []
    if rep["bad_blocks"]:
        # the report names the lowest-numbered bad block with its reason (a rejected block is bad
        # whatever its word); the others listed are the blocks whose words differ
        for i, (w, g) in enumerate(zip(cs.crcs, got)):
            if i == rep["first_bad_block"]:
                bad.append((i, int(mids[i]), w, g, rep["first_bad_reason"]))
            elif w != g:
                bad.append((i, int(mids[i]), w, g, _lib.CR_MISMATCH))
    return {"ok": rep["bad_blocks"] == 0, "blocks": rep["blocks"], "bad": bad, "reason": rep["first_bad_reason"],
            "stream_crc": rep["stream_crc"], "bytes": rep["bytes"], "ms_decode": rep["ms_decode"],
            "ms_crc": rep["ms_crc"]}
