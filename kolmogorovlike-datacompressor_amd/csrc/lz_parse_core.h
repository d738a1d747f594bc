// LZ77 decode: the serial token parse of one block (k_dec_lz_parse of k_decode.hip), shared
// with the CPU emulation tools/lz_parse_emu.cpp.  Plain C++, no HIP types.
//
// The payload is a byte-aligned token stream (PY:1765-1812):
//   00 <byte>                     literal
//   01 ULEB(len) ULEB(dist)       copy of len bytes from dist bytes back (overlap allowed),
//                                 cut at the block's length n
// parse() validates it and writes one record per token that produces output into the slot
// arrays tpos / tval: the token's first output position, and LIT | byte or the distance.
//
//   uleb_get   a ULEB128 value of any byte length, the loop bounded by plen; the value
//              saturates at 0xFFFFFFFF (a length is clamped by n - o anyway, a distance that
//              large is rejected anyway), so overlong and > 32-bit encodings read as PY reads
//              them.  false = the payload ends inside the value.
//   parse      a copy of length 0 is validated like any other copy (dist != 0 &&
//              dist <= min(o, 4096): stricter than PY, whose distance check runs once per
//              copied byte and so never for such a copy) and then emits NO record.  Every
//              record therefore advances the output position by at least one, which gives
//              the invariant the resolve kernel and the slot arrays rest on:
//                  tpos strictly increasing,  t <= o <= n  on every path
//              — a block never needs more than its own n slots, and no two records share an
//              output position.
// Nothing here writes outside tpos / tval [0, n) or reads outside p [0, plen).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LZP_HD __host__ __device__ inline
#else
#define LZP_HD inline
#endif

namespace lzp {

typedef uint8_t u8;
typedef uint32_t u32;

constexpr u32 LIT = 0x80000000u;  // tval of a literal: LIT | byte
constexpr u32 WINDOW = 4096;      // the largest distance (PY:1771)
// the values of DEC_OK / DEC_ELEN / DEC_EFORMAT (kolm_internal.h, checked there)
constexpr u32 OK = 0, ELEN = 1, EFORMAT = 2;

LZP_HD bool uleb_get(const u8* p, u32 plen, u32& j, u32& v) {
    v = 0;
    u32 sh = 0;  // 0, 7, .., 35: past 32 every non-zero group saturates
    while (j < plen) {
        const u32 b = p[j++];
        const uint64_t g = (uint64_t)(b & 0x7Fu) << sh;
        v = (g >> 32) ? 0xFFFFFFFFu : v | (u32)g;  // once saturated, v stays all ones
        if (sh < 35) sh += 7;
        if (!(b & 0x80u)) return true;
    }
    return false;
}

// Parses p[0, plen) for a block of n output bytes into tpos / tval [0, n) (the block's own
// slots).  Returns OK, ELEN or EFORMAT; *ntok = the records written (0 unless OK).
LZP_HD u32 parse(const u8* p, u32 plen, u32 n, u32* tpos, u32* tval, u32* ntok) {
    u32 j = 0, o = 0, t = 0, err = OK;
    while (j < plen && o < n) {
        const u32 flag = p[j++];
        u32 val, adv;
        if (flag == 0) {
            if (j >= plen) {
                err = EFORMAT;
                break;
            }
            val = LIT | p[j++];
            adv = 1;
        } else if (flag == 1) {
            u32 len, dist;
            if (!uleb_get(p, plen, j, len) || !uleb_get(p, plen, j, dist) || dist == 0 ||
                dist > (o < WINDOW ? o : WINDOW)) {
                err = EFORMAT;
                break;
            }
            if (len == 0) continue;  // validated, produces nothing: no record
            val = dist;
            adv = len < n - o ? len : n - o;  // PY cuts the last copy at orig_len
        } else {
            err = EFORMAT;
            break;
        }
        // Invariant: every record advances o by adv >= 1 and o < n here, so t <= o < n and
        // tpos is strictly increasing.  The guard keeps a later edit from writing a
        // neighbouring block's slots (or past the arrays) should the invariant be lost.
        if (t >= n) {
            err = EFORMAT;
            break;
        }
        tpos[t] = o;
        tval[t] = val;
        ++t;
        o += adv;
    }
    if (err == OK && o != n) err = ELEN;
    *ntok = err == OK ? t : 0u;
    return err;
}

}  // namespace lzp
