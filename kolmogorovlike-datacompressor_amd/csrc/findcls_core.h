// Search for class patterns: the integer core of k_findcls_count / k_findcls_emit (k_findcls.hip),
// shared with the CPU emulation tools/findcls_emu.cpp (which walks the same tiles, lanes and
// positions serially and records every load).  A class pattern is a sequence of 1..MAX_LEN byte
// classes (subsets of 0..255); position o matches when data[o + k] lies in class k for every k.
// Tiles, windows, the bounds rule, the records, the hold-back and the emit cut are find_core.h's.
//
// A class is one of
//   empty             its pattern has no match (len = 0 in Pats: the kernels skip it)
//   masked equality   {b : (b & mask) == value}: singletons, the full class, an ASCII case pair,
//                     [0-7], [\x00-\x7f] ...  With v = AND of the members and x = (OR of the
//                     members) ^ v the class is one iff it has 2^popcount(x) members; then
//                     mask = ~x, value = v
//   table class       every other; a call holds at most MAX_TABLES distinct ones.  T[b] bit k says
//                     that byte b is in table class k
// For any non-empty class (mask, value) as above is its hull: every member satisfies
// (b & mask) == value.  The candidate filter of a position is the masked 64-bit equality of
// find_core.h on the hulls of the pattern's first min(len, 8) classes (pre / pmask); it is exact
// on masked equalities.  Only a candidate looks at its table positions (T) and at the positions
// from 8 on: 8 at a time through window_at, a masked equality on val / mask (mask byte 0 at a
// table position, where the byte of val holds the table id instead, at the full class and past
// the pattern's end) and one look at T for every bit of tbl.
// Bounds: position o matches pattern i iff lo <= o < shi and o + len_i <= n, which is tested
// before any class is: what a window holds past n never decides a match (a class may hold 0x00).
// Load contract: find_core.h's.
#pragma once
#include <cstring>

#include "find_core.h"

namespace fcl {

using fnd::i64;
using fnd::u32;
using fnd::u64;
using fnd::u8;

constexpr u32 MAX_TABLES = 64;           // distinct table classes of a call
constexpr u32 BITMAP = 32;               // bytes of a class as the C ABI passes it: bit b & 7 of byte b >> 3
constexpr u32 WORDS = fnd::MAX_LEN / 8;  // 64-bit words of a pattern's row

// The class patterns of a call as the kernels keep them in LDS (a workgroup copies T and the
// words its patterns' lengths need).
struct Pats {
    u64 T[256];
    u64 val[fnd::MAX_PATTERNS][WORDS];
    u64 mask[fnd::MAX_PATTERNS][WORDS];
    u64 pre[fnd::MAX_PATTERNS];    // the hulls of positions 0..7
    u64 pmask[fnd::MAX_PATTERNS];
    u32 len[fnd::MAX_PATTERNS];    // 0: the pattern holds an empty class
    u8 tbl[fnd::MAX_PATTERNS][WORDS];  // bit j of tbl[i][k]: position 8 k + j is a table class
};

struct Class {
    u32 size;  // members
    u8 mask, value;  // the hull (size > 0)
    bool eq;   // a masked equality: the hull is the class
};

inline Class classify(const u8* bm) {
    u32 size = 0;
    u8 v = 0xFF, o = 0;
    for (u32 b = 0; b < 256; ++b)
        if ((bm[b >> 3] >> (b & 7)) & 1) ++size, v &= (u8)b, o |= (u8)b;
    if (!size) return Class{0, 0, 0, false};
    const u8 x = o ^ v;
    return Class{size, (u8)~x, v, size == (1u << __builtin_popcount(x))};
}

// bitmaps [pat_off[i], pat_off[i + 1]) = the classes of pattern i (1..MAX_LEN each, np <=
// MAX_PATTERNS: checked by the caller).  False when a call needs more than MAX_TABLES distinct
// table classes: the one too many is position *bad_pos of pattern *bad_pat.  ntab: table classes used.
inline bool make_pats(const u8* bitmaps, const u32* pat_off, u32 np, Pats& P, u32* ntab, u32* bad_pat, u32* bad_pos) {
    std::memset(&P, 0, sizeof P);
    const u8* seen[MAX_TABLES];
    u32 nt = 0;
    for (u32 i = 0; i < np; ++i) {
        const u32 len = pat_off[i + 1] - pat_off[i];
        bool dead = false;
        for (u32 k = 0; k < len; ++k) {
            const u8* bm = bitmaps + (size_t)(pat_off[i] + k) * BITMAP;
            const Class c = classify(bm);
            if (!c.size) {
                dead = true;
                continue;
            }
            const u32 sh = 8 * (k & 7);
            if (k < 8) P.pre[i] |= (u64)c.value << sh, P.pmask[i] |= (u64)c.mask << sh;
            if (c.eq) {
                P.val[i][k >> 3] |= (u64)c.value << sh, P.mask[i][k >> 3] |= (u64)c.mask << sh;
                continue;
            }
            u32 id = 0;
            while (id < nt && std::memcmp(seen[id], bm, BITMAP)) ++id;
            if (id == nt) {
                if (nt == MAX_TABLES) {
                    *bad_pat = i, *bad_pos = k;
                    return false;
                }
                seen[nt++] = bm;
                for (u32 b = 0; b < 256; ++b)
                    if ((bm[b >> 3] >> (b & 7)) & 1) P.T[b] |= 1ull << id;
            }
            P.val[i][k >> 3] |= (u64)id << sh;
            P.tbl[i][k >> 3] |= (u8)(1u << (k & 7));
        }
        P.len[i] = dead ? 0 : len;
    }
    *ntab = nt;
    return true;
}

// the table positions (bits) of the 8 bytes w: each byte in the class whose id val holds there
FND_HD bool tables_ok(const u64* T, u64 w, u64 val, u32 bits) {
    while (bits) {
        const u32 sh = 8 * (u32)__builtin_ctz(bits);
        bits &= bits - 1;
        if (!((T[(w >> sh) & 0xFF] >> ((val >> sh) & 0xFF)) & 1)) return false;
    }
    return true;
}

// what the candidate filter left of a candidate at o (o + len <= n): the table positions of its
// first 8 bytes w0, then the bytes [8, len)
template <class Ld>
FND_HD bool rest_ok(Ld& ld, u32 mis, u32 o, u32 n, u64 w0, const u64* T, const u64* val, const u64* mask, const u8* tbl,
                    u32 len) {
    if (!tables_ok(T, w0, val[0], tbl[0])) return false;
    for (u32 k = 8; k < len; k += 8) {
        const u64 m = mask[k >> 3];
        const u32 t = tbl[k >> 3];
        if (!m && !t) continue;  // full classes only
        const u64 w = fnd::window_at(ld, mis, o + k, n);
        if ((w ^ val[k >> 3]) & m) return false;
        if (!tables_ok(T, w, val[k >> 3], t)) return false;
    }
    return true;
}

// bit j: position p0 + j matches pattern i of P
template <class Ld>
FND_HD u32 match_mask(Ld& ld, const u64 w[fnd::PER], u32 mis, u32 p0, u32 lo, u32 shi, u32 n, const Pats& P, u32 i) {
    const u32 len = P.len[i];
    if (!len) return 0;
    const u64 pre = P.pre[i], pmask = P.pmask[i];
    u32 m = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (u32 j = 0; j < fnd::PER; ++j) {
        const u32 o = p0 + j;
        if (((w[j] ^ pre) & pmask) == 0 && o >= lo && o < shi && (u64)o + len <= n)
            if (rest_ok(ld, mis, o, n, w[j], P.T, P.val[i], P.mask[i], P.tbl[i], len)) m |= 1u << j;
    }
    return m;
}

}  // namespace fcl
