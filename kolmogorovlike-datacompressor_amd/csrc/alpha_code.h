// Order-preserving prefix codes for the round-0 keys of the cyclic sort (k_lsd.hip), shared by
// the kernels and the CPU emulation (tools/alpha_code_emu.cpp).  Integer-only.
//
// Rotation order inside a block depends only on the ORDER of its byte values.  An alphabetic
// code (prefix-free, left-aligned codes increasing in symbol order) has a concatenated bit string
// that sorts exactly like the symbol string, so the first 64 bits of a rotation's code stream are
// a valid sort key, and frequent symbols get short codes: text of 50 symbols (order-0 entropy
// ~4 bits) packs ~14.5 characters into the 64 bits that hold 10 fixed 6-bit codes.
//
// The builder: a recursive weight-balanced split of the present symbols in symbol order.  A node
// holds a run of symbols; the split point makes the left weight closest to half (ties: the
// smaller left side), clipped so that either side still fits the remaining depth (at most
// 2^(room - 1) leaves per side); depth limit AC_MAXLEN = 8; a leaf shallower than AC_MINLEN = 2
// is padded with zero bits to length 2 (a padded "0" -> "00" stays prefix-free: its sibling
// subtree starts with 1).  Every present symbol gets AC_MINLEN <= len <= AC_MAXLEN, so a 64-bit
// key holds at least 8 whole characters and reads at most 32.
//
// Nodes are heap-numbered (root 1, children 2 n and 2 n + 1): the nodes of depth d are
// 2^d .. 2^(d+1) - 1, independent of each other, and a node's code is its number without the
// leading bit.  ac_node() does one node, so a caller runs a level's nodes serially (ac_build) or
// one per thread with a barrier between levels (k_alpha_codes).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AC_HD __host__ __device__
#else
#define AC_HD
#endif

namespace kolm {

constexpr uint32_t AC_MAXLEN = 8;   // longest code: a key of 64 bits holds >= 8 whole characters
constexpr uint32_t AC_MINLEN = 2;   // shortest code: a key reads <= 32 characters
constexpr uint32_t AC_KEYBITS = 64;
constexpr uint32_t AC_R0_CHARS = AC_KEYBITS / AC_MAXLEN;  // characters round 0 guarantees: h0 of the doubling rounds
constexpr uint32_t AC_MAXREAD = AC_KEYBITS / AC_MINLEN;   // characters a key can read
constexpr uint32_t AC_NODES = 1u << (AC_MAXLEN + 1);      // heap slots (slot 0 unused)

// Work space of one block's build (the kernel keeps it in LDS).
struct AcWork {
    uint64_t cum[257];        // cum[i] = weight of the first i present symbols
    uint8_t sym[256];         // the present symbols in order
    uint16_t lo[AC_NODES];    // node -> its run [lo, hi) of present-symbol indices (empty: lo == hi)
    uint16_t hi[AC_NODES];
    uint32_t sigma;
};

// Symbols, cumulative weights and the root.  pres: 256 presence bits (bit c & 31 of word c >> 5);
// wts: sampled counts, a present symbol that was never sampled weighs 1.  Clears cw.
AC_HD inline void ac_init(const uint32_t* pres, const uint32_t* wts, AcWork& k, uint16_t* cw) {
    uint32_t n = 0;
    uint64_t acc = 0;
    k.cum[0] = 0;
    for (uint32_t c = 0; c < 256; ++c) {
        cw[c] = 0;
        if ((pres[c >> 5] >> (c & 31)) & 1u) {
            k.sym[n] = (uint8_t)c;
            acc += wts[c] ? wts[c] : 1u;
            k.cum[++n] = acc;
        }
    }
    k.sigma = n;
    for (uint32_t i = 0; i < AC_NODES; ++i) k.lo[i] = k.hi[i] = 0;
    k.lo[1] = 0;
    k.hi[1] = (uint16_t)n;
}

// One node of depth d (id in [2^d, 2^(d+1))): a leaf writes its symbol's code word
// cw[c] = len << 8 | code (right-aligned), an inner node its children's runs.
AC_HD inline void ac_node(AcWork& k, uint32_t id, uint32_t d, uint16_t* cw) {
    const uint32_t lo = k.lo[id], hi = k.hi[id];
    if (lo >= hi) return;
    if (hi - lo == 1) {
        const uint32_t len = d < AC_MINLEN ? AC_MINLEN : d;
        const uint32_t code = (id - (1u << d)) << (len - d);
        cw[k.sym[lo]] = (uint16_t)(len << 8 | code);
        return;
    }
    if (d >= AC_MAXLEN) return;  // (unreachable: the clip below keeps a run within 2^room leaves)
    const uint32_t cap = 1u << (AC_MAXLEN - d - 1);
    const uint64_t base = k.cum[lo], tot = k.cum[hi] - base;
    // the first split s in (lo, hi] with 2 * left(s) >= tot, left(s) = cum[s] - base
    uint32_t a = lo + 1, b = hi;
    while (a < b) {
        const uint32_t m = (a + b) >> 1;
        if (2 * (k.cum[m] - base) >= tot) b = m; else a = m + 1;
    }
    uint32_t s = a;
    if (s > lo + 1) {  // s - 1 (left below half) when it is at least as close
        const uint64_t over = 2 * (k.cum[s] - base) - tot, under = tot - 2 * (k.cum[s - 1] - base);
        if (under <= over) --s;
    }
    const uint32_t smin = hi - lo > cap ? hi - cap : lo + 1, smax = lo + cap < hi - 1 ? lo + cap : hi - 1;
    if (s < smin) s = smin;
    if (s > smax) s = smax;
    k.lo[2 * id] = (uint16_t)lo;
    k.hi[2 * id] = (uint16_t)s;
    k.lo[2 * id + 1] = (uint16_t)s;
    k.hi[2 * id + 1] = (uint16_t)hi;
}

// The serial build: cw[256] for one block (absent symbols 0).
AC_HD inline void ac_build(const uint32_t* pres, const uint32_t* wts, AcWork& k, uint16_t* cw) {
    ac_init(pres, wts, k, cw);
    for (uint32_t d = 0; d <= AC_MAXLEN; ++d)
        for (uint32_t id = 1u << d; id < (2u << d); ++id) ac_node(k, id, d, cw);
}

AC_HD inline uint32_t ac_len(uint16_t w) { return w >> 8; }
AC_HD inline uint32_t ac_bits(uint16_t w) { return w & 255u; }

// The 64-bit key of the rotation that starts at offset t of the factor text[0 .. m): codes
// appended cyclically until 64 bits are full (the last one cut).  A factor of one 2-bit symbol
// loops 32 times.  A symbol without a code (len 0: not of this block) ends the key.
AC_HD inline uint64_t ac_key_wrap(const uint8_t* text, uint32_t m, uint32_t t, const uint16_t* cw) {
    uint64_t key = 0;
    uint32_t nb = 0;
    for (uint32_t k = 0; k < AC_MAXREAD && nb < AC_KEYBITS; ++k) {
        const uint16_t w = cw[text[t]];
        const uint32_t l = ac_len(w), room = AC_KEYBITS - nb;
        if (!l) break;
        key |= l <= room ? (uint64_t)ac_bits(w) << (room - l) : (uint64_t)ac_bits(w) >> (l - room);
        nb += l;
        if (++t == m) t = 0;
    }
    return key;
}

}  // namespace kolm
