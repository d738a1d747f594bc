// Lyndon factor starts from prefix-minimum candidates: the integer core of the fast route of
// launch_lyndon (k_blocks.hip: k_lyn_min / k_lyn_scan / k_lyn_cand / k_lyn_resolve), shared with
// the CPU emulation tools/lyn_emu.cpp, which runs the same functions serially.
//
// Position p of a block [base, end) starts a Lyndon factor iff suffix(p) is smaller than every
// suffix that starts before it in the block (a proper prefix is smaller).
//   word        the word of p: the 8 bytes at p, big-endian; bytes at or past `end` read as 0.
//   candidate   p is a candidate iff word(p) <= word(q) for every q in [base, p).  Every factor
//               start is a candidate: were word(q) < word(p) for an earlier q, the words first
//               differ at a byte j < 8 with q's byte smaller.  p's byte there is larger, so it is
//               a text byte (not padding), and so is q's (q + j < p + j < end): the suffixes
//               agree on j text bytes and q's is smaller at the next, so p is no start.
//               Equality keeps a candidate, also against a zero-padded tail word.
//   order       for x < y: the words at x + l, y + l (l = 0, 8, ..) are compared.  Different
//               words decide (the smaller word is the smaller suffix: if a padded byte is the
//               smaller one, that suffix ran out first and is a proper prefix); equal words with
//               y + l + 8 >= end mean y's suffix ran out first, so y is smaller.
//   starts      the left-to-right minima, in suffix order, of the candidates in position order.
//               min under a total order is associative: an inclusive scan (Hillis-Steele,
//               scan_step) over the sorted candidates; candidate i is a start iff the scan's
//               value at i is i itself.
// Budgets: a block with more than `cap` candidates, or with a comparison whose common prefix is
// longer than `lcp_cap` bytes, is not resolved here (route FALLBACK): nothing is written for it and
// the Duval kernels factorise it.  A comparison reads at most lcp_cap + 16 bytes per side.
//
// Loads (Reader): b(i) one byte, d(i) a little-endian dword at a 4-byte aligned address, q(i, e) 16
// bytes at a 16-byte aligned address, amod() the address of text[0] modulo 16.  Every load lies
// inside [base, end) of the block it serves: never outside the batch, never in a neighbour's bytes.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LYN_HD __host__ __device__ inline
#else
#define LYN_HD inline
#endif
#if defined(__clang__)
#define LYN_UNROLL _Pragma("unroll")
#else
#define LYN_UNROLL
#endif

namespace lyn {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 THREADS = 256;             // lanes per tile
constexpr u32 PER = 16;                  // positions per lane (one 16-byte load + 8 bytes of overlap)
constexpr u32 TILE = THREADS * PER;      // 4 KiB
constexpr u32 CAND_MAX = 1024;           // candidates per block the resolver takes (KOLM_LYN_CAND_MAX lowers it)
constexpr u32 LCP_MAX = 512;             // longest common prefix of one comparison (KOLM_LYN_LCP_MAX)
constexpr u32 LCP_LIMIT = 1u << 16;      // upper bound of the override
constexpr u64 W_MAX = ~0ull;             // identity of min over words ("no earlier position")
constexpr u32 ACCEPT = 0, FALLBACK = 1;  // route word of a block

LYN_HD u64 min64(u64 a, u64 b) { return a < b ? a : b; }

// The 24 bytes from p as six big-endian dwords (bytes at or past end: 0); p in [base, end).
template <class R>
LYN_HD void load24(const R& rd, u32 p, u32 base, u32 end, u32 E[6]) {
    const u32 a = (rd.amod() + p) & 15u;
    u32 e[6];
    if (a == 0 && end - p >= 24) {
        rd.q(p, e);
        e[4] = rd.d(p + 16);
        e[5] = rd.d(p + 20);
    } else {
        const u32 sh = a & 3u;
        if (p - base >= sh && end - (p - sh) >= 28) {  // seven aligned dwords, funnel-shifted
            u32 d[7];
LYN_UNROLL
            for (u32 k = 0; k < 7; ++k) d[k] = rd.d(p - sh + 4 * k);
LYN_UNROLL
            for (u32 k = 0; k < 6; ++k) e[k] = sh ? (d[k] >> (8 * sh)) | (d[k + 1] << (32 - 8 * sh)) : d[k];
        } else {
LYN_UNROLL
            for (u32 k = 0; k < 6; ++k) {
                u32 v = 0;
                for (u32 j = 0; j < 4; ++j) {
                    const u32 i = p + 4 * k + j;
                    if (i < end) v |= rd.b(i) << (8 * j);
                }
                e[k] = v;
            }
        }
    }
LYN_UNROLL
    for (u32 k = 0; k < 6; ++k) E[k] = __builtin_bswap32(e[k]);
}

// word of position p + i (i < 16) from load24's dwords
LYN_HD u64 word_of(const u32 E[6], u32 i) {
    const u32 k = i >> 2, r = i & 3u;
    const u64 hi = ((u64)E[k] << 32) | E[k + 1];
    return r ? (hi << (8 * r)) | (E[k + 2] >> (32 - 8 * r)) : hi;
}

// minimum word of the lane's n (1..16) positions
LYN_HD u64 lane_min(const u32 E[6], u32 n) {
    u64 m = W_MAX;
LYN_UNROLL
    for (u32 i = 0; i < PER; ++i)
        if (i < n) m = min64(m, word_of(E, i));
    return m;
}

// bit i set: p + i is a candidate; run = the minimum word of every earlier position of the block
LYN_HD u32 lane_cands(const u32 E[6], u32 n, u64 run) {
    u32 mask = 0;
LYN_UNROLL
    for (u32 i = 0; i < PER; ++i) {
        if (i < n) {
            const u64 w = word_of(E, i);
            if (w <= run) mask |= 1u << i;
            run = min64(run, w);
        }
    }
    return mask;
}

// the word of any position p in [base, end]
template <class R>
LYN_HD u64 word_at(const R& rd, u32 p, u32 base, u32 end) {
    if (p < end && end - p >= 8) {
        const u32 sh = (rd.amod() + p) & 3u;
        if (sh == 0) return ((u64)__builtin_bswap32(rd.d(p)) << 32) | __builtin_bswap32(rd.d(p + 4));
        if (p - base >= sh && end - (p - sh) >= 12) {
            const u32 d0 = rd.d(p - sh), d1 = rd.d(p - sh + 4), d2 = rd.d(p - sh + 8);
            const u32 e0 = (d0 >> (8 * sh)) | (d1 << (32 - 8 * sh)), e1 = (d1 >> (8 * sh)) | (d2 << (32 - 8 * sh));
            return ((u64)__builtin_bswap32(e0) << 32) | __builtin_bswap32(e1);
        }
    }
    u64 w = 0;
    for (u32 j = 0; j < 8; ++j) w = (w << 8) | (p + j < end ? (u64)rd.b(p + j) : 0ull);
    return w;
}

// suffix(x) < suffix(y) inside [base, end), x != y.  lcp: the common prefix of the two suffixes
// (the shorter suffix's length when it is a proper prefix).  over: lcp > lcp_cap — the result is
// then meaningless and the block falls back.
template <class R>
LYN_HD bool suffix_less(const R& rd, u32 x, u32 y, u32 base, u32 end, u32 lcp_cap, u32& lcp, bool& over) {
    const bool sw = x > y;
    const u32 lo = sw ? y : x, hi = sw ? x : y;  // hi's suffix is the shorter one
    bool lo_less = false;
    over = false;
    for (u32 l = 0;; l += 8) {
        if (l > lcp_cap) {
            lcp = l;
            over = true;
            return false;
        }
        const u64 wa = word_at(rd, lo + l, base, end), wb = word_at(rd, hi + l, base, end);
        if (wa != wb) {
            lcp = l + (u32)__builtin_clzll(wa ^ wb) / 8;
            lo_less = wa < wb;
            break;
        }
        if (end - hi <= l + 8) {  // hi's suffix ran out inside this word
            lcp = end - hi;
            break;
        }
    }
    over = lcp > lcp_cap;
    return sw ? !lo_less : lo_less;
}

// One step of the inclusive min-scan at distance d: the smaller (suffix order) of in[i - d], in[i].
template <class R>
LYN_HD u32 scan_step(const R& rd, const u32* in, u32 i, u32 d, u32 base, u32 end, u32 lcp_cap, u32& lcp, bool& over) {
    const u32 a = in[i];
    over = false;
    lcp = 0;
    if (i < d) return a;
    const u32 b = in[i - d];
    if (a == b) return a;
    return suffix_less(rd, b, a, base, end, lcp_cap, lcp, over) ? b : a;
}

}  // namespace lyn
