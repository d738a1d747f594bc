// Search of a decoded buffer: the integer core of k_find_count / k_find_emit (k_find.hip), shared
// with the CPU emulation tools/find_emu.cpp (which walks the same tiles, lanes and positions
// serially and records every load).
//
// The scan buffer is n bytes at `buf` (any alignment; mis = buf mod 16).  It is cut into tiles of
// TILE = WG * PER bytes; thread l of tile t owns the PER positions t * TILE + l * PER + j.
//   windows      the 8 bytes that begin at each of a thread's positions, formed from the two or
//                three aligned 16-byte words that hold bytes [p0, p0 + 23) of the buffer (a funnel
//                shift by mis bytes, then by j)
//   match_mask   per pattern: bit j is set when position p0 + j is a match.  The prefix compare
//                is a masked 64-bit equality on the pattern's first min(len, 8) bytes; only a
//                candidate of a longer pattern reads further bytes (tail_ok: 8 bytes at a time
//                through window_at)
//   bounds rule  position o matches pattern i iff lo <= o < shi and o + len_i <= n: every byte
//                that decides a match lies inside [0, n); what a window holds past n never does
//   records      a match is (position relative to the scan buffer: u32, pattern index: u8), kept
//                in two arrays of the staging buffer (REC_BYTES per record); a tile's records are
//                in position order, then pattern order within a position
//   next_start   the hold-back between decode groups (below)
// Load contract: every load is an aligned 16-byte word that holds at least one byte of
// [buf, buf + n); a word that holds none is not loaded and counts as zeros.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FND_HD __host__ __device__ inline
#else
#define FND_HD inline
#endif

namespace fnd {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int64_t i64;

constexpr u32 WORD = 16;           // bytes per load
constexpr u32 WG = 256;            // threads per workgroup = per tile
constexpr u32 PER = 16;            // positions per thread
constexpr u32 TILE = WG * PER;     // positions per tile (4 KiB)
constexpr u32 MAX_PATTERNS = 16;   // KOLM_FIND_MAX_PATTERNS
constexpr u32 MAX_LEN = 256;       // KOLM_FIND_MAX_LEN
constexpr u32 REC_BYTES = 5;       // u32 position + u8 pattern index
constexpr u64 STAGE_DEFAULT = 64ull << 20;  // bytes of result staging on the device ($KOLM_FIND_STAGE)

// The patterns of a call as the kernels keep them in LDS: the bytes zero-padded to MAX_LEN (as
// 64-bit little-endian words), the first 8 bytes again with the mask of the bytes that count.
struct Pats {
    u64 pat[MAX_PATTERNS][MAX_LEN / 8];
    u64 pre[MAX_PATTERNS];
    u64 mask[MAX_PATTERNS];
    u32 len[MAX_PATTERNS];
};

struct Word {
    u64 q[2];  // bytes 0..7 and 8..15, little-endian
};

// the low `len` (1..8 and above: all 8) bytes of a 64-bit window
FND_HD u64 prefix_mask(u32 len) { return len >= 8 ? ~0ull : (1ull << (8 * len)) - 1; }

// pats[pat_off[i], pat_off[i + 1]) = pattern i (1..MAX_LEN bytes each, np <= MAX_PATTERNS: checked by the caller)
inline void make_pats(const u8* pats, const u32* pat_off, u32 np, Pats& P) {
    P = Pats{};
    for (u32 i = 0; i < np; ++i) {
        const u32 len = pat_off[i + 1] - pat_off[i];
        for (u32 k = 0; k < len; ++k) P.pat[i][k >> 3] |= (u64)pats[pat_off[i] + k] << (8 * (k & 7));
        P.len[i] = len;
        P.mask[i] = prefix_mask(len);
        P.pre[i] = P.pat[i][0];
    }
}

// (hi:lo) >> r, low 64 bits; r = 0, 8, .., 56 (r = 0: hi is not looked at)
FND_HD u64 funnel64(u64 lo, u64 hi, u32 r) { return r ? (lo >> r) | (hi << (64 - r)) : lo; }

// The aligned word at byte offset `off` from buf (off + mis = 0 mod 16), when it holds a byte of
// [0, n); zeros otherwise.  Ld: Word operator()(i64 off).
template <class Ld>
FND_HD Word word_or_zero(Ld& ld, i64 off, u32 n) {
    if (off < (i64)n && off + (i64)WORD > 0) return ld(off);
    return Word{{0, 0}};
}

// w[j] = bytes [p0 + j, p0 + j + 8) of the buffer, p0 = a thread's first position (a multiple of
// PER = WORD, so every thread's first word begins mis bytes before p0)
template <class Ld>
FND_HD void windows(Ld& ld, u32 mis, u32 p0, u32 n, u64 w[PER]) {
    const i64 a = (i64)p0 - (i64)mis;
    const Word A = word_or_zero(ld, a, n), B = word_or_zero(ld, a + WORD, n);
    // the last byte needed is p0 + 22 = byte mis + 22 of A:B:C
    const Word C = mis >= 9 ? word_or_zero(ld, a + 2 * WORD, n) : Word{{0, 0}};
    const u32 r = 8 * (mis & 7);
    u64 d[3];  // bytes [p0, p0 + 24)
    if (mis < 8) {
        d[0] = funnel64(A.q[0], A.q[1], r), d[1] = funnel64(A.q[1], B.q[0], r), d[2] = funnel64(B.q[0], B.q[1], r);
    } else {
        d[0] = funnel64(A.q[1], B.q[0], r), d[1] = funnel64(B.q[0], B.q[1], r), d[2] = funnel64(B.q[1], C.q[0], r);
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (u32 j = 0; j < PER; ++j) w[j] = funnel64(d[j >> 3], d[(j >> 3) + 1], 8 * (j & 7));
}

// bytes [o, o + 8) of the buffer for any o < n (the tail verify)
template <class Ld>
FND_HD u64 window_at(Ld& ld, u32 mis, u32 o, u32 n) {
    const u32 sh = (mis + o) & (WORD - 1);
    const i64 a = (i64)o - (i64)sh;
    const Word A = word_or_zero(ld, a, n);
    const Word B = sh > 8 ? word_or_zero(ld, a + WORD, n) : Word{{0, 0}};
    const u32 r = 8 * (sh & 7);
    return sh < 8 ? funnel64(A.q[0], A.q[1], r) : funnel64(A.q[1], B.q[0], r);
}

// bytes [8, len) of a candidate at o against the pattern (o + len <= n)
template <class Ld>
FND_HD bool tail_ok(Ld& ld, u32 mis, u32 o, u32 n, const u64* pat, u32 len) {
    for (u32 k = 8; k < len; k += 8)
        if ((window_at(ld, mis, o + k, n) ^ pat[k >> 3]) & prefix_mask(len - k)) return false;
    return true;
}

// bit j: position p0 + j matches the pattern
template <class Ld>
FND_HD u32 match_mask(Ld& ld, const u64 w[PER], u32 mis, u32 p0, u32 lo, u32 shi, u32 n, u64 pre, u64 mask, u32 len,
                      const u64* pat) {
    u32 m = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (u32 j = 0; j < PER; ++j) {
        const u32 o = p0 + j;
        if (((w[j] ^ pre) & mask) == 0 && o >= lo && o < shi && (u64)o + len <= n)
            if (len <= 8 || tail_ok(ld, mis, o, n, pat, len)) m |= 1u << j;
    }
    return m;
}

FND_HD u32 tiles(u32 n) { return (u32)(((u64)n + TILE - 1) / TILE); }

// records the staging buffer holds: never fewer than one tile can produce
FND_HD u64 stage_records(u64 stage_bytes, u32 np) {
    const u64 r = stage_bytes / REC_BYTES, least = (u64)TILE * np;
    return r < least ? least : r;
}

// Hold-back between decode groups.  A group covers stream bytes [a, b); S is the first start it
// reports, L the longest pattern.  A non-final group reports the starts in [S, next_start): a
// match that begins later might not end inside b, so those starts are left to the next group,
// which gets the bytes [next_start, b) (fewer than L) in front of its own.  The final group
// reports up to hi.
FND_HD u64 next_start(u64 S, u64 b, u32 L, bool final, u64 hi) {
    if (final) return hi;
    const u64 h = b >= (u64)(L - 1) ? b - (L - 1) : 0;
    return h > S ? h : S;
}

// What one decode group scans.  The group's blocks cover stream bytes [a, b); S is the first start
// not yet reported (S >= a only in the first group, where it is the window's lo).  The scan
// buffer is the stream bytes [start, n_abs): `carry` bytes of the previous groups in front of
// the group's own, cut at hi in the final group.  Positions are relative to `start`.
struct GroupScan {
    u64 start;   // stream offset of the scan buffer's first byte
    u64 S_next;  // the next group's S
    u32 carry;   // bytes in front of the group's decoded bytes (< L)
    u32 lo;      // matches start in [lo, shi)
    u32 shi;
    u32 n;       // bytes of the scan buffer
};
FND_HD GroupScan group_scan(u64 S, u64 a, u64 b, u32 L, bool final, u64 hi) {
    GroupScan g;
    g.start = S < a ? S : a;
    g.S_next = next_start(S, b, L, final, hi);
    g.carry = (u32)(a - g.start);
    g.lo = (u32)(S - g.start);
    g.shi = (u32)(g.S_next - g.start);
    g.n = (u32)((final ? hi : b) - g.start);
    return g;
}

// The emit launch that begins at tile t0 ends at the returned tile: as many tiles as the staging
// arrays (cap records, at least one tile's worth) hold, and no tile beyond the boundary at which
// `want` records, counted from tile 0, are reached.  tscan: exclusive scan of the tile totals.
inline u32 emit_cut(const u64* tscan, u32 ntiles, u32 t0, u64 cap, u64 want) {
    u32 t1 = t0 + 1;
    while (t1 < ntiles && tscan[t1 + 1] - tscan[t0] <= cap && tscan[t1] < want) ++t1;
    return t1;
}

}  // namespace fnd
