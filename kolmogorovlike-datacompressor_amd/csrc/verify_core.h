// Verify-after-encode: the integer core of the compare kernel (k_verify.hip), shared with the
// CPU emulation tools/verify_emu.cpp (which walks the same tiles with one virtual lane per
// thread of the kernel's workgroup).
//
// Two buffers of `total` bytes — the decoded batch and the original, block i at
// [bounds[i], bounds[i + 1]) of both — are compared; first_bad[i] ends as the offset within
// block i of its first differing byte, or EQUAL.  The buffers' addresses are congruent mod 16
// (`mis` = that residue), so one split serves both:
//   split         head = the bytes before the first 16-byte boundary (< 16, compared one by
//                 one), body = whole aligned 16-byte words, tail = the rest (< 16)
//   word_diff     OR of the four 32-bit xors: 0 when the two words are equal (the fast path
//                 needs nothing else: no block lookup, no atomic)
//   byte_mask     bit j = byte j of the word differs (memory order: little-endian words)
//   find_block    the block that holds a position: binary search in the nb + 1 bounds
//                 (empty blocks never match)
//   attribute     every differing byte of a word goes to its own block — a word spans many
//                 blocks when blocks are shorter than 16 bytes — but only the first one of
//                 each block: the rest of that block's bytes in the word are dropped, so a
//                 word costs at most one search and one minimum per block it touches
// Nothing here reads the data: the callers load [0, total) and nothing else.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VFY_HD __host__ __device__ inline
#else
#define VFY_HD inline
#endif

namespace vfy {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 WORD = 16;                // bytes per load
constexpr u32 WG = 256;                 // threads per workgroup
constexpr u32 UNROLL = 4;               // independent word pairs in flight per lane
constexpr u32 TILE_WORDS = WG * UNROLL; // words per workgroup iteration (16 KiB of each buffer)
constexpr u32 MAX_GRID = 2048;          // workgroups: grid-stride over the tiles beyond
constexpr u32 EQUAL = 0xFFFFFFFFu;      // first_bad: the block is equal
constexpr u32 REJECTED = 0xFFFFFFFEu;   // first_bad (host side): the decoder rejected the payload

struct Split {
    u32 head;   // bytes [0, head)
    u32 words;  // 16-byte words [head, head + 16 * words)
    u32 tail;   // bytes [head + 16 * words, total)
};

VFY_HD Split split(u32 mis, u32 total) {
    Split s;
    const u32 h = (WORD - (mis & (WORD - 1))) & (WORD - 1);
    s.head = h < total ? h : total;
    s.words = (total - s.head) / WORD;
    s.tail = total - s.head - s.words * WORD;
    return s;
}

VFY_HD u32 tiles(u32 words) { return (words + TILE_WORDS - 1) / TILE_WORDS; }

VFY_HD u32 grid_for(u32 words) {
    const u32 t = tiles(words);
    return t < 1 ? 1 : t < MAX_GRID ? t : MAX_GRID;
}

VFY_HD u32 word_diff(const u32 a[4], const u32 b[4]) {
    return (a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3]);
}

VFY_HD u32 byte_mask(const u32 a[4], const u32 b[4]) {
    u32 m = 0;
    for (u32 w = 0; w < 4; ++w) {
        const u32 x = a[w] ^ b[w];
        for (u32 j = 0; j < 4; ++j)
            if ((x >> (8 * j)) & 0xFFu) m |= 1u << (4 * w + j);
    }
    return m;
}

// largest i < nb with bounds[i] <= pos (pos < bounds[nb], bounds[0] = 0)
VFY_HD u32 find_block(const u32* bounds, u32 nb, u32 pos) {
    u32 lo = 0, hi = nb;  // bounds[lo] <= pos < bounds[hi]
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (bounds[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

// mask: differing bytes of the up to 16 bytes at pos0; amin(block, offset) lowers first_bad
template <class Min>
VFY_HD void attribute(const u32* bounds, u32 nb, u32 pos0, u32 mask, Min& amin) {
    while (mask) {
        u32 j = 0;
        while (!((mask >> j) & 1u)) ++j;
        const u32 pos = pos0 + j;
        const u32 b = find_block(bounds, nb, pos);
        amin(b, pos - bounds[b]);
        const u32 end = bounds[b + 1] - pos0;  // > j: the block holds pos
        if (end >= WORD) break;
        mask &= ~((1u << end) - 1u);
    }
}

}  // namespace vfy
