// Line index: the integer core of k_delim_count and k_delim_query (k_lines.hip), shared with the
// host planner (kolm_lines.cpp) and the CPU emulation tools/lines_emu.cpp (which walks the same
// runs, pieces, lanes and queries).
//
// A delimiter is one byte value.  A block is read as the 16-byte words of load_words.h (word j =
// bytes [16 j, 16 j + 16) of the block, the last one zero-filled past the block's end), cut into
// the 4 KiB pieces and runs of dedup_core.h:
//   eq_mask     bit i of the 16-bit mask = byte i of the word equals the delimiter.  Exact: the
//               SWAR zero-byte test with the carry kept inside each byte, so no neighbour's borrow
//               sets a bit, and the eight flag bits are gathered by one multiply whose partial
//               products land on distinct bit positions
//   valid       the mask of a word's nv valid bytes.  load_words zero-fills the bytes of a block's
//               last word past its end: with delimiter 0x00 those would match, so every mask is
//               restricted to ddp::word_bytes before anything is counted
//   count       set positions of a (restricted) mask
//   rank        set positions below byte index i (0..16)
//   select      byte index of the j-th set position (j < count)
// Position order inside a piece.  A lane holds words lane + 64 u (u = 0..3, the layout load_words
// gives), so position order is row-major over (u, lane): row u holds piece words [64 u, 64 u + 64)
// in lane order.  A count is a plain sum and needs no order; rank and select walk the rows in
// order and the lanes of one row in order:
//   word_of     (lane, u) -> piece word
//   row_of / lane_of   piece word -> (u, lane)
//   word_rank   what word w (mask m) adds to the count of the piece's bytes [0, r): the whole
//               word below byte r's word, the in-word rank in it, nothing above
// The host side of a query's answer:
//   NONE        SELECT's result when the block holds j or fewer delimiters (a stale table)
#pragma once
#include <cstdint>

#include "dedup_core.h"

#if defined(__HIPCC__)
#define LIN_HD __host__ __device__ inline
#else
#define LIN_HD inline
#endif

namespace lin {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 NONE = 0xFFFFFFFFu;
constexpr u32 OP_RANK = 0, OP_SELECT = 1;

// One query of k_delim_query: block = the block's slot in the decoded group, arg = the offset
// (RANK) or the in-block delimiter number (SELECT).
struct Query {
    u32 block;
    u32 arg;
    u32 op;
};

// bit i = byte i of x is zero (8 bits)
LIN_HD u32 zero_bytes(u64 x) {
    const u64 L = 0x7F7F7F7F7F7F7F7Full;
    const u64 t = ((x & L) + L) | x;       // bit 7 of a byte set unless the byte is zero; no carry leaves a byte
    const u64 z = (~t & ~L) >> 7;          // bit 0 of every zero byte
    return (u32)((z * 0x0102040810204080ull) >> 56);
}

// the equal-byte mask of the word (w0 = bytes 0..7, w1 = bytes 8..15) against delim
LIN_HD u32 eq_mask(u64 w0, u64 w1, u32 delim) {
    const u64 d = (u64)(delim & 0xFFu) * 0x0101010101010101ull;
    return zero_bytes(w0 ^ d) | zero_bytes(w1 ^ d) << 8;
}

// the positions of a word's first nv (0..16) bytes
LIN_HD u32 valid(u32 nv) { return (1u << nv) - 1u; }

// the restricted mask of word w of piece pc (w < pc.words)
LIN_HD u32 word_mask(u64 w0, u64 w1, u32 delim, const ddp::Piece& pc, u32 w) {
    return eq_mask(w0, w1, delim) & valid(ddp::word_bytes(pc, w));
}

LIN_HD u32 count(u32 m) { return (u32)__builtin_popcount(m); }
LIN_HD u32 rank(u32 m, u32 i) { return count(m & valid(i)); }
LIN_HD u32 select(u32 m, u32 j) {
    for (u32 k = 0; k < j; ++k) m &= m - 1;
    return m ? (u32)__builtin_ctz(m) : NONE;
}

LIN_HD u32 word_of(u32 lane, u32 u) { return lane + u * ddp::WAVE; }
LIN_HD u32 row_of(u32 w) { return w / ddp::WAVE; }
LIN_HD u32 lane_of(u32 w) { return w % ddp::WAVE; }

// word w's share of the delimiters in the piece's bytes [0, r), r <= the piece's bytes
LIN_HD u32 word_rank(u32 m, u32 w, u32 r) {
    const u32 wq = r / ddp::WORD;
    return w < wq ? count(m) : w == wq ? rank(m, r % ddp::WORD) : 0u;
}

}  // namespace lin
