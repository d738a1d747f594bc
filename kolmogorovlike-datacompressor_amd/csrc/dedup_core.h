// Duplicate-block detection: the integer core of k_block_fp and k_dedup_cmp (k_dedup.hip), shared
// with the CPU emulation tools/dedup_emu.cpp (which walks the same items, waves and lanes).
//
// A block is read as little-endian 16-byte words counted from the block's FIRST byte (word j =
// bytes [16 j, 16 j + 16) of the block, the last one zero-padded), whatever the block's address:
//   pieces      a block of len bytes is cut into ceil(len / ITEM) pieces of ITEM bytes (4 KiB, the
//               last one shorter): the items.  A wave takes one item at a time, lane l words l,
//               l + 64, l + 128, l + 192 of the piece
//   runs        the fingerprint kernel hands a wave RUN consecutive pieces of one block
//   piece       the piece's byte and word counts
//   fast        may word j be read with aligned 16-byte loads?  Its 16 bytes begin sh = (address
//               mod 16) bytes into an aligned word: that word and, when sh != 0, the next one are
//               loaded and funnel-shifted (rng::src_word).  Only when both lie inside the batch
//               [t0, t1) whole; otherwise the word's valid bytes are read one by one.  That
//               concerns the words at the batch's two ends alone, so no load touches a byte
//               outside the batch.
//   item_fast   the same for every word of an item at once (wave-uniform: the kernels' body
//               without the per-word test; the loads are the same either way)
//   mask        zeroes the bytes of a word past the block's end
//   mix         word, index -> two u64: keyed 64-bit multiplies of the word's four 32-bit quarters,
//               each offset by a key derived from the word's index in the block (the NH form of
//               UMAC: (a + k0)(b + k1) + (c + k2)(d + k3) with 32-bit wrapping adds and 32 x 32 ->
//               64 products, one v_mad_u64_u32 each), the quarters paired differently in the two
//               sums.  A zero word gives its index keys' products, not 0, and a word moved to
//               another index gives another value.  (A 64 x 64 -> 128 multiply-fold per sum, the
//               first form, measured 1.52 x the device-to-device copy: its 14 quarter-rate
//               multiplies per word bound the kernel.)
//   finish      the block's two sums (wrapping u64 adds of its words' mixes: commutative, so any
//               split over lanes, waves, pieces and atomics gives the same value and nothing
//               needs an order) with the block's length mixed in: b"x" and b"x\0" differ.
// The fingerprint depends on the block's bytes alone: not on its address or alignment, the batch
// geometry or its neighbours.  It only proposes candidates: equality is always settled by
// comparing bytes (k_dedup_cmp), so its quality affects speed and never correctness.  It is not a
// format: the function may change between versions and must not be persisted.
#pragma once
#include <cstdint>

#include "range_core.h"

#if defined(__HIPCC__)
#define DDP_HD __host__ __device__ inline
#else
#define DDP_HD inline
#endif

namespace ddp {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 WORD = rng::WORD;      // bytes per word
constexpr u32 WAVE = rng::WAVE;      // lanes: one wave takes one item
constexpr u32 UNROLL = rng::UNROLL;  // words per lane and item
constexpr u32 ITEM = rng::ITEM;      // bytes per piece (4 KiB)
constexpr u32 WPI = ITEM / WORD;     // words per piece
constexpr u32 WG = rng::WG;
constexpr u32 MAX_GRID = rng::MAX_GRID;

constexpr u64 K_IDX = 0x9E3779B97F4A7C15ull;  // index key stride (odd)
constexpr u64 K0 = 0xA0761D6478BD642Full, K1 = 0xE7037ED1A0B428DBull;  // first sum's keys
constexpr u64 K2 = 0x8EBC6AF09C88C6E3ull, K3 = 0x589965CC75374CC3ull;  // second sum's keys
constexpr u64 K4 = 0x1D8E4E27C47D124Full, K5 = 0xEB44ACCAB455D165ull;  // finish

struct Piece {
    u64 o0;     // the piece is bytes [o0, o0 + bytes) of its block
    u32 bytes;  // <= ITEM
    u32 words;  // ceil(bytes / WORD)
};

DDP_HD u64 pieces(u64 len) { return (len + ITEM - 1) / ITEM; }
// k_block_fp: a wave takes a run of up to RUN consecutive pieces of one block and adds its sums to
// the block's once per run (one cross-lane reduction and one pair of atomics per 32 KiB: with one
// pair per piece the atomics on a large block's two words bound the kernel)
constexpr u32 RUN = 8;
DDP_HD u64 runs(u64 len) { return (pieces(len) + RUN - 1) / RUN; }

// piece k (< pieces(len)) of a block of len bytes
DDP_HD Piece piece(u64 len, u64 k) {
    Piece p;
    p.o0 = k * ITEM;
    p.bytes = (u32)(len - p.o0 < ITEM ? len - p.o0 : ITEM);
    p.words = (p.bytes + WORD - 1) / WORD;
    return p;
}

// valid bytes of word w of a piece
DDP_HD u32 word_bytes(const Piece& p, u32 w) { return p.bytes - w * WORD < WORD ? p.bytes - w * WORD : WORD; }

// a = address of the word's first byte, sh = a mod 16, batch = addresses [t0, t1)
DDP_HD bool fast(u64 a, u32 sh, u64 t0, u64 t1) { return a - sh >= t0 && a - sh + (sh ? 2 * WORD : WORD) <= t1; }

// every word of an item of `words` words that begins at address a may be read that way
DDP_HD bool item_fast(u64 a, u32 sh, u32 words, u64 t0, u64 t1) {
    return a - sh >= t0 && a - sh + (u64)words * WORD + (sh ? WORD : 0) <= t1;
}

DDP_HD u64 rotl(u64 x, u32 r) { return (x << r) | (x >> (64 - r)); }

// the two halves of the 128-bit product, xored
DDP_HD u64 mulfold(u64 x, u64 y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (x * y) ^ __umul64hi(x, y);
#else
    const unsigned __int128 m = (unsigned __int128)x * y;
    return (u64)m ^ (u64)(m >> 64);
#endif
}

// keeps the first nv (1..16) bytes of the word (w0 = bytes 0..7, w1 = bytes 8..15)
// (two plain masks: a branch per half makes the compiler index the pair in scratch memory)
DDP_HD void mask(u64& w0, u64& w1, u32 nv) {
    const u32 n0 = nv < 8 ? nv : 8, n1 = nv > 8 ? nv - 8 : 0;  // bytes kept of each half: 1..8, 0..8
    w0 &= ~0ull >> (8 * (8 - n0));
    w1 &= n1 ? ~0ull >> (8 * (8 - n1)) : 0ull;
}

// word j of a block (zero-padded) adds to the block's two sums
DDP_HD void mix(u64 w0, u64 w1, u32 j, u64& s0, u64& s1) {
    const u64 t = ((u64)j + 1) * K_IDX;
    const u32 a = (u32)w0, b = (u32)(w0 >> 32), c = (u32)w1, d = (u32)(w1 >> 32);
    const u32 tl = (u32)t, th = (u32)(t >> 32);
    s0 += (u64)(a + (tl ^ (u32)K0)) * (b + (th ^ (u32)(K0 >> 32))) + (u64)(c + (th ^ (u32)K1)) * (d + (tl ^ (u32)(K1 >> 32)));
    s1 += (u64)(a + (th ^ (u32)K2)) * (d + (tl ^ (u32)(K2 >> 32))) + (u64)(b + (tl ^ (u32)K3)) * (c + (th ^ (u32)(K3 >> 32)));
}

// sums + length -> fingerprint
DDP_HD void finish(u64 s0, u64 s1, u64 len, u64 fp[2]) {
    const u64 l = (len + 1) * K_IDX;
    fp[0] = mulfold(s0 ^ K4, l | 1) + s1;
    fp[1] = mulfold(s1 ^ K5, rotl(l, 29) | 1) ^ rotl(s0, 17);
}

// workgroups for `nitems` items (one item per wave and pass)
DDP_HD u32 grid_for(u64 nitems) { return rng::grid_for(nitems); }

}  // namespace ddp
