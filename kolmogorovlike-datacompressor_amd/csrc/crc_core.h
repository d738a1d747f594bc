// Block CRC-32: the integer core of k_crc32 (k_crc.hip), shared with the host side (the finish and
// every combine, kolm_api.cpp) and the CPU emulation tools/crc_emu.cpp (which walks the same
// items, waves and lanes).
//
// The checksum is the standard CRC-32 (zlib / gzip / PNG): reflected polynomial 0xEDB88320, initial
// value and final xor 0xFFFFFFFF, crc32(b"123456789") = 0xCBF43926.  A register value stands for a
// polynomial over GF(2) modulo P, bit 31 the coefficient of x^0 (zlib's convention):
//   raw(M)        the table-driven reflected CRC with initial value 0 and no final xor: GF(2)-linear
//                 in M, and zero bytes in front of M do not change it
//   multmodp      a b mod P
//   xpow(e)       x^e mod P.  P is irreducible, so x^(2^32 - 1) = 1 and exponents count modulo
//                 2^32 - 1: a NEGATIVE power of x is the power with 2^32 - 1 added
//   xpow8(n)      x^(8 n), n a signed byte count (|n| < 2^60)
//   shift(c, n)   c x^(8 n): the register after n more zero bytes (n < 0: after taking them away)
//   finish        crc32(block) = raw(block) ^ shift(0xFFFFFFFF, len) ^ 0xFFFFFFFF
//   combine       crc32(A || B) = shift(crc32(A), |B|) ^ crc32(B)  (zlib's crc32_combine)
// raw(A || B) = shift(raw(A), |B|) ^ raw(B), so for any cut of a block into words raw(block) is the
// xor over the words of shift(raw(word), bytes of the block after the word): xor commutes, the words
// may meet lanes and waves in any order.
//
// The kernel's shape (the items, pieces and runs of dedup_core.h: a wave takes a run of up to
// ddp::RUN 4 KiB pieces of one block, lane l words l, l + 64, l + 128, l + 192 of each piece):
//   word          a 16-byte word is reduced by 16 lookups, one table per byte position (T16[k][v] =
//                 raw(v followed by k zero bytes))
//   Horner        a lane's consecutive words lie STRIDE = 1 KiB apart, inside a piece and from one
//                 piece to the next: acc = shift(acc, STRIDE) ^ raw(word), the shift four lookups in
//                 SK[j][v] = shift(v << 8 j, STRIDE).  No multiply per word
//   padding       a run of q pieces is walked as 4 q word rows whatever the block's length: the
//                 words past the block's end are zero (load_words masks the last word's bytes past
//                 it), which leaves raw(block) x^(8 pad) for a block that ends pad bytes before the
//                 run's last row does.  The weight takes the padding back out with a negative power
//   weight        lane l's sum is relative to the end of its last word, 16 (63 - l) bytes before the
//                 end of the run's last row: one multiply by LW[l] = x^(8 16 (63 - l)) per lane and
//                 run.  The wave's xor of those is multiplied by x^(8 (len - end of the last row)),
//                 wave-uniform, from the four byte tables XP[k][v] = x^(v << 8 k) (three multiplies)
//                 and xored into raw[block]
// The tables are generated from the polynomial (gen_tables): nothing is stored as literals.
#pragma once
#include <cstdint>

#include "dedup_core.h"

#if defined(__HIPCC__)
#define CRC_HD __host__ __device__ inline
#else
#define CRC_HD inline
#endif

namespace crc {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 POLY = 0xEDB88320u;              // reflected
constexpr u32 ONE = 0x80000000u;               // x^0
constexpr u32 STRIDE = ddp::WORD * ddp::WAVE;  // bytes between a lane's consecutive words (1 KiB)
constexpr u32 ROWS = ddp::UNROLL;              // word rows per piece

// the tables, one array of u32: offsets in words
constexpr u32 T16 = 0;                 // [16][256]
constexpr u32 SK = T16 + 16 * 256;     // [4][256]
constexpr u32 XP = SK + 4 * 256;       // [4][256]
constexpr u32 LW = XP + 4 * 256;       // [64]
constexpr u32 TABLE_WORDS = LW + ddp::WAVE;  // 6208 words, 24.25 KiB

// a b mod P (32 steps, no branch: the lanes of a wave take it together)
CRC_HD u32 multmodp(u32 a, u32 b) {
    u32 p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
    }
    return p;
}

// the register after one more zero bit: c x
CRC_HD u32 timesx(u32 c) { return (c >> 1) ^ (POLY & (0u - (c & 1u))); }

// x^e, e any u32 (square and multiply; x^(2^32 - 1) = 1, so e = 2^32 - 1 gives 1 as e = 0 does)
CRC_HD u32 xpow(u32 e) {
    u32 p = ONE, sq = ONE >> 1;  // x^(2^k)
    for (; e; e >>= 1) {
        if (e & 1u) p = multmodp(p, sq);
        sq = multmodp(sq, sq);
    }
    return p;
}

// the exponent of x^(8 n) modulo 2^32 - 1, n a signed byte count
CRC_HD u32 exp8(int64_t n) {
    const u64 m = 0xFFFFFFFFull;
    const u64 a = n < 0 ? (u64)(-n) : (u64)n;
    const u64 r = ((a % m) * 8) % m;
    return (u32)(n < 0 && r ? m - r : r);
}

CRC_HD u32 xpow8(int64_t n) { return xpow(exp8(n)); }
CRC_HD u32 shift(u32 c, int64_t n) { return multmodp(xpow8(n), c); }
CRC_HD u32 finish(u32 raw, u64 len) { return raw ^ shift(0xFFFFFFFFu, (int64_t)len) ^ 0xFFFFFFFFu; }
CRC_HD u32 combine(u32 a, u32 b, u64 len_b) { return shift(a, (int64_t)len_b) ^ b; }

// tab[TABLE_WORDS] from the polynomial
inline void gen_tables(u32* tab) {
    for (u32 v = 0; v < 256; ++v) {  // raw of the single byte v
        u32 c = v;
        for (int i = 0; i < 8; ++i) c = timesx(c);
        tab[T16 + v] = c;
    }
    for (u32 k = 1; k < 16; ++k)  // one more zero byte: the byte-wise step with a zero byte
        for (u32 v = 0; v < 256; ++v) {
            const u32 c = tab[T16 + (k - 1) * 256 + v];
            tab[T16 + k * 256 + v] = tab[T16 + (c & 0xFFu)] ^ (c >> 8);
        }
    const u32 xs = xpow8(STRIDE);
    for (u32 j = 0; j < 4; ++j)
        for (u32 v = 0; v < 256; ++v) tab[SK + j * 256 + v] = multmodp(xs, v << (8 * j));
    for (u32 k = 0; k < 4; ++k)
        for (u32 v = 0; v < 256; ++v) tab[XP + k * 256 + v] = xpow(v << (8 * k));
    for (u32 l = 0; l < ddp::WAVE; ++l) tab[LW + l] = xpow8((int64_t)ddp::WORD * (ddp::WAVE - 1 - l));
}

// raw of one 16-byte word (w0 = bytes 0..7, w1 = bytes 8..15, little-endian; zero-padded)
CRC_HD u32 word_raw(const u32* tab, u64 w0, u64 w1) {
    u32 c = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (u32 i = 0; i < 8; ++i) {
        c ^= tab[T16 + (15 - i) * 256 + (u32)((w0 >> (8 * i)) & 0xFFu)];
        c ^= tab[T16 + (7 - i) * 256 + (u32)((w1 >> (8 * i)) & 0xFFu)];
    }
    return c;
}

// shift(acc, STRIDE)
CRC_HD u32 stride_shift(const u32* tab, u32 acc) {
    return tab[SK + (acc & 0xFFu)] ^ tab[SK + 256 + ((acc >> 8) & 0xFFu)] ^ tab[SK + 512 + ((acc >> 16) & 0xFFu)] ^
           tab[SK + 768 + (acc >> 24)];
}

// x^e from the byte tables
CRC_HD u32 xpow_tab(const u32* tab, u32 e) {
    const u32 a = multmodp(tab[XP + (e & 0xFFu)], tab[XP + 256 + ((e >> 8) & 0xFFu)]);
    const u32 b = multmodp(tab[XP + 512 + ((e >> 16) & 0xFFu)], tab[XP + 768 + (e >> 24)]);
    return multmodp(a, b);
}

// the weight of a run of block length len whose last word row ends at block offset `end`
// (a multiple of STRIDE; past len for a block's last run)
CRC_HD u32 run_weight(const u32* tab, u64 len, u64 end) { return xpow_tab(tab, exp8((int64_t)len - (int64_t)end)); }

}  // namespace crc
