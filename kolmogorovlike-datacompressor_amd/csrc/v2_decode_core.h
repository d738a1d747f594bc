// Decode side of candidate 10 (v2_new, decode_new_pipeline PY:1578-1648): the pieces that are
// plain integer code, shared by the kernels of k_v2dec.hip and by the CPU emulation
// tools/v2_decode_emu.cpp (which decodes whole payloads with the kernels' tiling).
//
//   header        h0 (mode << 5 | plen), plen <= 4 little-endian param bytes, raw_mask, b1_mask,
//                 one Rice k per encoded plane, plane data.  k > 15 is malformed here (PY accepts
//                 any byte; no encoder writes one, PY:1489 tries k = 0..15).
//   Rice planes   a plane starts on a byte; codewords = q ones, a zero, k remainder bits MSB
//                 first, value q << k | r >= 1, read until the values sum to n exactly.  The
//                 plane is walked in tiles of TILE_WORDS 64-bit words, one word per thread:
//                   phase_fn      the word's phase transition for the plane's k: phase 0 = in a
//                                 unary run (or at a codeword start), p = p remainder bits
//                                 pending; 16 phases x 4 bits = one u64, composed by a scan
//                   word_summary  from the word's entry phase: codewords that end (their zero)
//                                 in the word, their value sum without the ones carried in, and
//                                 the trailing ones (joined across words by a segmented sum)
//                   word_emit     the values with the carry added: run starts marked at their
//                                 cumulative position until the sum reaches n
//                 Remainder bits are read at their absolute position, so only the phase, the
//                 pending ones, the running sum and the run count cross words and tiles.
//   automaton     r[i] = y[i] ^ p(r[i-1], r[i-2], r[i-3]) (PY:1056-1092 and the models'
//                 backward methods): auto_kind() says whether a mode is the identity, a strided
//                 prefix XOR (modes 1 and 3) or a serial recurrence (modes 2, 4, 5: serial_pred).
// Every loop here is bounded by the word's 64 bits; nothing reads outside [p, p + plen).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define V2D_HD __host__ __device__ inline
#else
#define V2D_HD inline
#endif

namespace v2d {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 TILE_WORDS = 256;             // 64-bit words per parse tile (one per thread)
constexpr u32 TILE_BYTES = TILE_WORDS * 8;  // payload bytes per parse tile
constexpr u32 AUTO_TILE = 4096;             // mapped bytes per automaton tile
constexpr u32 KMAX = 15;                    // largest Rice k decoded here
constexpr u64 PHASE_ID = 0xFEDCBA9876543210ull;

struct Header {
    u32 mode, param, raw_mask, b1_mask;
    u32 data;  // byte offset of the plane data
    u8 k[8];   // Rice k of the encoded planes, in plane order
};

// false: malformed (PY:1586-1604), or a k above KMAX
V2D_HD bool parse_header(const u8* p, u64 plen, Header& h) {
    if (plen < 3) return false;
    const u32 nparam = p[0] & 7u;
    h.mode = (p[0] >> 5) & 7u;
    if (nparam > 4 || plen < 1 + nparam + 2) return false;
    h.param = 0;
    for (u32 i = 0; i < nparam; ++i) h.param |= (u32)p[1 + i] << (8 * i);
    u32 pos = 1 + nparam;
    h.raw_mask = p[pos];
    h.b1_mask = p[pos + 1];
    pos += 2;
    u32 nenc = 0;
    for (u32 j = 0; j < 8; ++j) nenc += !((h.raw_mask >> j) & 1u);
    if ((u64)pos + nenc > plen) return false;
    for (u32 i = 0; i < 8; ++i) h.k[i] = 0;
    for (u32 i = 0; i < nenc; ++i) {
        h.k[i] = p[pos + i];
        if (h.k[i] > KMAX) return false;
    }
    h.data = pos + nenc;
    return true;
}

// ones at the top of x (0..64)
V2D_HD u32 lead_ones(u64 x) {
    const u64 y = ~x;
    if (!y) return 64;
#if defined(__HIP_DEVICE_COMPILE__)
    return (u32)__clzll((long long)y);
#else
    return (u32)__builtin_clzll(y);
#endif
}

// the 8 payload bytes from byte B, big-endian (stream order = MSB first), zero past plen;
// nv = bits of the word inside the payload
V2D_HD u64 load_word(const u8* p, u64 plen, u64 B, u32& nv) {
    u64 w = 0;
    const u64 left = B < plen ? plen - B : 0;
    nv = left >= 8 ? 64u : (u32)left * 8u;
    for (u32 i = 0; i < 8; ++i) w = (w << 8) | (i < left ? p[B + i] : 0u);
    return w;
}

// k <= 15 bits from absolute bit g, MSB first; the caller checked g + k <= 8 * plen
V2D_HD u32 read_bits(const u8* p, u64 g, u32 k) {
    u32 r = 0;
    for (u32 t = 0; t < k; ++t) {
        const u64 x = g + t;
        r = (r << 1) | ((p[x >> 3] >> (7 - (u32)(x & 7))) & 1u);
    }
    return r;
}

V2D_HD u32 phase_apply(u64 f, u32 e) { return (u32)(f >> (4 * e)) & 15u; }

// f first, then g
V2D_HD u64 phase_compose(u64 f, u64 g) {
    u64 h = 0;
    for (u32 e = 0; e < 16; ++e) h |= (u64)phase_apply(g, phase_apply(f, e)) << (4 * e);
    return h;
}

// exit phase of a word for every entry phase 0..k (entries above k never occur: 0)
V2D_HD u64 phase_fn(u64 w, u32 nv, u32 k) {
    if (nv == 0) return PHASE_ID;
    u64 f = 0;
    for (u32 e = 0; e <= k; ++e) {
        u32 ex;
        if (e >= nv) {
            ex = e - nv;
        } else {
            u32 pos = e;
            for (;;) {  // <= 64 codewords
                const u32 z = pos + lead_ones(w << pos);
                if (z >= nv) {
                    ex = 0;
                    break;
                }
                pos = z + 1 + k;
                if (pos >= nv) {
                    ex = pos - nv;
                    break;
                }
            }
        }
        f |= (u64)ex << (4 * e);
    }
    return f;
}

// trailing ones of a span of words; whole = the span is ones only and joins what precedes it
struct Ones {
    u64 tail;
    u32 whole;
    u32 pad;
};
V2D_HD Ones ones_join(Ones a, Ones b) {
    Ones r;
    r.tail = b.whole ? a.tail + b.tail : b.tail;
    r.whole = a.whole & b.whole;
    r.pad = 0;
    return r;
}

// Walks the codewords whose terminating zero lies in the word (entry phase e): on_term(z, q,
// joins) gets the zero's bit, the ones before it inside the word and whether the ones carried
// in from earlier words belong to it; it returns false to stop.  Result: the word's Ones.
template <class F>
V2D_HD Ones walk_word(u64 w, u32 nv, u32 e, u32 k, F&& on_term) {
    Ones o;
    o.tail = 0;
    o.whole = 0;
    o.pad = 0;
    u32 pos = e < nv ? e : nv;
    bool joins = e == 0;
    while (pos < nv || joins) {
        const u32 ones = pos < nv ? lead_ones(w << pos) : 0u;
        const u32 z = pos + ones;
        if (z >= nv) {
            o.tail = nv - pos;
            o.whole = joins ? 1u : 0u;
            return o;
        }
        if (!on_term(z, ones, joins)) return o;
        joins = false;
        pos = z + 1 + k;
    }
    return o;
}

struct WordSum {
    u32 cnt;    // codewords ending in the word
    u32 joins;  // the first of them takes the ones carried in
    u64 lsum;   // their values, without that carry
    Ones ones;
};

// B = the word's first payload byte.  A codeword whose remainder runs past the payload counts
// with r = 0 and ends the walk: word_emit reports it if it is reached.
V2D_HD WordSum word_summary(const u8* p, u64 plen, u64 B, u64 w, u32 nv, u32 e, u32 k) {
    WordSum s;
    s.cnt = 0;
    s.joins = 0;
    s.lsum = 0;
    s.ones = walk_word(w, nv, e, k, [&](u32 z, u32 q, bool j) {
        const u64 rb = B * 8 + z + 1;
        const bool ok = rb + k <= plen * 8;
        s.lsum += ((u64)q << k) | (ok ? read_bits(p, rb, k) : 0u);
        s.cnt += 1;
        if (j) s.joins = 1;
        return ok;
    });
    return s;
}

struct Emit {
    u32 bad;    // zero value, sum past n, or remainder past the payload
    u32 done;   // the sum reached n
    u64 endbit; // bit after the last codeword
};

// The word's values in order, from cum < n positions and `run` runs before it: mark(pos) for
// every run start but the plane's first, until the sum reaches n (PY:1462-1486).
template <class M>
V2D_HD Emit word_emit(const u8* p, u64 plen, u64 B, u64 w, u32 nv, u32 e, u32 k, u64 carry, u64 cum, u32 run, u32 n,
                      M&& mark) {
    Emit r;
    r.bad = 0;
    r.done = 0;
    r.endbit = 0;
    walk_word(w, nv, e, k, [&](u32 z, u32 q, bool j) {
        const u64 rb = B * 8 + z + 1;
        if (rb + k > plen * 8) {
            r.bad = 1;
            return false;
        }
        const u64 val = (((u64)q + (j ? carry : 0)) << k) | read_bits(p, rb, k);
        if (val == 0) {
            r.bad = 1;
            return false;
        }
        if (run) mark((u32)cum);
        ++run;
        cum += val;
        if (cum > n) {
            r.bad = 1;
            return false;
        }
        if (cum == n) {
            r.done = 1;
            r.endbit = rb + k;
            return false;
        }
        return true;
    });
    return r;
}

// ---- automaton inverse
enum : u32 { AUTO_ID = 0, AUTO_SCAN = 1, AUTO_SERIAL = 2 };
V2D_HD u32 auto_kind(u32 mode, u32 param) {
    if (mode == 0 || mode > 5 || (mode == 1 && param == 0)) return AUTO_ID;
    return mode == 1 || mode == 3 ? AUTO_SCAN : AUTO_SERIAL;
}

// Strided prefix XOR r[i] = v[i] ^ (r[i - d] & mask) for d <= 16, a chunk of chunk_len(d) bytes
// per thread held in 128 bits (byte q = position q of the chunk; the chunk length is a multiple of
// d, so position mod d is the same in every chunk and tile): chunk_scan inside the chunk, chunk_agg
// = its last d bytes (XOR-scanned over the threads and tiles), chunk_apply adds the carry.
typedef unsigned __int128 u128;
constexpr u32 AUTO_THREADS = 256;
V2D_HD u32 chunk_len(u32 d) { return d * (16u / d); }
V2D_HD u128 byte_mask(u32 mask) {
    u128 m = mask & 0xFFu;
    for (u32 s = 8; s < 128; s <<= 1) m |= m << s;
    return m;
}
V2D_HD u128 low_bytes(u32 d) { return d >= 16 ? ~(u128)0 : (((u128)1 << (8 * d)) - 1); }
V2D_HD u128 chunk_scan(u128 X, u32 d, u128 M) {
    for (u32 s = d; s < 16; s <<= 1) X ^= (X << (8 * s)) & M;
    return X;
}
V2D_HD u128 chunk_agg(u128 X, u32 d, u32 c, u128 M) { return (X >> (8 * (c - d))) & low_bytes(d) & M; }
V2D_HD u128 chunk_apply(u128 X, u128 carry, u32 d, u128 M) {
    carry &= low_bytes(d);
    for (u32 s = d; s < 16; s <<= 1) carry |= carry << (8 * s);
    return X ^ (carry & M);
}

V2D_HD u32 gray8(u32 v) { return (v ^ (v >> 1)) & 0xFFu; }
V2D_HD u32 dil1(u32 x) { return ((x << 1) | x | (x >> 1)) & 0xFFu; }
V2D_HD u32 ero1(u32 x) { return ~dil1(~x & 0xFFu) & 0xFFu; }

// predictor of byte i from the decoded bytes a = r[i-1], b = r[i-2], c = r[i-3] (modes 2, 4, 5)
V2D_HD u32 serial_pred(u32 mode, u32 param, u64 i, u32 a, u32 b, u32 c) {
    if (i == 0) return 0;
    if (mode == 2) {
        if (i == 1) return a;
        const u32 v = param & 3u;
        return gray8(v == 0 ? a : v == 1 ? b : v == 2 ? (a ^ b) : (a | b));
    }
    if (mode == 4) return i < 3 ? a : ((a & b) | (a & c) | (b & c));
    const u32 m = (param & 1u) == 0 ? ero1(dil1(a)) : dil1(ero1(a));
    const u32 ed = dil1(a) ^ ero1(a);
    return (m & ed) | (a & ~ed & 0xFFu);
}

}  // namespace v2d
