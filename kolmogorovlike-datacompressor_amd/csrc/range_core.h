// Random-access reads: the integer core of the gather kernel (k_range.hip), shared with the CPU
// emulation tools/range_emu.cpp (which walks the same items with one virtual lane per thread of
// a wave).
//
// nseg segments {src, dst, len} — byte offsets into a source and a destination buffer, each with
// its own alignment — are copied.  A segment is cut into items at the destination's ITEM-byte
// grid (the destination address rounded down to 16 is the grid's origin), so every item but a
// segment's first begins at an aligned destination word and no item is longer than ITEM bytes:
//   items         items of a segment: ceil((dst mod 16 + len) / ITEM), 0 when len = 0
//   find_seg      the segment that holds item t: binary search in the exclusive scan of the
//                 per-segment item counts (nseg + 1 words; segments without items never match)
//   item          the item's byte range [o0, o1) of its segment and its head / body / tail split:
//                 head = the bytes before the destination's first 16-byte boundary (< 16, only a
//                 segment's first item has one), body = whole aligned destination words, tail =
//                 the rest (< 16, only a segment's last item has one)
//   src_word      a destination word's 16 source bytes begin `sh` = (src - dst) mod 16 bytes
//                 into an aligned source word: they are formed from that word and the next one
//                 (a funnel shift by sh bytes; sh = 0 needs the first word alone)
// Contract of the callers, which nothing here can check: head and tail are read and written byte
// by byte; body words are written with aligned 16-byte stores, all of whose bytes belong to the
// segment; the loads are aligned 16-byte words that hold at least one byte of the segment (when
// sh != 0 both words hold bytes of the destination word's 16, all of them the segment's).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RNG_HD __host__ __device__ inline
#else
#define RNG_HD inline
#endif

namespace rng {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 WORD = 16;                 // bytes per load / store
constexpr u32 WAVE = 64;                 // lanes: one wave takes one item
constexpr u32 UNROLL = 4;                // destination words per lane and item
constexpr u32 ITEM = WORD * WAVE * UNROLL;  // bytes per item at the most (4 KiB)
constexpr u32 WG = 256;                  // threads per workgroup (4 waves)
constexpr u32 MAX_GRID = 2048;           // workgroups: the waves stride over the items beyond

struct Seg {
    u64 src;  // byte offset in the source buffer
    u64 dst;  // byte offset in the destination buffer
    u64 len;
};

struct Item {
    u64 o0;     // the item is bytes [o0, o0 + head + 16 * words + tail) of its segment
    u32 head;   // bytes, one by one
    u32 words;  // aligned 16-byte destination words (<= WAVE * UNROLL)
    u32 tail;   // bytes, one by one
};

// dmis = the destination address of the segment's first byte mod 16
RNG_HD u64 items(u32 dmis, u64 len) { return len ? (dmis + len + ITEM - 1) / ITEM : 0; }

// largest i < nseg with scan[i] <= t (t < scan[nseg], scan[0] = 0)
RNG_HD u32 find_seg(const u32* scan, u32 nseg, u32 t) {
    u32 lo = 0, hi = nseg;  // scan[lo] <= t < scan[hi]
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (scan[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// item k (< items(dmis, len)) of a segment
RNG_HD Item item(u32 dmis, u64 len, u64 k) {
    Item it;
    const u64 v0 = k * ITEM, v1 = v0 + ITEM;  // on the grid: segment byte o lies at dmis + o
    it.o0 = v0 > dmis ? v0 - dmis : 0;
    const u64 o1 = v1 - dmis < len ? v1 - dmis : len;
    const u32 n = (u32)(o1 - it.o0);
    const u32 h = (WORD - (u32)((dmis + it.o0) & (WORD - 1))) & (WORD - 1);
    it.head = h < n ? h : n;
    it.words = (n - it.head) / WORD;
    it.tail = n - it.head - it.words * WORD;
    return it;
}

// low 32 bits of (hi:lo) >> r, r = 0, 8, 16, 24
RNG_HD u32 funnel(u32 lo, u32 hi, u32 r) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, r);
#else
    return r ? (lo >> r) | (hi << (32 - r)) : lo;
#endif
}

// out = bytes [sh, sh + 16) of the 32 bytes a (aligned source word) : b (the next one); memory
// order (little-endian words).  sh = 0: b is not read.
RNG_HD void src_word(const u32 a[4], const u32 b[4], u32 sh, u32 out[4]) {
    const u32 r = 8 * (sh & 3u);
    switch (sh >> 2) {  // whole words of the shift: static register indices in every arm
    case 0:
        out[0] = funnel(a[0], a[1], r), out[1] = funnel(a[1], a[2], r), out[2] = funnel(a[2], a[3], r);
        out[3] = r ? funnel(a[3], b[0], r) : a[3];
        break;
    case 1:
        out[0] = funnel(a[1], a[2], r), out[1] = funnel(a[2], a[3], r), out[2] = funnel(a[3], b[0], r);
        out[3] = funnel(b[0], b[1], r);
        break;
    case 2:
        out[0] = funnel(a[2], a[3], r), out[1] = funnel(a[3], b[0], r), out[2] = funnel(b[0], b[1], r);
        out[3] = funnel(b[1], b[2], r);
        break;
    default:
        out[0] = funnel(a[3], b[0], r), out[1] = funnel(b[0], b[1], r), out[2] = funnel(b[1], b[2], r);
        out[3] = funnel(b[2], b[3], r);
        break;
    }
}

// workgroups for `nitems` items (one item per wave and pass)
RNG_HD u32 grid_for(u64 nitems) {
    const u64 g = (nitems + WG / WAVE - 1) / (WG / WAVE);
    return g < 1 ? 1 : g < MAX_GRID ? (u32)g : MAX_GRID;
}

}  // namespace rng
