// Search of a decoded buffer for a prepared set of up to 65 536 patterns: the integer core of
// k_findset_count / k_findset_emit (k_findset.hip), shared with the CPU emulation
// tools/findset_emu.cpp (which walks the same spans, tiles, threads and positions serially over
// tables of exact size).  Windows, tail verify, bounds rule, hold-back between decode groups and
// the emit cut are those of find_core.h; what is new is that the cost of a position does not grow
// with the set.
//   key          K = min(8, the shortest pattern).  key(pattern) = its first K bytes as a
//                little-endian u64; key(position) = window & prefix_mask(K).  Every pattern has at
//                least K bytes, so a key that takes in bytes past n belongs to no match: the
//                bounds rule rejects it
//   bucket       the patterns of one key, in ascending pattern index: a run of `entries`
//   entries      {word offset of the pattern in the blob, length, pattern index}
//   blob         every pattern zero-padded to whole little-endian u64 words (fnd::tail_ok as it is)
//   slots        open addressing, {key, first entry, count}, count == 0 = empty; a power of two
//                >= 2 x the distinct keys (load <= 0.5: a probe ends), multiply-shift hash, linear
//                probing
//   filter       a bitmap of a power-of-two number of bits >= 16 x the distinct keys, clamped to
//                [2^13, 2^18] (1 KiB .. 32 KiB: it is copied into LDS), one bit per key under a
//                second multiply-shift hash
//   lookup       filter bit, then the probe, then the bucket; verify = masked compare of the first
//                min(len, 8) bytes, tail_ok for the rest, the bounds rule
//   spans        a workgroup walks span_tiles(filter bytes) consecutive tiles, so that the copy of
//                the filter into LDS is paid once per span; counts stay per tile
//   records      (u32 position relative to the scan buffer, u32 pattern index): 8 bytes.  The
//                patterns are pairwise distinct, so the matches of one position are prefixes of
//                one another: at most min(np, 256) of them, which bounds a tile's records
#pragma once
#include "find_core.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace fst {

using fnd::i64;
using fnd::u32;
using fnd::u64;
using fnd::u8;

constexpr u32 MAX_PATTERNS = 65536;  // KOLM_FIND_SET_MAX_PATTERNS
constexpr u32 REC_BYTES = 8;         // u32 position + u32 pattern index
constexpr u32 MAX_PER_POS = 256;     // matches of one position: distinct prefixes of one string of <= 256 bytes
constexpr u32 FILTER_MIN_BITS = 1u << 13, FILTER_MAX_BITS = 1u << 18;
constexpr u64 MUL_SLOT = 0x9E3779B97F4A7C15ull;    // the slot hash: (key * MUL_SLOT) >> (64 - log2 slots)
constexpr u64 MUL_FILTER = 0xC2B2AE3D27D4EB4Full;  // the filter hash, likewise

struct Entry {
    u32 word;  // the pattern's first word in the blob
    u32 len;
    u32 idx;   // the pattern's index in the set
};

struct Slot {
    u64 key;
    u32 first;  // entries [first, first + count)
    u32 count;  // 0: empty
};

struct Info {  // kolm_patset_info_t
    u32 np, K, keys, slots, filter_bits, L, longest_bucket;
};

// The tables as the kernels see them (device pointers) or the emulation does (heap vectors).
struct Set {
    const u32* filter;
    const Slot* slots;
    const Entry* entries;
    const u64* blob;
    u64 kmask;        // prefix_mask(K)
    u32 slot_shift;   // 64 - log2(slots)
    u32 slot_mask;    // slots - 1
    u32 filter_shift; // 64 - log2(filter bits)
    u32 filter_words; // filter bits / 32
    u32 np;
};

FND_HD u32 slot_hash(u64 key, u32 shift) { return (u32)((key * MUL_SLOT) >> shift); }
FND_HD u32 filter_hash(u64 key, u32 shift) { return (u32)((key * MUL_FILTER) >> shift); }

// The bucket of `key`: its number of entries (0: none), the first in `first`.  `filter` is the
// bitmap wherever it lies (the kernels pass their LDS copy).
FND_HD u32 bucket_of(const Set& S, const u32* filter, u64 key, u32& first) {
    const u32 bit = filter_hash(key, S.filter_shift);
    if (!((filter[bit >> 5] >> (bit & 31)) & 1u)) return 0;
    for (u32 h = slot_hash(key, S.slot_shift);; h = (h + 1) & S.slot_mask) {
        const Slot s = S.slots[h];
        if (s.count == 0) return 0;
        if (s.key == key) {
            first = s.first;
            return s.count;
        }
    }
}

// Does the entry's pattern match at position o, whose window is w?
template <class Ld>
FND_HD bool entry_matches(Ld& ld, u64 w, u32 mis, u32 o, u32 lo, u32 shi, u32 n, const Entry& e, const u64* blob) {
    if (o < lo || o >= shi || (u64)o + e.len > n) return false;
    const u64* pat = blob + e.word;
    if ((w ^ pat[0]) & fnd::prefix_mask(e.len)) return false;
    return e.len <= 8 || fnd::tail_ok(ld, mis, o, n, pat, e.len);
}

// The matches of position o: f(entry) for each, in bucket order.  Returns their number.  The
// bucket is walked 32 entries at a time: first every entry of the batch is verified (bit k of m =
// entry k matches), then f runs for the set bits.  f is where the kernels write (a counter, a
// record); keeping it out of the verify loop is the form of the walk that was exact on the
// device ("Pattern sets").
template <class Ld, class F>
FND_HD u32 for_matches(const Set& S, const u32* filter, Ld& ld, u64 w, u32 mis, u32 o, u32 lo, u32 shi, u32 n, F&& f) {
    u32 first = 0, c = 0;
    const u32 cnt = bucket_of(S, filter, w & S.kmask, first);
    for (u32 k0 = 0; k0 < cnt; k0 += 32) {
        const u32 ke = cnt - k0 < 32 ? cnt - k0 : 32;
        u32 m = 0;
        for (u32 k = 0; k < ke; ++k)
            if (entry_matches(ld, w, mis, o, lo, shi, n, S.entries[first + k0 + k], S.blob)) m |= 1u << k;
        for (u32 k = 0; m && k < ke; ++k)
            if ((m >> k) & 1u) {
                f(S.entries[first + k0 + k]);
                ++c;
            }
    }
    return c;
}

// Tiles a workgroup walks: 8 x the filter's bytes of data, at least one tile.
FND_HD u32 span_tiles(u32 filter_bytes) {
    const u32 t = 8 * filter_bytes / fnd::TILE;
    return t ? t : 1;
}
FND_HD u32 spans(u32 ntiles, u32 span) { return (ntiles + span - 1) / span; }

// records the staging buffer holds: never fewer than one tile can produce
FND_HD u64 stage_records(u64 stage_bytes, u32 np) {
    const u64 r = stage_bytes / REC_BYTES, least = (u64)fnd::TILE * (np < MAX_PER_POS ? np : MAX_PER_POS);
    return r < least ? least : r;
}

// ---- host only: the tables of a set ----

struct Tables {
    std::vector<Entry> entries;
    std::vector<u64> blob;
    std::vector<Slot> slots;
    std::vector<u32> filter;
    Info info{};
    // the view over these vectors (a device copy replaces the four pointers)
    Set view() const {
        Set S{};
        S.filter = filter.data(), S.slots = slots.data(), S.entries = entries.data(), S.blob = blob.data();
        S.kmask = fnd::prefix_mask(info.K);
        S.slot_shift = 64 - log2u(info.slots), S.slot_mask = info.slots - 1;
        S.filter_shift = 64 - log2u(info.filter_bits), S.filter_words = info.filter_bits / 32;
        S.np = info.np;
        return S;
    }
    static u32 log2u(u32 v) {
        u32 k = 0;
        while ((1u << k) < v) ++k;
        return k;
    }
};

inline u32 pow2_at_least(u64 v) {
    u32 p = 1;
    while (p < v) p <<= 1;
    return p;
}

// pats[pat_off[i], pat_off[i + 1]) = pattern i; 1 <= np <= MAX_PATTERNS and every length in
// 1..fnd::MAX_LEN are checked by the caller.  Returns false when two patterns are equal, their
// indices (a < b) in dup.
inline bool build(const u8* pats, const u32* pat_off, u32 np, Tables& T, u32 dup[2]) {
    T = Tables{};
    u32 K = 8, L = 0;
    for (u32 i = 0; i < np; ++i) {
        const u32 len = pat_off[i + 1] - pat_off[i];
        K = std::min(K, len), L = std::max(L, len);
    }
    const u64 kmask = fnd::prefix_mask(K);
    // the blob, and every pattern's key from its first word
    std::vector<u32> word(np);
    std::vector<u64> key(np);
    for (u32 i = 0; i < np; ++i) {
        const u32 len = pat_off[i + 1] - pat_off[i];
        word[i] = (u32)T.blob.size();
        T.blob.resize(T.blob.size() + (len + 7) / 8, 0);
        for (u32 k = 0; k < len; ++k) T.blob[word[i] + (k >> 3)] |= (u64)pats[pat_off[i] + k] << (8 * (k & 7));
        key[i] = T.blob[word[i]] & kmask;
    }
    std::vector<u32> order(np);
    for (u32 i = 0; i < np; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return key[a] != key[b] ? key[a] < key[b] : a < b; });
    T.entries.resize(np);
    for (u32 k = 0; k < np; ++k) T.entries[k] = Entry{word[order[k]], pat_off[order[k] + 1] - pat_off[order[k]], order[k]};
    // the buckets; two equal patterns share a bucket, where a sort by content puts them side by side
    struct Run {
        u32 first, count;
    };
    std::vector<Run> runs;
    for (u32 k = 0; k < np;) {
        u32 e = k + 1;
        while (e < np && key[order[e]] == key[order[k]]) ++e;
        runs.push_back(Run{k, e - k});
        k = e;
    }
    auto less = [&](u32 a, u32 b) {  // by content, then by index
        const u32 la = pat_off[a + 1] - pat_off[a], lb = pat_off[b + 1] - pat_off[b];
        const int c = std::memcmp(pats + pat_off[a], pats + pat_off[b], std::min(la, lb));
        return c ? c < 0 : la != lb ? la < lb : a < b;
    };
    bool found = false;
    std::vector<u32> by;
    for (const Run& r : runs) {
        T.info.longest_bucket = std::max(T.info.longest_bucket, r.count);
        if (r.count < 2) continue;
        by.assign(order.begin() + r.first, order.begin() + r.first + r.count);
        std::sort(by.begin(), by.end(), less);
        for (u32 k = 0; k + 1 < by.size(); ++k) {
            const u32 a = by[k], b = by[k + 1];
            const u32 la = pat_off[a + 1] - pat_off[a], lb = pat_off[b + 1] - pat_off[b];
            if (la == lb && std::memcmp(pats + pat_off[a], pats + pat_off[b], la) == 0 && (!found || a < dup[0])) {
                dup[0] = a, dup[1] = b;  // the pair with the lowest first index: the same from run to run
                found = true;
            }
        }
    }
    if (found) return false;
    const u32 nkeys = (u32)runs.size();
    T.info.np = np, T.info.K = K, T.info.L = L, T.info.keys = nkeys;
    T.info.slots = pow2_at_least(2ull * nkeys);
    if (T.info.slots < 2) T.info.slots = 2;
    T.info.filter_bits = std::min(FILTER_MAX_BITS, std::max(FILTER_MIN_BITS, pow2_at_least(16ull * nkeys)));
    T.slots.assign(T.info.slots, Slot{0, 0, 0});
    T.filter.assign(T.info.filter_bits / 32, 0);
    const u32 sshift = 64 - Tables::log2u(T.info.slots), fshift = 64 - Tables::log2u(T.info.filter_bits);
    for (const Run& r : runs) {
        const u64 k = key[order[r.first]];
        u32 h = slot_hash(k, sshift);
        while (T.slots[h].count) h = (h + 1) & (T.info.slots - 1);
        T.slots[h] = Slot{k, r.first, r.count};
        const u32 bit = filter_hash(k, fshift);
        T.filter[bit >> 5] |= 1u << (bit & 31);
    }
    return true;
}

}  // namespace fst
