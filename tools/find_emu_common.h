// What the CPU emulations of the search kernels share (tools/find_emu.cpp, findcls_emu.cpp,
// findrx_emu.cpp, findset_emu.cpp): the recording loader, the tile skeleton of
// kolmogorovlike-datacompressor_amd/csrc/find_tile.h on virtual threads, one group as the host
// runs it (find_group and emit_matches of kolm_reader.cpp) and the grouped search with the carry
// (find_over_groups).  A file's own Emu mirrors its kernels' prologue and supplies
//   Which                                   the type of a record's pattern index (u8; u32 for a set)
//   ld                                      the loader of the scan buffer (ld.n = its bytes)
//   cols()                                  the pattern columns of cnt (k_find_scan's np; 0 for a set)
//   cap(stage_bytes)                        the records one emit launch may hold
//   count(ntiles, cnt)                      the count kernel: cnt[col * ntiles + tile], column cols() = the tile totals
//   emit(t0, t1, tscan, pos, which, cap)    the emit kernel over tiles [t0, t1); returns its errors
// The three Emus with per-pattern masks (run_tile) take count and emit from tile_count / tile_emit.
#pragma once
#include "../kolmogorovlike-datacompressor_amd/csrc/find_core.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace fnd;

namespace {

// Every load is recorded and checked against the contract: an aligned 16-byte word that holds a
// byte of [buf, buf + n).  The violations are counted.
struct Ld {
    const u8* buf;
    u32 n;
    u64 bad = 0, loads = 0;
    Word operator()(i64 off) {
        ++loads;
        const bool ok = (reinterpret_cast<uintptr_t>(buf + off) & (WORD - 1)) == 0 && off < (i64)n && off + (i64)WORD > 0;
        Word w{{0xA5A5A5A5A5A5A5A5ull, 0xA5A5A5A5A5A5A5A5ull}};
        if (!ok) {
            ++bad;
            return w;
        }
        std::memcpy(w.q, buf + off, WORD);
        return w;
    }
};

// The count kernels' epilogue.  e.run_tile(tile, pm): one workgroup, pm[i][t] = thread t's mask of pattern i.
template <class E>
void tile_count(E& e, u32 ntiles, std::vector<u32>& cnt) {
    const u32 np = e.cols();
    cnt.assign((size_t)(np + 1) * ntiles, 0);
    u32 pm[MAX_PATTERNS][WG];
    for (u32 tile = 0; tile < ntiles; ++tile) {
        e.run_tile(tile, pm);
        for (u32 i = 0; i < np; ++i)
            for (u32 t = 0; t < WG; ++t) {
                const u32 c = (u32)__builtin_popcount(pm[i][t]);
                cnt[(size_t)i * ntiles + tile] += c;
                cnt[(size_t)np * ntiles + tile] += c;
            }
    }
}

// The emit kernels' epilogue over tiles [t0, t1): records at tscan[tile] - tscan[t0] + the thread's offset
template <class E>
u64 tile_emit(E& e, u32 t0, u32 t1, const u64* tscan, u32* pos, u8* which, u64 cap) {
    const u32 np = e.cols();
    u64 over = 0;
    u32 pm[MAX_PATTERNS][WG];
    for (u32 tile = t0; tile < t1; ++tile) {
        e.run_tile(tile, pm);
        u64 slot = tscan[tile] - tscan[t0];
        for (u32 t = 0; t < WG; ++t)
            for (u32 j = 0; j < PER; ++j)
                for (u32 i = 0; i < np; ++i)
                    if ((pm[i][t] >> j) & 1u) {
                        if (slot < cap) pos[slot] = tile * TILE + t * PER + j, which[slot] = (u8)i;
                        else ++over;
                        ++slot;
                    }
        if (slot != tscan[tile + 1] - tscan[t0]) ++over;  // the count and the emit disagree
    }
    return over;
}

// One group as the host runs it: count, scan, the emit launches.  Appends (base + position,
// pattern) to offs / which until `limit` results are held; counts [e.cols()] accumulate.  Returns
// the emit errors and the loader's violations.
template <class E>
u64 find_group(E& e, u64 base, u64 stage_bytes, u64 limit, u64* counts, std::vector<u64>& offs,
               std::vector<typename E::Which>& which, u32* launches) {
    const u32 ntiles = tiles(e.ld.n), np = e.cols();
    if (!ntiles) return 0;
    std::vector<u32> cnt;
    e.count(ntiles, cnt);
    std::vector<u64> tscan((size_t)ntiles + 1, 0);
    for (u32 t = 0; t < ntiles; ++t) tscan[t + 1] = tscan[t] + cnt[(size_t)np * ntiles + t];
    for (u32 i = 0; i < np; ++i)
        for (u32 t = 0; t < ntiles; ++t) counts[i] += cnt[(size_t)i * ntiles + t];
    const u64 room = limit > offs.size() ? limit - offs.size() : 0;
    const u64 want = std::min<u64>(tscan[ntiles], room);
    const u64 cap = e.cap(stage_bytes);
    // a launch never holds more than either; exact, so that ASan sees a slot past them
    std::vector<u32> spos(std::min<u64>(cap, tscan[ntiles]));
    std::vector<typename E::Which> swhich(spos.size());
    u64 got = 0, bad = 0;
    for (u32 t0 = 0; got < want;) {
        while (tscan[t0 + 1] == tscan[t0]) ++t0;
        const u32 t1 = emit_cut(tscan.data(), ntiles, t0, cap, want);
        bad += e.emit(t0, t1, tscan.data(), spos.data(), swhich.data(), spos.size());
        const u64 take = std::min<u64>(tscan[t1] - tscan[t0], want - got);
        for (u64 k = 0; k < take; ++k) offs.push_back(base + spos[k]), which.push_back(swhich[k]);
        got += take;
        t0 = t1;
        ++*launches;
    }
    return bad + e.ld.bad;
}

// n bytes of src at misalignment m in a heap block of exactly the aligned words around them, `fill`
// in the rest of those words.  The data begins at the returned pointer + m; std::free releases it.
inline u8* aligned_block(const u8* src, u32 n, u32 m, u8 fill) {
    const u64 size = ((u64)m + n + WORD - 1) / WORD * WORD;
    u8* raw = (u8*)std::aligned_alloc(WORD, size ? size : WORD);
    std::memset(raw, fill, size);
    if (n) std::memcpy(raw + m, src, n);
    return raw;
}

// The grouped search as the reader runs it, on the CPU: data is the whole stream, group g its
// bytes [bounds[g], bounds[g + 1]) (the groups that hold a byte of the window [lo, hi)), L the
// hold-back.  Every group's scan buffer is a heap block of exactly the aligned words around
// [carry][the group's bytes], the carry ending at a 256-byte boundary as on the device.
// make(buf, n, lo, shi): the file's Emu over one scan buffer.
template <class Which, class Make>
u64 find_grouped(const u8* data, const u64* bounds, u32 ng, u64 lo, u64 hi, u32 L, u8 fill, u64 stage_bytes, u64 limit,
                 u64* counts, std::vector<u64>& offs, std::vector<Which>& which, u32* launches, Make&& make) {
    u64 bad = 0, S = lo;
    for (u32 g = 0; g < ng; ++g) {
        const GroupScan gs = group_scan(S, bounds[g], bounds[g + 1], L, g + 1 == ng, hi);
        const u32 front = (MAX_LEN - gs.carry) & (WORD - 1);  // misalignment of the scan buffer
        u8* raw = aligned_block(data + gs.start, gs.n, front, fill);
        auto e = make(raw + front, gs.n, gs.lo, gs.shi);
        bad += find_group(e, gs.start, stage_bytes, limit, counts, offs, which, launches);
        std::free(raw);
        S = gs.S_next;
    }
    return bad;
}

// the first cap results to the caller's arrays; nfound = all that are held
template <class Which>
void hand_out(const std::vector<u64>& o, const std::vector<Which>& w, u64* offs, Which* which, u64 cap, u64* nfound) {
    *nfound = o.size();
    for (u64 k = 0; k < o.size() && k < cap; ++k) offs[k] = o[k], which[k] = w[k];
}

std::vector<u8> noise(u32 n, u32 seed, u32 letters) {
    std::vector<u8> d(n);
    u64 x = 0x9E3779B97F4A7C15ull * (seed + 1);
    for (u32 i = 0; i < n; ++i) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        d[i] = letters ? (u8)('a' + (x >> 33) % letters) : (u8)(x >> 29);
    }
    return d;
}

u64 g_cases = 0;  // the cases a main() has run

}  // namespace
