// CPU emulation of the class-pattern search kernels: the header k_findcls_count / k_findcls_emit of
// kolmogorovlike-datacompressor_amd/csrc/k_findcls.hip compile (csrc/findcls_core.h, over
// csrc/find_core.h), driven with the kernels' shape as tools/find_emu.cpp drives find_core.h — 4 KiB
// tiles, 256 virtual threads with 16 positions each, the per-pattern masks of a tile, the counts,
// the exclusive scan of the tile totals, the emit launches cut at scanned tile boundaries — behind
// a C interface for tests/test_findcls_core.py, and a main() that runs the sweeps on its own over
// heap buffers of exactly the aligned words the load contract allows (built with
// -fsanitize=address,undefined by the test: a load outside them is an error there).  Every load
// is recorded and checked against the contract: an aligned 16-byte word that holds a byte of
// [buf, buf + n).  The violations are counted.  What such a word holds outside [buf, buf + n) is
// 0x00 here, the byte a class is most likely to hold by accident.
//   g++ -O2 -std=c++17 -shared -fPIC tools/findcls_emu.cpp -o findcls_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/findcls_emu.cpp -o findcls_emu
//   ./findcls_emu     exit status 0 when every case matches the byte-by-byte reference
#include "../kolmogorovlike-datacompressor_amd/csrc/findcls_core.h"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

using namespace fnd;

namespace {

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

struct Emu {
    Ld ld;
    u32 lo, shi;
    const fcl::Pats& P;
    u32 np;
    u32 mis() const { return (u32)(reinterpret_cast<uintptr_t>(ld.buf) & (WORD - 1)); }

    // one workgroup: pm[i][t] = thread t's mask of pattern i
    void run_tile(u32 tile, u32 pm[MAX_PATTERNS][WG]) {
        for (u32 t = 0; t < WG; ++t) {
            const u32 p0 = tile * TILE + t * PER;
            u64 w[PER];
            windows(ld, mis(), p0, ld.n, w);
            for (u32 i = 0; i < np; ++i) pm[i][t] = fcl::match_mask(ld, w, mis(), p0, lo, shi, ld.n, P, i);
        }
    }
    // k_findcls_count: cnt[col * ntiles + tile]
    void count(u32 ntiles, std::vector<u32>& cnt) {
        cnt.assign((size_t)(np + 1) * ntiles, 0);
        u32 pm[MAX_PATTERNS][WG];
        for (u32 tile = 0; tile < ntiles; ++tile) {
            run_tile(tile, pm);
            for (u32 i = 0; i < np; ++i)
                for (u32 t = 0; t < WG; ++t) {
                    const u32 c = (u32)__builtin_popcount(pm[i][t]);
                    cnt[(size_t)i * ntiles + tile] += c;
                    cnt[(size_t)np * ntiles + tile] += c;
                }
        }
    }
    // k_findcls_emit over tiles [t0, t1): records at tscan[tile] - tscan[t0] + the thread's offset
    u64 emit(u32 t0, u32 t1, const u64* tscan, u32* pos, u8* which, u64 cap) {
        u64 over = 0;
        u32 pm[MAX_PATTERNS][WG];
        for (u32 tile = t0; tile < t1; ++tile) {
            run_tile(tile, pm);
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
};

// One group as the host runs it: count, scan, the emit launches.  Appends (base + position,
// pattern) to offs / which until `limit` results are held; counts [np] accumulate.
u64 find_group(const u8* buf, u32 n, u32 lo, u32 shi, const fcl::Pats& P, u32 np, u64 base, u64 stage_bytes, u64 limit,
               u64* counts, std::vector<u64>& offs, std::vector<u8>& which, u32* launches) {
    Emu e{Ld{buf, n}, lo, shi, P, np};
    const u32 ntiles = tiles(n);
    if (!ntiles) return 0;
    std::vector<u32> cnt;
    e.count(ntiles, cnt);
    std::vector<u64> tscan((size_t)ntiles + 1, 0);
    for (u32 t = 0; t < ntiles; ++t) tscan[t + 1] = tscan[t] + cnt[(size_t)np * ntiles + t];
    for (u32 i = 0; i < np; ++i)
        for (u32 t = 0; t < ntiles; ++t) counts[i] += cnt[(size_t)i * ntiles + t];
    const u64 room = limit > offs.size() ? limit - offs.size() : 0;
    const u64 want = std::min<u64>(tscan[ntiles], room);
    const u64 cap = stage_records(stage_bytes, np);
    std::vector<u32> spos(std::min<u64>(cap, tscan[ntiles]));  // a launch never holds more than either
    std::vector<u8> swhich(spos.size());
    u64 got = 0, bad = 0;
    for (u32 t0 = 0; got < want;) {
        while (tscan[t0 + 1] == tscan[t0]) ++t0;
        const u32 t1 = emit_cut(tscan.data(), ntiles, t0, cap, want);
        bad += e.emit(t0, t1, tscan.data(), spos.data(), swhich.data(), cap);
        const u64 take = std::min<u64>(tscan[t1] - tscan[t0], want - got);
        for (u64 k = 0; k < take; ++k) offs.push_back(base + spos[k]), which.push_back(swhich[k]);
        got += take;
        t0 = t1;
        ++*launches;
    }
    return bad + e.ld.bad;
}

// the checks of the library (findcls_check_pats in kolm_reader.cpp) and the tables
bool prepare(const u8* bitmaps, const u32* pat_off, u32 np, fcl::Pats& P, u32* L) {
    if (np < 1 || np > MAX_PATTERNS) return false;
    *L = 0;
    for (u32 i = 0; i < np; ++i) {
        if (pat_off[i + 1] <= pat_off[i] || pat_off[i + 1] - pat_off[i] > MAX_LEN) return false;
        *L = std::max(*L, pat_off[i + 1] - pat_off[i]);
    }
    u32 ntab, bp, bq;
    return fcl::make_pats(bitmaps, pat_off, np, P, &ntab, &bp, &bq);
}

}  // namespace

// The search of buf [0, n) (any alignment; the aligned words around it must be readable) for
// matches that start in [lo, n).  bitmaps: 32 bytes per position, pattern i the positions
// [pat_off[i], pat_off[i + 1]).  counts [np] exact; the first min(total, limit) matches to
// offs / which (cap entries; fewer are written when cap is smaller); nfound = their number;
// launches = emit launches.  Returns the number of contract violations; ~0 for arguments the
// library refuses (65 distinct table classes among them).
extern "C" uint64_t fcl_emu_find(const uint8_t* buf, uint32_t n, uint32_t lo, const uint8_t* bitmaps, const uint32_t* pat_off,
                                 uint32_t np, uint64_t stage_bytes, uint64_t limit, uint64_t* counts, uint64_t* offs,
                                 uint8_t* which, uint64_t cap, uint64_t* nfound, uint32_t* launches) {
    fcl::Pats P;
    u32 L;
    if (!prepare(bitmaps, pat_off, np, P, &L)) return ~0ull;
    std::vector<u64> o;
    std::vector<u8> w;
    u32 l = 0;
    for (u32 i = 0; i < np; ++i) counts[i] = 0;
    const u64 bad = find_group(buf, n, lo, n, P, np, 0, stage_bytes, limit, counts, o, w, &l);
    *nfound = o.size();
    *launches = l;
    for (u64 k = 0; k < o.size() && k < cap; ++k) offs[k] = o[k], which[k] = w[k];
    return bad;
}

// The grouped search as the reader runs it, on the CPU: data is the whole stream, group g its
// bytes [bounds[g], bounds[g + 1]) (the groups that hold a byte of the window [lo, hi)).  Every
// group's scan buffer is a heap block of exactly the aligned words around [carry][the group's
// bytes], the carry ending at a 256-byte boundary as on the device; the rest of those words is 0x00.
extern "C" uint64_t fcl_emu_find_grouped(const uint8_t* data, const uint64_t* bounds, uint32_t ng, uint64_t lo, uint64_t hi,
                                         const uint8_t* bitmaps, const uint32_t* pat_off, uint32_t np, uint64_t stage_bytes,
                                         uint64_t limit, uint64_t* counts, uint64_t* offs, uint8_t* which, uint64_t cap,
                                         uint64_t* nfound, uint32_t* launches) {
    fcl::Pats P;
    u32 L;
    if (!prepare(bitmaps, pat_off, np, P, &L)) return ~0ull;
    std::vector<u64> o;
    std::vector<u8> w;
    u32 l = 0;
    u64 bad = 0, S = lo;
    for (u32 i = 0; i < np; ++i) counts[i] = 0;
    for (u32 g = 0; g < ng; ++g) {
        const GroupScan gs = group_scan(S, bounds[g], bounds[g + 1], L, g + 1 == ng, hi);
        const u32 front = (MAX_LEN - gs.carry) & (WORD - 1);  // misalignment of the scan buffer
        const u64 size = ((u64)front + gs.n + WORD - 1) / WORD * WORD;
        u8* raw = (u8*)std::aligned_alloc(WORD, size ? size : WORD);
        std::memset(raw, 0, size);
        std::memcpy(raw + front, data + gs.start, gs.n);
        bad += find_group(raw + front, gs.n, gs.lo, gs.shi, P, np, gs.start, stage_bytes, limit, counts, o, w, &l);
        std::free(raw);
        S = gs.S_next;
    }
    *nfound = o.size();
    *launches = l;
    for (u64 k = 0; k < o.size() && k < cap; ++k) offs[k] = o[k], which[k] = w[k];
    return bad;
}

// A class as the library sorts it: 0 empty, 1 masked equality (mask, value written), 2 table class.
extern "C" uint32_t fcl_emu_classify(const uint8_t* bitmap, uint8_t* mask, uint8_t* value) {
    const fcl::Class c = fcl::classify(bitmap);
    *mask = c.mask, *value = c.value;
    return !c.size ? 0 : c.eq ? 1 : 2;
}

extern "C" uint32_t fcl_emu_tile_bytes(void) { return TILE; }

namespace {

u64 g_cases = 0;

typedef std::array<bool, 256> Cls;  // a class: its members
typedef std::vector<Cls> Pat;   // a class per position
typedef std::vector<std::pair<u64, u8>> Hits;

Hits reference(const std::vector<u8>& d, const std::vector<Pat>& pats) {
    Hits h;
    for (u64 o = 0; o < d.size(); ++o)
        for (size_t i = 0; i < pats.size(); ++i) {
            bool ok = o + pats[i].size() <= d.size();
            for (size_t k = 0; ok && k < pats[i].size(); ++k) ok = pats[i][k][d[o + k]];
            if (ok) h.push_back({o, (u8)i});
        }
    return h;
}

// data at misalignment m in a heap block of exactly the aligned words around it, zeros around the data
int run_case(const std::vector<u8>& d, u32 m, const std::vector<Pat>& pats, u64 stage, const char* what) {
    const u32 n = (u32)d.size();
    const u64 size = ((u64)m + n + WORD - 1) / WORD * WORD;
    u8* raw = (u8*)std::aligned_alloc(WORD, size ? size : WORD);
    std::memset(raw, 0, size);
    if (n) std::memcpy(raw + m, d.data(), n);
    std::vector<u8> flat;
    std::vector<u32> off{0};
    for (auto& p : pats) {
        for (auto& c : p) {
            u8 bm[fcl::BITMAP] = {};
            for (u32 b = 0; b < 256; ++b)
                if (c[b]) bm[b >> 3] |= (u8)(1u << (b & 7));
            flat.insert(flat.end(), bm, bm + fcl::BITMAP);
        }
        off.push_back(off.back() + (u32)p.size());
    }
    const Hits want = reference(d, pats);
    std::vector<u64> counts(pats.size()), offs(want.size() + 1);
    std::vector<u8> which(want.size() + 1);
    u64 nfound = 0;
    u32 launches = 0;
    const u64 bad = fcl_emu_find(raw + m, n, 0, flat.data(), off.data(), (u32)pats.size(), stage, ~0ull, counts.data(),
                                 offs.data(), which.data(), offs.size(), &nfound, &launches);
    int fail = bad != 0 || nfound != want.size();
    for (size_t k = 0; k < want.size() && !fail; ++k) fail = offs[k] != want[k].first || which[k] != want[k].second;
    if (fail)
        std::fprintf(stderr, "%s: n %u, misalignment %u, %zu patterns (first of %zu positions): %llu violations, %llu found, %zu expected\n",
                     what, n, m, pats.size(), pats[0].size(), (unsigned long long)bad, (unsigned long long)nfound, want.size());
    std::free(raw);
    ++g_cases;
    return fail;
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

Cls range(u32 a, u32 b) {
    Cls s{};
    for (u32 x = a; x <= b; ++x) s[x] = true;
    return s;
}

Cls of(std::initializer_list<u8> l) {
    Cls s{};
    for (u8 x : l) s[x] = true;
    return s;
}

}  // namespace

#ifndef FCL_EMU_NO_MAIN
int main() {
    int bad = 0;
    const u32 ns[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8193};
    const u32 lens[] = {1, 2, 7, 8, 9, 16, 17, 255, 256};
    const Cls any = range(0, 255), digit = range('0', '9'), low = range(0, 9), zero_or_z = of({0, 'z'});
    for (u32 m = 0; m < 16; ++m)
        for (u32 n : ns)
            for (u32 len : lens) {
                // wildcards only: every start at which the pattern fits
                bad |= run_case(noise(n, n + len, 0), m, {Pat(len, any)}, STAGE_DEFAULT, "wildcards");
                // zeros under classes that hold 0x00: table classes everywhere, then a masked equality
                bad |= run_case(std::vector<u8>(n, 0), m, {Pat(len, low), Pat(len, range(0, 7))}, STAGE_DEFAULT, "zeros");
                // two-letter noise: a case-pair prefix and a table class at the last position
                std::vector<u8> ab = noise(n, 3 * n + len, 2);
                Pat q;
                for (u32 k = 0; k < len; ++k) q.push_back(k < n ? of({ab[k], (u8)(ab[k] ^ 0x20)}) : of({'a', 'A'}));
                Pat q2 = q;
                q2.back() = of({'a', 'b', 'c'});
                bad |= run_case(ab, m, {q, q2}, STAGE_DEFAULT, "two letters");
                // random bytes with a digit pattern planted at 0, at n - len, across the tile
                // boundaries and across the lane boundaries; a pattern whose last class holds 0x00
                // while the data end one byte before it
                std::vector<u8> r = noise(n, 77 * m + len, 0), pat = noise(len, 1000 + len, 10);
                for (auto& b : pat) b = (u8)('0' + (b - 'a'));
                auto plant = [&](u64 o) {
                    if (o + len <= n) std::memcpy(r.data() + o, pat.data(), len);
                };
                plant(0);
                for (u32 k = 1; k < 9 && len < 64; ++k) plant(512 + k * 272 - k);
                plant(TILE - (len + 1) / 2);
                plant(2 * (u64)TILE - 1);
                if (n >= len) plant(n - len);
                Pat digits(len, digit), mixed(len, digit), trunc(len, digit);
                for (u32 k = 0; k < len; k += 3) mixed[k] = of({pat[k]});
                trunc.push_back(zero_or_z);
                std::vector<Pat> ps{digits, mixed};
                if (trunc.size() <= MAX_LEN) ps.push_back(trunc);
                bad |= run_case(r, m, ps, STAGE_DEFAULT, "planted");
            }
    // several emit launches: the least staging the kernels accept
    for (u32 m : {0u, 5u})
        bad |= run_case(std::vector<u8>(5 * TILE + 3, 0), m, {Pat(1, low), Pat(2, any)}, 1, "small stage");
    std::printf("findcls_emu: %llu cases %s\n", (unsigned long long)g_cases, bad ? "FAILED" : "ok");
    return bad;
}
#endif
