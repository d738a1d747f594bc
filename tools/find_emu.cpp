// CPU emulation of the search kernels: the header k_find_count / k_find_emit of
// kolmogorovlike-datacompressor_amd/csrc/k_find.hip compile (csrc/find_core.h), driven with the
// kernels' shape — 4 KiB tiles, 256 virtual threads with 16 positions each, the per-pattern masks
// of a tile, the per-pattern and per-tile counts, the exclusive scan of the tile totals, the emit
// launches cut at scanned tile boundaries so that each fits the staging arrays — behind a C
// interface for tests/test_find_core.py, and a main() that runs the sweeps on its own over heap
// buffers of exactly the aligned words the load contract allows (built with
// -fsanitize=address,undefined by the test: a load outside them is an error there).  Every load
// is recorded and checked against the contract: an aligned 16-byte word that holds a byte of
// [buf, buf + n).  The violations are counted.
//   g++ -O2 -std=c++17 -shared -fPIC tools/find_emu.cpp -o find_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/find_emu.cpp -o find_emu
//   ./find_emu        exit status 0 when every case matches the byte-by-byte reference
#include "find_emu_common.h"  // Ld (the recording loader), tile_count / tile_emit, find_group, find_grouped, noise

#include <cstdio>
#include <utility>

namespace {

struct Emu {
    typedef u8 Which;
    Ld ld;
    u32 lo, shi;
    const Pats& P;
    u32 np;
    u32 mis() const { return (u32)(reinterpret_cast<uintptr_t>(ld.buf) & (WORD - 1)); }
    u32 cols() const { return np; }
    u64 cap(u64 stage_bytes) const { return stage_records(stage_bytes, np); }

    // one workgroup: pm[i][t] = thread t's mask of pattern i
    void run_tile(u32 tile, u32 pm[MAX_PATTERNS][WG]) {
        for (u32 t = 0; t < WG; ++t) {
            const u32 p0 = tile * TILE + t * PER;
            u64 w[PER];
            windows(ld, mis(), p0, ld.n, w);
            for (u32 i = 0; i < np; ++i)
                pm[i][t] = match_mask(ld, w, mis(), p0, lo, shi, ld.n, P.pre[i], P.mask[i], P.len[i], P.pat[i]);
        }
    }
    // k_find_count and k_find_emit
    void count(u32 ntiles, std::vector<u32>& cnt) { tile_count(*this, ntiles, cnt); }
    u64 emit(u32 t0, u32 t1, const u64* tscan, u32* pos, u8* which, u64 cap) {
        return tile_emit(*this, t0, t1, tscan, pos, which, cap);
    }
};

bool pats_ok(const u32* pat_off, u32 np) {
    if (np < 1 || np > MAX_PATTERNS) return false;
    for (u32 i = 0; i < np; ++i)
        if (pat_off[i + 1] <= pat_off[i] || pat_off[i + 1] - pat_off[i] > MAX_LEN) return false;
    return true;
}

}  // namespace

// The search of buf [0, n) (any alignment; the aligned words around it must be readable) for
// matches that start in [lo, n).  counts [np] exact; the first min(total, limit) matches to
// offs / which (cap entries; fewer are written when cap is smaller); nfound = their number;
// launches = emit launches.  Returns the number of contract violations; ~0 for bad arguments.
extern "C" uint64_t fnd_emu_find(const uint8_t* buf, uint32_t n, uint32_t lo, const uint8_t* pats, const uint32_t* pat_off,
                                 uint32_t np, uint64_t stage_bytes, uint64_t limit, uint64_t* counts, uint64_t* offs,
                                 uint8_t* which, uint64_t cap, uint64_t* nfound, uint32_t* launches) {
    if (!pats_ok(pat_off, np)) return ~0ull;
    Pats P;
    make_pats(pats, pat_off, np, P);
    std::vector<u64> o;
    std::vector<u8> w;
    *launches = 0;
    for (u32 i = 0; i < np; ++i) counts[i] = 0;
    Emu e{Ld{buf, n}, lo, n, P, np};
    const u64 bad = find_group(e, 0, stage_bytes, limit, counts, o, w, launches);
    hand_out(o, w, offs, which, cap, nfound);
    return bad;
}

// The hold-back over synthetic groups: group g covers stream bytes [bounds[g], bounds[g + 1]).
// S [ng + 1] receives S_0 = lo .. S_ng = hi; carry [ng] the bytes in front of each group's own.
extern "C" void fnd_emu_groups(const uint64_t* bounds, uint32_t ng, uint64_t lo, uint64_t hi, uint32_t L, uint64_t* S,
                               uint32_t* carry) {
    S[0] = lo;
    for (u32 g = 0; g < ng; ++g) {
        const GroupScan gs = group_scan(S[g], bounds[g], bounds[g + 1], L, g + 1 == ng, hi);
        S[g + 1] = gs.S_next;
        carry[g] = gs.carry;
    }
}

// The grouped search as the reader runs it (find_grouped), the aligned words around a scan buffer
// filled with 0xEE.
extern "C" uint64_t fnd_emu_find_grouped(const uint8_t* data, const uint64_t* bounds, uint32_t ng, uint64_t lo, uint64_t hi,
                                         const uint8_t* pats, const uint32_t* pat_off, uint32_t np, uint64_t stage_bytes,
                                         uint64_t limit, uint64_t* counts, uint64_t* offs, uint8_t* which, uint64_t cap,
                                         uint64_t* nfound, uint32_t* launches) {
    if (!pats_ok(pat_off, np)) return ~0ull;
    Pats P;
    make_pats(pats, pat_off, np, P);
    u32 L = 0;
    for (u32 i = 0; i < np; ++i) L = std::max(L, P.len[i]);
    std::vector<u64> o;
    std::vector<u8> w;
    *launches = 0;
    for (u32 i = 0; i < np; ++i) counts[i] = 0;
    const u64 bad = find_grouped(data, bounds, ng, lo, hi, L, 0xEE, stage_bytes, limit, counts, o, w, launches,
                                 [&](const u8* buf, u32 n, u32 glo, u32 shi) { return Emu{Ld{buf, n}, glo, shi, P, np}; });
    hand_out(o, w, offs, which, cap, nfound);
    return bad;
}

extern "C" uint32_t fnd_emu_tile_bytes(void) { return TILE; }

namespace {

typedef std::vector<std::pair<u64, u8>> Hits;

Hits reference(const std::vector<u8>& d, u64 lo, u64 hi, const std::vector<std::vector<u8>>& pats) {
    Hits h;
    for (u64 o = lo; o < hi; ++o)
        for (size_t i = 0; i < pats.size(); ++i)
            if (o + pats[i].size() <= hi && std::memcmp(d.data() + o, pats[i].data(), pats[i].size()) == 0)
                h.push_back({o, (u8)i});
    return h;
}

// data at misalignment m in a heap block of exactly the aligned words around it
int run_case(const std::vector<u8>& d, u32 m, const std::vector<std::vector<u8>>& pats, u64 stage, const char* what) {
    const u32 n = (u32)d.size();
    u8* raw = aligned_block(d.data(), n, m, 0xEE);
    std::vector<u8> flat;
    std::vector<u32> off{0};
    for (auto& p : pats) flat.insert(flat.end(), p.begin(), p.end()), off.push_back((u32)flat.size());
    const Hits want = reference(d, 0, n, pats);
    std::vector<u64> counts(pats.size()), offs(want.size() + 1);
    std::vector<u8> which(want.size() + 1);
    u64 nfound = 0;
    u32 launches = 0;
    const u64 bad = fnd_emu_find(raw + m, n, 0, flat.data(), off.data(), (u32)pats.size(), stage, ~0ull, counts.data(),
                                 offs.data(), which.data(), offs.size(), &nfound, &launches);
    int fail = bad != 0 || nfound != want.size();
    for (size_t k = 0; k < want.size() && !fail; ++k) fail = offs[k] != want[k].first || which[k] != want[k].second;
    if (fail)
        std::fprintf(stderr, "%s: n %u, misalignment %u, %zu patterns (first of %zu bytes): %llu violations, %llu found, %zu expected\n",
                     what, n, m, pats.size(), pats[0].size(), (unsigned long long)bad, (unsigned long long)nfound, want.size());
    std::free(raw);
    ++g_cases;
    return fail;
}

}  // namespace

#ifndef FND_EMU_NO_MAIN
int main() {
    int bad = 0;
    const u32 ns[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8193};
    const u32 lens[] = {1, 2, 3, 7, 8, 9, 15, 16, 17, 255, 256};
    for (u32 m = 0; m < 16; ++m)
        for (u32 n : ns)
            for (u32 len : lens) {
                // zeros: every position a match; period 3; two-letter noise
                bad |= run_case(std::vector<u8>(n, 0), m, {std::vector<u8>(len, 0)}, STAGE_DEFAULT, "zeros");
                std::vector<u8> abc(n), p(len);
                for (u32 i = 0; i < n; ++i) abc[i] = (u8)("abc"[i % 3]);
                for (u32 i = 0; i < len; ++i) p[i] = (u8)("abc"[(i + 1) % 3]);
                bad |= run_case(abc, m, {p}, STAGE_DEFAULT, "abc");
                std::vector<u8> ab = noise(n, n + len, 2);
                std::vector<u8> q(ab.begin(), ab.begin() + std::min<u32>(len, n));
                q.resize(len, 'a');
                bad |= run_case(ab, m, {q, std::vector<u8>(std::min<u32>(len, 3), 'a')}, STAGE_DEFAULT, "two letters");
                // random bytes with the pattern planted at 0, at n - len, across the tile boundary
                // and across every lane boundary of one stretch; its prefix alone at the very end
                std::vector<u8> r = noise(n, 77 * m + len, 0), pat = noise(len, 1000 + len, 0);
                auto plant = [&](u64 o) {
                    if (o + len <= n) std::memcpy(r.data() + o, pat.data(), len);
                };
                plant(0);
                for (u32 k = 1; k < 9 && len < 64; ++k) plant(512 + k * 272 - k);
                plant(TILE - (len + 1) / 2);
                plant(2 * (u64)TILE - 1);
                if (n >= len) plant(n - len);
                std::vector<u8> trunc = pat;  // the pattern with a different last byte: its prefix ends the buffer
                trunc.push_back((u8)(pat.back() ^ 0x55));
                if (trunc.size() <= MAX_LEN) bad |= run_case(r, m, {pat, trunc}, STAGE_DEFAULT, "planted");
                else bad |= run_case(r, m, {pat}, STAGE_DEFAULT, "planted");
            }
    // several emit launches: the least staging the kernels accept
    for (u32 m : {0u, 5u})
        bad |= run_case(std::vector<u8>(5 * TILE + 3, 0), m, {std::vector<u8>(1, 0), std::vector<u8>(2, 0)}, 1, "small stage");
    std::printf("find_emu: %llu cases %s\n", (unsigned long long)g_cases, bad ? "FAILED" : "ok");
    return bad;
}
#endif
