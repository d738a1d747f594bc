// CPU emulation of the regular-expression search kernels: the header k_findrx_count /
// k_findrx_emit of kolmogorovlike-datacompressor_amd/csrc/k_findrx.hip compile
// (csrc/findrx_core.h, over csrc/find_core.h), driven with the kernels' shape as
// tools/findcls_emu.cpp drives findcls_core.h — 4 KiB tiles, the tile's stage of class ids built
// word by word, 256 virtual threads with 16 positions each, the per-expression masks of a tile,
// the counts, the exclusive scan of the tile totals, the emit launches cut at scanned tile
// boundaries — behind a C interface for tests/test_findrx_core.py, and a main() that runs the
// sweeps on its own over heap buffers of exactly the aligned words the load contract allows and
// tables of exactly nstates x ncls entries (built with -fsanitize=address,undefined by the test:
// a load or a table index outside them is an error there).  Every load is recorded and checked
// against the contract: an aligned 16-byte word that holds a byte of [buf, buf + n).  The
// violations are counted.  What such a word holds outside [buf, buf + n) is 0x00 here.
//   g++ -O2 -std=c++17 -shared -fPIC tools/findrx_emu.cpp -o findrx_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/findrx_emu.cpp -o findrx_emu
//   ./findrx_emu     exit status 0 when every case matches the byte-by-byte reference
#include "../kolmogorovlike-datacompressor_amd/csrc/findrx_core.h"

#include "find_emu_common.h"  // Ld (the recording loader), tile_count / tile_emit, find_group, find_grouped, noise

#include <array>
#include <cstdio>
#include <utility>

using frx::u16;

namespace {

// a validated automaton: exactly its own entries on the heap
struct Dfa {
    std::vector<u8> cls;
    std::vector<u16> T, starts;
    u32 nstates, ncls, np, L;
};

struct Emu {
    typedef u8 Which;
    Ld ld;
    u32 lo, shi;
    const Dfa& D;
    u32 mis() const { return (u32)(reinterpret_cast<uintptr_t>(ld.buf) & (WORD - 1)); }
    u32 cols() const { return D.np; }
    u64 cap(u64 stage_bytes) const { return stage_records(stage_bytes, D.np); }

    // one workgroup: the stage, then pm[i][t] = thread t's mask of expression i
    void run_tile(u32 tile, u32 pm[MAX_PATTERNS][WG]) {
        std::vector<u8> stage(frx::STAGE_BYTES);  // on the heap: a read past it is an error under ASan
        for (u32 w = 0; w < frx::STAGE_WORDS; ++w) {
            u32 o[4];
            frx::stage_word(ld, mis(), tile, w, ld.n, D.cls.data(), o);
            std::memcpy(stage.data() + (size_t)w * WORD, o, WORD);
        }
        for (u32 t = 0; t < WG; ++t) {
            const u32 p0 = tile * TILE + t * PER;
            for (u32 i = 0; i < D.np; ++i)
                pm[i][t] = frx::match_mask(D.T.data(), D.ncls, stage.data() + mis() + t * PER, p0, lo, shi, ld.n, D.starts[i]);
        }
    }
    // k_findrx_count and k_findrx_emit
    void count(u32 ntiles, std::vector<u32>& cnt) { tile_count(*this, ntiles, cnt); }
    u64 emit(u32 t0, u32 t1, const u64* tscan, u32* pos, u8* which, u64 cap) {
        return tile_emit(*this, t0, t1, tscan, pos, which, cap);
    }
};

// the checks of the library (findrx_check in kolm_reader.cpp), the copies and the hold-back
bool prepare(const u8* cls, const u16* T, u32 nstates, u32 ncls, const u16* starts, u32 np, Dfa& D) {
    char why[200];
    if (frx::validate(cls, T, nstates, ncls, starts, np, why, sizeof why)) return false;
    D.cls.assign(cls, cls + frx::MAP);
    D.T.assign(T, T + (size_t)nstates * ncls);
    D.starts.assign(starts, starts + np);
    D.nstates = nstates, D.ncls = ncls, D.np = np;
    std::vector<u8> scratch(2 * (size_t)nstates);
    D.L = frx::hold_back(D.T.data(), nstates, ncls, starts, np, scratch.data());
    return true;
}

}  // namespace

// The search of buf [0, n) (any alignment; the aligned words around it must be readable) for
// matches that start in [lo, n).  The automaton as the C ABI takes it.  counts [np] exact; the
// first min(total, limit) matches to offs / which (cap entries; fewer are written when cap is
// smaller); nfound = their number; launches = emit launches.  Returns the number of contract
// violations; ~0 for an automaton the library refuses.
extern "C" uint64_t frx_emu_find(const uint8_t* buf, uint32_t n, uint32_t lo, const uint8_t* cls, const uint16_t* T,
                                 uint32_t nstates, uint32_t ncls, const uint16_t* starts, uint32_t np, uint64_t stage_bytes,
                                 uint64_t limit, uint64_t* counts, uint64_t* offs, uint8_t* which, uint64_t cap,
                                 uint64_t* nfound, uint32_t* launches) {
    Dfa D;
    if (!prepare(cls, T, nstates, ncls, starts, np, D)) return ~0ull;
    std::vector<u64> o;
    std::vector<u8> w;
    *launches = 0;
    for (u32 i = 0; i < np; ++i) counts[i] = 0;
    Emu e{Ld{buf, n}, lo, n, D};
    const u64 bad = find_group(e, 0, stage_bytes, limit, counts, o, w, launches);
    hand_out(o, w, offs, which, cap, nfound);
    return bad;
}

// The grouped search as the reader runs it (find_grouped).  The hold-back is the table's own
// (frx::hold_back); the rest of the aligned words around a scan buffer is 0x00.
extern "C" uint64_t frx_emu_find_grouped(const uint8_t* data, const uint64_t* bounds, uint32_t ng, uint64_t lo, uint64_t hi,
                                         const uint8_t* cls, const uint16_t* T, uint32_t nstates, uint32_t ncls,
                                         const uint16_t* starts, uint32_t np, uint64_t stage_bytes, uint64_t limit,
                                         uint64_t* counts, uint64_t* offs, uint8_t* which, uint64_t cap, uint64_t* nfound,
                                         uint32_t* launches) {
    Dfa D;
    if (!prepare(cls, T, nstates, ncls, starts, np, D)) return ~0ull;
    std::vector<u64> o;
    std::vector<u8> w;
    *launches = 0;
    for (u32 i = 0; i < np; ++i) counts[i] = 0;
    const u64 bad = find_grouped(data, bounds, ng, lo, hi, D.L, 0, stage_bytes, limit, counts, o, w, launches,
                                 [&](const u8* buf, u32 n, u32 glo, u32 shi) { return Emu{Ld{buf, n}, glo, shi, D}; });
    hand_out(o, w, offs, which, cap, nfound);
    return bad;
}

// frx::validate: 0 when the library accepts the automaton, else 1 and the reason in msg (cap bytes).
extern "C" uint32_t frx_emu_validate(const uint8_t* cls, const uint16_t* T, uint32_t nstates, uint32_t ncls,
                                     const uint16_t* starts, uint32_t np, char* msg, uint32_t cap) {
    if (cap) msg[0] = 0;
    return frx::validate(cls, T, nstates, ncls, starts, np, msg, cap) ? 1 : 0;
}

// frx::hold_back of an automaton the library accepts; 0 for one it refuses.
extern "C" uint32_t frx_emu_hold_back(const uint8_t* cls, const uint16_t* T, uint32_t nstates, uint32_t ncls,
                                      const uint16_t* starts, uint32_t np) {
    Dfa D;
    return prepare(cls, T, nstates, ncls, starts, np, D) ? D.L : 0;
}

extern "C" uint32_t frx_emu_tile_bytes(void) { return TILE; }
extern "C" uint32_t frx_emu_max_entries(void) { return frx::MAX_ENTRIES; }

namespace {

typedef std::vector<std::pair<u64, u8>> Hits;

// An expression of the sweeps: the classes head[0..], then any number of bytes of `loop` (none when
// loop is empty), then the byte `tail` when has_tail.  Its reference is the direct scan below.
typedef std::array<bool, 256> Cls;
struct Expr {
    std::vector<Cls> head;
    Cls loop{};
    bool looped = false, has_tail = false;
    u8 tail = 0;
};

bool ref_match(const std::vector<u8>& d, u64 o, const Expr& e) {
    const u64 end = std::min<u64>(d.size(), o + frx::MAX_WALK);
    u64 p = o;
    for (const Cls& c : e.head) {
        if (p >= end || !c[d[p]]) return false;
        ++p;
    }
    if (!e.has_tail) return true;  // the head alone accepts (a loop behind it changes no start)
    for (;;) {
        if (p >= end) return false;
        if (d[p] == e.tail) return true;  // the first accept ends the walk
        if (!e.looped || !e.loop[d[p]]) return false;
        ++p;
    }
}

Hits reference(const std::vector<u8>& d, const std::vector<Expr>& es) {
    Hits h;
    for (u64 o = 0; o < d.size(); ++o)
        for (size_t i = 0; i < es.size(); ++i)
            if (ref_match(d, o, es[i])) h.push_back({o, (u8)i});
    return h;
}

// The expressions as one automaton, built without a subset construction (these shapes are
// deterministic as they stand): bytes that every set of the call treats alike share a class, and
// every expression owns its states: head.size() chain states, one loop state when it has a tail.
struct Built {
    std::vector<u8> cls;
    std::vector<u16> T, starts;
    u32 nstates, ncls;
};

Built build(const std::vector<Expr>& es) {
    // classes: bytes with the same membership in every set of the call
    std::vector<std::vector<bool>> sigs;
    Built B;
    B.cls.assign(256, 0);
    for (u32 b = 0; b < 256; ++b) {
        std::vector<bool> s;
        for (const Expr& e : es) {
            for (const Cls& c : e.head) s.push_back(c[b]);
            s.push_back(e.looped && e.loop[b]);
            s.push_back(e.has_tail && b == e.tail);
        }
        size_t k = 0;
        while (k < sigs.size() && sigs[k] != s) ++k;
        if (k == sigs.size()) sigs.push_back(s);
        B.cls[b] = (u8)k;
    }
    B.ncls = (u32)sigs.size();
    std::vector<u32> rep(B.ncls);
    for (u32 b = 256; b-- > 0;) rep[B.cls[b]] = b;
    u32 ns = 2;
    for (const Expr& e : es) ns += (u32)e.head.size() + (e.has_tail ? 1 : 0);
    B.nstates = ns;
    B.T.assign((size_t)ns * B.ncls, 0);
    u32 s = 2;
    for (const Expr& e : es) {
        B.starts.push_back((u16)s);
        const u32 h = (u32)e.head.size();
        for (u32 k = 0; k < h; ++k)
            for (u32 c = 0; c < B.ncls; ++c)
                if (e.head[k][rep[c]]) B.T[(size_t)(s + k) * B.ncls + c] = (u16)(k + 1 < h || e.has_tail ? s + k + 1 : 1);
        if (e.has_tail)
            for (u32 c = 0; c < B.ncls; ++c)
                B.T[(size_t)(s + h) * B.ncls + c] = rep[c] == e.tail ? 1 : e.looped && e.loop[rep[c]] ? (u16)(s + h) : 0;
        s += h + (e.has_tail ? 1 : 0);
    }
    return B;
}

// data at misalignment m in a heap block of exactly the aligned words around it, zeros around the data
int run_case(const std::vector<u8>& d, u32 m, const std::vector<Expr>& es, u64 stage, const char* what) {
    const u32 n = (u32)d.size();
    u8* raw = aligned_block(d.data(), n, m, 0);
    const Built B = build(es);
    const Hits want = reference(d, es);
    std::vector<u64> counts(es.size()), offs(want.size() + 1);
    std::vector<u8> which(want.size() + 1);
    u64 nfound = 0;
    u32 launches = 0;
    const u64 bad = frx_emu_find(raw + m, n, 0, B.cls.data(), B.T.data(), B.nstates, B.ncls, B.starts.data(), (u32)es.size(),
                                 stage, ~0ull, counts.data(), offs.data(), which.data(), offs.size(), &nfound, &launches);
    int fail = bad != 0 || nfound != want.size();
    for (size_t k = 0; k < want.size() && !fail; ++k) fail = offs[k] != want[k].first || which[k] != want[k].second;
    if (fail)
        std::fprintf(stderr, "%s: n %u, misalignment %u, %zu expressions (%u states x %u classes): %llu violations, %llu found, %zu expected\n",
                     what, n, m, es.size(), B.nstates, B.ncls, (unsigned long long)bad, (unsigned long long)nfound, want.size());
    std::free(raw);
    ++g_cases;
    return fail;
}

Cls range(u32 a, u32 b) {
    Cls s{};
    for (u32 x = a; x <= b; ++x) s[x] = true;
    return s;
}

Expr chain(u32 len, const Cls& c) {
    Expr e;
    e.head.assign(len, c);
    return e;
}

Expr run(const Cls& first, const Cls& loop, u8 tail) {  // first loop* tail
    Expr e;
    e.head.push_back(first);
    e.loop = loop, e.looped = true, e.has_tail = true, e.tail = tail;
    return e;
}

}  // namespace

#ifndef FRX_EMU_NO_MAIN
int main() {
    int bad = 0;
    const u32 ns[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8193};
    const u32 lens[] = {1, 2, 16, 17, 255, 256, 257};
    const Cls any = range(0, 255), digit = range('0', '9'), low = range(0, 9), ab = range('a', 'b'), zero = range(0, 0);
    for (u32 m = 0; m < 16; ++m)
        for (u32 n : ns) {
            for (u32 len : lens) {
                // wildcards only: every start at which the witness fits; 257 bytes never do
                bad |= run_case(noise(n, n + len, 0), m, {chain(len, any)}, STAGE_DEFAULT, "wildcards");
                // zeros under classes that hold 0x00: what lies past n is zeros and decides nothing
                bad |= run_case(std::vector<u8>(n, 0), m, {chain(len, low), run(zero, zero, 0)}, STAGE_DEFAULT, "zeros");
            }
            // two-letter noise with runs: a b* c walks as far as the b's go, across lanes and tiles
            std::vector<u8> t = noise(n, 3 * n + m, 3);
            if (n > 600) std::fill(t.begin() + 100, t.begin() + 500, (u8)'b'), t[99] = 'a', t[380] = 'c';
            if (n > TILE + 200) std::fill(t.begin() + TILE - 200, t.begin() + TILE + 54, (u8)'b'), t[TILE - 201] = 'a', t[TILE + 54] = 'c';
            if (n > TILE + 200) t[TILE - 1] = 'a';  // a start in the tile's last byte
            bad |= run_case(t, m, {run(range('a', 'a'), range('b', 'b'), 'c'), run(ab, ab, 'c'), chain(2, ab)}, STAGE_DEFAULT, "runs");
            // digits planted in random bytes: at 0, at the end, across tile and lane boundaries
            std::vector<u8> r = noise(n, 77 * m + n, 0);
            for (u64 o : {(u64)0, (u64)TILE - 3, (u64)2 * TILE - 1, (u64)n - std::min<u64>(n, 5), (u64)777})
                for (u32 k = 0; k < 5 && o + k < n; ++k) r[o + k] = (u8)('0' + k);
            bad |= run_case(r, m, {chain(3, digit), run(digit, digit, '4'), chain(1, digit)}, STAGE_DEFAULT, "planted");
        }
    // 16 expressions at once; several emit launches: the least staging the kernels accept
    std::vector<Expr> sixteen;
    for (u32 i = 0; i < 16; ++i) sixteen.push_back(i & 1 ? chain(1 + i, ab) : run(range('a' + i % 3, 'a' + i % 3), ab, (u8)('a' + i % 2)));
    for (u32 m : {0u, 5u}) {
        bad |= run_case(noise(8193, m, 3), m, sixteen, STAGE_DEFAULT, "sixteen");
        bad |= run_case(std::vector<u8>(5 * TILE + 3, 0), m, {chain(1, low), chain(2, any)}, 1, "small stage");
    }
    std::printf("findrx_emu: %llu cases %s\n", (unsigned long long)g_cases, bad ? "FAILED" : "ok");
    return bad;
}
#endif
