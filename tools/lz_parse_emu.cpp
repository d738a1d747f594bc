// CPU emulation of the LZ77 decoder's token parse: the header k_dec_lz_parse of
// kolmogorovlike-datacompressor_amd/csrc/k_decode.hip compiles (csrc/lz_parse_core.h), driven
// the way the kernel drives it — a batch of blocks, block b owning the token slots
// [obase[b], obase[b] + n_b) of two arrays shared by the whole batch — behind a C interface
// for tests/test_lz_parse_core.py, and a main() that runs a sweep on its own (built with
// -fsanitize=address,undefined by the test).
//
// The slot arrays hold exactly `total` entries between poisoned guard words.  A block's parse
// must leave everything outside that block's own slots unchanged (a write into a neighbour's
// slots or into a guard is the overrun this guards against), t <= n, and the record positions
// strictly increase from 0.  The records are then resolved serially to bytes
// (a copy reads the output dist bytes back), so the result can be compared with a decoder that
// never builds records.
//   g++ -O2 -std=c++17 -shared -fPIC tools/lz_parse_emu.cpp -o lz_parse_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/lz_parse_emu.cpp -o lz_parse_emu
//   ./lz_parse_emu [cases.txt]   exit status 0 when every case matches the serial reference
//                                decoder below; cases.txt: one "n payload-hex|-" per line
#include "../kolmogorovlike-datacompressor_amd/csrc/lz_parse_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using lzp::u32;
using lzp::u8;
typedef uint64_t u64;

namespace {

constexpr u32 POISON = 0xDEADBEEFu;
constexpr u32 GUARD = 16;  // guard words on each side of the slot arrays
constexpr u32 NEAR = 64;   // words after a block checked right after its parse

enum : u32 { V_OUTSIDE = 1, V_COUNT = 2, V_ORDER = 4, V_STATUS = 8 };

}  // namespace

// Decodes nb blocks: payload b = pay[poff[b], poff[b + 1]), lens[b] output bytes at
// out[sum of lens before b].  status[b] = lzp::OK / ELEN / EFORMAT, ntok[b] = records.
// Returns 0, or the V_* violations of the parse's contract.
extern "C" uint32_t lzp_emu_decode(const uint8_t* pay, const uint64_t* poff, const uint32_t* lens, uint32_t nb,
                                   uint8_t* out, uint32_t* status, uint32_t* ntok) {
    u64 total = 0;
    for (u32 b = 0; b < nb; ++b) total += lens[b];
    const u64 words = total + 2 * GUARD;
    u32* tp = (u32*)std::malloc(words * sizeof(u32));
    u32* tv = (u32*)std::malloc(words * sizeof(u32));
    std::vector<u32> sp(words, POISON), sv(words, POISON);  // what the arrays must hold outside the block
    for (u64 i = 0; i < words; ++i) tp[i] = tv[i] = POISON;
    u32* tpos = tp + GUARD;
    u32* tval = tv + GUARD;
    u32 viol = 0;
    u64 o0 = 0;
    for (u32 b = 0; b < nb; ++b) {
        const u32 n = lens[b];
        const u32 plen = (u32)(poff[b + 1] - poff[b]);
        // the payload in a buffer of exactly plen bytes: a read past it is the sanitizer's
        u8* p = (u8*)std::malloc(plen ? plen : 1);
        if (plen) std::memcpy(p, pay + poff[b], plen);
        u32 nt = 0;
        const u32 err = lzp::parse(p, plen, n, tpos + o0, tval + o0, &nt);
        std::free(p);
        status[b] = err;
        ntok[b] = nt;
        // unchanged outside the block's own slots: the words just before and after it (where an
        // overrun lands) now, every word of the batch once more at the end; the block's own slots
        // past its records stay untouched when it parses cleanly
        const u64 own0 = GUARD + o0, own1 = own0 + n;
        for (u64 i = own0 - GUARD; i < own0; ++i)
            if (tp[i] != sp[i] || tv[i] != sv[i]) viol |= V_OUTSIDE;
        for (u64 i = own1; i < own1 + NEAR && i < words; ++i)
            if (tp[i] != sp[i] || tv[i] != sv[i]) viol |= V_OUTSIDE;
        for (u64 i = own0; i < own1; ++i) {
            if (err == lzp::OK && i >= own0 + nt && (tp[i] != POISON || tv[i] != POISON)) viol |= V_OUTSIDE;
            sp[i] = tp[i];
            sv[i] = tv[i];
        }
        if (nt > n) viol |= V_COUNT;
        if (err != lzp::OK && err != lzp::ELEN && err != lzp::EFORMAT) viol |= V_STATUS;
        if (err == lzp::OK) {
            if (n && (nt == 0 || tpos[o0] != 0)) viol |= V_ORDER;
            for (u32 t = 0; t < nt && t < n; ++t) {
                const u32 lo = tpos[o0 + t], hi = t + 1 < nt ? tpos[o0 + t + 1] : n;
                if (lo >= hi || hi > n) {
                    viol |= V_ORDER;
                    break;
                }
                const u32 v = tval[o0 + t];
                for (u32 o = lo; o < hi; ++o) {
                    if (v & lzp::LIT) {
                        out[o0 + o] = (u8)v;
                    } else if (v == 0 || v > o) {
                        viol |= V_ORDER;  // a distance the parse should have rejected
                        break;
                    } else {
                        out[o0 + o] = out[o0 + o - v];
                    }
                }
                if ((v & lzp::LIT) && hi != lo + 1) viol |= V_ORDER;
            }
        } else if (nt != 0) {
            viol |= V_COUNT;
        }
        o0 += n;
    }
    for (u64 i = 0; i < words; ++i)
        if (tp[i] != sp[i] || tv[i] != sv[i]) viol |= V_OUTSIDE;
    std::free(tp);
    std::free(tv);
    return viol;
}

namespace {

// The decoder the parse must agree with, restated serially without records (kolm/decode.py
// decode_lz77: PY:1765-1812 with the distance checked once per copy, zero-length ones included).
bool ref_uleb(const std::vector<u8>& d, size_t& i, u64& v) {
    v = 0;  // saturating at 2^64 - 1: far past every length and distance that matters
    for (u32 sh = 0;;) {
        if (i >= d.size()) return false;
        const u8 b = d[i++];
        const u64 g = b & 0x7F;
        if (sh >= 64) {
            if (g) v = ~0ull;
        } else {
            if (sh > 57 && (g >> (64 - sh))) v = ~0ull;
            else v |= g << sh;
            sh += 7;
        }
        if (!(b & 0x80)) return true;
    }
}

bool ref_decode(const std::vector<u8>& d, u32 n, std::vector<u8>& out) {
    out.clear();
    size_t i = 0;
    while (i < d.size() && out.size() < n) {
        const u8 flag = d[i++];
        if (flag == 0) {
            if (i >= d.size()) return false;
            out.push_back(d[i++]);
        } else if (flag == 1) {
            u64 len, dist;
            if (!ref_uleb(d, i, len) || !ref_uleb(d, i, dist)) return false;
            if (dist == 0 || dist > out.size() || dist > 4096) return false;
            const size_t start = out.size() - dist;
            const u64 room = n - out.size(), cnt = len < room ? len : room;
            for (u64 t = 0; t < cnt; ++t) out.push_back(out[start + t]);
        } else {
            return false;
        }
    }
    return out.size() == n;
}

struct Case {
    u32 n;
    std::vector<u8> pay;
};

// one batch through the emulator against ref_decode; prints the first disagreement
int run_batch(const std::vector<Case>& cs, const char* what) {
    std::vector<u8> arena;
    std::vector<u64> poff{0};
    std::vector<u32> lens;
    u64 total = 0;
    for (const Case& c : cs) {
        arena.insert(arena.end(), c.pay.begin(), c.pay.end());
        poff.push_back(arena.size());
        lens.push_back(c.n);
        total += c.n;
    }
    u8* out = (u8*)std::malloc(total ? total : 1);  // exactly total bytes
    std::memset(out, 0xA5, total ? total : 1);
    std::vector<u32> st(cs.size() + 1), nt(cs.size() + 1);
    const u32 viol = lzp_emu_decode(arena.data(), poff.data(), lens.data(), (u32)cs.size(), out, st.data(), nt.data());
    int bad = 0;
    if (viol) {
        std::fprintf(stderr, "%s: contract violations %u\n", what, viol);
        bad = 1;
    }
    u64 o0 = 0;
    std::vector<u8> want;
    for (size_t b = 0; b < cs.size(); ++b) {
        const bool ok = ref_decode(cs[b].pay, cs[b].n, want);
        const bool same = ok == (st[b] == lzp::OK) && (!ok || cs[b].n == 0 || std::memcmp(out + o0, want.data(), cs[b].n) == 0);
        if (!same && !bad) {
            std::fprintf(stderr, "%s: block %zu (n %u, %zu payload bytes): status %u, reference %s\n", what, b,
                         cs[b].n, cs[b].pay.size(), st[b], ok ? "decodes" : "rejects");
            bad = 1;
        }
        o0 += cs[b].n;
    }
    std::free(out);
    return bad;
}

void uleb_put(std::vector<u8>& v, u64 x) {
    do {
        v.push_back((u8)((x & 0x7F) | (x >> 7 ? 0x80 : 0)));
        x >>= 7;
    } while (x);
}

}  // namespace

#ifndef LZP_EMU_NO_MAIN
int main(int argc, char** argv) {
    int bad = 0;
    u64 cases = 0;
    // every token string of up to 4 tokens over {literal, copy len 0/1/2/5 x dist 1/2/7} at
    // n = 0..6 (7 exceeds every output position here), each n as one batch: a block that
    // writes past its slots lands in its neighbour's
    for (u32 n = 0; n <= 6; ++n) {
        std::vector<Case> cs;
        for (u32 k = 0; k <= 4; ++k) {
            u32 cnt = 1;
            for (u32 i = 0; i < k; ++i) cnt *= 13;
            for (u32 code = 0; code < cnt; ++code) {
                Case c{n, {}};
                u32 x = code;
                for (u32 i = 0; i < k; ++i, x /= 13) {
                    const u32 tk = x % 13;
                    if (tk == 0) {
                        c.pay.push_back(0);
                        c.pay.push_back((u8)('A' + i));
                    } else {
                        static const u32 lens[] = {0, 1, 2, 5}, dists[] = {1, 2, 7};
                        c.pay.push_back(1);
                        uleb_put(c.pay, lens[(tk - 1) / 3]);
                        uleb_put(c.pay, dists[(tk - 1) % 3]);
                    }
                }
                cs.push_back(c);
            }
        }
        cases += cs.size();
        bad |= run_batch(cs, "sweep");
    }
    // many zero-length copies in small blocks (more tokens than output bytes), wide and
    // overlong ULEB values, the last block of the batch included
    {
        std::vector<Case> cs;
        for (u32 rep : {1u, 3u, 50u, 5000u}) {
            Case c{2, {0, 'A'}};
            for (u32 i = 0; i < rep; ++i) c.pay.insert(c.pay.end(), {1, 0, 1});
            c.pay.insert(c.pay.end(), {0, 'B'});
            cs.push_back(c);
            cs.push_back(Case{3, {0, 'x', 0, 'y', 0, 'z'}});
        }
        cs.push_back(Case{9, {0, 'A', 1, 0x80, 0x80, 0x80, 0x80, 0x10, 1}});        // length 2^32
        cs.push_back(Case{4, {0, 'A', 1, 0x83, 0x80, 0x80, 0x80, 0x80, 0x00, 1}});  // 6-byte overlong 3
        cs.push_back(Case{4, {0, 'A', 1, 3, 0x81, 0x80, 0x80, 0x80, 0x80, 0x00}});  // 6-byte overlong distance
        cs.push_back(Case{4, {0, 'A', 1, 3, 0x81, 0x80, 0x80, 0x80, 0x80, 0x01}});  // distance 2^35 + 1
        cs.push_back(Case{4, {0, 'A', 1, 3, 0x81, 0x80, 0x80}});                    // truncated ULEB
        Case z{2, {0, 'A'}};
        for (u32 i = 0; i < 50; ++i) z.pay.insert(z.pay.end(), {1, 0, 1});
        z.pay.insert(z.pay.end(), {0, 'B'});
        cs.push_back(z);  // last block: an overrun would leave the arrays
        cases += cs.size();
        bad |= run_batch(cs, "zero-length copies");
    }
    if (argc > 1) {
        std::FILE* f = std::fopen(argv[1], "r");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        std::vector<Case> cs;
        char* line = nullptr;
        size_t cap = 0;
        while (getline(&line, &cap, f) > 0) {
            char* end;
            Case c{(u32)std::strtoul(line, &end, 10), {}};
            while (*end == ' ') ++end;
            for (; end[0] && end[1] && end[0] != '-' && end[0] != '\n'; end += 2) {
                const char h[3] = {end[0], end[1], 0};
                c.pay.push_back((u8)std::strtoul(h, nullptr, 16));
            }
            cs.push_back(c);
        }
        std::free(line);
        std::fclose(f);
        bad |= run_batch(cs, "file, one batch");
        for (const Case& c : cs) bad |= run_batch({c}, "file, alone");
        cases += cs.size();
    }
    std::printf("lz_parse_emu: %llu cases %s\n", (unsigned long long)cases, bad ? "FAILED" : "ok");
    return bad;
}
#endif
