// CPU emulation of the fast Lyndon route (kolmogorovlike-datacompressor_amd/csrc/lyndon_core.h):
// the same core functions the kernels of k_blocks.hip call, walked serially in the kernels' own
// structure (tiles of 256 lanes, per-block exclusive prefix-min of the tile minima, live tiles
// only, unordered append, rank sort, Hillis-Steele min-scan, compaction).  Every text load is
// recorded: an index outside the block's [base, end), a dword load at an address that is not
// 4-byte aligned or a 16-byte load that is not 16-byte aligned counts as a violation.
//
// Library (tests/test_lyndon_core.py, via ctypes): lyn_emu_block, lyn_emu_cands, lyn_emu_consts.
// Stand-alone (its own main; builds with -fsanitize=address,undefined):
//   lyn_emu                 self-test: exhaustive small strings and random strings against a
//                           textbook Duval, on heap buffers of exactly the block's size
//   lyn_emu FILE BS [NB]    per-block candidate / comparison / LCP figures of FILE in blocks of BS
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../kolmogorovlike-datacompressor_amd/csrc/lyndon_core.h"

using lyn::u32;
using lyn::u64;
using lyn::u8;

namespace {

struct Reader {
    const u8* t;  // text[0]
    u32 lo, hi;   // the block the loads serve
    u32 am;       // address of text[0] modulo 16 (virtual: the host reads by memcpy)
    mutable u64 bad = 0, loads = 0;
    void touch(u32 i, u32 n, u32 align) const {
        ++loads;
        if (i < lo || i > hi || hi - i < n) ++bad;
        if ((am + i) % align) ++bad;
    }
    bool ok(u32 i, u32 n) const { return i >= lo && i <= hi && hi - i >= n; }
    u32 amod() const { return am; }
    u32 b(u32 i) const {
        touch(i, 1, 1);
        return ok(i, 1) ? t[i] : 0u;
    }
    u32 d(u32 i) const {
        touch(i, 4, 4);
        u32 v = 0;
        if (ok(i, 4)) memcpy(&v, t + i, 4);
        return v;
    }
    void q(u32 i, u32 e[4]) const {
        touch(i, 16, 16);
        if (ok(i, 16)) memcpy(e, t + i, 16);
        else e[0] = e[1] = e[2] = e[3] = 0;
    }
};

struct Info {
    u32 ncand, live_tiles, ncmp, max_lcp;
    u64 lcp_sum, bad, loads;
};

// The candidate list of the block as k_lyn_min / k_lyn_scan / k_lyn_cand produce it (tile order
// forward or reversed: the kernel's append is unordered).  Returns the route so far; cand holds
// min(count, cap) entries, count the candidates counted.
u32 candidates(const Reader& rd, u32 base, u32 end, u32 cap, u32 order, std::vector<u32>& cand, u32& count,
               u32& live) {
    const u32 ntile = (end - base + lyn::TILE - 1) / lyn::TILE;
    std::vector<u64> tmin(ntile), tin(ntile);
    for (u32 k = 0; k < ntile; ++k) {  // k_lyn_min
        u64 m = lyn::W_MAX;
        for (u32 tid = 0; tid < lyn::THREADS; ++tid) {
            const u32 p = base + k * lyn::TILE + tid * lyn::PER;
            if (p >= end) continue;
            u32 E[6];
            lyn::load24(rd, p, base, end, E);
            m = lyn::min64(m, lyn::lane_min(E, std::min(lyn::PER, end - p)));
        }
        tmin[k] = m;
    }
    u64 run = lyn::W_MAX;
    for (u32 k = 0; k < ntile; ++k) {  // k_lyn_scan
        tin[k] = run;
        run = lyn::min64(run, tmin[k]);
    }
    u32 route = lyn::ACCEPT;
    count = 0;
    live = 0;
    cand.assign(cap, 0xFFFFFFFFu);
    for (u32 kk = 0; kk < ntile; ++kk) {  // k_lyn_cand
        const u32 k = order ? ntile - 1 - kk : kk;
        if (tmin[k] > tin[k]) continue;
        ++live;
        u64 r = tin[k];
        u32 total = 0;
        std::vector<u32> found;
        for (u32 tid = 0; tid < lyn::THREADS; ++tid) {
            const u32 p = base + k * lyn::TILE + tid * lyn::PER;
            if (p >= end) continue;
            const u32 n = std::min(lyn::PER, end - p);
            u32 E[6];
            lyn::load24(rd, p, base, end, E);
            const u32 mask = lyn::lane_cands(E, n, r);
            r = lyn::min64(r, lyn::lane_min(E, n));
            for (u32 i = 0; i < lyn::PER; ++i)
                if (mask >> i & 1) found.push_back(p + i);
            total += (u32)__builtin_popcount(mask);
        }
        const u32 g = count;
        count += total;
        if (g + total > cap) route = lyn::FALLBACK;
        for (u32 j = 0; j < total; ++j)
            if (g + j < cap) cand[g + j] = found[j];
    }
    return route;
}

}  // namespace

extern "C" {

void lyn_emu_consts(u32* out) {
    out[0] = lyn::TILE;
    out[1] = lyn::CAND_MAX;
    out[2] = lyn::LCP_MAX;
}

// Candidates of block [base, end) of text in position order -> out (at most room); returns the
// count, or -1 after a load violation.
long long lyn_emu_cands(const u8* text, u32 base, u32 end, u32 amod, u32* out, u32 room) {
    Reader rd{text, base, end, amod & 15u};
    std::vector<u32> cand;
    u32 count = 0, live = 0;
    candidates(rd, base, end, end - base, 1, cand, count, live);
    if (rd.bad) return -1;
    std::sort(cand.begin(), cand.begin() + count);
    for (u32 i = 0; i < count && i < room; ++i) out[i] = cand[i];
    return count;
}

// The fast route on block [base, end).  Accepted (returns 0): the factor starts (absolute
// positions, increasing) -> starts[0 .. *nstarts), flag[p] = 1 at every start (flag is indexed
// like the text).  Fallback (returns 1): starts, nstarts and flag are left untouched.  info (may be
// null) receives the figures either way; info->bad counts the load violations.
int lyn_emu_block(const u8* text, u32 base, u32 end, u32 amod, u32 cap, u32 lcp_cap, u32 order, u32* starts,
                  u32* nstarts, u8* flag, Info* info) {
    Reader rd{text, base, end, amod & 15u};
    Info inf{};
    std::vector<u32> cand;
    u32 count = 0, live = 0;
    cap = std::max(1u, std::min(cap, lyn::CAND_MAX));
    u32 route = candidates(rd, base, end, cap, order, cand, count, live);
    inf.ncand = count;
    inf.live_tiles = live;
    if (count > cap) route = lyn::FALLBACK;
    std::vector<u32> S, A, B;
    if (route == lyn::ACCEPT) {  // k_lyn_resolve
        const u32 n = count;
        S.assign(n, 0);
        for (u32 i = 0; i < n; ++i) {  // rank sort by position
            u32 r = 0;
            for (u32 j = 0; j < n; ++j) r += cand[j] < cand[i];
            S[r] = cand[i];
        }
        A = S;
        B.assign(n, 0);
        bool fb = false;
        for (u32 d = 1; d < n; d <<= 1) {
            for (u32 i = 0; i < n; ++i) {
                u32 lcp;
                bool over;
                B[i] = lyn::scan_step(rd, A.data(), i, d, base, end, lcp_cap, lcp, over);
                if (i >= d && A[i] != A[i - d]) {
                    ++inf.ncmp;
                    inf.lcp_sum += lcp;
                    inf.max_lcp = std::max(inf.max_lcp, lcp);
                }
                fb |= over;
            }
            A.swap(B);
        }
        if (fb) route = lyn::FALLBACK;
    }
    inf.bad = rd.bad;
    inf.loads = rd.loads;
    if (info) *info = inf;
    if (route == lyn::ACCEPT) {
        u32 m = 0;
        for (u32 i = 0; i < count; ++i)
            if (A[i] == S[i]) {
                starts[m++] = S[i];
                flag[S[i]] = 1;
            }
        *nstarts = m;
    }
    return (int)route;
}

}  // extern "C"

namespace {

std::vector<u32> duval(const u8* s, u32 n) {  // textbook Duval: factor starts
    std::vector<u32> out;
    u32 i = 0;
    while (i < n) {
        u32 j = i + 1, k = i;
        while (j < n && s[k] <= s[j]) {
            k = s[k] < s[j] ? i : k + 1;
            ++j;
        }
        while (i <= k) {
            out.push_back(i);
            i += j - k;
        }
    }
    return out;
}

u64 g_checked = 0;

// one string as a block of its own at offset `base` of a heap buffer of exactly base + n bytes
bool check(const std::vector<u8>& s, u32 base, u32 amod, u32 order) {
    const u32 n = (u32)s.size();
    u8* buf = (u8*)malloc(base + n);
    memset(buf, 0xEE, base);
    memcpy(buf + base, s.data(), n);
    std::vector<u32> st(n + 1);
    std::vector<u8> fl(base + n, 0);
    u32 ns = 0;
    Info inf{};
    const int r = lyn_emu_block(buf, base, base + n, amod, lyn::CAND_MAX, lyn::LCP_LIMIT, order, st.data(), &ns,
                                fl.data(), &inf);
    bool ok = inf.bad == 0;
    if (r == 0) {
        const std::vector<u32> want = duval(s.data(), n);
        ok = ok && ns == want.size();
        for (u32 i = 0; ok && i < ns; ++i) ok = st[i] == base + want[i];
    } else {
        ok = ok && inf.ncand > lyn::CAND_MAX;
    }
    free(buf);
    ++g_checked;
    if (!ok) {
        fprintf(stderr, "lyn_emu: mismatch (n %u base %u amod %u order %u route %d bad %llu):", n, base, amod, order, r,
                (unsigned long long)inf.bad);
        for (u32 i = 0; i < n && i < 40; ++i) fprintf(stderr, " %u", s[i]);
        fprintf(stderr, "\n");
    }
    return ok;
}

int self_test() {
    bool ok = true;
    for (u32 alpha = 2; alpha <= 3; ++alpha) {
        const u32 maxn = alpha == 2 ? 12 : 8;
        for (u32 n = 1; n <= maxn; ++n) {
            u64 total = 1;
            for (u32 i = 0; i < n; ++i) total *= alpha;
            for (u64 c = 0; c < total; ++c) {
                std::vector<u8> s(n);
                u64 x = c;
                for (u32 i = 0; i < n; ++i) {
                    s[i] = (u8)(x % alpha);
                    x /= alpha;
                }
                ok &= check(s, (u32)(c % 5), (u32)(c % 16), (u32)(c & 1));
            }
        }
    }
    u64 z = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() {
        z ^= z << 13;
        z ^= z >> 7;
        z ^= z << 17;
        return z;
    };
    const u32 lens[] = {1, 7, 8, 9, 23, 24, 31, 32, 33, 4095, 4096, 4097, 8191, 8192, 8193, 20000};
    for (u32 n : lens)
        for (u32 rep = 0; rep < 6; ++rep) {
            const u32 alpha = rep < 2 ? 2 : rep < 4 ? 4 : 200;
            std::vector<u8> s(n);
            for (u32 i = 0; i < n; ++i) s[i] = (u8)(255 - rnd() % alpha);
            ok &= check(s, (u32)(rnd() % 40), (u32)(rnd() % 16), rep & 1);
        }
    printf("lyn_emu self-test: %llu strings, %s\n", (unsigned long long)g_checked, ok ? "ok" : "FAILED");
    return ok ? 0 : 1;
}

int file_mode(const char* path, u32 bs, u32 nbmax) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        perror(path);
        return 2;
    }
    std::vector<u8> data;
    u8 chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) data.insert(data.end(), chunk, chunk + got);
    fclose(f);
    const u64 N = data.size();
    u32 nb = 0, acc = 0, mc = 0, ml = 0, mcmp = 0, mlive = 0, mfac = 0;
    u64 bad = 0;
    std::vector<u32> st(bs + 1);
    std::vector<u8> fl(N, 0);
    for (u64 base = 0; base < N && nb < nbmax; base += bs, ++nb) {
        const u32 end = (u32)std::min<u64>(N, base + bs);
        Info inf{};
        u32 ns = 0;
        const int r = lyn_emu_block(data.data(), (u32)base, end, 0, lyn::CAND_MAX, lyn::LCP_MAX, nb & 1, st.data(), &ns,
                                    fl.data(), &inf);
        bool same = true;
        if (r == 0) {
            const std::vector<u32> want = duval(data.data() + base, end - (u32)base);
            same = ns == want.size();
            for (u32 i = 0; same && i < ns; ++i) same = st[i] == base + want[i];
            ++acc;
        }
        bad += inf.bad + (same ? 0 : 1);
        mc = std::max(mc, inf.ncand);
        ml = std::max(ml, inf.max_lcp);
        mcmp = std::max(mcmp, inf.ncmp);
        mlive = std::max(mlive, inf.live_tiles);
        mfac = std::max(mfac, ns);
    }
    printf("{\"blocks\": %u, \"accepted\": %u, \"max_candidates\": %u, \"max_lcp\": %u, \"max_comparisons\": %u, "
           "\"max_live_tiles\": %u, \"max_factors\": %u, \"violations_or_mismatches\": %llu}\n",
           nb, acc, mc, ml, mcmp, mlive, mfac, (unsigned long long)bad);
    return bad ? 1 : 0;
}

}  // namespace

#if !defined(LYN_EMU_NO_MAIN)
int main(int argc, char** argv) {
    if (argc >= 3) return file_mode(argv[1], (u32)strtoul(argv[2], nullptr, 10), argc > 3 ? (u32)strtoul(argv[3], nullptr, 10) : ~0u);
    return self_test();
}
#endif
