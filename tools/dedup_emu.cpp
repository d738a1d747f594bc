// CPU emulation of the duplicate-detection kernels: the header k_block_fp and k_dedup_cmp of
// kolmogorovlike-datacompressor_amd/csrc/k_dedup.hip compile (csrc/dedup_core.h), driven with the
// kernels' shape — waves striding over (block, 4 KiB piece) items (the fingerprint kernel: over
// runs of 8 such items of one block), 64 virtual lanes with up to 4
// block-relative words each, every word formed from the aligned word that holds its first byte
// and the next one, the words at the batch's ends byte by byte, per-lane sums added per wave and
// then into the block's two sums — behind a C interface for tests/test_dedup_core.py, and a
// main() that runs the sweeps on its own over heap buffers of exactly the batch's size (built
// with -fsanitize=address,undefined by the test: a load outside them is an error there).  Every
// load is also checked against the contract itself, and the violations are counted:
//   loads   aligned 16-byte words that lie inside the batch [0, N) whole; single bytes of the
//           block at hand
// The items can be walked in reverse and in an interleaved wave order: the sums are wrapping
// adds, so every order must give the same fingerprints.
//   g++ -O2 -std=c++17 -shared -fPIC tools/dedup_emu.cpp -o dedup_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/dedup_emu.cpp -o dedup_emu
//   ./dedup_emu        exit status 0 when every case matches the byte-by-byte reference
#include "../kolmogorovlike-datacompressor_amd/csrc/dedup_core.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ddp;

namespace {

struct Words {
    u64 w0[UNROLL], w1[UNROLL];
};

struct Emu {
    const u8* text;  // the batch: [text, text + n), any alignment
    u64 n;
    u64 bad = 0;     // contract violations
    u64 b0 = 0, b1 = 0;  // the block at hand, as batch offsets

    void load_word(const u8* p, u32 x[4]) {
        const bool ok = (reinterpret_cast<uintptr_t>(p) & (WORD - 1)) == 0 && p >= text && p + WORD <= text + n;
        if (!ok) {
            ++bad;
            std::memset(x, 0xA5, WORD);
            return;
        }
        std::memcpy(x, p, WORD);
    }
    u8 load_byte(const u8* p) {
        if (p < text + b0 || p >= text + b1) {
            ++bad;
            return 0xA5;
        }
        return *p;
    }

    // one lane's words of an item, as load_words of k_dedup.hip
    void lane_words(const u8* p0, const Piece& pc, u32 lane, Words& out) {
        const u32 sh = (u32)(reinterpret_cast<uintptr_t>(p0) & (WORD - 1));
        const u64 t0 = reinterpret_cast<uintptr_t>(text), t1 = t0 + n;
        // the kernel's wave-uniform choice of body: with `all` it skips the per-word test, which
        // must then hold for every word of the item (a word it would fail counts as a violation)
        const bool all = item_fast(reinterpret_cast<uintptr_t>(p0), sh, pc.words, t0, t1);
        const u32 q = sh >> 2;  // the kernel's bodies: whole 32-bit words of the shift ...
        u32 xa[UNROLL][4], xb[UNROLL][4];
        bool fs[UNROLL];
        for (u32 u = 0; u < UNROLL; ++u) {
            const u32 w = lane + u * WAVE;
            const u8* p = p0 + (u64)w * WORD;
            const bool wf = fast(reinterpret_cast<uintptr_t>(p), sh, t0, t1);
            if (all && w < pc.words && !wf) ++bad;
            fs[u] = w < pc.words && (all || wf);
            std::memset(xa[u], 0, WORD);
            std::memset(xb[u], 0, WORD);
            if (fs[u]) {
                load_word(p - sh, xa[u]);
                if (sh) load_word(p - sh + WORD, xb[u]);
            }
        }
        for (u32 u = 0; u < UNROLL; ++u) {
            const u32 w = lane + u * WAVE;
            out.w0[u] = out.w1[u] = 0;
            if (w >= pc.words) continue;
            const u32 nv = word_bytes(pc, w);
            if (fs[u]) {
                u32 o[4];
                rng::src_word(xa[u], xb[u], 4 * q + (sh & 3u), o);  // ... and its 0..3 bytes
                out.w0[u] = (u64)o[0] | (u64)o[1] << 32;
                out.w1[u] = (u64)o[2] | (u64)o[3] << 32;
            } else {
                const u8* p = p0 + (u64)w * WORD;
                for (u32 i = 0; i < nv; ++i) {
                    const u64 v = (u64)load_byte(p + i) << (8 * (i & 7));
                    if (i < 8) out.w0[u] |= v;
                    else out.w1[u] |= v;
                }
            }
            mask(out.w0[u], out.w1[u], nv);
        }
    }

    // run r of block b (its pieces r RUN .. r RUN + RUN - 1, one after the other) on one wave: adds
    // into sums[2 b], sums[2 b + 1] once
    void fp_run(const u64* bounds, u32 b, u64 r, u64* sums) {
        b0 = bounds[b], b1 = bounds[b + 1];
        const u64 np = pieces(b1 - b0);
        u64 ls0[WAVE] = {0}, ls1[WAVE] = {0};  // the lanes' sums over the run
        for (u64 k = r * RUN; k < np && k < (r + 1) * RUN; ++k) {
            const Piece pc = piece(b1 - b0, k);
            for (u32 lane = 0; lane < WAVE; ++lane) {
                Words x;
                lane_words(text + b0 + pc.o0, pc, lane, x);
                for (u32 u = 0; u < UNROLL; ++u) {
                    const u32 w = lane + u * WAVE;
                    if (w < pc.words) mix(x.w0[u], x.w1[u], (u32)(k * WPI + w), ls0[lane], ls1[lane]);
                }
            }
        }
        u64 s0 = 0, s1 = 0;  // the wave's sums: the lanes' sums added
        for (u32 lane = 0; lane < WAVE; ++lane) s0 += ls0[lane], s1 += ls1[lane];
        sums[2 * (u64)b] += s0;
        sums[2 * (u64)b + 1] += s1;
    }

    // item (pair, piece k): true when the wave saw a difference
    bool cmp_item(const u64* bounds, u32 a, u32 b, u64 k) {
        const Piece pc = piece(bounds[a + 1] - bounds[a], k);
        bool diff = false;
        for (u32 lane = 0; lane < WAVE; ++lane) {
            Words x, y;
            b0 = bounds[a], b1 = bounds[a + 1];
            lane_words(text + bounds[a] + pc.o0, pc, lane, x);
            b0 = bounds[b], b1 = bounds[b + 1];
            lane_words(text + bounds[b] + pc.o0, pc, lane, y);
            for (u32 u = 0; u < UNROLL; ++u) diff |= x.w0[u] != y.w0[u] || x.w1[u] != y.w1[u];
        }
        return diff;
    }
};

// the order in which the items meet the waves: 0 wave after wave, each striding over its items;
// 1 the same sequence reversed; 2 pass by pass, the odd waves before the even ones
std::vector<u64> sequence(u64 nitems, u32 waves, u32 order) {
    if (waves == 0) waves = grid_for(nitems) * (WG / WAVE);
    std::vector<u64> seq;
    if (order == 2) {
        for (u64 base = 0; base < nitems; base += waves)
            for (u32 par = 0; par < 2; ++par)
                for (u32 w = 1 - par; w < waves; w += 2)
                    if (base + w < nitems) seq.push_back(base + w);
    } else {
        for (u32 w = 0; w < waves; ++w)
            for (u64 t = w; t < nitems; t += waves) seq.push_back(t);
        if (order == 1) std::reverse(seq.begin(), seq.end());
    }
    return seq;
}

// item t of the scan -> (entry, piece)
void locate(const std::vector<u64>& scan, u64 t, u32& e, u64& k) {
    e = (u32)(std::upper_bound(scan.begin(), scan.end(), t) - scan.begin()) - 1;
    k = t - scan[e];
}

}  // namespace

// The definition restated byte by byte: words from the block's first byte, zero-padded.
extern "C" void ddp_ref_fp(const uint8_t* p, uint64_t len, uint64_t* fp) {
    u64 s0 = 0, s1 = 0;
    for (u64 j = 0; j * WORD < len; ++j) {
        u8 w[WORD] = {0};
        std::memcpy(w, p + j * WORD, (size_t)std::min<u64>(WORD, len - j * WORD));
        u64 w0, w1;
        std::memcpy(&w0, w, 8);
        std::memcpy(&w1, w + 8, 8);
        mix(w0, w1, (u32)j, s0, s1);
    }
    finish(s0, s1, len, fp);
}

// Fingerprints of the nb blocks [bounds[i], bounds[i + 1]) of the batch text[0, n) (bounds[0] = 0,
// non-decreasing, bounds[nb] = n) as k_block_fp and the host's finish compute them: fp[2 nb].
// waves = the grid's waves (0: the kernel's own grid); order as sequence().  Returns the number of
// contract violations (0 for a correct kernel).
extern "C" uint64_t ddp_emu_fp(const uint8_t* text, uint64_t n, const uint64_t* bounds, uint32_t nb, uint32_t waves,
                               uint32_t order, uint64_t* fp) {
    std::vector<u64> scan((size_t)nb + 1, 0), sums(2 * (size_t)nb, 0);
    for (u32 b = 0; b < nb; ++b) scan[b + 1] = scan[b] + runs(bounds[b + 1] - bounds[b]);
    Emu e{text, n};
    const std::vector<u64> seq = sequence(scan[nb], waves, order);
    for (u64 t : seq) {
        u32 b;
        u64 k;
        locate(scan, t, b, k);
        e.fp_run(bounds, b, k, sums.data());
    }
    for (u32 b = 0; b < nb; ++b) finish(sums[2 * (u64)b], sums[2 * (u64)b + 1], bounds[b + 1] - bounds[b], fp + 2 * (u64)b);
    return e.bad + (seq.size() == scan[nb] ? 0 : 1);
}

// differ[p] = 1 when blocks pairs[2 p] and pairs[2 p + 1] (equal lengths) differ, as k_dedup_cmp
// sets it (differ zeroed here).  Returns the contract violations.
extern "C" uint64_t ddp_emu_cmp(const uint8_t* text, uint64_t n, const uint64_t* bounds, const uint32_t* pairs,
                                uint32_t npairs, uint32_t waves, uint32_t order, uint32_t* differ) {
    std::vector<u64> scan((size_t)npairs + 1, 0);
    u64 bad = 0;
    for (u32 p = 0; p < npairs; ++p) {
        const u64 la = bounds[pairs[2 * p] + 1] - bounds[pairs[2 * p]];
        if (la != bounds[pairs[2 * p + 1] + 1] - bounds[pairs[2 * p + 1]]) ++bad;  // the plan pairs equal lengths
        scan[p + 1] = scan[p] + pieces(la);
        differ[p] = 0;
    }
    if (bad) return bad;
    Emu e{text, n};
    const std::vector<u64> seq = sequence(scan[npairs], waves, order);
    for (u64 t : seq) {
        u32 p;
        u64 k;
        locate(scan, t, p, k);
        if (e.cmp_item(bounds, pairs[2 * p], pairs[2 * p + 1], k)) differ[p] |= 1u;
    }
    return e.bad + (seq.size() == scan[npairs] ? 0 : 1);
}

extern "C" uint32_t ddp_emu_item_bytes(void) { return ITEM; }

namespace {

u64 g_cases = 0;
const u64 LENS[] = {1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8193};

u8 content(u64 i) { return (u8)(i * 131 + (i >> 8) * 7 + 3); }

// The batch: a heap block of exactly lead + pre + len + post bytes whose first `lead` bytes are
// not part of it (the batch then begins `lead` bytes past an aligned address).  Blocks: the
// prefix (pre bytes, when pre > 0), the block under test (content(0..len)), a copy of it when
// post >= len, the rest.  Checks the block's fingerprint against the reference and the copy's
// against the block's; compares block and copy, then a copy with byte `flip` changed.
int run_case(u32 lead, u32 pre, u64 len, bool twin, u32 waves, u32 order, const char* what) {
    const u64 n = pre + len + (twin ? len + 5 + len : 0);
    u8* raw = (u8*)std::malloc(lead + n ? lead + n : 1);
    u8* text = raw + lead;
    for (u64 i = 0; i < pre; ++i) text[i] = (u8)(0xE0 + i);
    for (u64 i = 0; i < len; ++i) text[pre + i] = content(i);
    std::vector<u64> bounds{0};
    if (pre) bounds.push_back(pre);
    const u32 blk = (u32)bounds.size() - 1;
    bounds.push_back(pre + len);
    if (twin) {  // block, equal copy, 5 other bytes, copy with one byte changed
        for (u64 i = 0; i < len; ++i) text[pre + len + i] = content(i);
        for (u64 i = 0; i < 5; ++i) text[pre + 2 * len + i] = (u8)(0x11 * i);
        for (u64 i = 0; i < len; ++i) text[pre + 2 * len + 5 + i] = content(i);
        text[pre + 2 * len + 5 + (len * 2) / 3] ^= 0x40;
        bounds.push_back(pre + 2 * len);
        bounds.push_back(pre + 2 * len + 5);
        bounds.push_back(n);
    }
    const u32 nb = (u32)bounds.size() - 1;
    std::vector<u64> fp(2 * (size_t)nb), want(2);
    u64 bad = ddp_emu_fp(text, n, bounds.data(), nb, waves, order, fp.data());
    ddp_ref_fp(text + pre, len, want.data());
    int fail = 0;
    if (bad) std::fprintf(stderr, "%s: %llu contract violations (fingerprints)\n", what, (unsigned long long)bad), fail = 1;
    if (fp[2 * blk] != want[0] || fp[2 * blk + 1] != want[1] || (want[0] | want[1]) == 0) {
        std::fprintf(stderr, "%s: fingerprint differs from the reference (lead %u, prefix %u, length %llu)\n", what, lead,
                     pre, (unsigned long long)len);
        fail = 1;
    }
    if (twin) {
        if (fp[2 * (blk + 1)] != want[0] || fp[2 * (blk + 1) + 1] != want[1]) fail = 1;
        if (fp[2 * (blk + 3)] == want[0] && fp[2 * (blk + 3) + 1] == want[1]) fail = 1;
        const u32 pairs[4] = {blk + 1, blk, blk + 3, blk};
        u32 differ[2] = {7, 7};
        bad = ddp_emu_cmp(text, n, bounds.data(), pairs, 2, waves, order, differ);
        if (bad || differ[0] != 0 || differ[1] != 1) {
            std::fprintf(stderr, "%s: compare gives %u %u with %llu violations (lead %u, prefix %u, length %llu)\n", what,
                         differ[0], differ[1], (unsigned long long)bad, lead, pre, (unsigned long long)len);
            fail = 1;
        }
    }
    std::free(raw);
    ++g_cases;
    return fail;
}

}  // namespace

#ifndef DDP_EMU_NO_MAIN
int main() {
    int bad = 0;
    for (u64 len : LENS)
        for (u32 pre = 0; pre < 16; ++pre) {
            bad |= run_case(0, pre, len, false, 0, 0, "one block");
            bad |= run_case(0, pre, len, true, 0, 0, "twins");
            bad |= run_case((pre * 7 + 3) & 15, pre, len, true, 2, 1 + pre % 2, "twins, batch not aligned");
        }
    for (u64 len = 1; len <= 80; ++len)
        for (u32 lead = 0; lead < 16; lead += 5) bad |= run_case(lead, (u32)(len * 3) & 15, len, true, 3, (u32)len % 3, "short");
    for (u64 len : {(u64)3 * ITEM + 5, (u64)5 * ITEM, (u64)RUN * ITEM + 7, (u64)(2 * RUN + 1) * ITEM})  // one run, several
        for (u32 waves : {1u, 2u, 5u})
            for (u32 order = 0; order < 3; ++order) bad |= run_case(9, 7, len, true, waves, order, "several pieces");
    std::printf("dedup_emu: %llu cases %s\n", (unsigned long long)g_cases, bad ? "FAILED" : "ok");
    return bad;
}
#endif
