// CPU emulation of the gather kernel of the random-access reads: the header k_range_gather of
// kolmogorovlike-datacompressor_amd/csrc/k_range.hip compiles (csrc/range_core.h), driven with
// the kernel's shape — waves striding over items of at most 4 KiB of one segment, 64 virtual
// lanes with up to 4 aligned destination words each, every word formed from the two aligned
// source words that straddle it, the head and tail bytes on lanes 0..31 — behind a C interface
// for tests/test_range_core.py, and a main() that runs the sweeps on its own over heap buffers
// of exactly the size the kernel's contract allows (built with -fsanitize=address,undefined by
// the test: a load or store outside them is an error there).  Every access is also checked
// against the contract itself, and the violations are counted:
//   loads   aligned 16-byte words inside the source buffer that hold a byte of the segment;
//           single bytes of the segment
//   stores  aligned 16-byte words that lie inside [dst, dst + len) whole; single bytes of it
// The items can be walked in reverse and in an interleaved wave order: segments packed back to
// back share destination words, and a store wider than the segment's own bytes would overwrite
// what a neighbour wrote earlier.
//   g++ -O2 -std=c++17 -shared -fPIC tools/range_emu.cpp -o range_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/range_emu.cpp -o range_emu
//   ./range_emu        exit status 0 when every case matches the byte-by-byte reference
#include "../kolmogorovlike-datacompressor_amd/csrc/range_core.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

using namespace rng;

namespace {

struct Emu {
    const u8* src;   // the source buffer as allocated: [src, src + src_size), src 16-byte aligned
    u64 src_size;
    u8* dst;
    u64 bad = 0;     // contract violations
    Seg sg{};        // the segment of the item at hand

    void load_word(const u8* p, u32 x[4]) {
        const u64 o = (u64)(p - src);
        const bool ok = (reinterpret_cast<uintptr_t>(p) & (WORD - 1)) == 0 && p >= src && o + WORD <= src_size &&
                        o < sg.src + sg.len && o + WORD > sg.src;
        if (!ok) {
            ++bad;
            std::memset(x, 0xA5, WORD);
            return;
        }
        std::memcpy(x, p, WORD);
    }
    void store_word(u8* p, const u32 x[4]) {
        const u64 o = (u64)(p - dst);
        if ((reinterpret_cast<uintptr_t>(p) & (WORD - 1)) != 0 || p < dst || o < sg.dst || o + WORD > sg.dst + sg.len) {
            ++bad;
            return;
        }
        std::memcpy(p, x, WORD);
    }
    void copy_byte(u8* d, const u8* s) {
        const u64 od = (u64)(d - dst), os = (u64)(s - src);
        if (d < dst || od < sg.dst || od >= sg.dst + sg.len || s < src || os < sg.src || os >= sg.src + sg.len) {
            ++bad;
            return;
        }
        *d = *s;
    }

    // one item on one wave, as the kernel's loop body
    void run_item(const Seg* segs, const u32* scan, u32 nseg, u32 t) {
        const u32 si = find_seg(scan, nseg, t);
        sg = segs[si];
        u8* d = dst + sg.dst;
        const u8* s = src + sg.src;
        const u32 dmis = (u32)(reinterpret_cast<uintptr_t>(d) & (WORD - 1));
        const Item it = item(dmis, sg.len, t - scan[si]);
        d += it.o0;
        s += it.o0;
        for (u32 lane = 0; lane < 2 * WORD; ++lane) {
            const bool tl = lane >= WORD;
            const u32 j = lane & (WORD - 1);
            const u32 pos = tl ? it.head + it.words * WORD + j : j;
            if (j < (tl ? it.tail : it.head)) copy_byte(d + pos, s + pos);
        }
        if (it.words == 0) return;
        const u8* sb = s + it.head;
        const u32 sh = (u32)(reinterpret_cast<uintptr_t>(sb) & (WORD - 1));
        const u8* sw = sb - sh;
        u8* dw = d + it.head;
        for (u32 lane = 0; lane < WAVE; ++lane) {
            u32 xa[UNROLL][4], xb[UNROLL][4];
            for (u32 k = 0; k < UNROLL; ++k) {
                const u32 w = lane + k * WAVE, wc = w < it.words ? w : it.words - 1;
                load_word(sw + (u64)wc * WORD, xa[k]);
                if (sh) load_word(sw + (u64)(wc + 1) * WORD, xb[k]);
                else std::memset(xb[k], 0, WORD);
            }
            for (u32 k = 0; k < UNROLL; ++k) {
                const u32 w = lane + k * WAVE;
                u32 o[4];
                src_word(xa[k], xb[k], sh, o);
                if (w < it.words) store_word(dw + (u64)w * WORD, o);
            }
        }
    }
};

}  // namespace

// Copies the segments (offsets into src / dst) as the kernel does.  src is the source buffer as
// allocated (16-byte aligned, src_size bytes).  waves = the grid's waves (0: the kernel's own
// grid); order 0: wave after wave, each striding over its items; 1: the same sequence reversed;
// 2: pass by pass, the odd waves before the even ones.  Returns the number of contract
// violations (0 for a correct kernel); ~0 when the items do not fit 32 bits.
extern "C" uint64_t rng_emu_gather(const uint8_t* src, uint64_t src_size, uint8_t* dst, const Seg* segs, uint32_t nseg,
                                   uint32_t waves, uint32_t order) {
    std::vector<u32> scan((size_t)nseg + 1, 0);
    u64 n = 0;
    for (u32 i = 0; i < nseg; ++i) {
        n += items((u32)((reinterpret_cast<uintptr_t>(dst) + segs[i].dst) & (WORD - 1)), segs[i].len);
        if (n > 0xFFFFFFFFull) return ~0ull;
        scan[i + 1] = (u32)n;
    }
    if (n == 0) return 0;
    if (waves == 0) waves = grid_for(n) * (WG / WAVE);
    std::vector<u32> seq;
    if (order == 2) {
        for (u64 base = 0; base < n; base += waves)
            for (u32 par = 0; par < 2; ++par)
                for (u32 w = 1 - par; w < waves; w += 2)
                    if (base + w < n) seq.push_back((u32)(base + w));
    } else {
        for (u32 w = 0; w < waves; ++w)
            for (u64 t = w; t < n; t += waves) seq.push_back((u32)t);
        if (order == 1) std::reverse(seq.begin(), seq.end());
    }
    Emu e{src, src_size, dst};
    for (u32 t : seq) e.run_item(segs, scan.data(), nseg, t);
    return e.bad + (seq.size() == n ? 0 : 1);
}

extern "C" uint32_t rng_emu_item_bytes(void) { return ITEM; }

namespace {

u64 g_cases = 0;

// Source buffer: a 16-byte aligned heap block of exactly the aligned words up to src_span (the
// end of the last segment's source); destination: a heap block of exactly dst_size bytes.
int run_case(const std::vector<Seg>& segs, u64 src_span, u64 dst_size, u32 waves, u32 order, const char* what) {
    const u64 src_size = (src_span + WORD - 1) / WORD * WORD;
    u8* src = (u8*)std::aligned_alloc(WORD, src_size ? src_size : WORD);
    u8* dst = (u8*)std::malloc(dst_size ? dst_size : 1);
    std::vector<u8> want(dst_size, 0xCC);
    for (u64 i = 0; i < src_size; ++i) src[i] = (u8)(i * 131 + (i >> 8) + 7);
    std::memset(dst, 0xCC, dst_size);
    for (const Seg& s : segs)
        for (u64 j = 0; j < s.len; ++j) want[s.dst + j] = src[s.src + j];
    const u64 bad = rng_emu_gather(src, src_size, dst, segs.data(), (u32)segs.size(), waves, order);
    int fail = bad != 0;
    if (bad) std::fprintf(stderr, "%s: %llu contract violations\n", what, (unsigned long long)bad);
    for (u64 i = 0; i < dst_size && !fail; ++i)
        if (dst[i] != want[i]) {
            std::fprintf(stderr, "%s: byte %llu is %02x, want %02x (segments %zu, first {%llu, %llu, %llu})\n", what,
                         (unsigned long long)i, dst[i], want[i], segs.size(), (unsigned long long)segs[0].src,
                         (unsigned long long)segs[0].dst, (unsigned long long)segs[0].len);
            fail = 1;
        }
    std::free(src);
    std::free(dst);
    ++g_cases;
    return fail;
}

// one segment: source misalignment sm, destination misalignment dm (the dm bytes in front of the
// destination are canaries; the buffer ends with the segment)
int one_segment(u32 sm, u32 dm, u64 len, u32 waves, u32 order) {
    return run_case({Seg{sm, dm, len}}, sm + len, dm + len, waves, order, "one segment");
}

// segments of the given lengths packed back to back in dst from dm on; sources spread over the
// source buffer with varying misalignment
int packed(const std::vector<u32>& lens, u32 dm, u32 waves, u32 order) {
    std::vector<Seg> segs;
    u64 so = 3, d = dm;
    for (size_t i = 0; i < lens.size(); ++i) {
        segs.push_back(Seg{so, d, lens[i]});
        so += lens[i] + (i * 7) % 23;
        d += lens[i];
    }
    return run_case(segs, so, d, waves, order, "packed segments");
}

}  // namespace

#ifndef RNG_EMU_NO_MAIN
int main() {
    int bad = 0;
    for (u32 sm = 0; sm < 16; ++sm)
        for (u32 dm = 0; dm < 16; ++dm)
            for (u64 len = 0; len <= 80; ++len) bad |= one_segment(sm, dm, len, 0, 0);
    for (u64 len : {(u64)ITEM - 1, (u64)ITEM, (u64)ITEM + 1, 2 * (u64)ITEM + 17})
        for (auto m : {std::pair<u32, u32>{0, 0}, {3, 9}, {15, 1}})
            for (u32 order = 0; order < 3; ++order) bad |= one_segment(m.first, m.second, len, order ? 2 : 0, order);
    // many short segments back to back: neighbours share destination words
    std::vector<u32> lens;
    for (u32 rep = 0; rep < 3; ++rep)
        for (u32 l = 0; l <= 33; ++l) lens.push_back((l * 5 + rep) % 34);
    for (u32 dm : {0u, 5u, 15u})
        for (u32 order = 0; order < 3; ++order) bad |= packed(lens, dm, order == 1 ? 3 : 0, order);
    // several items per wave under a grid stride, mixed with short segments
    std::vector<u32> mixed{1, 3 * ITEM + 5, 0, 17, ITEM, 2 * ITEM - 1, 33, 16, ITEM + 16};
    for (u32 waves : {1u, 2u, 5u})
        for (u32 order = 0; order < 3; ++order) bad |= packed(mixed, 7, waves, order);
    std::printf("range_emu: %llu cases %s\n", (unsigned long long)g_cases, bad ? "FAILED" : "ok");
    return bad;
}
#endif
