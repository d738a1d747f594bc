// Random-access reads on gfx950: a segmented byte copy with independent source and destination
// alignment (range_core.h).
//   k_range_gather  copies nseg segments {src, dst, len} from one buffer to another.  The work is
//                   cut into items of at most 4 KiB of one segment, aligned to the destination's
//                   16-byte words; one wave takes one item, and the waves of a grid of at most
//                   2048 workgroups stride over the items.  A wave finds its segment by binary
//                   search in the exclusive scan of the per-segment item counts (wave-uniform:
//                   scalar loads), then every lane stores up to 4 aligned 16-byte destination
//                   words.  A word's source bytes begin sh = (src - dst) mod 16 bytes into an
//                   aligned source word: the lane loads that word and, when sh != 0, the next
//                   one (8 independent loads in flight per lane) and funnel-shifts the pair
//                   (v_alignbit_b32 on the 32-bit words; the whole-word part of the shift is a
//                   wave-uniform switch).  The head and the tail of a segment (< 16 bytes each)
//                   are copied byte by byte by lanes 0..15 and 16..31.
// Stores write bytes of [dst, dst + len) only: a destination word that a segment covers in part
// is written byte by byte, never with a 16-byte store or a read-modify-write, since the
// neighbouring segments' waves write the rest of it at the same time.
// Loads touch only aligned 16-byte words that hold at least one byte of the segment, so up to 15
// bytes before src and after src + len are read (and dropped).  The sources of the two callers
// are allocated for that (kolm_api.cpp): the decode scratch ("rd_dec") and the readers' resident
// payload areas begin at a hipMalloc address (256-byte aligned) and are padded past their last
// byte to beyond the next 16-byte boundary.
#include "kolm_internal.h"
#include "range_core.h"

namespace kolm {

namespace {

// The body of one item: `words` (1..256) aligned destination words at dw, their source bytes
// 4 * Q + rb bytes into the aligned source words at sw (Q whole 32-bit words: compile time, so the
// funnel's register indices are static; rb = 0..3 bytes: wave-uniform).  TWO = the shift is not 0:
// every destination word also needs the next source word.  Every lane issues its UNROLL (x 2)
// loads back to back; the lanes past the item's end load its last word again (a word the item
// owns) and store nothing.
template <u32 Q, bool TWO>
__device__ __forceinline__ void copy_body(const uint4* __restrict__ sw, uint4* __restrict__ dw, u32 words, u32 rb,
                                          u32 lane) {
    uint4 xa[rng::UNROLL], xb[rng::UNROLL];
#pragma unroll
    for (u32 k = 0; k < rng::UNROLL; ++k) {
        const u32 w = lane + k * rng::WAVE, wc = w < words ? w : words - 1;
        xa[k] = sw[wc];
        xb[k] = TWO ? sw[wc + 1] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (u32 k = 0; k < rng::UNROLL; ++k) {
        const u32 w = lane + k * rng::WAVE;
        const u32 a[4] = {xa[k].x, xa[k].y, xa[k].z, xa[k].w};
        const u32 b[4] = {xb[k].x, xb[k].y, xb[k].z, xb[k].w};
        u32 o[4];
        rng::src_word(a, b, 4 * Q + (rb & 3u), o);
        if (w < words) dw[w] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

__global__ __launch_bounds__(rng::WG) void k_range_gather(const u8* __restrict__ src, u8* __restrict__ dst,
                                                          const rng::Seg* __restrict__ segs,
                                                          const u32* __restrict__ scan, u32 nseg) {
    const u32 lane = threadIdx.x & (rng::WAVE - 1);
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x / rng::WAVE);
    const u32 nitems = scan[nseg];
    const u32 stride = gridDim.x * (rng::WG / rng::WAVE);
    for (u32 t = blockIdx.x * (rng::WG / rng::WAVE) + wave; t < nitems; t += stride) {
        const u32 si = rng::find_seg(scan, nseg, t);
        const rng::Seg sg = segs[si];
        u8* d = dst + sg.dst;
        const u8* s = src + sg.src;
        const u32 dmis = (u32)(reinterpret_cast<uintptr_t>(d) & (rng::WORD - 1));
        const rng::Item it = rng::item(dmis, sg.len, t - scan[si]);
        d += it.o0;
        s += it.o0;
        if (lane < 2 * rng::WORD) {  // lanes 0..15: the head, 16..31: the tail
            const bool tl = lane >= rng::WORD;
            const u32 j = lane & (rng::WORD - 1);
            const u32 pos = tl ? it.head + it.words * rng::WORD + j : j;
            if (j < (tl ? it.tail : it.head)) d[pos] = s[pos];
        }
        if (it.words == 0) continue;
        const u8* sb = s + it.head;  // the source of the first body word
        const u32 sh = (u32)(reinterpret_cast<uintptr_t>(sb) & (rng::WORD - 1));
        const uint4* sw = reinterpret_cast<const uint4*>(sb - sh);
        uint4* dw = reinterpret_cast<uint4*>(d + it.head);
        const u32 rb = sh & 3u;
        if (sh == 0) copy_body<0, false>(sw, dw, it.words, 0, lane);
        else if (sh < 4) copy_body<0, true>(sw, dw, it.words, rb, lane);
        else if (sh < 8) copy_body<1, true>(sw, dw, it.words, rb, lane);
        else if (sh < 12) copy_body<2, true>(sw, dw, it.words, rb, lane);
        else copy_body<3, true>(sw, dw, it.words, rb, lane);
    }
}

}  // namespace

void launch_range_gather(const u8* src, u8* dst, const rng::Seg* segs, const u32* scan, u32 nseg, u64 nitems,
                         hipStream_t s) {
    if (nseg == 0 || nitems == 0) return;
    k_range_gather<<<rng::grid_for(nitems), rng::WG, 0, s>>>(src, dst, segs, scan, nseg);
}

}  // namespace kolm
