// Duplicate-block detection on gfx950 (dedup_core.h): one streaming read of the batch gives a
// 128-bit fingerprint per block, and candidate pairs of blocks are compared byte for byte.
//   k_block_fp    items are (block, 4 KiB piece of the block); a wave takes a run of up to 8
//                 consecutive items of one block, one after the other, and the waves of a grid of
//                 at most 2048 workgroups stride over the runs.  A lane takes
//                 words l, l + 64, l + 128, l + 192 of the piece: block-relative 16-byte words,
//                 each formed from the aligned word that holds its first byte and, when the block
//                 does not start on a 16-byte boundary, the next one (4 or 8 independent loads in
//                 flight per lane, funnel-shifted by rng::src_word).  Every word is mixed with its
//                 index; after the run the lane sums are added across the wave and lane 0 issues
//                 two u64 atomic adds into fp[block] (zeroed by the caller on the same stream).
//                 Wrapping adds commute: the sums do not depend on how the items meet the waves.
//   k_dedup_cmp   items are (pair, 4 KiB piece): blocks a and b of equal length, each at its own
//                 alignment, both read through the funnel.  A wave that finds a difference ORs 1
//                 into differ[pair] (one vector atomic); equal waves write nothing.
// Blocks are addressed through Geom (base / end).  A run (item) finds its block (pair) by division
// when every block has the same run count (fixed geometry: scan == null) and otherwise by binary
// search in the exclusive scan of the per-block run (per-pair piece) counts.
// Loads: aligned 16-byte words that lie inside the batch [text, text + N) whole; the words at the
// batch's two ends whose aligned neighbours would leave it are read byte by byte.  No load
// touches a byte outside the batch.
#include "kolm_internal.h"
#include "dedup_core.h"
#include "load_words.h"

namespace kolm {

namespace {

__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(ddp::WG) void k_block_fp(const u8* __restrict__ text, Geom geo,
                                                      const u32* __restrict__ scan, u32 rpb, u64 nruns,
                                                      unsigned long long* __restrict__ fp) {
    const u32 lane = threadIdx.x & (ddp::WAVE - 1);
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x / ddp::WAVE);
    const u64 stride = (u64)gridDim.x * (ddp::WG / ddp::WAVE);
    const u64 t0 = reinterpret_cast<uintptr_t>(text), t1 = t0 + geo.N;
    for (u64 t = (u64)blockIdx.x * (ddp::WG / ddp::WAVE) + wave; t < nruns; t += stride) {
        u32 b, r;
        if (scan) {
            b = rng::find_seg(scan, geo.nb, (u32)t);
            r = (u32)t - scan[b];
        } else {
            b = (u32)(t / rpb);
            r = (u32)(t % rpb);
        }
        const u32 base = geo.base(b);
        const u64 len = geo.end(b) - base;
        const u32 np = (u32)ddp::pieces(len);
        if (r * ddp::RUN >= np) continue;  // fixed geometry: the short last block's missing runs
        const u32 k1 = (r + 1) * ddp::RUN < np ? (r + 1) * ddp::RUN : np;
        u64 s0 = 0, s1 = 0;
        for (u32 k = r * ddp::RUN; k < k1; ++k) {
            const ddp::Piece pc = ddp::piece(len, k);
            Words x;
            load_words(text + base + pc.o0, pc, t0, t1, lane, x);
#pragma unroll
            for (u32 u = 0; u < ddp::UNROLL; ++u) {
                const u32 w = lane + u * ddp::WAVE;
                if (w < pc.words) ddp::mix(x.w0[u], x.w1[u], k * ddp::WPI + w, s0, s1);
            }
        }
        s0 = wave_sum64(s0);
        s1 = wave_sum64(s1);
        if (lane == 0) {
            atomicAdd(fp + 2 * (u64)b, (unsigned long long)s0);
            atomicAdd(fp + 2 * (u64)b + 1, (unsigned long long)s1);
        }
    }
}

__global__ __launch_bounds__(ddp::WG) void k_dedup_cmp(const u8* __restrict__ text, Geom geo,
                                                       const uint2* __restrict__ pairs, const u32* __restrict__ scan,
                                                       u32 npairs, u32* __restrict__ differ) {
    const u32 lane = threadIdx.x & (ddp::WAVE - 1);
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x / ddp::WAVE);
    const u32 nitems = scan[npairs];
    const u32 stride = gridDim.x * (ddp::WG / ddp::WAVE);
    const u64 t0 = reinterpret_cast<uintptr_t>(text), t1 = t0 + geo.N;
    for (u32 t = blockIdx.x * (ddp::WG / ddp::WAVE) + wave; t < nitems; t += stride) {
        const u32 pi = rng::find_seg(scan, npairs, t);
        const uint2 pr = pairs[pi];
        const u32 ba = geo.base(pr.x), bb = geo.base(pr.y);
        const u64 len = geo.end(pr.x) - ba;  // = the other block's length (the plan pairs equal lengths)
        const ddp::Piece pc = ddp::piece(len, t - scan[pi]);
        Words x, y;
        load_words(text + ba + pc.o0, pc, t0, t1, lane, x);
        load_words(text + bb + pc.o0, pc, t0, t1, lane, y);
        bool diff = false;
#pragma unroll
        for (u32 u = 0; u < ddp::UNROLL; ++u) diff |= x.w0[u] != y.w0[u] || x.w1[u] != y.w1[u];
        if (__ballot(diff) != 0 && lane == 0) atomicOr(differ + pi, 1u);
    }
}

}  // namespace

void launch_block_fp(const u8* text, const Geom& geo, const u32* scan, u64 nruns, u64* fp, hipStream_t s) {
    if (geo.nb == 0 || nruns == 0) return;
    const u32 rpb = (u32)ddp::runs(geo.bs);  // fixed geometry: runs per block
    k_block_fp<<<ddp::grid_for(nruns), ddp::WG, 0, s>>>(text, geo, scan, rpb ? rpb : 1, nruns,
                                                        reinterpret_cast<unsigned long long*>(fp));
}

void launch_dedup_cmp(const u8* text, const Geom& geo, const u32* pairs, const u32* scan, u32 npairs, u64 nitems,
                      u32* differ, hipStream_t s) {
    if (npairs == 0 || nitems == 0) return;
    k_dedup_cmp<<<ddp::grid_for(nitems), ddp::WG, 0, s>>>(text, geo, reinterpret_cast<const uint2*>(pairs), scan, npairs,
                                                         differ);
}

}  // namespace kolm
