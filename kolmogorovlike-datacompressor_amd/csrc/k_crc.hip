// Block CRC-32 on gfx950 (crc_core.h): one streaming read of a resident batch gives the raw CRC
// word of every block; the host finishes and combines them (crc::finish, crc::combine).
//   k_crc32   the items and grid of k_block_fp (k_dedup.hip): items are (block, 4 KiB piece of the
//             block), a wave takes a run of up to 8 consecutive pieces of one block and the waves of
//             a grid of at most 2048 workgroups stride over the runs.  A lane takes words l, l + 64,
//             l + 128, l + 192 of every piece through load_words (load_words.h: the same loads as
//             the fingerprint, no byte outside the batch is touched; the bytes of a block's last
//             word past its end are zero).  The workgroup first copies the tables (24.25 KiB,
//             generated on the host from the polynomial) into LDS.  A word costs 16 lookups, one
//             table per byte position; the lane's words of a run lie 1 KiB apart, so its sum is
//             carried from word to word by four more lookups (Horner, crc::stride_shift).  After
//             the run one multiply per lane puts the lane's position in, the lanes are xored
//             across the wave, and lane 0 multiplies by the wave-uniform weight of the bytes of the
//             block after the run (negative for a block's last run, whose rows are walked to the
//             piece's end: crc_core.h) and issues one atomicXor into raw[block] (zeroed by the
//             caller on the same stream).  Xor commutes: the words do not depend on how the runs
//             meet the waves.
// Blocks are addressed through Geom (base / end only).  A run finds its block by division when
// every block has the same run count (fixed geometry: scan == null) and otherwise by binary
// search in the exclusive scan of the per-block run counts; an empty block has no run.
#include "kolm_internal.h"
#include "crc_core.h"
#include "load_words.h"

namespace kolm {

namespace {

__device__ __forceinline__ u32 wave_xor32(u32 v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v ^= __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(ddp::WG) void k_crc32(const u8* __restrict__ text, Geom geo,
                                                   const u32* __restrict__ scan, u32 rpb, u64 nruns,
                                                   const u32* __restrict__ tab_g, u32* __restrict__ raw) {
    __shared__ __attribute__((aligned(16))) u32 tab[crc::TABLE_WORDS];
    for (u32 i = threadIdx.x; i < crc::TABLE_WORDS / 4; i += ddp::WG)
        reinterpret_cast<uint4*>(tab)[i] = reinterpret_cast<const uint4*>(tab_g)[i];
    __syncthreads();
    const u32 lane = threadIdx.x & (ddp::WAVE - 1);
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x / ddp::WAVE);
    const u64 stride = (u64)gridDim.x * (ddp::WG / ddp::WAVE);
    const u64 t0 = reinterpret_cast<uintptr_t>(text), t1 = t0 + geo.N;
    const u32 lw = tab[crc::LW + lane];
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
        u32 acc = 0;
        for (u32 k = r * ddp::RUN; k < k1; ++k) {
            const ddp::Piece pc = ddp::piece(len, k);
            Words x;
            load_words(text + base + pc.o0, pc, t0, t1, lane, x);
#pragma unroll
            for (u32 u = 0; u < ddp::UNROLL; ++u)  // the words past the piece's end are zero
                acc = crc::stride_shift(tab, acc) ^ crc::word_raw(tab, x.w0[u], x.w1[u]);
        }
        const u32 v = wave_xor32(crc::multmodp(acc, lw));
        const u32 wgt = crc::run_weight(tab, len, (u64)k1 * ddp::ITEM);  // wave-uniform
        if (lane == 0) atomicXor(raw + b, crc::multmodp(v, wgt));
    }
}

}  // namespace

void launch_crc32(const u8* text, const Geom& geo, const u32* scan, u64 nruns, const u32* tab, u32* raw, hipStream_t s) {
    if (geo.nb == 0 || nruns == 0) return;
    const u32 rpb = (u32)ddp::runs(geo.bs);  // fixed geometry: runs per block
    k_crc32<<<ddp::grid_for(nruns), ddp::WG, 0, s>>>(text, geo, scan, rpb ? rpb : 1, nruns, tab, raw);
}

}  // namespace kolm
