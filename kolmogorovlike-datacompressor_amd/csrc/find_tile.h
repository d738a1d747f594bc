// The tile skeleton of the search kernels on gfx950 (k_find.hip, k_findcls.hip, k_findrx.hip), device
// only: what every variant does with a tile once it can say which of a thread's 16 positions match
// a pattern.  A kernel keeps its prologue (what it puts into LDS, the windows) and hands the two
// epilogues one callable, mask(i): pattern i's match mask of this thread, bit j = position p0 + j.
//   tile_count  per pattern the wave sums, then cnt[col * ntiles + tile]: col = the pattern, col np
//               = the tile's total (the columns k_find_scan sums and scans).
//   tile_emit   keeps the thread's masks in LDS, scans the per-thread counts in the workgroup and
//               writes the records at tscan[tile] - tscan[t0] + the thread's offset: position
//               order, then pattern order within a position; every slot is checked against cap.
// The callable marks its match_mask call [[clang::always_inline]]: behind a closure the inliner no
// longer sees that the windows are the kernel's own array, and a call left standing would put
// them into scratch memory.
// Both are called by all 256 threads of a workgroup, once per kernel (they hold __syncthreads and
// own their LDS arrays: 272 and 8208 bytes).  DevLd is the loader of every search kernel,
// k_findset.hip's included.
#pragma once
#include "kolm_internal.h"
#include "find_core.h"

namespace kolm {
namespace ftl {

// an aligned 16-byte word of the scanned buffer (find_core.h: which words are read)
struct DevLd {
    const u8* buf;
    __device__ __forceinline__ fnd::Word operator()(fnd::i64 off) const {
        const uint4 v = *reinterpret_cast<const uint4*>(buf + off);
        return fnd::Word{{(u64)v.x | ((u64)v.y << 32), (u64)v.z | ((u64)v.w << 32)}};
    }
};

// a thread's first position in `tile`, and the buffer's misalignment to the 16-byte words
__device__ __forceinline__ u32 first_pos(u32 tile) { return tile * fnd::TILE + threadIdx.x * fnd::PER; }
__device__ __forceinline__ u32 misalign(const u8* buf) { return (u32)(reinterpret_cast<uintptr_t>(buf) & (fnd::WORD - 1)); }

template <class Mask>
__device__ __forceinline__ void tile_count(u32 np, u32 ntiles, u32 tile, u32* __restrict__ cnt, Mask&& mask) {
    __shared__ u32 s_c[fnd::WG / 64][fnd::MAX_PATTERNS + 1];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 total = 0;
    for (u32 i = 0; i < np; ++i) {
        const u32 c = (u32)__popc(mask(i));
        total += c;
        const u32 r = wave_reduce(c, OpAddU(), 0u);
        if (lane == 0) s_c[wave][i] = r;
    }
    const u32 rt = wave_reduce(total, OpAddU(), 0u);
    if (lane == 0) s_c[wave][fnd::MAX_PATTERNS] = rt;
    __syncthreads();
    if (threadIdx.x <= np) {
        const u32 k = threadIdx.x < np ? threadIdx.x : fnd::MAX_PATTERNS;
        u32 v = 0;
        for (u32 x = 0; x < fnd::WG / 64; ++x) v += s_c[x][k];
        cnt[(size_t)threadIdx.x * ntiles + tile] = v;
    }
}

template <class Mask>
__device__ __forceinline__ void tile_emit(u32 np, u32 tile, u32 t0, const u64* __restrict__ tscan, u32* __restrict__ out_pos,
                                          u8* __restrict__ out_which, u32 cap, Mask&& mask) {
    __shared__ uint16_t s_pm[fnd::MAX_PATTERNS][fnd::WG];
    __shared__ u32 s_w[fnd::WG / 64];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p0 = first_pos(tile);
    u32 any = 0, c = 0;
    for (u32 i = 0; i < np; ++i) {
        const u32 m = mask(i);
        s_pm[i][tid] = (uint16_t)m;
        any |= m;
        c += (u32)__popc(m);
    }
    const u32 incl = wave_incl_scan(c, OpAddU(), 0u);
    const u32 wtot = (u32)__builtin_amdgcn_readlane((int)incl, 63);
    if (lane == 0) s_w[wave] = wtot;
    __syncthreads();
    u32 slot = (u32)(tscan[tile] - tscan[t0]) + incl - c;
    for (u32 x = 0; x < wave; ++x) slot += s_w[x];
    while (any) {  // the thread's own masks: positions ascending, patterns ascending within one
        const u32 j = (u32)__ffs((int)any) - 1;
        any &= any - 1;
        for (u32 i = 0; i < np; ++i)
            if ((s_pm[i][tid] >> j) & 1u) {
                if (slot < cap) {
                    out_pos[slot] = p0 + j;
                    out_which[slot] = (u8)i;
                }
                ++slot;
            }
    }
}

}  // namespace ftl
}  // namespace kolm
