// Search of a resident buffer on gfx950 (find_core.h): every occurrence of up to 16 patterns of
// 1..256 bytes, counted and listed in (position, pattern) order.  Three kernels, ordered by their
// launch boundaries only: no spinning, no tickets, no look-back, no atomics.
//   k_find_count  one workgroup per 4 KiB tile, 256 threads x 16 positions.  The patterns, their
//                 prefix words and masks sit in LDS (fnd::Pats, 4416 bytes).  A thread loads the
//                 two or three aligned 16-byte words that hold its 16 positions' 8-byte windows
//                 and funnel-shifts them into 16 64-bit windows; per pattern and position the
//                 prefix compare is one masked 64-bit equality, and only a candidate of a pattern
//                 longer than 8 bytes reads further bytes.  Writes the tile's count per pattern
//                 and the tile total (cnt[col * ntiles + tile], col = pattern, np = the total).
//   k_find_scan   np + 1 workgroups: workgroup i < np sums column i (the pattern's total);
//                 workgroup np writes the exclusive scan of the tile totals (64-bit: a group can
//                 hold more than 2^32 matches) with the grand total behind it.
//   k_find_emit   tiles [t0, t0 + grid): recomputes the tile, keeps each thread's per-pattern
//                 masks in LDS, scans the per-thread counts in the workgroup and writes the
//                 records at tscan[tile] - tscan[t0] + the thread's offset: position order, then
//                 pattern order within a position.  The host cuts the tile ranges so that a
//                 launch's records fit the staging arrays; the slot is checked against their
//                 capacity all the same.
// What the two tile kernels do with their masks (the count columns, the record slots) is the tile
// skeleton's, find_tile.h, shared with k_findcls.hip and k_findrx.hip.
// Loads: aligned 16-byte words that hold a byte of [buf, buf + n) (find_core.h), so up to 15 bytes
// before buf and after buf + n are read and dropped; the callers' buffers are device allocations
// (256-byte aligned, padded), which such a word never leaves.
#include "kolm_internal.h"
#include "find_core.h"
#include "find_tile.h"

namespace kolm {

namespace {

__device__ __forceinline__ void load_pats(fnd::Pats& sp, const fnd::Pats* __restrict__ P) {
    const u64* src = reinterpret_cast<const u64*>(P);
    u64* dst = reinterpret_cast<u64*>(&sp);
    for (u32 i = threadIdx.x; i < sizeof(fnd::Pats) / sizeof(u64); i += fnd::WG) dst[i] = src[i];
    __syncthreads();
}

__global__ __launch_bounds__(fnd::WG) void k_find_count(const u8* __restrict__ buf, u32 n, u32 lo, u32 shi,
                                                        const fnd::Pats* __restrict__ P, u32 np, u32 ntiles,
                                                        u32* __restrict__ cnt) {
    __shared__ fnd::Pats sp;
    load_pats(sp, P);
    const u32 tile = blockIdx.x, p0 = ftl::first_pos(tile), mis = ftl::misalign(buf);
    ftl::DevLd ld{buf};
    u64 w[fnd::PER];
    fnd::windows(ld, mis, p0, n, w);
    ftl::tile_count(np, ntiles, tile, cnt, [&](u32 i) {
        [[clang::always_inline]] return fnd::match_mask(ld, w, mis, p0, lo, shi, n, sp.pre[i], sp.mask[i], sp.len[i], sp.pat[i]);
    });
}

__global__ __launch_bounds__(fnd::WG) void k_find_scan(const u32* __restrict__ cnt, u32 ntiles, u32 np,
                                                       u64* __restrict__ tot, u64* __restrict__ tscan) {
    __shared__ u64 s_s[fnd::WG];
    const u32 col = blockIdx.x, tid = threadIdx.x;
    const u32* c = cnt + (size_t)col * ntiles;
    if (col < np) {  // a pattern's total
        u64 s = 0;
        for (u32 t = tid; t < ntiles; t += fnd::WG) s += c[t];
        s_s[tid] = s;
        __syncthreads();
        for (u32 h = fnd::WG / 2; h; h >>= 1) {
            if (tid < h) s_s[tid] += s_s[tid + h];
            __syncthreads();
        }
        if (tid == 0) tot[col] = s_s[0];
        return;
    }
    // the tile totals: every thread a contiguous share
    const u32 per = (ntiles + fnd::WG - 1) / fnd::WG;
    const u32 b = tid * per < ntiles ? tid * per : ntiles, e = b + per < ntiles ? b + per : ntiles;
    u64 s = 0;
    for (u32 t = b; t < e; ++t) s += c[t];
    s_s[tid] = s;
    __syncthreads();
    if (tid == 0) {
        u64 run = 0;
        for (u32 i = 0; i < fnd::WG; ++i) {
            const u64 v = s_s[i];
            s_s[i] = run;
            run += v;
        }
        tscan[ntiles] = run;
        tot[np] = run;
    }
    __syncthreads();
    u64 run = s_s[tid];
    for (u32 t = b; t < e; ++t) {
        tscan[t] = run;
        run += c[t];
    }
}

__global__ __launch_bounds__(fnd::WG) void k_find_emit(const u8* __restrict__ buf, u32 n, u32 lo, u32 shi,
                                                       const fnd::Pats* __restrict__ P, u32 np, u32 t0,
                                                       const u64* __restrict__ tscan, u32* __restrict__ out_pos,
                                                       u8* __restrict__ out_which, u32 cap) {
    __shared__ fnd::Pats sp;
    load_pats(sp, P);
    const u32 tile = t0 + blockIdx.x, p0 = ftl::first_pos(tile), mis = ftl::misalign(buf);
    ftl::DevLd ld{buf};
    u64 w[fnd::PER];
    fnd::windows(ld, mis, p0, n, w);
    ftl::tile_emit(np, tile, t0, tscan, out_pos, out_which, cap, [&](u32 i) {
        [[clang::always_inline]] return fnd::match_mask(ld, w, mis, p0, lo, shi, n, sp.pre[i], sp.mask[i], sp.len[i], sp.pat[i]);
    });
}

}  // namespace

void launch_find_count(const u8* buf, u32 n, u32 lo, u32 shi, const fnd::Pats* P, u32 np, u32* cnt, hipStream_t s) {
    const u32 ntiles = fnd::tiles(n);
    if (ntiles) k_find_count<<<ntiles, fnd::WG, 0, s>>>(buf, n, lo, shi, P, np, ntiles, cnt);
}

void launch_find_scan(const u32* cnt, u32 ntiles, u32 np, u64* tot, u64* tscan, hipStream_t s) {
    if (ntiles) k_find_scan<<<np + 1, fnd::WG, 0, s>>>(cnt, ntiles, np, tot, tscan);
}

void launch_find_emit(const u8* buf, u32 n, u32 lo, u32 shi, const fnd::Pats* P, u32 np, u32 t0, u32 t1,
                      const u64* tscan, u32* out_pos, u8* out_which, u32 cap, hipStream_t s) {
    if (t1 > t0) k_find_emit<<<t1 - t0, fnd::WG, 0, s>>>(buf, n, lo, shi, P, np, t0, tscan, out_pos, out_which, cap);
}

}  // namespace kolm
