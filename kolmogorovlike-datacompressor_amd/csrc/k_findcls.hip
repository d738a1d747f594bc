// Search of a resident buffer for class patterns on gfx950 (findcls_core.h): every match of up to
// 16 patterns of 1..256 byte classes, counted and listed in (position, pattern) order.  The tile
// geometry, the count columns and the record slots are the tile skeleton's (find_tile.h), k_find_scan
// runs between the two kernels; ordering is by launch boundaries only: no spinning, no tickets, no atomics.
//   k_findcls_count  one workgroup per 4 KiB tile, 256 threads x 16 positions.  The call's table
//                    T (2 KiB) and, of every pattern, the words its length needs sit in LDS
//                    (fcl::Pats, 10.6 KiB at most).  A thread forms its 16 64-bit windows as
//                    k_find_count does; per pattern and position the candidate filter is one
//                    masked 64-bit equality on the hulls of the first 8 classes, and only a
//                    candidate reads T (indexed by data bytes: equal bytes broadcast, others may
//                    meet in a bank, which only candidates pay) and the bytes from 8 on.
//   k_findcls_emit   tiles [t0, t0 + grid): as k_find_emit.
// Loads: aligned 16-byte words that hold a byte of [buf, buf + n), as in k_find.hip.
#include "kolm_internal.h"
#include "findcls_core.h"
#include "find_tile.h"

namespace kolm {

namespace {

// T, the prefix words and the lengths; of pattern i < np the ceil(len / 8) words of its row
__device__ __forceinline__ void load_pats(fcl::Pats& sp, const fcl::Pats* __restrict__ P, u32 np) {
    const u32 tid = threadIdx.x;
    sp.T[tid] = P->T[tid];  // WG = 256 entries
    if (tid < fnd::MAX_PATTERNS) sp.pre[tid] = P->pre[tid], sp.pmask[tid] = P->pmask[tid], sp.len[tid] = P->len[tid];
    for (u32 x = tid; x < np * fcl::WORDS; x += fnd::WG) {
        const u32 i = x / fcl::WORDS, k = x % fcl::WORDS;
        if (8 * k < P->len[i]) sp.val[i][k] = P->val[i][k], sp.mask[i][k] = P->mask[i][k], sp.tbl[i][k] = P->tbl[i][k];
    }
    __syncthreads();
}

__global__ __launch_bounds__(fnd::WG) void k_findcls_count(const u8* __restrict__ buf, u32 n, u32 lo, u32 shi,
                                                           const fcl::Pats* __restrict__ P, u32 np, u32 ntiles,
                                                           u32* __restrict__ cnt) {
    __shared__ fcl::Pats sp;
    load_pats(sp, P, np);
    const u32 tile = blockIdx.x, p0 = ftl::first_pos(tile), mis = ftl::misalign(buf);
    ftl::DevLd ld{buf};
    u64 w[fnd::PER];
    fnd::windows(ld, mis, p0, n, w);
    ftl::tile_count(np, ntiles, tile, cnt, [&](u32 i) { [[clang::always_inline]] return fcl::match_mask(ld, w, mis, p0, lo, shi, n, sp, i); });
}

__global__ __launch_bounds__(fnd::WG) void k_findcls_emit(const u8* __restrict__ buf, u32 n, u32 lo, u32 shi,
                                                          const fcl::Pats* __restrict__ P, u32 np, u32 t0,
                                                          const u64* __restrict__ tscan, u32* __restrict__ out_pos,
                                                          u8* __restrict__ out_which, u32 cap) {
    __shared__ fcl::Pats sp;
    load_pats(sp, P, np);
    const u32 tile = t0 + blockIdx.x, p0 = ftl::first_pos(tile), mis = ftl::misalign(buf);
    ftl::DevLd ld{buf};
    u64 w[fnd::PER];
    fnd::windows(ld, mis, p0, n, w);
    ftl::tile_emit(np, tile, t0, tscan, out_pos, out_which, cap,
                   [&](u32 i) { [[clang::always_inline]] return fcl::match_mask(ld, w, mis, p0, lo, shi, n, sp, i); });
}

}  // namespace

void launch_findcls_count(const u8* buf, u32 n, u32 lo, u32 shi, const fcl::Pats* P, u32 np, u32* cnt, hipStream_t s) {
    const u32 ntiles = fnd::tiles(n);
    if (ntiles) k_findcls_count<<<ntiles, fnd::WG, 0, s>>>(buf, n, lo, shi, P, np, ntiles, cnt);
}

void launch_findcls_emit(const u8* buf, u32 n, u32 lo, u32 shi, const fcl::Pats* P, u32 np, u32 t0, u32 t1,
                         const u64* tscan, u32* out_pos, u8* out_which, u32 cap, hipStream_t s) {
    if (t1 > t0) k_findcls_emit<<<t1 - t0, fnd::WG, 0, s>>>(buf, n, lo, shi, P, np, t0, tscan, out_pos, out_which, cap);
}

}  // namespace kolm
