// Search of a resident buffer for class patterns on gfx950 (findcls_core.h): every match of up to
// 16 patterns of 1..256 byte classes, counted and listed in (position, pattern) order.  The tile
// geometry, the count columns, k_find_scan between the two kernels and the record slots are
// k_find.hip's; ordering is by launch boundaries only: no spinning, no tickets, no atomics.
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

namespace kolm {

namespace {

struct DevLd {
    const u8* buf;
    __device__ __forceinline__ fnd::Word operator()(fnd::i64 off) const {
        const uint4 v = *reinterpret_cast<const uint4*>(buf + off);
        return fnd::Word{{(u64)v.x | ((u64)v.y << 32), (u64)v.z | ((u64)v.w << 32)}};
    }
};

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
    __shared__ u32 s_c[fnd::WG / 64][fnd::MAX_PATTERNS + 1];
    load_pats(sp, P, np);
    const u32 tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 p0 = tile * fnd::TILE + threadIdx.x * fnd::PER;
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(buf) & (fnd::WORD - 1));
    DevLd ld{buf};
    u64 w[fnd::PER];
    fnd::windows(ld, mis, p0, n, w);
    u32 total = 0;
    for (u32 i = 0; i < np; ++i) {
        const u32 m = fcl::match_mask(ld, w, mis, p0, lo, shi, n, sp, i);
        const u32 c = (u32)__popc(m);
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

__global__ __launch_bounds__(fnd::WG) void k_findcls_emit(const u8* __restrict__ buf, u32 n, u32 lo, u32 shi,
                                                          const fcl::Pats* __restrict__ P, u32 np, u32 t0,
                                                          const u64* __restrict__ tscan, u32* __restrict__ out_pos,
                                                          u8* __restrict__ out_which, u32 cap) {
    __shared__ fcl::Pats sp;
    __shared__ uint16_t s_pm[fnd::MAX_PATTERNS][fnd::WG];
    __shared__ u32 s_w[fnd::WG / 64];
    load_pats(sp, P, np);
    const u32 tile = t0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 p0 = tile * fnd::TILE + tid * fnd::PER;
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(buf) & (fnd::WORD - 1));
    DevLd ld{buf};
    u64 w[fnd::PER];
    fnd::windows(ld, mis, p0, n, w);
    u32 any = 0, c = 0;
    for (u32 i = 0; i < np; ++i) {
        const u32 m = fcl::match_mask(ld, w, mis, p0, lo, shi, n, sp, i);
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
