// Search of a resident buffer for a prepared pattern set on gfx950 (findset_core.h): every
// occurrence of up to 65 536 distinct patterns of 1..256 bytes, counted per pattern and listed in
// (position, pattern) order, at a cost per position that does not grow with the set.  Two kernels
// around the existing k_find_scan, ordered by their launch boundaries only: no spinning, no
// tickets, no look-back.
//   k_findset_count  one workgroup of 256 threads per span of consecutive 4 KiB tiles
//                    (fst::span_tiles).  It copies the set's filter bitmap (1..32 KiB) into
//                    dynamic LDS once, then per tile forms the 16 windows of each thread as
//                    k_find_count does and, per position: the filter bit in LDS; on a hit the
//                    probe of the slot table; on a key match the walk of the bucket with the full
//                    verify (fst::for_matches: a batch of entries is verified, then counted).  Writes the tile's total to cnt[tile] and adds every match to its
//                    pattern's 64-bit counter with an ordinary global atomic (integer adds: the
//                    same sums in any order).
//   k_find_scan      (k_find.hip) with np = 0: the exclusive scan of the tile totals, the grand
//                    total in tot[0].
//   k_findset_emit   spans of the tiles [t0, t1): recomputes each tile, scans the per-thread match
//                    counts in the workgroup and writes the 8-byte records at tscan[tile] -
//                    tscan[t0] + the thread's offset: positions ascending, bucket order (ascending
//                    pattern index) within a position.  The host cuts the tile ranges so that a
//                    launch's records fit the staging array; every slot is checked against its
//                    capacity all the same.
// Loads of the data: as k_find.hip (aligned 16-byte words that hold a byte of [buf, buf + n)).
// Loads of the tables: slots [0, slot_mask], entries [first, first + count) of a slot, blob words
// [word, word + ceil(len / 8)) of an entry: all inside the set's own allocations.
#include "kolm_internal.h"
#include "findset_core.h"
#include "find_tile.h"

namespace kolm {

namespace {

__device__ __forceinline__ void load_filter(u32* sf, const fst::Set& S) {
    for (u32 i = threadIdx.x; i < S.filter_words; i += fnd::WG) sf[i] = S.filter[i];
    __syncthreads();
}

__global__ __launch_bounds__(fnd::WG) void k_findset_count(const u8* __restrict__ buf, u32 n, u32 lo, u32 shi,
                                                           const fst::Set S, u32 span, u32 ntiles,
                                                           u32* __restrict__ cnt, u64* __restrict__ pcnt) {
    extern __shared__ u32 s_filter[];  // the filter, then the waves' counts: one dynamic block, nothing static beside it
    u32* s_c = s_filter + S.filter_words;
    load_filter(s_filter, S);
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(buf) & (fnd::WORD - 1));
    ftl::DevLd ld{buf};
    const u32 tb = blockIdx.x * span, te = tb + span < ntiles ? tb + span : ntiles;
    for (u32 tile = tb; tile < te; ++tile) {
        const u32 p0 = tile * fnd::TILE + threadIdx.x * fnd::PER;
        u64 w[fnd::PER];
        fnd::windows(ld, mis, p0, n, w);
        u32 c = 0;
#pragma unroll
        for (u32 j = 0; j < fnd::PER; ++j)
            c += fst::for_matches(S, s_filter, ld, w[j], mis, p0 + j, lo, shi, n, [&](const fst::Entry& e) {
                atomicAdd(reinterpret_cast<unsigned long long*>(pcnt + e.idx), 1ull);
            });
        const u32 r = wave_reduce(c, OpAddU(), 0u);
        if (lane == 0) s_c[wave] = r;
        __syncthreads();
        if (threadIdx.x == 0) {
            u32 v = 0;
            for (u32 x = 0; x < fnd::WG / 64; ++x) v += s_c[x];
            cnt[tile] = v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(fnd::WG) void k_findset_emit(const u8* __restrict__ buf, u32 n, u32 lo, u32 shi,
                                                          const fst::Set S, u32 span, u32 t0, u32 t1,
                                                          const u64* __restrict__ tscan, uint2* __restrict__ out,
                                                          u32 cap) {
    extern __shared__ u32 s_filter[];  // the filter, then the waves' totals
    u32* s_w = s_filter + S.filter_words;
    load_filter(s_filter, S);
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(buf) & (fnd::WORD - 1));
    ftl::DevLd ld{buf};
    const u32 tb = t0 + blockIdx.x * span, te = tb + span < t1 ? tb + span : t1;
    const u64 base = tscan[t0];
    for (u32 tile = tb; tile < te; ++tile) {
        const u32 p0 = tile * fnd::TILE + tid * fnd::PER;
        u64 w[fnd::PER];
        fnd::windows(ld, mis, p0, n, w);
        u32 c = 0;
#pragma unroll
        for (u32 j = 0; j < fnd::PER; ++j)
            c += fst::for_matches(S, s_filter, ld, w[j], mis, p0 + j, lo, shi, n, [](const fst::Entry&) {});
        const u32 incl = wave_incl_scan(c, OpAddU(), 0u);
        const u32 wtot = (u32)__builtin_amdgcn_readlane((int)incl, 63);
        if (lane == 0) s_w[wave] = wtot;
        __syncthreads();
        u64 slot = tscan[tile] - base + (incl - c);
        for (u32 x = 0; x < wave; ++x) slot += s_w[x];
        if (c) {  // the thread's own matches again: positions ascending, bucket order within one
#pragma unroll
            for (u32 j = 0; j < fnd::PER; ++j)
                fst::for_matches(S, s_filter, ld, w[j], mis, p0 + j, lo, shi, n, [&](const fst::Entry& e) {
                    if (slot < cap) out[slot] = make_uint2(p0 + j, e.idx);
                    ++slot;
                });
        }
        __syncthreads();
    }
}

// dynamic LDS of both kernels: the filter and one word per wave
u32 lds_bytes(const fst::Set& S) { return (S.filter_words + fnd::WG / 64) * 4; }

}  // namespace

void launch_findset_count(const u8* buf, u32 n, u32 lo, u32 shi, const fst::Set& S, u32* cnt, u64* pcnt, hipStream_t s) {
    const u32 ntiles = fnd::tiles(n);
    if (!ntiles) return;
    const u32 span = fst::span_tiles(S.filter_words * 4);
    k_findset_count<<<fst::spans(ntiles, span), fnd::WG, lds_bytes(S), s>>>(buf, n, lo, shi, S, span, ntiles, cnt, pcnt);
}

void launch_findset_emit(const u8* buf, u32 n, u32 lo, u32 shi, const fst::Set& S, u32 t0, u32 t1, const u64* tscan,
                         uint2* out, u32 cap, hipStream_t s) {
    if (t1 <= t0) return;
    const u32 span = fst::span_tiles(S.filter_words * 4);
    k_findset_emit<<<fst::spans(t1 - t0, span), fnd::WG, lds_bytes(S), s>>>(buf, n, lo, shi, S, span, t0, t1, tscan, out,
                                                                              cap);
}

}  // namespace kolm
