// Search of a resident buffer for regular expressions on gfx950 (findrx_core.h): every start of up
// to 16 expressions, compiled to one deterministic automaton, counted and listed in (position,
// expression) order.  The tile geometry, the count columns and the record slots are the tile
// skeleton's (find_tile.h), k_find_scan runs between the two kernels; ordering is by launch
// boundaries only: no spinning, no tickets, no atomics.
//   k_findrx_count  one workgroup per 4 KiB tile, 256 threads x 16 positions.  The table (dynamic
//                   LDS: its own padded size, 32 KiB at most, so small automata leave room for
//                   more workgroups per CU), the class map (256 B) and the tile's stage (4 368 B:
//                   the tile and the 255 bytes behind it as class ids, findrx_core.h) sit in LDS.
//                   A thread walks its 16 positions for every expression: a step is one LDS read
//                   of a class id and one dependent LDS read of the table.  On text nearly every
//                   walk is dead after the first step.
//   k_findrx_emit   tiles [t0, t0 + grid): as k_find_emit.
// Loads: aligned 16-byte words that hold a byte of [buf, buf + n), as in k_find.hip.
// The device image of an automaton: the class map, then the table in whole 16-byte words.
#include "kolm_internal.h"
#include "findrx_core.h"
#include "find_tile.h"

namespace kolm {

namespace {

// the automaton and the stage of `tile` into LDS
__device__ __forceinline__ void load_tile(const u8* __restrict__ buf, u32 n, u32 mis, u32 tile, const u8* __restrict__ img,
                                          u32 words, uint16_t* s_T, u8* s_cls, u8* s_stage) {
    const u32 tid = threadIdx.x;
    const uint4* g = reinterpret_cast<const uint4*>(img);
    if (tid < frx::MAP / 16) reinterpret_cast<uint4*>(s_cls)[tid] = g[tid];
    for (u32 x = tid; x < words; x += fnd::WG) reinterpret_cast<uint4*>(s_T)[x] = g[frx::MAP / 16 + x];
    __syncthreads();
    ftl::DevLd ld{buf};
    for (u32 w = tid; w < frx::STAGE_WORDS; w += fnd::WG) {
        u32 o[4];
        frx::stage_word(ld, mis, tile, w, n, s_cls, o);
        reinterpret_cast<uint4*>(s_stage)[w] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
}

__global__ __launch_bounds__(fnd::WG) void k_findrx_count(const u8* __restrict__ buf, u32 n, u32 lo, u32 shi,
                                                          const u8* __restrict__ img, u32 words, u32 ncls, frx::Starts st,
                                                          u32 np, u32 ntiles, u32* __restrict__ cnt) {
    extern __shared__ __align__(16) uint16_t s_T[];  // frx::padded_entries(nstates, ncls) entries
    __shared__ __align__(16) u8 s_cls[frx::MAP];
    __shared__ __align__(16) u8 s_stage[frx::STAGE_BYTES];
    const u32 tile = blockIdx.x, mis = ftl::misalign(buf);
    load_tile(buf, n, mis, tile, img, words, s_T, s_cls, s_stage);
    const u32 p0 = ftl::first_pos(tile);
    const u8* sc = s_stage + mis + threadIdx.x * fnd::PER;
    ftl::tile_count(np, ntiles, tile, cnt, [&](u32 i) { [[clang::always_inline]] return frx::match_mask(s_T, ncls, sc, p0, lo, shi, n, st.s[i]); });
}

__global__ __launch_bounds__(fnd::WG) void k_findrx_emit(const u8* __restrict__ buf, u32 n, u32 lo, u32 shi,
                                                         const u8* __restrict__ img, u32 words, u32 ncls, frx::Starts st,
                                                         u32 np, u32 t0, const u64* __restrict__ tscan,
                                                         u32* __restrict__ out_pos, u8* __restrict__ out_which, u32 cap) {
    extern __shared__ __align__(16) uint16_t s_T[];  // frx::padded_entries(nstates, ncls) entries
    __shared__ __align__(16) u8 s_cls[frx::MAP];
    __shared__ __align__(16) u8 s_stage[frx::STAGE_BYTES];
    const u32 tile = t0 + blockIdx.x, mis = ftl::misalign(buf);
    load_tile(buf, n, mis, tile, img, words, s_T, s_cls, s_stage);
    const u32 p0 = ftl::first_pos(tile);
    const u8* sc = s_stage + mis + threadIdx.x * fnd::PER;
    ftl::tile_emit(np, tile, t0, tscan, out_pos, out_which, cap,
                   [&](u32 i) { [[clang::always_inline]] return frx::match_mask(s_T, ncls, sc, p0, lo, shi, n, st.s[i]); });
}

}  // namespace

void launch_findrx_count(const u8* buf, u32 n, u32 lo, u32 shi, const u8* img, u32 nstates, u32 ncls,
                         const frx::Starts& st, u32 np, u32* cnt, hipStream_t s) {
    const u32 ntiles = fnd::tiles(n), entries = frx::padded_entries(nstates, ncls);
    if (ntiles)
        k_findrx_count<<<ntiles, fnd::WG, entries * sizeof(uint16_t), s>>>(buf, n, lo, shi, img, entries / 8, ncls, st, np,
                                                                           ntiles, cnt);
}

void launch_findrx_emit(const u8* buf, u32 n, u32 lo, u32 shi, const u8* img, u32 nstates, u32 ncls, const frx::Starts& st,
                        u32 np, u32 t0, u32 t1, const u64* tscan, u32* out_pos, u8* out_which, u32 cap, hipStream_t s) {
    const u32 entries = frx::padded_entries(nstates, ncls);
    if (t1 > t0)
        k_findrx_emit<<<t1 - t0, fnd::WG, entries * sizeof(uint16_t), s>>>(buf, n, lo, shi, img, entries / 8, ncls, st, np, t0,
                                                                          tscan, out_pos, out_which, cap);
}

}  // namespace kolm
