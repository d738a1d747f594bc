// Search of a resident buffer for regular expressions on gfx950 (findrx_core.h): every start of up
// to 16 expressions, compiled to one deterministic automaton, counted and listed in (position,
// expression) order.  The tile geometry, the count columns, k_find_scan between the two kernels
// and the record slots are k_find.hip's; ordering is by launch boundaries only: no spinning, no
// tickets, no atomics.
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

namespace kolm {

namespace {

struct DevLd {
    const u8* buf;
    __device__ __forceinline__ fnd::Word operator()(fnd::i64 off) const {
        const uint4 v = *reinterpret_cast<const uint4*>(buf + off);
        return fnd::Word{{(u64)v.x | ((u64)v.y << 32), (u64)v.z | ((u64)v.w << 32)}};
    }
};

// the automaton and the stage of `tile` into LDS
__device__ __forceinline__ void load_tile(const u8* __restrict__ buf, u32 n, u32 mis, u32 tile, const u8* __restrict__ img,
                                          u32 words, uint16_t* s_T, u8* s_cls, u8* s_stage) {
    const u32 tid = threadIdx.x;
    const uint4* g = reinterpret_cast<const uint4*>(img);
    if (tid < frx::MAP / 16) reinterpret_cast<uint4*>(s_cls)[tid] = g[tid];
    for (u32 x = tid; x < words; x += fnd::WG) reinterpret_cast<uint4*>(s_T)[x] = g[frx::MAP / 16 + x];
    __syncthreads();
    DevLd ld{buf};
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
    __shared__ u32 s_c[fnd::WG / 64][fnd::MAX_PATTERNS + 1];
    const u32 tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(buf) & (fnd::WORD - 1));
    load_tile(buf, n, mis, tile, img, words, s_T, s_cls, s_stage);
    const u32 p0 = tile * fnd::TILE + threadIdx.x * fnd::PER;
    const u8* sc = s_stage + mis + threadIdx.x * fnd::PER;
    u32 total = 0;
    for (u32 i = 0; i < np; ++i) {
        const u32 m = frx::match_mask(s_T, ncls, sc, p0, lo, shi, n, st.s[i]);
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

__global__ __launch_bounds__(fnd::WG) void k_findrx_emit(const u8* __restrict__ buf, u32 n, u32 lo, u32 shi,
                                                         const u8* __restrict__ img, u32 words, u32 ncls, frx::Starts st,
                                                         u32 np, u32 t0, const u64* __restrict__ tscan,
                                                         u32* __restrict__ out_pos, u8* __restrict__ out_which, u32 cap) {
    extern __shared__ __align__(16) uint16_t s_T[];  // frx::padded_entries(nstates, ncls) entries
    __shared__ __align__(16) u8 s_cls[frx::MAP];
    __shared__ __align__(16) u8 s_stage[frx::STAGE_BYTES];
    __shared__ uint16_t s_pm[fnd::MAX_PATTERNS][fnd::WG];
    __shared__ u32 s_w[fnd::WG / 64];
    const u32 tile = t0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(buf) & (fnd::WORD - 1));
    load_tile(buf, n, mis, tile, img, words, s_T, s_cls, s_stage);
    const u32 p0 = tile * fnd::TILE + tid * fnd::PER;
    const u8* sc = s_stage + mis + tid * fnd::PER;
    u32 any = 0, c = 0;
    for (u32 i = 0; i < np; ++i) {
        const u32 m = frx::match_mask(s_T, ncls, sc, p0, lo, shi, n, st.s[i]);
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
    while (any) {  // the thread's own masks: positions ascending, expressions ascending within one
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
