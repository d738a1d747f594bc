// Line index on gfx950 (lines_core.h): the delimiter counts of a resident batch's blocks, and rank /
// select queries against them.  Ordered by launch boundaries only: no spinning, no tickets.
//   k_delim_count  the items, runs and grid of k_block_fp / k_crc32: items are (block, 4 KiB piece),
//                  a wave takes a run of up to 8 consecutive pieces of one block and the waves of a
//                  grid of at most 2048 workgroups stride over the runs.  A lane takes words l,
//                  l + 64, l + 128, l + 192 of every piece through load_words (no byte outside the
//                  batch is touched; the bytes of a block's last word past its end are zero and are
//                  masked out of the count: delimiter 0x00).  Per piece one popcount per word and one
//                  wave reduction; lane 0 stores the piece's count to pcnt[pbase[block] + piece]
//                  (pcnt may be null: counts only) and adds the run's sum to cnt[block] (zeroed by
//                  the caller on the same stream) with one atomicAdd.  Integer add commutes: the
//                  words do not depend on how the runs meet the waves.  No LDS.
//   (scan)         the exclusive scan of pcnt over the whole group is launch_find_scan (k_find.hip)
//                  with np = 0: one u32 column in, a u64 scan with the total behind it out.  The
//                  delimiters before piece k of block b are pscan[pbase[b] + k] - pscan[pbase[b]].
//   k_delim_query  one wave per query, grid-stride.  RANK(b, off): the scanned count of the pieces
//                  below off plus the partial count of the one piece that holds it.  SELECT(b, j):
//                  a binary search of the block's scanned piece counts names the piece, its four
//                  word rows' totals name the row, a wave scan in lane order names the word and
//                  lin::select the byte.  j at or above the block's count gives lin::NONE.  A query
//                  reads at most one 4 KiB piece of text; its result is one u32 vector store.
// Blocks are addressed through Geom (base / end only).  A run finds its block by division when
// every block has the same run count (fixed geometry: scan == null) and otherwise by binary
// search in the exclusive scan of the per-block run counts; an empty block has no run.
#include "kolm_internal.h"
#include "lines_core.h"
#include "load_words.h"

namespace kolm {

namespace {

__global__ __launch_bounds__(ddp::WG) void k_delim_count(const u8* __restrict__ text, Geom geo,
                                                         const u32* __restrict__ scan, u32 rpb, u64 nruns, u32 delim,
                                                         const u32* __restrict__ pbase, u32* __restrict__ pcnt,
                                                         u32* __restrict__ cnt) {
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
        u32 sum = 0;  // wave-uniform
        for (u32 k = r * ddp::RUN; k < k1; ++k) {
            const ddp::Piece pc = ddp::piece(len, k);
            Words x;
            load_words(text + base + pc.o0, pc, t0, t1, lane, x);
            u32 c = 0;
#pragma unroll
            for (u32 u = 0; u < ddp::UNROLL; ++u) {
                const u32 w = lin::word_of(lane, u);
                if (w < pc.words) c += lin::count(lin::word_mask(x.w0[u], x.w1[u], delim, pc, w));
            }
            const u32 pc_total = wave_reduce(c, OpAddU(), 0u);
            if (pcnt && lane == 0) pcnt[pbase[b] + k] = pc_total;
            sum += pc_total;
        }
        if (lane == 0 && sum) atomicAdd(cnt + b, sum);
    }
}

__global__ __launch_bounds__(ddp::WG) void k_delim_query(const u8* __restrict__ text, Geom geo, u32 delim,
                                                         const u32* __restrict__ pbase, const u64* __restrict__ pscan,
                                                         const lin::Query* __restrict__ q, u32 nq, u32* __restrict__ res) {
    const u32 lane = threadIdx.x & (ddp::WAVE - 1);
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x / ddp::WAVE);
    const u32 stride = gridDim.x * (ddp::WG / ddp::WAVE);
    const u64 t0 = reinterpret_cast<uintptr_t>(text), t1 = t0 + geo.N;
    for (u32 i = blockIdx.x * (ddp::WG / ddp::WAVE) + wave; i < nq; i += stride) {
        const u32 b = q[i].block, arg = q[i].arg, op = q[i].op;  // wave-uniform
        if (b >= geo.nb) {
            if (lane == 0) res[i] = lin::NONE;
            continue;
        }
        const u32 base = geo.base(b);
        const u64 len = geo.end(b) - base;
        const u32 np = (u32)ddp::pieces(len);
        const u64* ps = pscan + pbase[b];  // ps[0 .. np]: np + 1 entries (the next block's first, or the total)
        const u64 s0 = ps[0];
        if (op == lin::OP_RANK) {
            if (arg > len) {
                if (lane == 0) res[i] = lin::NONE;
                continue;
            }
            const u32 k = arg / ddp::ITEM, r = arg % ddp::ITEM;
            u32 v = (u32)(ps[k] - s0);  // k <= np
            if (r) {                    // then k < np: byte k ITEM + r - 1 lies in the block
                const ddp::Piece pc = ddp::piece(len, k);
                Words x;
                load_words(text + base + pc.o0, pc, t0, t1, lane, x);
                u32 c = 0;
#pragma unroll
                for (u32 u = 0; u < ddp::UNROLL; ++u) {
                    const u32 w = lin::word_of(lane, u);
                    if (w < pc.words) c += lin::word_rank(lin::word_mask(x.w0[u], x.w1[u], delim, pc, w), w, r);
                }
                v += wave_reduce(c, OpAddU(), 0u);
            }
            if (lane == 0) res[i] = v;
            continue;
        }
        // SELECT: the piece with (delimiters before it) <= arg < (delimiters through it)
        if ((u64)arg >= ps[np] - s0) {
            if (lane == 0) res[i] = lin::NONE;
            continue;
        }
        u32 lo = 0, n = np;  // largest k < np with ps[k] - s0 <= arg
        while (n > 1) {
            const u32 half = n >> 1;
            if (ps[lo + half] - s0 <= arg) lo += half;
            n -= half;
        }
        u32 j = arg - (u32)(ps[lo] - s0);  // the piece's j-th delimiter
        const ddp::Piece pc = ddp::piece(len, lo);
        Words x;
        load_words(text + base + pc.o0, pc, t0, t1, lane, x);
        u32 m[ddp::UNROLL], tot[ddp::UNROLL];
#pragma unroll
        for (u32 u = 0; u < ddp::UNROLL; ++u) {
            const u32 w = lin::word_of(lane, u);
            m[u] = w < pc.words ? lin::word_mask(x.w0[u], x.w1[u], delim, pc, w) : 0u;
            tot[u] = wave_reduce(lin::count(m[u]), OpAddU(), 0u);
        }
        u32 row = ddp::UNROLL, mine = 0;  // rows in position order; the row's masks in `mine`
#pragma unroll
        for (u32 u = 0; u < ddp::UNROLL; ++u) {
            if (row == ddp::UNROLL) {
                if (j < tot[u]) row = u, mine = m[u];
                else j -= tot[u];
            }
        }
        const u32 c = lin::count(mine);
        const u32 incl = wave_incl_scan(c, OpAddU(), 0u);
        const bool hit = row < ddp::UNROLL && incl - c <= j && j < incl;  // one lane
        if (hit) res[i] = (u32)pc.o0 + lin::word_of(lane, row) * ddp::WORD + lin::select(mine, j - (incl - c));
        if (__ballot(hit) == 0 && lane == 0) res[i] = lin::NONE;  // the scanned counts and the text disagree
    }
}

}  // namespace

void launch_delim_count(const u8* text, const Geom& geo, const u32* scan, u64 nruns, u32 delim, const u32* pbase, u32* pcnt,
                        u32* cnt, hipStream_t s) {
    if (geo.nb == 0 || nruns == 0) return;
    const u32 rpb = (u32)ddp::runs(geo.bs);  // fixed geometry: runs per block
    k_delim_count<<<ddp::grid_for(nruns), ddp::WG, 0, s>>>(text, geo, scan, rpb ? rpb : 1, nruns, delim, pbase, pcnt, cnt);
}

void launch_delim_query(const u8* text, const Geom& geo, u32 delim, const u32* pbase, const u64* pscan, const lin::Query* q,
                        u32 nq, u32* res, hipStream_t s) {
    if (geo.nb == 0 || nq == 0) return;
    k_delim_query<<<ddp::grid_for(nq), ddp::WG, 0, s>>>(text, geo, delim, pbase, pscan, q, nq, res);
}

}  // namespace kolm
