// The block-relative 16-byte words of one item (dedup_core.h), as the kernels that stream a batch
// block by block read them: k_block_fp and k_dedup_cmp (k_dedup.hip), k_crc32 (k_crc.hip), and
// k_delim_count and k_delim_query (k_lines.hip).
// Loads: aligned 16-byte words that lie inside the batch [t0, t1) whole; the words at the batch's
// two ends whose aligned neighbours would leave it are read byte by byte.  No load touches a byte
// outside the batch.  Bytes of a word past the block's end are zero.
#pragma once
#include "kolm_internal.h"
#include "dedup_core.h"

namespace kolm {

// The words of one item of the block at p0 (= the piece's first byte): lane's word u is piece
// word lane + 64 u.  Phase 1 issues every aligned load (predicated: lanes past the piece's end
// and the words at the batch's ends load nothing), phase 2 forms the words.
struct Words {
    u64 w0[ddp::UNROLL], w1[ddp::UNROLL];
};

// Q = the whole 32-bit words of the block's misalignment sh (compile time, so the funnel's register
// indices are static), sh = 4 Q + 0..3 (wave-uniform).  ALL = every aligned word the item needs lies
// inside the batch (ddp::item_fast, wave-uniform: all items but the few at the batch's ends): the
// per-word test and the byte path drop out of the body.
template <u32 Q, bool ALL>
__device__ __forceinline__ void load_words_q(const u8* p0, const ddp::Piece& pc, u64 t0, u64 t1, u32 lane, u32 sh,
                                             Words& out) {
    uint4 xa[ddp::UNROLL], xb[ddp::UNROLL];
    bool fs[ddp::UNROLL];
#pragma unroll
    for (u32 u = 0; u < ddp::UNROLL; ++u) {
        const u32 w = lane + u * ddp::WAVE;
        const u8* p = p0 + (u64)w * ddp::WORD;
        fs[u] = w < pc.words && (ALL || ddp::fast(reinterpret_cast<uintptr_t>(p), sh, t0, t1));
        xa[u] = xb[u] = make_uint4(0, 0, 0, 0);
        if (fs[u]) {
            const uint4* sw = reinterpret_cast<const uint4*>(p - sh);
            xa[u] = sw[0];
            if (sh) xb[u] = sw[1];
        }
    }
#pragma unroll
    for (u32 u = 0; u < ddp::UNROLL; ++u) {
        const u32 w = lane + u * ddp::WAVE;
        const u32 nv = w < pc.words ? ddp::word_bytes(pc, w) : 0;
        const u32 a[4] = {xa[u].x, xa[u].y, xa[u].z, xa[u].w};
        const u32 b[4] = {xb[u].x, xb[u].y, xb[u].z, xb[u].w};
        u32 o[4];
        rng::src_word(a, b, 4 * Q + (sh & 3u), o);  // zeros where nothing was loaded
        u64 w0 = (u64)o[0] | (u64)o[1] << 32, w1 = (u64)o[2] | (u64)o[3] << 32;
        if (!ALL && nv && !fs[u]) {  // a word at one of the batch's ends: its own bytes, one by one
            const u8* p = p0 + (u64)w * ddp::WORD;
            for (u32 i = 0; i < (nv < 8 ? nv : 8); ++i) w0 |= (u64)p[i] << (8 * i);
            for (u32 i = 8; i < nv; ++i) w1 |= (u64)p[i] << (8 * (i - 8));
        }
        if (nv) ddp::mask(w0, w1, nv);
        out.w0[u] = nv ? w0 : 0;
        out.w1[u] = nv ? w1 : 0;
    }
}

__device__ __forceinline__ void load_words(const u8* p0, const ddp::Piece& pc, u64 t0, u64 t1, u32 lane, Words& out) {
    const u32 sh = __builtin_amdgcn_readfirstlane((u32)(reinterpret_cast<uintptr_t>(p0) & (ddp::WORD - 1)));
    if (ddp::item_fast(reinterpret_cast<uintptr_t>(p0), sh, pc.words, t0, t1)) {
        if (sh < 4) load_words_q<0, true>(p0, pc, t0, t1, lane, sh, out);
        else if (sh < 8) load_words_q<1, true>(p0, pc, t0, t1, lane, sh, out);
        else if (sh < 12) load_words_q<2, true>(p0, pc, t0, t1, lane, sh, out);
        else load_words_q<3, true>(p0, pc, t0, t1, lane, sh, out);
    } else {
        if (sh < 4) load_words_q<0, false>(p0, pc, t0, t1, lane, sh, out);
        else if (sh < 8) load_words_q<1, false>(p0, pc, t0, t1, lane, sh, out);
        else if (sh < 12) load_words_q<2, false>(p0, pc, t0, t1, lane, sh, out);
        else load_words_q<3, false>(p0, pc, t0, t1, lane, sh, out);
    }
}

}  // namespace kolm
