// Verify-after-encode on gfx950: the decoded batch against the original, both resident.
//   k_verify_cmp   streams the two buffers once (2 * total bytes, nothing written on the equal
//                  path): a grid of at most 2048 workgroups strides over tiles of 1024 aligned
//                  16-byte words, every lane holding 4 independent word pairs (8 loads) in
//                  flight.  The buffers are congruent mod 16 (the caller places the decode
//                  scratch that way), so one head / body / tail split (verify_core.h) aligns
//                  both; the head and the tail (< 16 bytes each) are compared byte by byte by
//                  workgroup 0.  A wave whose 256 word pairs are all equal — one __any on the
//                  ORed xors — goes on to its next tile; otherwise the lanes that saw a
//                  difference attribute their differing bytes to blocks (binary search in the
//                  nb + 1 bounds, one candidate per block and word) and lower first_bad[block]
//                  with atomicMin, skipped when the word there is already no larger: a buffer
//                  that differs everywhere settles each block's word after a few atomics and
//                  then only reads it.
//   k_verify_flip  the test switch KOLM_VERIFY_INJECT: xors 0x80 into one payload byte.
// No load touches a byte outside [0, total) of either buffer: words beyond the body are
// not loaded (their lanes compare zeros).
#include "kolm_internal.h"
#include "verify_core.h"

namespace kolm {

namespace {

struct DevMin {
    u32* fb;
    __device__ void operator()(u32 b, u32 off) {
        if (__atomic_load_n(fb + b, __ATOMIC_RELAXED) > off) atomicMin(fb + b, off);
    }
};

__global__ __launch_bounds__(vfy::WG) void k_verify_cmp(const u8* __restrict__ a, const u8* __restrict__ b, u32 total,
                                                        u32 mis, const u32* __restrict__ bounds, u32 nb, u32* fb) {
    const vfy::Split sp = vfy::split(mis, total);
    const u32 tid = threadIdx.x;
    DevMin amin{fb};
    if (blockIdx.x == 0 && tid < 2 * vfy::WORD) {  // lanes 0..15: the head, 16..31: the tail
        const bool tl = tid >= vfy::WORD;
        const u32 j = tid & (vfy::WORD - 1);
        const u32 pos = tl ? sp.head + sp.words * vfy::WORD + j : j;
        if (j < (tl ? sp.tail : sp.head) && a[pos] != b[pos]) vfy::attribute(bounds, nb, pos, 1u, amin);
    }
    const uint4* aw = reinterpret_cast<const uint4*>(a + sp.head);
    const uint4* bw = reinterpret_cast<const uint4*>(b + sp.head);
    const u32 ntiles = vfy::tiles(sp.words);
    for (u32 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const u32 w0 = t * vfy::TILE_WORDS + tid;
        uint4 xa[vfy::UNROLL], xb[vfy::UNROLL];
#pragma unroll
        for (u32 k = 0; k < vfy::UNROLL; ++k) {
            const u32 w = w0 + k * vfy::WG;
            xa[k] = xb[k] = make_uint4(0, 0, 0, 0);
            if (w < sp.words) {
                xa[k] = aw[w];
                xb[k] = bw[w];
            }
        }
        u32 d = 0;
#pragma unroll
        for (u32 k = 0; k < vfy::UNROLL; ++k)
            d |= (xa[k].x ^ xb[k].x) | (xa[k].y ^ xb[k].y) | (xa[k].z ^ xb[k].z) | (xa[k].w ^ xb[k].w);
        if (!__any(d != 0)) continue;  // the whole wave equal: no lookup, no atomic
        if (d == 0) continue;
#pragma unroll
        for (u32 k = 0; k < vfy::UNROLL; ++k) {
            const u32 wa[4] = {xa[k].x, xa[k].y, xa[k].z, xa[k].w};
            const u32 wb[4] = {xb[k].x, xb[k].y, xb[k].z, xb[k].w};
            if (vfy::word_diff(wa, wb) == 0) continue;
            vfy::attribute(bounds, nb, sp.head + (w0 + k * vfy::WG) * vfy::WORD, vfy::byte_mask(wa, wb), amin);
        }
    }
}

__global__ void k_verify_flip(u8* p) { *p ^= 0x80; }

}  // namespace

void launch_verify_cmp(const u8* dec, const u8* orig, u32 total, const u32* bounds, u32 nb, u32* first_bad,
                       hipStream_t s) {
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(orig) & (vfy::WORD - 1));
    const vfy::Split sp = vfy::split(mis, total);
    k_verify_cmp<<<vfy::grid_for(sp.words), vfy::WG, 0, s>>>(dec, orig, total, mis, bounds, nb, first_bad);
}

void launch_verify_flip(u8* p, hipStream_t s) { k_verify_flip<<<1, 1, 0, s>>>(p); }

}  // namespace kolm
