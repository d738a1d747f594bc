// Candidate 10 (v2_new) decoded on gfx950: decode_new_pipeline PY:1578-1648 with the automaton
// inverse PY:1056-1092.  The integer core is csrc/v2_decode_core.h (shared with the CPU
// emulation tools/v2_decode_emu.cpp).  A block's 8 bit planes live in 8 consecutive "plane
// blocks" of the block's length (plane pb = 8 * list index + j at pbase[pb]); every grid is
// sized for 8 encoded planes per block and a raw / failed plane exits early (pstat != 0), so
// nothing is read back before the launches.
//
//   1. k_v2d_parse    one workgroup per block: header, then the planes in order (their byte
//                     boundaries are data-dependent).  A raw plane only records its payload
//                     offset.  An encoded plane is walked in tiles of 256 64-bit words, one word
//                     per thread: phase functions composed by a workgroup scan, trailing ones
//                     joined by a segmented sum, values scanned into cumulative positions, run
//                     starts marked in the plane's L array; the walk stops where the sum reaches
//                     n and the next plane starts at the next byte.  Loops: planes x tiles of
//                     the payload x 64 bits of a word — bounded by the payload size whatever it
//                     holds; a sum that never reaches n ends at the payload's last tile.
//   2. k_v2d_chunkpar / k_v2d_fill   marks -> L: parity of the marks up to each position
//                     (4 KiB chunks: chunk parities, then prefix + in-chunk scan), ^ first bit.
//   3. launch_bwi     the inverse BBWT kernels of k_decode.hip over the plane blocks.
//   4. k_v2d_pack     grid-wide, one thread per 8 positions: the 8 planes packed into mapped
//                     bytes (raw planes straight from the payload) in the block's output range.
//   5. k_v2d_auto     (one launch over every id-10 block of the batch, after the scratch groups)
//                     one workgroup per block, in place over 4 KiB tiles in LDS: the automaton
//                     inverse: modes 1 and 3 as strided prefix-XOR scans (strides up to 16: a
//                     16-byte chunk per thread scanned in registers, the chunks' last d bytes
//                     XOR-scanned over the workgroup and carried over the tiles; longer strides:
//                     doubling in LDS, the carry from the bytes already written), modes 2, 4 and 5 walked by one lane
//                     over the LDS tile (the recurrence is serial per block; blocks run
//                     concurrently), everything else the identity.
// A malformed block sets its status and its planes' pstat; later stages skip it.
#include "kolm_internal.h"
#include "v2_decode_core.h"

namespace kolm {

namespace {

constexpr u32 PW = 256;                  // threads of the per-block workgroups
constexpr u32 FCH = V2D_CHUNK;           // positions per mark chunk (16 per thread)

// inclusive scan over the workgroup's 256 threads in thread order (op(a, b): a precedes b);
// sh = 2 x 256 elements.  excl = the value before this thread (ident for thread 0).
template <class T, class Op>
__device__ inline T wg_scan(T v, T* sh, Op op, T ident, T& excl, T& total) {
    const u32 t = threadIdx.x;
    u32 cur = 0;
    sh[t] = v;
    __syncthreads();
    for (u32 s = 1; s < PW; s <<= 1) {
        T x = sh[cur * PW + t];
        if (t >= s) x = op(sh[cur * PW + t - s], x);
        sh[(cur ^ 1) * PW + t] = x;
        cur ^= 1;
        __syncthreads();
    }
    const T incl = sh[cur * PW + t];
    excl = t ? sh[cur * PW + t - 1] : ident;
    total = sh[cur * PW + PW - 1];
    __syncthreads();
    return incl;
}

struct CntSum {
    u64 sum;
    u32 cnt;
    u32 pad;
};

__global__ __launch_bounds__(PW) void k_v2d_parse(V2dArgs a) {
    __shared__ u64 shf[2 * PW];
    __shared__ v2d::Ones sho[2 * PW];
    __shared__ CntSum shc[2 * PW];
    __shared__ v2d::Header hd;
    __shared__ u32 s_ok, s_bad, s_done;
    __shared__ u64 s_end;
    const u32 li = blockIdx.x, tid = threadIdx.x;
    const u32 b = a.d.list[li];
    const u64 p0 = a.d.poff[b], plen = a.d.poff[b + 1] - p0;
    const u32 n = a.d.obase[b + 1] - a.d.obase[b];
    const u8* p = a.d.pay + p0;
    if (tid == 0) s_ok = n && v2d::parse_header(p, plen, hd) ? 1u : 0u;
    __syncthreads();
    if (!s_ok) {  // empty block (nothing to write) or malformed header
        if (tid < 8) a.pstat[8 * li + tid] = 1;
        if (tid == 0 && n) a.d.status[b] = DEC_EFORMAT;
        return;
    }
    u64 pos = hd.data;
    u32 ki = 0;
    bool ok = true;
    for (u32 j = 0; j < 8 && ok; ++j) {
        if ((hd.raw_mask >> j) & 1u) {  // PY:1611-1617
            const u64 need = ((u64)n + 7) / 8;
            if (pos + need > plen) {
                ok = false;
                break;
            }
            if (tid == 0) a.info[V2D_INFO * li + 4 + j] = (u32)pos;
            pos += need;
            continue;
        }
        const u32 k = hd.k[ki++];
        u8* L = a.L + a.pbase[8 * li + j];
        u32 ph = 0, runs = 0;
        u64 pend = 0, cum = 0;
        for (u64 B0 = pos;; B0 += v2d::TILE_BYTES) {  // <= plen / TILE_BYTES + 1 tiles
            if (tid == 0) {
                s_bad = 0;
                s_done = 0;
            }
            const u64 B = B0 + 8ull * tid;
            u32 nv;
            const u64 w = v2d::load_word(p, plen, B, nv);
            u64 fex, ftot;
            wg_scan(v2d::phase_fn(w, nv, k), shf, [](u64 x, u64 y) { return v2d::phase_compose(x, y); }, v2d::PHASE_ID,
                    fex, ftot);
            const u32 e = v2d::phase_apply(fex, ph);
            const v2d::WordSum ws = v2d::word_summary(p, plen, B, w, nv, e, k);
            v2d::Ones oex, otot;
            wg_scan(ws.ones, sho, [](v2d::Ones x, v2d::Ones y) { return v2d::ones_join(x, y); }, v2d::Ones{0, 1, 0}, oex,
                    otot);
            const u64 carry = oex.tail + (oex.whole ? pend : 0);
            CntSum cex, ctot;
            wg_scan(CntSum{ws.lsum + (ws.joins ? carry << k : 0), ws.cnt, 0}, shc,
                    [](CntSum x, CntSum y) { return CntSum{x.sum + y.sum, x.cnt + y.cnt, 0}; }, CntSum{0, 0, 0}, cex, ctot);
            if (ws.cnt && cum + cex.sum < n) {
                const v2d::Emit em = v2d::word_emit(p, plen, B, w, nv, e, k, carry, cum + cex.sum, runs + cex.cnt, n,
                                                    [&](u32 at) { L[at] = 1; });
                if (em.bad) s_bad = 1;
                if (em.done) {
                    s_done = 1;
                    s_end = em.endbit;
                }
            }
            __syncthreads();
            const bool bad = s_bad, done = s_done;
            const u64 end = s_end;
            __syncthreads();
            if (bad || (!done && B0 + v2d::TILE_BYTES >= plen)) {  // PY: bad value / overrun / out of data
                ok = false;
                break;
            }
            if (done) {
                pos = (end + 7) / 8;
                break;
            }
            ph = v2d::phase_apply(ftot, ph);
            pend = otot.tail + (otot.whole ? pend : 0);
            cum += ctot.sum;
            runs += ctot.cnt;
        }
    }
    if (tid < 8) a.pstat[8 * li + tid] = ok && !((hd.raw_mask >> tid) & 1u) ? 0u : 1u;
    if (tid == 0) {
        if (!ok) a.d.status[b] = DEC_EFORMAT;
        a.info[V2D_INFO * li + 0] = hd.mode;
        a.info[V2D_INFO * li + 1] = hd.param;
        a.info[V2D_INFO * li + 2] = hd.raw_mask;
        a.info[V2D_INFO * li + 3] = hd.b1_mask;
    }
}

// parity of the marks of each chunk of each encoded plane
__global__ __launch_bounds__(PW) void k_v2d_chunkpar(V2dArgs a) {
    const u32 pb = blockIdx.y;
    if (a.pstat[pb]) return;
    const u32 o0 = a.pbase[pb], n = a.pbase[pb + 1] - o0;
    const u32 lo = blockIdx.x * FCH;
    if (lo >= n) return;
    const u32 hi = min(lo + FCH, n);
    u32 par = 0;
    for (u32 i = lo + threadIdx.x; i < hi; i += PW) par ^= a.L[o0 + i];
    const u32 c = __syncthreads_count(par & 1u);
    if (threadIdx.x == 0) a.cpar[(u64)pb * a.tpc + blockIdx.x] = c & 1u;
}

// L[i] = first bit ^ parity of the marks in [0, i]  (runs alternate, PY:1629-1637)
__global__ __launch_bounds__(PW) void k_v2d_fill(V2dArgs a) {
    __shared__ u32 wpar[PW / 64];
    const u32 pb = blockIdx.y, tid = threadIdx.x;
    if (a.pstat[pb]) return;
    const u32 o0 = a.pbase[pb], n = a.pbase[pb + 1] - o0;
    const u32 lo = blockIdx.x * FCH;
    if (lo >= n) return;
    u32 pre = 0;
    for (u32 c = tid; c < blockIdx.x; c += PW) pre ^= a.cpar[(u64)pb * a.tpc + c];
    const u32 before = __syncthreads_count(pre & 1u) & 1u;
    const u32 first = (a.info[V2D_INFO * (pb >> 3) + 3] >> (pb & 7)) & 1u;
    u8* L = a.L + o0;
    const u32 i0 = lo + tid * (FCH / PW);
    u32 m[FCH / PW], lp = 0;
#pragma unroll
    for (u32 q = 0; q < FCH / PW; ++q) {
        m[q] = i0 + q < n ? L[i0 + q] : 0u;
        lp ^= m[q];
    }
    const u64 bal = __ballot(lp & 1u);
    const u32 lane = tid & 63, wv = tid >> 6;
    if (lane == 0) wpar[wv] = __popcll(bal) & 1u;
    __syncthreads();
    u32 run = first ^ before ^ (__popcll(bal & ((1ull << lane) - 1ull)) & 1u);
    for (u32 q = 0; q < wv; ++q) run ^= wpar[q];
#pragma unroll
    for (u32 q = 0; q < FCH / PW; ++q) {
        run ^= m[q];
        if (i0 + q < n) L[i0 + q] = (u8)run;
    }
}

// 4. pack, grid-wide: one thread per 8 positions.  Plane j gives bit 7 - j of every mapped
// byte (PY:1639); a raw plane is read straight from the payload (one byte = 8 positions), an
// encoded plane from its 0/1 bytes after the inverse BBWT.  The mapped bytes go to the block's
// output range, where the automaton inverse then works in place.
__global__ __launch_bounds__(PW) void k_v2d_pack(V2dArgs a) {
    const u32 li = blockIdx.y;
    const u32 b = a.d.list[li];
    const u32 o0 = a.d.obase[b], n = a.d.obase[b + 1] - o0;
    const u32 i0 = (blockIdx.x * PW + threadIdx.x) * 8;
    if (i0 >= n || a.d.status[b] != DEC_OK) return;
    const u32* info = a.info + V2D_INFO * li;
    const u32 raw_mask = info[2];
    const u8* p = a.d.pay + a.d.poff[b];
    const u32 m = min(8u, n - i0);
    u64 y = 0;  // byte q = mapped byte i0 + q
#pragma unroll
    for (u32 j = 0; j < 8; ++j) {
        u64 w = 0;  // byte q = the plane's bit at i0 + q
        if ((raw_mask >> j) & 1u) {
            const u32 rb = p[info[4 + j] + (i0 >> 3)];
#pragma unroll
            for (u32 q = 0; q < 8; ++q) w |= (u64)((rb >> (7 - q)) & 1u) << (8 * q);
        } else {
            const u8* u = a.U + a.pbase[8 * li + j] + i0;
            if (m == 8 && !(reinterpret_cast<uintptr_t>(u) & 7)) {
                w = *reinterpret_cast<const u64*>(u) & 0x0101010101010101ull;
            } else {
                for (u32 q = 0; q < m; ++q) w |= (u64)(u[q] & 1u) << (8 * q);
            }
        }
        y |= w << (7 - j);
    }
    u8* out = a.d.out + o0 + i0;
    if (m == 8 && !(reinterpret_cast<uintptr_t>(out) & 7)) {
        *reinterpret_cast<u64*>(out) = y;
    } else {
        for (u32 q = 0; q < m; ++q) out[q] = (u8)(y >> (8 * q));
    }
}

// r[i] = v[i] ^ (r[i - d] & mask) over the tile in A (global offset g0, m bytes): the first d
// positions take the carry from the bytes already written, then log2(m / d) doubling steps.
__device__ inline u8* tile_xor_scan(u8* A, u8* B, const u8* out, u32 g0, u32 m, u32 d, u32 mask) {
    const u32 tid = threadIdx.x;
    for (u32 i = tid; i < m && i < d; i += PW)
        if (g0 + i >= d) A[i] ^= out[g0 + i - d] & mask;
    __syncthreads();
    for (u64 s = d; s < m; s <<= 1) {
        for (u32 i = tid; i < m; i += PW) B[i] = A[i] ^ (i >= s ? A[i - (u32)s] & mask : 0u);
        __syncthreads();
        u8* t = A;
        A = B;
        B = t;
    }
    return A;
}

// strides up to 16 (all an encoder selects): 16-byte chunks in registers, see v2_decode_core.h
typedef v2d::u128 u128;
__device__ inline u128 load_chunk(const u8* out, u32 base, u32 c, u32 m) {
    u128 X = 0;
#pragma unroll
    for (u32 q = 0; q < 16; ++q)
        if (q < c && base + q < m) X |= (u128)out[base + q] << (8 * q);
    return X;
}
__device__ inline void store_chunk(u8* out, u32 base, u32 c, u32 m, u128 X) {
#pragma unroll
    for (u32 q = 0; q < 16; ++q)
        if (q < c && base + q < m) out[base + q] = (u8)(X >> (8 * q));
}
__device__ inline u128 scan_pass(u128 X, u32 d, u32 c, u128 M, u128& carry, u128* sh) {
    X = v2d::chunk_scan(X, d, M);
    u128 ex, tot;
    wg_scan(v2d::chunk_agg(X, d, c, M), sh, [](u128 x, u128 y) { return x ^ y; }, (u128)0, ex, tot);
    X = v2d::chunk_apply(X, carry ^ ex, d, M);
    carry ^= tot;
    return X;
}

template <u32 MODE>
__device__ inline void serial_tile(u32* A32, u32 g0, u32 m, u32 param, u32& ra, u32& rb, u32& rc) {
    u32 a = ra, b = rb, c = rc;
    for (u32 i = 0; i < m; i += 4) {  // <= AUTO_TILE / 4 words
        const u32 x = A32[i >> 2];
        u32 o = 0;
#pragma unroll
        for (u32 q = 0; q < 4; ++q) {
            const u32 r = ((x >> (8 * q)) & 0xFFu) ^ v2d::serial_pred(MODE, param, (u64)g0 + i + q, a, b, c);
            c = b;
            b = a;
            a = r;
            o |= r << (8 * q);
        }
        A32[i >> 2] = o;
    }
    // bytes past m in the last word moved a, b, c on; the block ends there
    ra = a;
    rb = b;
    rc = c;
}

__global__ __launch_bounds__(PW) void k_v2d_auto(V2dArgs a) {
    __shared__ u32 bufA[v2d::AUTO_TILE / 4], bufB[v2d::AUTO_TILE / 4];
    const u32 li = blockIdx.x, tid = threadIdx.x;
    const u32 b = a.d.list[li];
    const u32 o0 = a.d.obase[b], n = a.d.obase[b + 1] - o0;
    if (n == 0 || a.d.status[b] != DEC_OK) return;
    const u32* info = a.info + V2D_INFO * li;
    const u32 mode = info[0], param = info[1];
    const u32 kind = v2d::auto_kind(mode, param);
    if (kind == v2d::AUTO_ID) return;  // the packed bytes are the block
    u8* out = a.d.out + o0;
    if (kind == v2d::AUTO_SCAN && (mode == 3 || param <= 16)) {
        __shared__ u128 sh[2 * PW];
        const u32 c = mode == 3 ? 16u : v2d::chunk_len(param), TL = PW * c;
        const u128 Mall = v2d::byte_mask(0xFF), Mhi = v2d::byte_mask(0xF0), Mlo = v2d::byte_mask(0x0F);
        u128 c1 = 0, c2 = 0;
        for (u32 g0 = 0; g0 < n; g0 += TL) {  // <= n / TL + 1 tiles
            const u32 m = min(TL, n - g0);
            u128 X = load_chunk(out + g0, tid * c, c, m);
            if (mode == 1) {
                X = scan_pass(X, param, c, Mall, c1, sh);
            } else {  // mode 3: high nibble from r[i-1], low nibble from r[i-2] (r[0] at i = 1)
                if (g0 == 0 && tid == 0 && n > 1) X ^= (X & 0x0F) << 8;
                X = scan_pass(X, 1, c, Mhi, c1, sh);
                X = scan_pass(X, 2, c, Mlo, c2, sh);
            }
            store_chunk(out + g0, tid * c, c, m, X);
        }
        return;
    }
    u32 ra = 0, rb = 0, rc = 0;  // lane 0: the last three decoded bytes
    for (u32 g0 = 0; g0 < n; g0 += v2d::AUTO_TILE) {  // <= n / AUTO_TILE + 1 tiles
        const u32 m = min(v2d::AUTO_TILE, n - g0);
        u8* A = reinterpret_cast<u8*>(bufA);
        u8* B = reinterpret_cast<u8*>(bufB);
        for (u32 i = tid; i < m; i += PW) A[i] = out[g0 + i];
        __syncthreads();
        if (kind == v2d::AUTO_SCAN) {
            A = tile_xor_scan(A, B, out, g0, m, param, 0xFFu);  // mode 1, stride above 16
        } else if (kind == v2d::AUTO_SERIAL) {
            if (tid == 0) {
                if (mode == 2)
                    serial_tile<2>(bufA, g0, m, param, ra, rb, rc);
                else if (mode == 4)
                    serial_tile<4>(bufA, g0, m, param, ra, rb, rc);
                else
                    serial_tile<5>(bufA, g0, m, param, ra, rb, rc);
            }
            __syncthreads();
        }
        for (u32 i = tid; i < m; i += PW) out[g0 + i] = A[i];
        __syncthreads();  // the next tile's carry reads these bytes
    }
}

}  // namespace

void launch_dec_v2_parse(const V2dArgs& a, hipStream_t s) {
    if (!a.d.nlist) return;
    k_v2d_parse<<<a.d.nlist, PW, 0, s>>>(a);
    k_v2d_chunkpar<<<dim3(a.tpc, 8 * a.d.nlist), PW, 0, s>>>(a);
    k_v2d_fill<<<dim3(a.tpc, 8 * a.d.nlist), PW, 0, s>>>(a);
}

void launch_dec_v2_pack(const V2dArgs& a, hipStream_t s) {
    if (a.d.nlist) k_v2d_pack<<<dim3((a.tpc * V2D_CHUNK / 8 + PW - 1) / PW, a.d.nlist), PW, 0, s>>>(a);
}

// uses d and info only: one launch over all id-10 blocks of a batch, after the groups
void launch_dec_v2_auto(const V2dArgs& a, hipStream_t s) {
    if (a.d.nlist) k_v2d_auto<<<a.d.nlist, PW, 0, s>>>(a);
}

}  // namespace kolm
