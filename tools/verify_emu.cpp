// CPU emulation of the verify compare kernel: the header k_verify_cmp of
// kolmogorovlike-datacompressor_amd/csrc/k_verify.hip compiles (csrc/verify_core.h), driven with
// the kernel's shape — a grid of workgroups striding over tiles of 1024 aligned 16-byte words,
// 4 waves of 64 virtual lanes with 4 word pairs each, the wave-wide vote that skips equal
// tiles, the head and tail bytes on workgroup 0 — behind a C interface for
// tests/test_verify_core.py, and a main() that runs the small sweep on its own over buffers
// of exactly `total` bytes (built with -fsanitize=address,undefined by the test: a load
// outside [0, total) of either buffer is an error there).
//   g++ -O2 -std=c++17 -shared -fPIC tools/verify_emu.cpp -o verify_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/verify_emu.cpp -o verify_emu
//   ./verify_emu       exit status 0 when every case matches the byte-by-byte reference
#include "../kolmogorovlike-datacompressor_amd/csrc/verify_core.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace vfy;

namespace {

struct HostMin {
    u32* fb;
    u64 calls = 0;
    void operator()(u32 b, u32 off) {
        ++calls;
        if (fb[b] > off) fb[b] = off;
    }
};

void load_word(const u8* p, u32 x[4]) { std::memcpy(x, p, WORD); }

// the kernel, one virtual lane at a time; `mis` stands for the buffers' address mod 16
u64 compare(const u8* a, const u8* b, u32 total, u32 mis, const u32* bounds, u32 nb, u32* fb, u32 grid) {
    const Split sp = split(mis, total);
    HostMin amin{fb};
    if (grid == 0) grid = grid_for(sp.words);
    const u32 ntiles = tiles(sp.words);
    for (u32 wg = 0; wg < grid; ++wg) {
        if (wg == 0)
            for (u32 tid = 0; tid < 2 * WORD; ++tid) {
                const bool tl = tid >= WORD;
                const u32 j = tid & (WORD - 1);
                const u32 pos = tl ? sp.head + sp.words * WORD + j : j;
                if (j < (tl ? sp.tail : sp.head) && a[pos] != b[pos]) attribute(bounds, nb, pos, 1u, amin);
            }
        for (u32 t = wg; t < ntiles; t += grid)
            for (u32 wave = 0; wave < WG / 64; ++wave) {
                u32 xa[64][UNROLL][4], xb[64][UNROLL][4], d[64];
                bool any = false;
                for (u32 lane = 0; lane < 64; ++lane) {
                    const u32 w0 = t * TILE_WORDS + wave * 64 + lane;
                    d[lane] = 0;
                    for (u32 k = 0; k < UNROLL; ++k) {
                        const u32 w = w0 + k * WG;
                        std::memset(xa[lane][k], 0, WORD);
                        std::memset(xb[lane][k], 0, WORD);
                        if (w < sp.words) {
                            load_word(a + sp.head + (u64)w * WORD, xa[lane][k]);
                            load_word(b + sp.head + (u64)w * WORD, xb[lane][k]);
                        }
                        d[lane] |= word_diff(xa[lane][k], xb[lane][k]);
                    }
                    any = any || d[lane] != 0;
                }
                if (!any) continue;
                for (u32 lane = 0; lane < 64; ++lane) {
                    if (d[lane] == 0) continue;
                    const u32 w0 = t * TILE_WORDS + wave * 64 + lane;
                    for (u32 k = 0; k < UNROLL; ++k) {
                        if (word_diff(xa[lane][k], xb[lane][k]) == 0) continue;
                        attribute(bounds, nb, sp.head + (w0 + k * WG) * WORD, byte_mask(xa[lane][k], xb[lane][k]), amin);
                    }
                }
            }
    }
    return amin.calls;
}

}  // namespace

// first_bad[nb] is set to EQUAL, then lowered; returns the number of minimum operations (the
// work of the slow path: 0 when the buffers are equal).  grid 0 = the kernel's own grid.
extern "C" uint64_t vfy_emu_compare(const uint8_t* a, const uint8_t* b, uint32_t total, uint32_t mis,
                                    const uint32_t* bounds, uint32_t nb, uint32_t* first_bad, uint32_t grid) {
    for (u32 i = 0; i < nb; ++i) first_bad[i] = EQUAL;
    return compare(a, b, total, mis, bounds, nb, first_bad, grid);
}

namespace {

std::vector<u32> layout(int kind, u32 total) {
    std::vector<u32> b{0};
    if (kind == 0) {
        for (u32 i = 1; i <= total; ++i) b.push_back(i);
    } else if (kind == 1) {
        static const u32 lens[] = {1, 2, 3, 15, 16, 17};
        for (u32 i = 0; b.back() < total; ++i) b.push_back(std::min(total, b.back() + lens[i % 6]));
    } else if (total) {
        b.push_back(total);
    }
    return b;
}

int run_case(const std::vector<u8>& A, const std::vector<u8>& B, u32 mis, const std::vector<u32>& bounds, u32 grid,
             const char* what) {
    const u32 total = (u32)A.size(), nb = (u32)bounds.size() - 1;
    // exactly total bytes each, on the heap: the sanitizer sees any load outside them
    u8* a = (u8*)std::malloc(total ? total : 1);
    u8* b = (u8*)std::malloc(total ? total : 1);
    if (total) {
        std::memcpy(a, A.data(), total);
        std::memcpy(b, B.data(), total);
    }
    std::vector<u32> got(nb + 1, 0), want(nb + 1, EQUAL);
    vfy_emu_compare(total ? a : nullptr, total ? b : nullptr, total, mis, bounds.data(), nb, got.data(), grid);
    for (u32 i = 0; i < nb; ++i)
        for (u32 p = bounds[i]; p < bounds[i + 1]; ++p)
            if (A[p] != B[p]) {
                want[i] = p - bounds[i];
                break;
            }
    int bad = 0;
    for (u32 i = 0; i < nb; ++i)
        if (got[i] != want[i]) {
            if (!bad)
                std::fprintf(stderr, "%s: total %u mis %u block %u: got %u, want %u\n", what, total, mis, i, got[i], want[i]);
            bad = 1;
        }
    std::free(a);
    std::free(b);
    return bad;
}

}  // namespace

#ifndef VFY_EMU_NO_MAIN
int main() {
    int bad = 0;
    u64 cases = 0;
    for (u32 mis = 0; mis < 16; ++mis)
        for (u32 total = 0; total <= 48; ++total)
            for (int kind = 0; kind < 3; ++kind) {
                const std::vector<u32> bounds = layout(kind, total);
                std::vector<u8> A(total), B;
                for (u32 i = 0; i < total; ++i) A[i] = (u8)(i * 7 + 3);
                B = A;
                bad |= run_case(A, B, mis, bounds, 0, "equal");
                for (u32 p = 0; p < total; ++p) {
                    B = A;
                    B[p] ^= 0x80;
                    bad |= run_case(A, B, mis, bounds, 0, "one byte");
                    ++cases;
                }
                for (u32 i = 0; i < total; ++i) B[i] = (u8)~A[i];
                bad |= run_case(A, B, mis, bounds, 0, "all differ");
                cases += 2;
            }
    // several tiles and a grid smaller than the tile count (the grid stride), odd ends
    for (u32 mis : {0u, 5u, 15u})
        for (u32 total : {16u * TILE_WORDS, 3u * 16u * TILE_WORDS + 37u, 2u * 16u * TILE_WORDS - 1u}) {
            std::vector<u32> bounds{0, 1, 4097, total - 3, total};
            std::vector<u8> A(total), B;
            for (u32 i = 0; i < total; ++i) A[i] = (u8)(i * 13 + (i >> 8));
            for (u32 p : {0u, 1u, 4096u, 4097u, 16u * TILE_WORDS - 1u, total - 4, total - 3, total - 1}) {
                B = A;
                B[p] ^= 1;
                bad |= run_case(A, B, mis, bounds, 2, "tiles");
                ++cases;
            }
            B = A;
            for (u32 i = 0; i < total; ++i) B[i] ^= 0xFF;
            bad |= run_case(A, B, mis, bounds, 0, "tiles, all differ");
            bad |= run_case(A, A, mis, bounds, 1, "tiles, equal");
            cases += 2;
        }
    std::printf("verify_emu: %llu cases %s\n", (unsigned long long)cases, bad ? "FAILED" : "ok");
    return bad;
}
#endif
