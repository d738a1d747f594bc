// CPU emulation of the v2_new (id 10) block decoder: the header the kernels of
// kolmogorovlike-datacompressor_amd/csrc/k_v2dec.hip compile (csrc/v2_decode_core.h), driven with
// the kernels' tiling — parse tiles of 256 words with one virtual thread per word and the three
// scans (phase functions, joined ones, value sums) between the per-word steps, the automaton's
// strided XOR scans in 16-byte chunks per virtual thread (strides above 16: doubling over 4 KiB
// tiles with the carry from the bytes already written) — behind a C
// interface for tests/test_v2_decode_core.py, and a main() that runs cases on its own (built with
// -fsanitize=address,undefined by the test).  The inverse BBWT of a plane is a plain CPU one.
//   g++ -O2 -std=c++17 -shared -fPIC tools/v2_decode_emu.cpp -o v2_decode_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/v2_decode_emu.cpp -o v2_decode_emu
//   ./v2_decode_emu [cases.bin]    cases.bin: u32 count, then per case u32 n, u32 plen, u32 ok,
//                                  payload[plen], expected[n] (ok = 1) — written by the test
#include "../kolmogorovlike-datacompressor_amd/csrc/v2_decode_core.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace v2d;

namespace {

// PY:425-454: PI = stable counting sort of L; every cycle of PI is a Lyndon factor, read from
// its minimum slot m as L[PI(m)], L[PI^2(m)], ..., L[m]; factors in descending order of m
std::vector<u8> bbwt_inverse(const std::vector<u8>& L) {
    const size_t n = L.size();
    size_t cnt[257] = {};
    for (u8 c : L) ++cnt[c + 1];
    for (int c = 0; c < 256; ++c) cnt[c + 1] += cnt[c];
    std::vector<u32> PI(n);
    for (size_t i = 0; i < n; ++i) PI[cnt[L[i]]++] = (u32)i;
    std::vector<char> seen(n, 0);
    std::vector<std::vector<u8>> factors;
    for (size_t m = 0; m < n; ++m) {
        if (seen[m]) continue;
        std::vector<u8> f;
        size_t x = m;
        do {
            seen[x] = 1;
            x = PI[x];
            f.push_back(L[x]);
        } while (x != m);
        factors.push_back(f);
    }
    std::vector<u8> out;
    for (size_t i = factors.size(); i-- > 0;) out.insert(out.end(), factors[i].begin(), factors[i].end());
    return out;
}

// one encoded plane from byte `pos`: marks -> L (0/1 bytes); returns false when malformed
bool parse_plane(const u8* p, u64 plen, u64& pos, u32 k, u32 first, u32 n, std::vector<u8>& L) {
    L.assign(n, 0);
    u32 ph = 0, runs = 0;
    u64 pend = 0, cum = 0;
    for (u64 B0 = pos;; B0 += TILE_BYTES) {
        u64 w[TILE_WORDS], f[TILE_WORDS];
        u32 nv[TILE_WORDS], e[TILE_WORDS];
        WordSum ws[TILE_WORDS];
        for (u32 t = 0; t < TILE_WORDS; ++t) {
            w[t] = load_word(p, plen, B0 + 8ull * t, nv[t]);
            f[t] = phase_fn(w[t], nv[t], k);
        }
        u64 fin = PHASE_ID;  // scan 1: phase functions
        for (u32 t = 0; t < TILE_WORDS; ++t) {
            e[t] = phase_apply(fin, ph);
            fin = phase_compose(fin, f[t]);
        }
        for (u32 t = 0; t < TILE_WORDS; ++t) ws[t] = word_summary(p, plen, B0 + 8ull * t, w[t], nv[t], e[t], k);
        Ones oin = Ones{0, 1, 0};  // scan 2: trailing ones; scan 3: counts and sums
        u64 sum = 0;
        u32 cnt = 0;
        bool bad = false, done = false;
        u64 end = 0;
        for (u32 t = 0; t < TILE_WORDS; ++t) {
            const u64 carry = oin.tail + (oin.whole ? pend : 0);
            if (ws[t].cnt && cum + sum < n) {
                const Emit em = word_emit(p, plen, B0 + 8ull * t, w[t], nv[t], e[t], k, carry, cum + sum, runs + cnt, n,
                                          [&](u32 at) { L.at(at) = 1; });
                bad = bad || em.bad;
                if (em.done) {
                    done = true;
                    end = em.endbit;
                }
            }
            sum += ws[t].lsum + (ws[t].joins ? carry << k : 0);
            cnt += ws[t].cnt;
            oin = ones_join(oin, ws[t].ones);
        }
        if (bad || (!done && B0 + TILE_BYTES >= plen)) return false;
        if (done) {
            pos = (end + 7) / 8;
            break;
        }
        ph = phase_apply(fin, ph);
        pend = oin.tail + (oin.whole ? pend : 0);
        cum += sum;
        runs += cnt;
    }
    u32 run = first;
    for (u32 i = 0; i < n; ++i) {
        run ^= L[i];
        L[i] = (u8)run;
    }
    return true;
}

// r[i] = v[i] ^ (r[i - d] & mask) over one tile, as tile_xor_scan of k_v2dec.hip
void tile_xor_scan(std::vector<u8>& A, const u8* out, u32 g0, u32 m, u32 d, u32 mask) {
    for (u32 i = 0; i < m && i < d; ++i)
        if (g0 + i >= d) A[i] ^= out[g0 + i - d] & mask;
    std::vector<u8> B(m);
    for (u64 s = d; s < m; s <<= 1) {
        for (u32 i = 0; i < m; ++i) B[i] = A[i] ^ (i >= s ? A[i - (u32)s] & mask : 0u);
        std::copy(B.begin(), B.end(), A.begin());
    }
}

}  // namespace

extern "C" {

// 0 = decoded into out[0, n); 2 = malformed payload
uint32_t v2d_emu_decode(const uint8_t* p, uint64_t plen, uint32_t n, uint8_t* out) {
    if (n == 0) return 0;
    Header h;
    if (!parse_header(p, plen, h)) return 2;
    std::vector<std::vector<u8>> planes(8);
    u64 pos = h.data;
    u32 ki = 0;
    for (u32 j = 0; j < 8; ++j) {
        if ((h.raw_mask >> j) & 1u) {
            const u64 need = ((u64)n + 7) / 8;
            if (pos + need > plen) return 2;
            planes[j].resize(n);
            for (u32 i = 0; i < n; ++i) planes[j][i] = (p[pos + (i >> 3)] >> (7 - (i & 7))) & 1u;
            pos += need;
        } else {
            std::vector<u8> L;
            if (!parse_plane(p, plen, pos, h.k[ki++], (h.b1_mask >> j) & 1u, n, L)) return 2;
            planes[j] = bbwt_inverse(L);
        }
    }
    const u32 kind = auto_kind(h.mode, h.param);
    std::vector<u8> y(n);
    for (u32 i = 0; i < n; ++i)
        for (u32 j = 0; j < 8; ++j) y[i] |= (u8)((planes[j][i] & 1u) << (7 - j));
    if (kind == AUTO_ID) {
        std::copy(y.begin(), y.end(), out);
        return 0;
    }
    if (kind == AUTO_SCAN && (h.mode == 3 || h.param <= 16)) {  // chunks of 16 bytes per thread
        const u32 c = h.mode == 3 ? 16u : chunk_len(h.param), TL = AUTO_THREADS * c;
        const u128 Mall = byte_mask(0xFF), Mhi = byte_mask(0xF0), Mlo = byte_mask(0x0F);
        u128 c1 = 0, c2 = 0;
        for (u32 g0 = 0; g0 < n; g0 += TL) {
            const u32 m = std::min(TL, n - g0);
            std::vector<u128> X(AUTO_THREADS, 0);
            for (u32 t = 0; t < AUTO_THREADS; ++t)
                for (u32 q = 0; q < c && t * c + q < m; ++q) X[t] |= (u128)y[g0 + t * c + q] << (8 * q);
            auto pass = [&](u32 d, u128 M, u128& carry) {
                u128 ex = 0;
                for (u32 t = 0; t < AUTO_THREADS; ++t) {
                    X[t] = chunk_scan(X[t], d, M);
                    const u128 agg = chunk_agg(X[t], d, c, M);
                    X[t] = chunk_apply(X[t], carry ^ ex, d, M);
                    ex ^= agg;
                }
                carry ^= ex;
            };
            if (h.mode == 1) {
                pass(h.param, Mall, c1);
            } else {
                if (g0 == 0 && n > 1) X[0] ^= (X[0] & 0x0F) << 8;
                pass(1, Mhi, c1);
                pass(2, Mlo, c2);
            }
            for (u32 t = 0; t < AUTO_THREADS; ++t)
                for (u32 q = 0; q < c && t * c + q < m; ++q) out[g0 + t * c + q] = (u8)(X[t] >> (8 * q));
        }
        return 0;
    }
    u32 a = 0, b = 0, c = 0;
    for (u32 g0 = 0; g0 < n; g0 += AUTO_TILE) {
        const u32 m = std::min(AUTO_TILE, n - g0);
        std::vector<u8> A(y.begin() + g0, y.begin() + g0 + m);
        if (kind == AUTO_SCAN) {
            tile_xor_scan(A, out, g0, m, h.param, 0xFFu);  // mode 1, stride above 16
        } else if (kind == AUTO_SERIAL) {
            for (u32 i = 0; i < m; ++i) {
                const u32 r = A[i] ^ serial_pred(h.mode, h.param, (u64)g0 + i, a, b, c);
                c = b;
                b = a;
                a = r;
                A[i] = (u8)r;
            }
        }
        std::copy(A.begin(), A.end(), out + g0);
    }
    return 0;
}

}  // extern "C"

namespace {

int fails = 0;

void expect(const char* name, const std::vector<u8>& pay, u32 n, bool ok, const std::vector<u8>& want) {
    std::vector<u8> out(n ? n : 1, 0xEE);
    const u32 st = v2d_emu_decode(pay.data(), pay.size(), n, out.data());
    const bool good = ok ? (st == 0 && std::equal(want.begin(), want.end(), out.begin())) : st != 0;
    if (!good) {
        std::printf("FAIL %s (status %u)\n", name, st);
        ++fails;
    }
}

std::vector<u8> B(std::initializer_list<int> head, size_t zeros = 0) {
    std::vector<u8> v;
    for (int x : head) v.push_back((u8)x);
    v.insert(v.end(), zeros, 0);
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    // the malformed payloads of the decoder's tests (n = 4) and their valid neighbour
    expect("short", B({0x00, 0xff}), 4, false, {});
    expect("plen5", B({0x05}, 12), 4, false, {});
    expect("param_trunc", B({0x24, 1, 2, 3}), 4, false, {});
    expect("klist_trunc", B({0, 0, 0, 4, 4, 4, 4, 4, 4, 4}), 4, false, {});
    expect("raw_trunc", B({0x00, 0xff, 0x00}, 7), 4, false, {});
    expect("no_terminator", B({0x00, 0xfe, 0x00, 0x00, 0xff}), 4, false, {});
    expect("zero_run", B({0x00, 0xfe, 0x00, 0x00, 0x00}, 7), 4, false, {});
    expect("overrun", B({0x00, 0xfe, 0x00, 0x00, 0xfc}, 7), 4, false, {});
    expect("k16", B({0x00, 0xfe, 0x00, 16, 0x00, 0x04}, 7), 4, false, {});
    expect("valid", B({0x00, 0xfe, 0x00, 0x00, 0xf0}, 7), 4, true, std::vector<u8>(4, 0));
    expect("empty", B({}), 0, true, {});
    // a unary run over many tiles: n zero bytes, plane 0 one run of n ones at k = 0
    {
        const u32 n = 3 * TILE_BYTES * 8 + 5;
        std::vector<u8> pay = B({0x00, 0xfe, 0x00, 0x00});
        pay.insert(pay.end(), n / 8, 0xff);
        pay.push_back((u8)(0xff << (8 - n % 8)));  // the last ones, the terminator, padding
        pay.insert(pay.end(), (n + 7) / 8 * 7, 0);
        expect("long_unary", pay, n, true, std::vector<u8>(n, 0));
    }
    if (argc > 1) {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) {
            std::printf("cannot open %s\n", argv[1]);
            return 2;
        }
        u32 count = 0;
        if (std::fread(&count, 4, 1, f) != 1) count = 0;
        for (u32 i = 0; i < count; ++i) {
            u32 hd[3];
            if (std::fread(hd, 4, 3, f) != 3) {
                std::printf("FAIL truncated case file\n");
                ++fails;
                break;
            }
            std::vector<u8> pay(hd[1]), want(hd[2] ? hd[0] : 0);
            if ((pay.size() && std::fread(pay.data(), 1, pay.size(), f) != pay.size()) ||
                (want.size() && std::fread(want.data(), 1, want.size(), f) != want.size())) {
                std::printf("FAIL truncated case file\n");
                ++fails;
                break;
            }
            char name[32];
            std::snprintf(name, sizeof name, "case %u", i);
            expect(name, pay, hd[0], hd[2] != 0, want);
        }
        std::fclose(f);
        std::printf("v2_decode_emu: %u file cases\n", count);
    }
    if (fails) return 1;
    std::printf("v2_decode_emu: ok\n");
    return 0;
}
