// CPU emulation of the round-0 prefix codes (kolmogorovlike-datacompressor_amd/csrc/alpha_code.h):
// the same header the kernels compile, behind a C interface for tests/test_alpha_code.py, and a
// main() that checks the builder's properties and the wrap-around key routine on its own (built
// with -fsanitize=address,undefined by the test).
//   g++ -O2 -std=c++17 -shared -fPIC tools/alpha_code_emu.cpp -o alpha_code_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/alpha_code_emu.cpp -o alpha_code_emu && ./alpha_code_emu
#include "../kolmogorovlike-datacompressor_amd/csrc/alpha_code.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace kolm;

extern "C" {

// cw[256] from 256 presence bits (8 words) and 256 weights; returns sigma
uint32_t ac_emu_build(const uint32_t* pres, const uint32_t* wts, uint16_t* cw) {
    AcWork k;
    ac_build(pres, wts, k, cw);
    return k.sigma;
}

// the same with one virtual thread per node and a barrier between levels, the nodes of a level
// in descending order (the kernel's schedule; the order inside a level must not matter)
uint32_t ac_emu_build_levels(const uint32_t* pres, const uint32_t* wts, uint16_t* cw) {
    AcWork k;
    ac_init(pres, wts, k, cw);
    for (uint32_t d = 0; d <= AC_MAXLEN; ++d)
        for (uint32_t c = 1u << d; c-- > 0;) ac_node(k, (1u << d) + c, d, cw);
    return k.sigma;
}

// keys[t] = the 64-bit key of the rotation at offset t of the factor text[0 .. m)
void ac_emu_keys(const uint8_t* text, uint32_t m, const uint16_t* cw, uint64_t* keys) {
    for (uint32_t t = 0; t < m; ++t) keys[t] = ac_key_wrap(text, m, t, cw);
}

}  // extern "C"

namespace {

int fails = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            ++fails;                                   \
            fprintf(stderr, "FAIL %s: ", #c);          \
            fprintf(stderr, __VA_ARGS__);              \
            fprintf(stderr, "\n");                     \
        }                                              \
    } while (0)

void check_code(const char* what, const std::vector<uint32_t>& syms, const std::vector<uint32_t>& w) {
    uint32_t pres[8] = {0}, wts[256] = {0};
    for (size_t i = 0; i < syms.size(); ++i) {
        pres[syms[i] >> 5] |= 1u << (syms[i] & 31);
        wts[syms[i]] = w[i];
    }
    uint16_t cw[256], cw2[256];
    const uint32_t sigma = ac_emu_build(pres, wts, cw);
    ac_emu_build_levels(pres, wts, cw2);
    CHECK(sigma == syms.size(), "%s sigma %u", what, sigma);
    CHECK(!memcmp(cw, cw2, sizeof cw), "%s level order", what);
    uint64_t prev_end = 0;  // one past the previous symbol's left-aligned code interval
    bool first = true;
    for (uint32_t c = 0; c < 256; ++c) {
        const bool here = (pres[c >> 5] >> (c & 31)) & 1u;
        if (!here) {
            CHECK(cw[c] == 0, "%s absent %u", what, c);
            continue;
        }
        const uint32_t l = ac_len(cw[c]), b = ac_bits(cw[c]);
        CHECK(l >= AC_MINLEN && l <= AC_MAXLEN, "%s len %u of %u", what, l, c);
        CHECK(l && b < (1u << l), "%s bits %u of %u", what, b, c);
        if (!l) continue;
        // prefix-free and increasing: the intervals [b << (8 - l), (b + 1) << (8 - l)) are disjoint and in order
        const uint64_t lo = (uint64_t)b << (AC_MAXLEN - l), hi = (uint64_t)(b + 1) << (AC_MAXLEN - l);
        CHECK(first || lo >= prev_end, "%s order at %u", what, c);
        prev_end = hi;
        first = false;
    }
    CHECK(prev_end <= (1u << AC_MAXLEN), "%s overflow", what);
}

std::string bitstring(const std::string& f, uint32_t t, const uint16_t* cw) {
    std::string s;
    while (s.size() < 64) {
        const uint16_t w = cw[(uint8_t)f[t]];
        for (int i = (int)ac_len(w) - 1; i >= 0; --i) s.push_back(((ac_bits(w) >> i) & 1) ? '1' : '0');
        if (++t == f.size()) t = 0;
    }
    return s.substr(0, 64);
}

void check_keys(const std::string& f) {
    uint32_t pres[8] = {0}, wts[256] = {0};
    for (unsigned char c : f) {
        pres[c >> 5] |= 1u << (c & 31);
        ++wts[c];
    }
    uint16_t cw[256];
    ac_emu_build(pres, wts, cw);
    std::vector<uint64_t> keys(f.size());
    ac_emu_keys(reinterpret_cast<const uint8_t*>(f.data()), (uint32_t)f.size(), cw, keys.data());
    for (uint32_t t = 0; t < f.size(); ++t) {
        const std::string want = bitstring(f, t, cw);
        uint64_t v = 0;
        for (char c : want) v = v << 1 | (uint64_t)(c == '1');
        CHECK(keys[t] == v, "key of '%.20s' at %u", f.c_str(), t);
    }
    // key order implies rotation order (over two periods)
    const std::string ff = f + f + f;
    for (uint32_t p = 0; p < f.size(); ++p)
        for (uint32_t q = 0; q < f.size(); q += 1 + f.size() / 40)
            if (keys[p] < keys[q])
                CHECK(ff.compare(p, 2 * f.size(), ff, q, 2 * f.size()) < 0, "order of '%.20s' %u %u", f.c_str(), p, q);
}

}  // namespace

int main() {
    const uint32_t sigmas[] = {1, 2, 3, 16, 17, 50, 255, 256};
    for (uint32_t sg : sigmas) {
        std::vector<uint32_t> syms(sg), w(sg);
        for (uint32_t i = 0; i < sg; ++i) syms[i] = sg > 1 ? i * 255u / (sg - 1) : 65u;  // spread over 0..255
        for (uint32_t i = 0; i < sg; ++i) w[i] = 7;
        check_code("uniform", syms, w);
        for (uint32_t i = 0; i < sg; ++i) w[i] = i < 31 ? 1u << i : 1u << 31;
        check_code("geometric up", syms, w);
        for (uint32_t i = 0; i < sg; ++i) w[i] = i < 31 ? 1u << (30 - i) : 0u;
        check_code("geometric down, zero weights", syms, w);
        for (uint32_t i = 0; i < sg; ++i) w[i] = i == sg / 2 ? 1u << 31 : 1u;
        check_code("one heavy", syms, w);
        for (uint32_t i = 0; i < sg; ++i) w[i] = 0;
        check_code("never sampled", syms, w);
        for (uint32_t i = 0; i < sg; ++i) w[i] = 0xFFFFFFFFu;
        check_code("largest weights", syms, w);
    }
    {  // 256 uniform symbols: the raw bytes
        uint32_t pres[8], wts[256];
        uint16_t cw[256];
        for (auto& p : pres) p = 0xFFFFFFFFu;
        for (auto& x : wts) x = 3;
        ac_emu_build(pres, wts, cw);
        for (uint32_t c = 0; c < 256; ++c) CHECK(cw[c] == (8u << 8 | c), "raw byte %u", c);
    }
    check_keys("a");
    check_keys("ab");
    check_keys("aab");
    check_keys(std::string("abababababababababababababababababababab"));
    check_keys("aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaab");
    {
        std::string t;
        uint32_t x = 12345;
        for (int i = 0; i < 300; ++i) {
            x = x * 1103515245u + 12345u;
            const uint32_t r = (x >> 16) % 100;
            t.push_back(r < 18 ? ' ' : r < 60 ? "etaoin"[r % 6] : (char)('a' + r % 26));
        }
        check_keys(t);
    }
    printf(fails ? "alpha_code_emu: %d failures\n" : "alpha_code_emu: ok\n", fails);
    return fails ? 1 : 0;
}
