// CPU emulation of k_crc32 (kolmogorovlike-datacompressor_amd/csrc/k_crc.hip): the header the kernel
// compiles (csrc/crc_core.h) driven with the kernel's shape — waves striding over runs of up to 8
// (block, 4 KiB piece) items of one block, 64 virtual lanes with 4 block-relative words per piece,
// every lane carrying its sum from word to word by the 1 KiB stride shift, one multiply per lane
// and run, the lanes xored per wave, the wave's word weighted and xored into the block's — behind
// a C interface for tests/test_crc_core.py, and a main() that runs the sweep on its own over heap
// buffers of exactly the batch's size (built with -fsanitize=address,undefined by the test: a
// load outside them is an error there).  The loads are those of the fingerprint kernel: this file
// compiles tools/dedup_emu.cpp's Emu (lane_words, the contract check of every load, the orders in
// which the items meet the waves) instead of copying it.  Contract violations are counted:
//   loads   aligned 16-byte words that lie inside the batch [0, N) whole; single bytes of the
//           block at hand
// The runs can be walked in reverse and in an interleaved wave order: the sums are xors, so every
// order must give the same words.
//   g++ -O2 -std=c++17 -shared -fPIC tools/crc_emu.cpp -o crc_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/crc_emu.cpp -o crc_emu
//   ./crc_emu        exit status 0 when every case matches the bit-by-bit reference
#define DDP_EMU_NO_MAIN
#include "dedup_emu.cpp"

#include "../kolmogorovlike-datacompressor_amd/csrc/crc_core.h"

namespace {

const crc::u32* tables() {
    static std::vector<crc::u32> t;
    if (t.empty()) {
        t.resize(crc::TABLE_WORDS);
        crc::gen_tables(t.data());
    }
    return t.data();
}

// run r of block b on one wave: xors into raw[b] once
void crc_run(Emu& e, const u64* bounds, u32 b, u64 r, u32* raw) {
    const u32* tab = tables();
    e.b0 = bounds[b], e.b1 = bounds[b + 1];
    const u64 len = e.b1 - e.b0, np = pieces(len);
    const u64 k1 = std::min<u64>((r + 1) * RUN, np);
    u32 acc[WAVE] = {0};  // the lanes' sums over the run
    for (u64 k = r * RUN; k < k1; ++k) {
        const Piece pc = piece(len, k);
        for (u32 lane = 0; lane < WAVE; ++lane) {
            Words x;
            e.lane_words(e.text + e.b0 + pc.o0, pc, lane, x);
            for (u32 u = 0; u < UNROLL; ++u) acc[lane] = crc::stride_shift(tab, acc[lane]) ^ crc::word_raw(tab, x.w0[u], x.w1[u]);
        }
    }
    u32 v = 0;
    for (u32 lane = 0; lane < WAVE; ++lane) v ^= crc::multmodp(acc[lane], tab[crc::LW + lane]);
    raw[b] ^= crc::multmodp(v, crc::run_weight(tab, len, k1 * ITEM));
}

}  // namespace

// The definition restated bit by bit (no table, no core).
extern "C" uint32_t crc_ref(const uint8_t* p, uint64_t len) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < len; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return c ^ 0xFFFFFFFFu;
}

// CRC-32 of the nb blocks [bounds[i], bounds[i + 1]) of the batch text[0, n) (bounds[0] = 0,
// non-decreasing, bounds[nb] = n; empty blocks allowed) as k_crc32 and the host's finish compute
// them.  waves = the grid's waves (0: the kernel's own grid); order as sequence() of
// dedup_emu.cpp.  Returns the number of contract violations (0 for a correct kernel).
extern "C" uint64_t crc_emu_blocks(const uint8_t* text, uint64_t n, const uint64_t* bounds, uint32_t nb, uint32_t waves,
                                   uint32_t order, uint32_t* out) {
    std::vector<u64> scan((size_t)nb + 1, 0);
    std::vector<u32> raw(nb, 0);
    for (u32 b = 0; b < nb; ++b) scan[b + 1] = scan[b] + runs(bounds[b + 1] - bounds[b]);
    Emu e{text, n};
    const std::vector<u64> seq = sequence(scan[nb], waves, order);
    for (u64 t : seq) {
        u32 b;
        u64 k;
        locate(scan, t, b, k);
        crc_run(e, bounds, b, k, raw.data());
    }
    for (u32 b = 0; b < nb; ++b) out[b] = crc::finish(raw[b], bounds[b + 1] - bounds[b]);
    return e.bad + (seq.size() == scan[nb] ? 0 : 1);
}

extern "C" uint32_t crc_emu_combine(uint32_t a, uint32_t b, uint64_t len_b) { return crc::combine(a, b, len_b); }
extern "C" uint32_t crc_emu_xpow(uint32_t e) { return crc::xpow(e); }

namespace {

const u64 CRC_LENS[] = {1,    3,    4,    15,   16,    17,    63,    64,    65,    1023,
                        1024, 1025, 4095, 4096, 4097,  32767, 32768, 32769, 100000};

// 0 zeros, 1 0xFF, 2 content()
u8 fill(u32 kind, u64 i) { return kind == 0 ? 0 : kind == 1 ? 0xFF : content(i); }

// The batch: a heap block of exactly lead + n bytes whose first `lead` bytes are not part of it.
// Blocks: a prefix of pre bytes (when pre > 0), the block under test, an empty block, 7 bytes.
int crc_case(u32 lead, u32 pre, u64 len, u32 kind, bool packed, u32 waves, u32 order) {
    const u64 n = pre + len + (packed ? 7 : 0);
    u8* rawbuf = (u8*)std::malloc(lead + n ? lead + n : 1);
    u8* text = rawbuf + lead;
    for (u64 i = 0; i < pre; ++i) text[i] = (u8)(0xE0 + i);
    for (u64 i = 0; i < len; ++i) text[pre + i] = fill(kind, i);
    std::vector<u64> bounds{0};
    if (pre) bounds.push_back(pre);
    const u32 blk = (u32)bounds.size() - 1;
    bounds.push_back(pre + len);
    if (packed) {
        for (u64 i = 0; i < 7; ++i) text[pre + len + i] = (u8)(0x11 * i);
        bounds.push_back(pre + len);  // empty
        bounds.push_back(n);
    }
    const u32 nb = (u32)bounds.size() - 1;
    std::vector<u32> got(nb, 0xDEADBEEFu);
    const u64 bad = crc_emu_blocks(text, n, bounds.data(), nb, waves, order, got.data());
    int fail = 0;
    if (bad) std::fprintf(stderr, "crc: %llu contract violations\n", (unsigned long long)bad), fail = 1;
    for (u32 b = 0; b < nb; ++b)
        if (got[b] != crc_ref(text + bounds[b], bounds[b + 1] - bounds[b])) fail = 1;
    if (fail)
        std::fprintf(stderr, "crc: block %u differs from the reference (lead %u, prefix %u, length %llu, content %u)\n", blk,
                     lead, pre, (unsigned long long)len, kind);
    std::free(rawbuf);
    ++g_cases;
    return fail;
}

}  // namespace

#ifndef CRC_EMU_NO_MAIN
int main() {
    int bad = 0;
    const uint8_t check[] = "123456789";
    if (crc_ref(check, 9) != 0xCBF43926u || crc::xpow(0xFFFFFFFFu) != crc::ONE) bad = 1;
    for (u64 len : CRC_LENS)
        for (u32 kind = 0; kind < 3; ++kind)
            for (u32 lead = 0; lead < 16; ++lead) {
                bad |= crc_case(lead, 0, len, kind, false, 0, 0);
                bad |= crc_case(lead, (lead * 7 + 3) & 15, len, kind, true, 1 + lead % 3, lead % 3);
            }
    std::printf("crc_emu: %llu cases %s\n", (unsigned long long)g_cases, bad ? "FAILED" : "ok");
    return bad;
}
#endif
