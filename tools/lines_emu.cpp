// CPU emulation of k_delim_count and k_delim_query (kolmogorovlike-datacompressor_amd/csrc/k_lines.hip):
// the header the kernels compile (csrc/lines_core.h) driven with the kernels' shape — waves striding
// over runs of up to 8 (block, 4 KiB piece) items of one block, 64 virtual lanes with 4
// block-relative words per piece, a popcount per word and a sum per piece; the scan of the pieces'
// counts; one wave per query, RANK as the scanned count plus one piece's partial count, SELECT as a
// binary search of the scanned counts, the four word rows' totals, a scan over the lanes of one row
// and the core's in-word select — behind a C interface for tests/test_lines_core.py, and a main()
// that runs the sweep on its own over heap buffers of exactly the batch's size (built with
// -fsanitize=address,undefined by the test: a load outside them is an error there).  The loads are
// those of the fingerprint kernel: this file compiles tools/dedup_emu.cpp's Emu (lane_words, the
// contract check of every load, the orders in which the runs meet the waves) instead of copying it.
// Contract violations are counted:
//   loads   aligned 16-byte words that lie inside the batch [0, N) whole; single bytes of the
//           block at hand
// The runs can be walked in reverse and in an interleaved wave order: the sums are integer adds, so
// every order must give the same counts.
//   g++ -O2 -std=c++17 -shared -fPIC tools/lines_emu.cpp -o lines_emu.so
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/lines_emu.cpp -o lines_emu
//   ./lines_emu        exit status 0 when every case matches the byte-by-byte reference
#define DDP_EMU_NO_MAIN
#include "dedup_emu.cpp"

#include "../kolmogorovlike-datacompressor_amd/csrc/lines_core.h"

namespace {

// the restricted masks of one piece as the wave holds them: m[lane][u]
struct PieceMasks {
    u32 m[WAVE][UNROLL];
};

void piece_masks(Emu& e, const Piece& pc, u32 delim, PieceMasks& pm) {
    for (u32 lane = 0; lane < WAVE; ++lane) {
        Words x;
        e.lane_words(e.text + e.b0 + pc.o0, pc, lane, x);
        for (u32 u = 0; u < UNROLL; ++u) {
            const u32 w = lin::word_of(lane, u);
            pm.m[lane][u] = w < pc.words ? lin::word_mask(x.w0[u], x.w1[u], delim, pc, w) : 0u;
        }
    }
}

// run r of block b on one wave: stores its pieces' counts, adds into cnt[b] once
void count_run(Emu& e, const u64* bounds, u32 b, u64 r, u32 delim, const u64* pbase, u32* pcnt, u32* cnt) {
    e.b0 = bounds[b], e.b1 = bounds[b + 1];
    const u64 len = e.b1 - e.b0, np = pieces(len);
    const u64 k1 = std::min<u64>((r + 1) * RUN, np);
    u32 sum = 0;
    for (u64 k = r * RUN; k < k1; ++k) {
        const Piece pc = piece(len, k);
        PieceMasks pm;
        piece_masks(e, pc, delim, pm);
        u32 total = 0;  // the wave reduction of the lanes' sums
        for (u32 lane = 0; lane < WAVE; ++lane) {
            u32 c = 0;
            for (u32 u = 0; u < UNROLL; ++u) c += lin::count(pm.m[lane][u]);
            total += c;
        }
        if (pcnt) pcnt[pbase[b] + k] = total;
        sum += total;
    }
    cnt[b] += sum;
}

void count_blocks(Emu& e, const u64* bounds, u32 nb, u32 delim, u32 waves, u32 order, const u64* pbase, u32* pcnt, u32* cnt,
                  u64& bad) {
    std::vector<u64> scan((size_t)nb + 1, 0);
    for (u32 b = 0; b < nb; ++b) scan[b + 1] = scan[b] + runs(bounds[b + 1] - bounds[b]);
    const std::vector<u64> seq = sequence(scan[nb], waves, order);
    for (u64 t : seq) {
        u32 b;
        u64 k;
        locate(scan, t, b, k);
        count_run(e, bounds, b, k, delim, pbase, pcnt, cnt);
    }
    bad += seq.size() == scan[nb] ? 0 : 1;
}

// The masks of the pieces the queries of one call read, each loaded (and every load checked) once:
// a piece's loads are the same for every query that reads it.
struct PieceCache {
    std::vector<PieceMasks> pm;
    std::vector<u8> have;
    const PieceMasks& get(Emu& e, const Piece& pc, u32 delim, u64 at) {
        if (!have[at]) piece_masks(e, pc, delim, pm[at]), have[at] = 1;
        return pm[at];
    }
};

// one query on one wave, as k_delim_query answers it (ps = the scan of the pieces' counts)
u32 query(Emu& e, PieceCache& pcache, const u64* bounds, u32 nb, u32 delim, const u64* pbase, const u64* pscan, u32 b,
          u32 arg, u32 op) {
    if (b >= nb) return lin::NONE;
    e.b0 = bounds[b], e.b1 = bounds[b + 1];
    const u64 len = e.b1 - e.b0;
    const u32 np = (u32)pieces(len);
    const u64* ps = pscan + pbase[b];
    const u64 s0 = ps[0];
    if (op == lin::OP_RANK) {
        if (arg > len) return lin::NONE;
        const u32 k = arg / ITEM, r = arg % ITEM;
        u32 v = (u32)(ps[k] - s0);
        if (r) {
            const Piece pc = piece(len, k);
            const PieceMasks& pm = pcache.get(e, pc, delim, pbase[b] + k);
            for (u32 lane = 0; lane < WAVE; ++lane)
                for (u32 u = 0; u < UNROLL; ++u) v += lin::word_rank(pm.m[lane][u], lin::word_of(lane, u), r);
        }
        return v;
    }
    if ((u64)arg >= ps[np] - s0) return lin::NONE;
    u32 lo = 0, n = np;
    while (n > 1) {
        const u32 half = n >> 1;
        if (ps[lo + half] - s0 <= arg) lo += half;
        n -= half;
    }
    u32 j = arg - (u32)(ps[lo] - s0);
    const Piece pc = piece(len, lo);
    const PieceMasks& pm = pcache.get(e, pc, delim, pbase[b] + lo);
    u32 row = UNROLL;
    for (u32 u = 0; u < UNROLL && row == UNROLL; ++u) {  // the rows in position order
        u32 tot = 0;
        for (u32 lane = 0; lane < WAVE; ++lane) tot += lin::count(pm.m[lane][u]);
        if (j < tot) row = u;
        else j -= tot;
    }
    if (row == UNROLL) return lin::NONE;
    u32 incl = 0;  // the inclusive scan over the row's lanes
    for (u32 lane = 0; lane < WAVE; ++lane) {
        const u32 c = lin::count(pm.m[lane][row]);
        incl += c;
        if (incl - c <= j && j < incl) return (u32)pc.o0 + lin::word_of(lane, row) * WORD + lin::select(pm.m[lane][row], j - (incl - c));
    }
    return lin::NONE;
}

void piece_base(const u64* bounds, u32 nb, std::vector<u64>& pbase) {
    pbase.assign((size_t)nb + 1, 0);
    for (u32 b = 0; b < nb; ++b) pbase[b + 1] = pbase[b] + pieces(bounds[b + 1] - bounds[b]);
}

}  // namespace

// Delimiter counts of the nb blocks [bounds[i], bounds[i + 1]) of the batch text[0, n) (bounds[0] =
// 0, non-decreasing, bounds[nb] = n; empty blocks allowed) as k_delim_count computes them: cnt[nb]
// and (optional) pcnt, the pieces' counts, block after block.  waves = the grid's waves (0: the
// kernel's own grid); order as sequence() of dedup_emu.cpp.  Returns the number of contract
// violations (0 for a correct kernel).
extern "C" uint64_t lines_emu_count(const uint8_t* text, uint64_t n, const uint64_t* bounds, uint32_t nb, uint32_t delim,
                                    uint32_t waves, uint32_t order, uint32_t* cnt, uint32_t* pcnt) {
    std::vector<u64> pbase;
    piece_base(bounds, nb, pbase);
    for (u32 b = 0; b < nb; ++b) cnt[b] = 0;
    Emu e{text, n};
    u64 bad = 0;
    count_blocks(e, bounds, nb, delim, waves, order, pbase.data(), pcnt, cnt, bad);
    return e.bad + bad;
}

// nq queries (block, arg, op: 0 RANK, 1 SELECT) as three u32 each, answered as the kernels answer
// them: the counting pass with piece counts, their scan, one wave per query.  res[nq].
extern "C" uint64_t lines_emu_query(const uint8_t* text, uint64_t n, const uint64_t* bounds, uint32_t nb, uint32_t delim,
                                    const uint32_t* q, uint32_t nq, uint32_t* res) {
    std::vector<u64> pbase;
    piece_base(bounds, nb, pbase);
    std::vector<u32> cnt(nb, 0), pcnt((size_t)pbase[nb] + 1, 0);
    Emu e{text, n};
    u64 bad = 0;
    count_blocks(e, bounds, nb, delim, 0, 0, pbase.data(), pcnt.data(), cnt.data(), bad);
    std::vector<u64> pscan((size_t)pbase[nb] + 1, 0);
    for (u64 i = 0; i < pbase[nb]; ++i) pscan[i + 1] = pscan[i] + pcnt[i];
    PieceCache pcache{std::vector<PieceMasks>((size_t)pbase[nb]), std::vector<u8>((size_t)pbase[nb], 0)};
    for (u32 i = 0; i < nq; ++i) res[i] = query(e, pcache, bounds, nb, delim, pbase.data(), pscan.data(), q[3 * i], q[3 * i + 1], q[3 * i + 2]);
    return e.bad + bad;
}

extern "C" uint32_t lines_emu_eq_mask(uint64_t w0, uint64_t w1, uint32_t delim) { return lin::eq_mask(w0, w1, delim); }
extern "C" uint32_t lines_emu_select(uint32_t m, uint32_t j) { return lin::select(m, j); }
extern "C" uint32_t lines_emu_rank(uint32_t m, uint32_t i) { return lin::rank(m, i); }

namespace {

const u64 LIN_LENS[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8193, 32768, 32773};
const u32 LIN_DELIMS[] = {0x0A, 0x00, 0xFF};

// data kinds: 0 all delimiters, 1 none, 2 word edges (16 i + 15, 16 i), 3 piece edges (4096 i - 1,
// 4096 i), 4 a two-symbol mix
u8 lin_fill(u32 kind, u64 i, u8 d) {
    const u8 other = (u8)(d ^ 0x5A);
    switch (kind) {
    case 0: return d;
    case 1: return other;
    case 2: return (i & 15) == 15 || (i & 15) == 0 ? d : other;
    case 3: return (i & 4095) == 4095 || (i & 4095) == 0 ? d : other;
    default: return ((i * 2654435761u) >> 13) & 1 ? d : other;
    }
}

// The batch: a heap block of exactly lead + n bytes whose first `lead` bytes are not part of it.
// Blocks: a prefix of delimiters, the block under test, an empty block, a tail of delimiters — the
// neighbours are the delimiter itself, so a count that leaks past a block's end shows.
int lin_case(u32 lead, u64 len, u32 kind, u32 delim, u32 waves, u32 order) {
    const u8 d = (u8)delim;
    const u64 pre = (lead * 7 + 3) & 15, tail = 21, n = pre + len + tail;
    u8* rawbuf = (u8*)std::malloc(lead + n);
    u8* text = rawbuf + lead;
    std::memset(rawbuf, d, lead + n);
    for (u64 i = 0; i < len; ++i) text[pre + i] = lin_fill(kind, i, d);
    const u64 bounds[] = {0, pre, pre + len, pre + len, n};
    const u32 nb = 4;
    std::vector<u64> pbase;
    piece_base(bounds, nb, pbase);
    std::vector<u32> cnt(nb, 0xDEADBEEFu), pcnt((size_t)pbase[nb] + 1, 0xDEADBEEFu);
    u64 bad = lines_emu_count(text, n, bounds, nb, delim, waves, order, cnt.data(), pcnt.data());
    int fail = 0;
    std::vector<u32> where;  // the block's delimiter positions
    for (u64 i = 0; i < len; ++i)
        if (text[pre + i] == d) where.push_back((u32)i);
    if (cnt[0] != pre || cnt[1] != where.size() || cnt[2] != 0 || cnt[3] != tail) fail = 1;
    for (u64 k = 0; k < pieces(len); ++k) {
        u32 c = 0;
        for (u64 i = k * ITEM; i < len && i < (k + 1) * ITEM; ++i) c += text[pre + i] == d;
        if (pcnt[pbase[1] + k] != c) fail = 1;
    }
    if (len <= 8193) {  // every RANK and every SELECT of the block, and the sentinel
        std::vector<u32> q, want;
        size_t below = 0;
        for (u32 off = 0; off <= len; ++off) {
            while (below < where.size() && where[below] < off) ++below;
            q.insert(q.end(), {1u, off, lin::OP_RANK});
            want.push_back((u32)below);
        }
        for (u32 j = 0; j <= where.size(); ++j) {
            q.insert(q.end(), {1u, j, lin::OP_SELECT});
            want.push_back(j < where.size() ? where[j] : lin::NONE);
        }
        std::vector<u32> res(want.size(), 0xDEADBEEFu);
        bad += lines_emu_query(text, n, bounds, nb, delim, q.data(), (u32)want.size(), res.data());
        if (res != want) fail = 1;
    }
    if (bad) std::fprintf(stderr, "lines: %llu contract violations\n", (unsigned long long)bad), fail = 1;
    if (fail)
        std::fprintf(stderr, "lines: lead %u, length %llu, kind %u, delimiter %u differs from the reference\n", lead,
                     (unsigned long long)len, kind, delim);
    std::free(rawbuf);
    ++g_cases;
    return fail;
}

}  // namespace

#ifndef LINES_EMU_NO_MAIN
int main() {
    int bad = 0;
    for (u32 delim : LIN_DELIMS)
        for (u64 len : LIN_LENS)
            for (u32 kind = 0; kind < 5; ++kind)
                for (u32 lead = 0; lead < 16; ++lead) bad |= lin_case(lead, len, kind, delim, lead % 4 ? 1 + lead % 3 : 0, lead % 3);
    std::printf("lines_emu: %llu cases %s\n", (unsigned long long)g_cases, bad ? "FAILED" : "ok");
    return bad;
}
#endif
