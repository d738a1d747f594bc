// kolm_range.cpp — planning of random-access reads, host side (C ABI: kolm_range_plan,
// include/kolm.h).  No device code: from a container's block lengths and a list of byte ranges
// it derives the blocks to decode, their groups (bounded decode scratch), the runs of blocks
// whose payloads are contiguous in the container, and the copy segments that pack the ranges
// back to back in request order (the segment tables of k_range_gather, range_core.h).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <vector>

#include "../../include/kolm.h"
#include "kolm_internal.h"

using kolm::set_err;
using kolm::u32;
using kolm::u64;

namespace kolm {

u64 range_group_limit(u64 limit) {
    if (limit == 0) {
        limit = 1ull << 30;
        if (const char* e = getenv("KOLM_READ_BYTES")) limit = std::max<u64>(1, strtoull(e, nullptr, 10));
    }
    return std::min<u64>(limit, (1ull << 31) - 1);
}

namespace {
// largest i < nb with starts[i] <= pos (pos < starts[nb]): the block that holds pos (never an
// empty one)
u32 block_of(const u64* starts, u32 nb, u64 pos) {
    return (u32)(std::upper_bound(starts, starts + nb + 1, pos) - starts) - 1;
}
}  // namespace

int range_plan(const u32* orig_lens, const u64* starts, u32 nb, const u64* offs, const u64* lens, u32 nr, u64 limit,
               RangePlan& p) {
    const u64 total = starts[nb];
    for (u32 r = 0; r < nr; ++r)
        if (offs[r] > total || lens[r] > total - offs[r]) {
            char msg[160];
            snprintf(msg, sizeof msg, "range %u: [%llu, +%llu) is not inside the container's %llu bytes", r,
                     (unsigned long long)offs[r], (unsigned long long)lens[r], (unsigned long long)total);
            set_err(msg);
            return KOLM_EARG;
        }
    limit = range_group_limit(limit);
    // first and last block of every non-empty range; the blocks between are marked through a
    // difference array
    std::vector<u32> fb(nr), lb(nr);
    std::vector<int32_t> mark((size_t)nb + 1, 0);
    for (u32 r = 0; r < nr; ++r) {
        if (!lens[r]) continue;
        fb[r] = block_of(starts, nb, offs[r]);
        lb[r] = block_of(starts, nb, offs[r] + lens[r] - 1);
        ++mark[fb[r]];
        --mark[lb[r] + 1];
    }
    p = RangePlan{};
    std::vector<u32> selidx(nb, 0);  // block -> index in sel
    int32_t depth = 0;
    for (u32 b = 0; b < nb; ++b) {
        depth += mark[b];
        if (depth > 0 && orig_lens[b]) {
            selidx[b] = (u32)p.sel.size();
            p.sel.push_back(b);
        }
    }
    // groups of consecutive selected blocks (a single block always forms one), runs, and every
    // selected block's offset in its group's scratch
    const u32 ns = (u32)p.sel.size();
    std::vector<u64> soff(ns);
    std::vector<u32> gof(ns);
    u64 gbytes = 0;
    for (u32 i = 0; i < ns; ++i) {
        const u32 b = p.sel[i];
        const bool new_group = i == 0 || gbytes + orig_lens[b] > limit;
        if (new_group) {
            p.group_first.push_back(i);
            gbytes = 0;
        }
        if (new_group || b != p.sel[i - 1] + 1) p.run_first.push_back(i);
        gof[i] = (u32)p.group_first.size() - 1;
        soff[i] = gbytes;
        gbytes += orig_lens[b];
    }
    p.group_first.push_back(ns);
    p.run_first.push_back(ns);
    const u32 ng = (u32)p.group_first.size() - 1;
    // copy segments: one per (range, group the range has bytes in), grouped by group and in
    // request order within a group (counting pass, then placement)
    p.group_seg.assign((size_t)ng + 1, 0);
    u64 nseg = 0;
    for (u32 r = 0; r < nr; ++r) {
        if (!lens[r]) continue;
        for (u32 g = gof[selidx[fb[r]]]; g <= gof[selidx[lb[r]]]; ++g) ++p.group_seg[g + 1];
        nseg += gof[selidx[lb[r]]] - gof[selidx[fb[r]]] + 1;
    }
    if (nseg > 0xFFFFFFFFull) {
        set_err("more than 2^32 - 1 copy segments");
        return KOLM_EARG;
    }
    for (u32 g = 0; g < ng; ++g) p.group_seg[g + 1] += p.group_seg[g];
    p.segs.resize(nseg);
    std::vector<u32> fill(p.group_seg.begin(), p.group_seg.end() - 1);
    u64 out = 0;
    for (u32 r = 0; r < nr; ++r) {
        if (!lens[r]) continue;
        const u32 i0 = selidx[fb[r]], i1 = selidx[lb[r]];
        const u64 end = offs[r] + lens[r];
        for (u32 g = gof[i0]; g <= gof[i1]; ++g) {
            const u32 a = std::max(i0, p.group_first[g]), z = std::min(i1, p.group_first[g + 1] - 1);
            const u64 lo = std::max(offs[r], starts[p.sel[a]]), hi = std::min(end, starts[p.sel[z] + 1]);
            p.segs[fill[g]++] = rng::Seg{soff[a] + (lo - starts[p.sel[a]]), out + (lo - offs[r]), hi - lo};
        }
        out += lens[r];
    }
    return KOLM_OK;
}

}  // namespace kolm

extern "C" int kolm_range_plan(const uint32_t* orig_lens, uint32_t nblocks, const uint64_t* offs, const uint64_t* lens,
                               uint32_t nranges, uint64_t group_limit, uint32_t* sel, uint32_t* group_first,
                               uint32_t* run_first, uint32_t* group_seg, kolm_range_seg* segs, const uint64_t* caps,
                               uint64_t* counts) {
    if ((nblocks && !orig_lens) || (nranges && (!offs || !lens)) || !counts) return KOLM_EARG;
    try {
        std::vector<u64> starts((size_t)nblocks + 1, 0);
        for (u32 i = 0; i < nblocks; ++i) starts[i + 1] = starts[i] + orig_lens[i];
        kolm::RangePlan p;
        if (int rc = kolm::range_plan(orig_lens, starts.data(), nblocks, offs, lens, nranges, group_limit, p)) return rc;
        counts[0] = p.sel.size();
        counts[1] = p.group_first.size() - 1;
        counts[2] = p.run_first.size() - 1;
        counts[3] = p.segs.size();
        const u64 c[4] = {caps ? caps[0] : 0, caps ? caps[1] : 0, caps ? caps[2] : 0, caps ? caps[3] : 0};
        if (c[0] < counts[0] || c[1] < counts[1] || c[2] < counts[2] || c[3] < counts[3] || (counts[0] && !sel) ||
            !group_first || !run_first || !group_seg || (counts[3] && !segs)) {
            set_err("kolm_range_plan: an output array is too small");
            return KOLM_ECAP;
        }
        std::copy(p.sel.begin(), p.sel.end(), sel);
        std::copy(p.group_first.begin(), p.group_first.end(), group_first);
        std::copy(p.run_first.begin(), p.run_first.end(), run_first);
        std::copy(p.group_seg.begin(), p.group_seg.end(), group_seg);
        for (size_t i = 0; i < p.segs.size(); ++i) segs[i] = kolm_range_seg{p.segs[i].src, p.segs[i].dst, p.segs[i].len};
        return KOLM_OK;
    } catch (const std::bad_alloc&) {
        set_err("host allocation failed");
        return KOLM_EHIP;
    }
}
