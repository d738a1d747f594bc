// kolm_dedup.cpp — planning of duplicate-block detection, host side (C ABI: kolm_dedup_plan,
// include/kolm.h).  No device code: from the blocks' lengths, fingerprints and forced method ids
// it derives the candidate pairs the device compares (phase A) and, from the comparison's words,
// the block -> representative map, the distinct blocks, and the copy segments that pack the
// distinct blocks into a dense text and spread their payloads over every block that shares them
// (phase B; the segment tables of k_range_gather, range_core.h).
#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

#include "../../include/kolm.h"
#include "kolm_internal.h"

using kolm::set_err;
using kolm::u32;
using kolm::u64;

namespace kolm {

// Blocks are grouped by (length, forced id or -1, the fingerprint's low `bits` bits); a group's
// representative is its lowest-numbered block and every other member gives a pair (member,
// representative).  Pairs in ascending member order.
void dedup_pairs(const u32* lens, const u64* fp, const int32_t* force, u32 nb, u32 bits, std::vector<u32>& pairs) {
    const u64 m0 = bits >= 64 ? ~0ull : (1ull << bits) - 1;
    const u64 m1 = bits >= 128 ? ~0ull : bits > 64 ? (1ull << (bits - 64)) - 1 : 0;
    struct Key {
        u32 len;
        int32_t force;
        u64 f0, f1;
        u32 idx;
    };
    std::vector<Key> k(nb);
    for (u32 i = 0; i < nb; ++i)
        k[i] = Key{lens[i], force && force[i] >= 0 ? force[i] : -1, fp[2 * (u64)i] & m0, fp[2 * (u64)i + 1] & m1, i};
    auto same = [](const Key& a, const Key& b) { return a.len == b.len && a.force == b.force && a.f0 == b.f0 && a.f1 == b.f1; };
    std::sort(k.begin(), k.end(), [](const Key& a, const Key& b) {
        if (a.len != b.len) return a.len < b.len;
        if (a.force != b.force) return a.force < b.force;
        if (a.f0 != b.f0) return a.f0 < b.f0;
        if (a.f1 != b.f1) return a.f1 < b.f1;
        return a.idx < b.idx;
    });
    std::vector<u32> of(nb);  // representative of every block's group
    for (u32 i = 0, g = 0; i < nb; ++i) {
        if (!same(k[i], k[g])) g = i;
        of[k[i].idx] = k[g].idx;
    }
    pairs.clear();
    for (u32 i = 0; i < nb; ++i)
        if (of[i] != i) {
            pairs.push_back(i);
            pairs.push_back(of[i]);
        }
}

// rep[i] = i for distinct blocks, the representative for confirmed duplicates.  A member that
// differs from its representative (a fingerprint collision) is encoded itself and is nobody's
// representative: the simplest rule, which costs dedup opportunities only under collisions.
// Returns the collisions.
u32 dedup_map(u32 nb, const std::vector<u32>& pairs, const u32* differ, std::vector<u32>& rep, std::vector<u32>& distinct) {
    rep.resize(nb);
    std::iota(rep.begin(), rep.end(), 0u);
    u32 coll = 0;
    for (size_t p = 0; p < pairs.size() / 2; ++p) {
        if (differ[p]) ++coll;
        else rep[pairs[2 * p]] = pairs[2 * p + 1];
    }
    distinct.clear();
    for (u32 i = 0; i < nb; ++i)
        if (rep[i] == i) distinct.push_back(i);
    return coll;
}

// the distinct blocks packed back to back: src = the block's start in the batch
void dedup_compact(const u32* lens, u32 nb, const std::vector<u32>& distinct, std::vector<rng::Seg>& segs) {
    std::vector<u64> start((size_t)nb + 1, 0);
    for (u32 i = 0; i < nb; ++i) start[i + 1] = start[i] + lens[i];
    segs.resize(distinct.size());
    u64 at = 0;
    for (size_t q = 0; q < distinct.size(); ++q) {
        segs[q] = rng::Seg{start[distinct[q]], at, lens[distinct[q]]};
        at += lens[distinct[q]];
    }
}

// dist_off [ndistinct + 1]: the distinct blocks' payload offsets.  payload_off [nb + 1]: every
// block's, a prefix sum in block order; segs [nb]: block i's payload from its representative's.
void dedup_expand(const std::vector<u32>& rep, const std::vector<u32>& distinct, const u64* dist_off, u64* payload_off,
                  std::vector<rng::Seg>& segs) {
    const u32 nb = (u32)rep.size();
    std::vector<u32> q(nb, 0);
    for (size_t j = 0; j < distinct.size(); ++j) q[distinct[j]] = (u32)j;
    segs.resize(nb);
    payload_off[0] = 0;
    for (u32 i = 0; i < nb; ++i) {
        const u32 j = q[rep[i]];
        const u64 len = dist_off[j + 1] - dist_off[j];
        segs[i] = rng::Seg{dist_off[j] - dist_off[0], payload_off[i], len};
        payload_off[i + 1] = payload_off[i] + len;
    }
}

}  // namespace kolm

extern "C" int kolm_dedup_plan(const uint32_t* lens, const uint64_t* fps, const int32_t* force_method, uint32_t nblocks,
                               uint32_t fp_bits, const uint32_t* differ, uint32_t* pairs, uint32_t* rep,
                               uint32_t* distinct, kolm_range_seg* compact, const uint64_t* distinct_off,
                               uint64_t* payload_off, kolm_range_seg* expand, uint32_t* counts) {
    if ((nblocks && (!lens || !fps)) || !counts) return KOLM_EARG;
    if (fp_bits > 128) {
        set_err("kolm_dedup_plan: fp_bits must be in [0, 128]");
        return KOLM_EARG;
    }
    try {
        std::vector<u32> pr, rp, ds;
        kolm::dedup_pairs(lens, fps, force_method, nblocks, fp_bits, pr);
        counts[0] = (u32)(pr.size() / 2);
        counts[1] = counts[2] = 0;
        if (pairs) std::copy(pr.begin(), pr.end(), pairs);
        if (!differ && !pr.empty()) return KOLM_OK;  // phase A: the pairs to compare
        counts[2] = kolm::dedup_map(nblocks, pr, differ, rp, ds);
        counts[1] = (u32)ds.size();
        if (rep) std::copy(rp.begin(), rp.end(), rep);
        if (distinct) std::copy(ds.begin(), ds.end(), distinct);
        std::vector<rng::Seg> sg;
        if (compact) {
            kolm::dedup_compact(lens, nblocks, ds, sg);
            for (size_t i = 0; i < sg.size(); ++i) compact[i] = kolm_range_seg{sg[i].src, sg[i].dst, sg[i].len};
        }
        if (distinct_off) {
            if (!payload_off) return KOLM_EARG;
            kolm::dedup_expand(rp, ds, distinct_off, payload_off, sg);
            if (expand)
                for (size_t i = 0; i < sg.size(); ++i) expand[i] = kolm_range_seg{sg[i].src, sg[i].dst, sg[i].len};
        }
        return KOLM_OK;
    } catch (const std::bad_alloc&) {
        set_err("host allocation failed");
        return KOLM_EHIP;
    }
}
