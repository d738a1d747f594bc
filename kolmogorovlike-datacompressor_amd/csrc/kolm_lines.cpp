// kolm_lines.cpp — planning of line queries, host side (C ABI: kolm_lines_locate,
// kolm_lines_locate_offsets, include/kolm.h).  No device code: from a container's per-block
// delimiter counts (the line index) it maps a delimiter number to the one block that holds it and
// its number inside that block, and a stream offset to its block, the offset inside it and the
// delimiters in front of the block.  Sums are 64-bit: a stream may hold more than 2^32 delimiters.
#include <algorithm>
#include <cstdio>
#include <new>
#include <vector>

#include "../../include/kolm.h"
#include "kolm_internal.h"

using kolm::set_err;
using kolm::u32;
using kolm::u64;

namespace kolm {

void lines_prefix(const u32* counts, u32 nb, std::vector<u64>& prefix) {
    prefix.assign((size_t)nb + 1, 0);
    for (u32 b = 0; b < nb; ++b) prefix[b + 1] = prefix[b] + counts[b];
}

u32 lines_block_of(const std::vector<u64>& prefix, u64 k) {
    return (u32)(std::upper_bound(prefix.begin(), prefix.end(), k) - prefix.begin()) - 1;
}

}  // namespace kolm

extern "C" int kolm_lines_locate(const uint32_t* counts, uint32_t nblocks, const uint64_t* idx, uint32_t n, uint32_t* block,
                                 uint32_t* j) {
    if ((nblocks && !counts) || (n && (!idx || !block || !j))) return KOLM_EARG;
    try {
        std::vector<u64> prefix;
        kolm::lines_prefix(counts, nblocks, prefix);
        const u64 D = prefix[nblocks];
        for (u32 i = 0; i < n; ++i) {
            if (idx[i] >= D) {
                char msg[160];
                snprintf(msg, sizeof msg, "kolm_lines_locate: entry %u: delimiter %llu of %llu", i, (unsigned long long)idx[i],
                         (unsigned long long)D);
                set_err(msg);
                return KOLM_EARG;
            }
            block[i] = kolm::lines_block_of(prefix, idx[i]);
            j[i] = (u32)(idx[i] - prefix[block[i]]);
        }
        return KOLM_OK;
    } catch (const std::bad_alloc&) {
        set_err("host allocation failed");
        return KOLM_EHIP;
    }
}

extern "C" int kolm_lines_locate_offsets(const uint32_t* orig_lens, const uint32_t* counts, uint32_t nblocks,
                                         const uint64_t* offs, uint32_t n, uint32_t* block, uint32_t* in_block,
                                         uint64_t* before) {
    if ((nblocks && (!orig_lens || !counts)) || (n && (!offs || !block || !in_block || !before))) return KOLM_EARG;
    try {
        std::vector<u64> prefix, starts((size_t)nblocks + 1, 0);
        kolm::lines_prefix(counts, nblocks, prefix);
        for (u32 b = 0; b < nblocks; ++b) starts[b + 1] = starts[b] + orig_lens[b];
        const u64 total = starts[nblocks];
        for (u32 i = 0; i < n; ++i) {
            if (offs[i] > total) {
                char msg[160];
                snprintf(msg, sizeof msg, "kolm_lines_locate_offsets: entry %u: offset %llu is not inside the container's %llu bytes",
                         i, (unsigned long long)offs[i], (unsigned long long)total);
                set_err(msg);
                return KOLM_EARG;
            }
            // the block that holds byte offs[i] (never an empty one); the stream's end is block nblocks
            const u32 b = offs[i] == total ? nblocks : (u32)(std::upper_bound(starts.begin(), starts.end(), offs[i]) - starts.begin()) - 1;
            block[i] = b;
            in_block[i] = (u32)(offs[i] - starts[b]);
            before[i] = prefix[b];
        }
        return KOLM_OK;
    } catch (const std::bad_alloc&) {
        set_err("host allocation failed");
        return KOLM_EHIP;
    }
}
