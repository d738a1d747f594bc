// libkolm_hip.so — readers of a container on the device (include/kolm.h): random-access reads,
// searches (patterns of a call, prepared pattern sets) and the line index.  See DESIGN.md §8
// ("Random-access reads", "Search", "Pattern sets", "Line index").
//
// Every call that decodes goes through one path: the plan's blocks are checked before the first
// launch (reader_check_blocks) and decoded group by group (reader_decode_group: payload runs,
// compaction, decode_batch, status and checksum checks); what a call does with a group's bytes --
// gather the ranges, search them, count or locate delimiters -- is all that differs.
#include "kolm_ctx.h"

// ---- random-access reads: decode the blocks a range touches, pack the ranges on the device ----
struct kolm_reader {
    kolm_ctx* c = nullptr;
    u32 mode = 0, size_field = 0, nb = 0;
    u64 total = 0, pbytes = 0;
    std::vector<u32> methods, lens;
    std::vector<u64> poff, starts;  // payload offsets / decoded block starts, nb + 1 entries each
    // the payload area, resident (its own allocation: it outlives the calls).  A source of
    // k_range_gather (payload compaction): hipMalloc aligns it to 256 bytes and it is padded by
    // 64 + 16 bytes, the decoders' read-ahead plus the gather's last aligned word.
    u8* dpay = nullptr;
    // the blocks' expected CRC-32 (kolm_reader_set_checksums): nb words, or empty = reads are not checked
    std::vector<u32> crcs;
    // the line index (kolm_reader_set_lines / kolm_reader_index_lines): the blocks' counts of bytes
    // equal to ldelim, nb words, when has_lines
    bool has_lines = false;
    u32 ldelim = 0x0A;
    std::vector<u32> lcounts;
    // the result of the last kolm_reader_find: absolute offsets and pattern indices, in
    // (offset, pattern) order (kolm_reader_find_copy)
    std::vector<u64> f_offs;
    std::vector<u8> f_which;
    // the result of the last kolm_reader_find_set (kolm_reader_find_copy32); either call empties
    // the other's result
    std::vector<u64> fs_offs;
    std::vector<u32> fs_which;
};

// Uploads a segment table with the exclusive scan of its item counts and launches k_range_gather
// on c->stream between the event pair (e0, e1).  dst: the segments' destination base.
void kolm::gather_segments(kolm_ctx* c, const char* name, const u8* src, u8* dst, const rng::Seg* segs, u32 nseg,
                           std::vector<u32>& scan, hipEvent_t e0, hipEvent_t e1) {
    hipStream_t s = c->stream;
    scan.assign((size_t)nseg + 1, 0);
    u64 items = 0, bytes = 0;
    for (u32 i = 0; i < nseg; ++i) {
        const u32 dmis = (u32)((reinterpret_cast<uintptr_t>(dst) + segs[i].dst) & (rng::WORD - 1));
        items += rng::items(dmis, segs[i].len);
        bytes += segs[i].len;
        if (items > 0xFFFFFFFFull) throw kolm::HipError(hipErrorInvalidValue, "more than 2^32 - 1 gather items", __LINE__);
        scan[i + 1] = (u32)items;
    }
    const std::string nseg_name = std::string(name) + "_seg", nscan_name = std::string(name) + "_scan";
    rng::Seg* dseg = c->get<rng::Seg>(nseg_name.c_str(), nseg);
    u32* dscan = c->get<u32>(nscan_name.c_str(), (size_t)nseg + 1);
    KOLM_HIP_CHECK(hipMemcpyAsync(dseg, segs, sizeof(rng::Seg) * nseg, hipMemcpyHostToDevice, s));
    KOLM_HIP_CHECK(hipMemcpyAsync(dscan, scan.data(), sizeof(u32) * ((size_t)nseg + 1), hipMemcpyHostToDevice, s));
    KOLM_HIP_CHECK(hipEventRecord(e0, s));
    {
        TScope t(c, KOLM_KT_EMIT, "k_range_gather", 2 * bytes);
        launch_range_gather(src, dst, dseg, dscan, nseg, items, s);
    }
    KOLM_HIP_CHECK(hipEventRecord(e1, s));
}

namespace {

// The start of a reader call that launches: the context's lock for the scope, its device selected,
// the timing events of the call before forgotten, launches on the main stream.  A call that does
// something under the lock first (and may find nothing to launch) holds the lock itself and calls
// enter().
struct ReaderCall {
    std::lock_guard<std::mutex> g;
    explicit ReaderCall(kolm_ctx* c) : g(c->mu) { enter(c); }
    static void enter(kolm_ctx* c) {
        KOLM_HIP_CHECK(hipSetDevice(c->device));
        c->timing_reset();
        c->active = c->stream;
    }
};

// Every selected block must be one the device decodes; fills the three figures all stats share
// (kolm_read_stats, kolm_find_stats, kolm_lines_stats).  No launch precedes it.
template <class Stats>
int reader_check_blocks(const kolm_reader* r, const RangePlan& p, Stats& st) {
    st.blocks_decoded = (u32)p.sel.size();
    st.groups = (u32)p.group_first.size() - 1;
    for (u32 b : p.sel) {
        const u32 m = r->methods[b];
        if (m >= 32 || !((KOLM_DECODE_MASK >> m) & 1u) || (m == KOLM_M_V2NEW && r->lens[b] >= (1u << 28)) ||
            r->lens[b] >= (1u << 31)) {
            char msg[128];
            snprintf(msg, sizeof msg, "block %u (method %u, %u bytes) is not decoded on the device", b, m, r->lens[b]);
            set_err(msg);
            return KOLM_EARG;
        }
        st.bytes_decoded += r->lens[b];
    }
    return KOLM_OK;
}

// Host scratch reused across the groups of one call, and what the last group left.
struct GroupDecode {
    std::vector<u32> gm, gl, status, scan, words;  // gm / gl: the group's methods and decoded lengths
    std::vector<u64> gp;
    std::vector<rng::Seg> runs;
    u32 i0 = 0, n = 0;  // the group's slice of p.sel
    u8* dec = nullptr;  // its blocks, back to back
    u64 tot = 0;
    bool compacted = false;
    double ms_decode = 0, ms_compact = 0;
};

// Group g of the plan decoded into c->get<u8>(scratch, headroom + tot + 64 + rng::WORD) + headroom:
// payload runs, compaction when there are several, decode_batch, then the status and checksum
// checks before anything else looks at the bytes.  The caller holds the context's lock.  On a
// failure w's figures cover what ran.
int reader_decode_group(kolm_reader* r, const RangePlan& p, u32 g, const char* scratch, u32 headroom, GroupDecode& w) {
    kolm_ctx* c = r->c;
    const u32 i0 = p.group_first[g], i1 = p.group_first[g + 1], n = i1 - i0;
    w.i0 = i0, w.n = n, w.tot = 0;
    w.compacted = false;
    w.ms_decode = w.ms_compact = 0;
    w.gm.resize(n), w.gl.resize(n), w.gp.assign((size_t)n + 1, 0);
    w.runs.clear();
    for (u32 i = i0; i < i1; ++i) {
        const u32 b = p.sel[i];
        w.gm[i - i0] = r->methods[b];
        w.gl[i - i0] = r->lens[b];
        w.tot += r->lens[b];
        const u64 plen = r->poff[b + 1] - r->poff[b];
        if (i == i0 || b != p.sel[i - 1] + 1) w.runs.push_back(rng::Seg{r->poff[b] - r->poff[0], w.gp[i - i0], 0});
        w.runs.back().len += plen;
        w.gp[i - i0 + 1] = w.gp[i - i0] + plen;
    }
    // one run is decoded where it lies; several are gathered into a staging buffer first
    // (decode_batch takes contiguous payloads).  "rd_pay": read-ahead padding as dec_pay.
    const u8* pay = r->dpay + w.runs[0].src;
    w.compacted = w.runs.size() > 1;
    if (w.compacted) {
        u8* stage = c->get<u8>("rd_pay", w.gp[n] + 64);
        gather_segments(c, "rd_c", r->dpay, stage, w.runs.data(), (u32)w.runs.size(), w.scan, c->ev[4], c->ev[5]);
        pay = stage;
    }
    // the decode scratch, a source of k_range_gather: 256-byte aligned (hipMalloc; a caller's
    // headroom keeps that), padded by the decoders' 64 bytes and the gather's last aligned 16-byte word
    w.dec = c->get<u8>(scratch, headroom + w.tot + 64 + rng::WORD) + headroom;
    double ms = 0.0;
    if (int e = decode_batch(c, pay, w.gp.data(), w.gm.data(), w.gl.data(), n, w.tot, w.dec, &ms, &w.status)) return e;
    w.ms_decode = ms;  // a decode_batch that fails itself adds nothing to the call's figures
    if (w.compacted) w.ms_compact = ev_ms(c->ev[4], c->ev[5]);  // retired: decode_batch drained the stream
    for (u32 i = 0; i < n; ++i)
        if (w.status[i]) {
            char msg[128];
            snprintf(msg, sizeof msg, "block %u (method %u): %s", p.sel[i0 + i], w.gm[i],
                     w.status[i] == DEC_ELEN ? "decoded length mismatch" : "malformed payload");
            set_err(msg);
            return KOLM_EARG;
        }
    if (!r->crcs.empty()) {  // the group's blocks lie back to back in the scratch: one pass, one round trip
        w.words.resize(n);
        crc_blocks_at(c, w.dec, w.gl.data(), n, w.words.data());
        for (u32 i = 0; i < n; ++i) {
            const u32 b = p.sel[i0 + i];
            if (w.words[i] != r->crcs[b]) {
                checksum_message(b, w.gm[i], r->crcs[b], w.words[i]);
                return KOLM_ECHECKSUM;
            }
        }
    }
    return KOLM_OK;
}

// out (host) or d_out (device) receives the packed ranges.  Context lock not held on entry.
int reader_read(kolm_reader* r, const uint64_t* offs, const uint64_t* lens, uint32_t nr, uint8_t* out, void* d_out,
                uint64_t out_cap, kolm_read_stats* stats) {
    if (stats) *stats = kolm_read_stats{};
    if (!r || !r->c || (nr && (!offs || !lens))) return KOLM_EARG;
    // every argument check before the first launch: the plan (ranges), the output, the selected blocks
    RangePlan p;
    if (int rc = range_plan(r->lens.data(), r->starts.data(), r->nb, offs, lens, nr, 0, p)) return rc;
    u64 want = 0;
    for (u32 i = 0; i < nr; ++i) want += lens[i];
    if (want > out_cap) {
        set_err("output capacity too small");
        return KOLM_ECAP;
    }
    if (want && !out && !d_out) return KOLM_EARG;
    kolm_read_stats st{};
    st.ranges = nr;
    st.bytes_returned = want;
    if (int rc = reader_check_blocks(r, p, st)) return rc;
    if (p.sel.empty()) {
        if (stats) *stats = st;
        return KOLM_OK;
    }
    kolm_ctx* c = r->c;
    int rc = guarded([&] {
        ReaderCall call(c);
        hipStream_t s = c->stream;
        // Checked reads write nothing to the caller's buffer on a mismatch: with several groups the
        // ranges are packed in the context's own buffer and copied once every group has passed.
        const bool checked = !r->crcs.empty();
        const bool staged = checked && d_out && p.group_first.size() > 2;
        u8* dout = d_out && !staged ? static_cast<u8*>(d_out) : c->get<u8>("rd_out", want + 64);
        GroupDecode w;
        for (u32 g = 0; g + 1 < p.group_first.size(); ++g) {
            const int e = reader_decode_group(r, p, g, "rd_dec", 0, w);
            st.ms_decode += w.ms_decode;
            if (w.compacted) {
                ++st.compactions;
                st.ms_gather += w.ms_compact;
            }
            if (e) return e;
            const u32 s0 = p.group_seg[g], s1 = p.group_seg[g + 1];
            if (s1 > s0) {
                gather_segments(c, "rd_g", w.dec, dout, p.segs.data() + s0, s1 - s0, w.scan, c->ev[2], c->ev[3]);
                c->sync();  // the next group reuses the scratch tables; the events are retired
                st.ms_gather += ev_ms(c->ev[2], c->ev[3]);
            }
        }
        if (c->timing) c->timing_collect_tail(0, nullptr);
        if (staged && want) {  // on the context's stream and waited for: a device-to-device hipMemcpy does not wait
            KOLM_HIP_CHECK(hipMemcpyAsync(d_out, dout, want, hipMemcpyDeviceToDevice, s));
            c->sync();
        }
        if (!d_out && want) KOLM_HIP_CHECK(hipMemcpy(out, dout, want, hipMemcpyDeviceToHost));
        return KOLM_OK;
    });
    if (stats) *stats = st;
    return rc;
}

// ---- search of decoded bytes on the device (find_core.h, k_find.hip) ----

u64 find_stage_bytes() {  // read per call, like KOLM_READ_BYTES
    u64 v = fnd::STAGE_DEFAULT;
    if (const char* e = getenv("KOLM_FIND_STAGE")) v = std::max<u64>(1, strtoull(e, nullptr, 10));
    return v;
}

// A pattern list: np in 1..max_np patterns, pattern i = the units [pat_off[i], pat_off[i + 1]) of
// `pats` ("bytes" or "positions"), none empty, none longer than KOLM_FIND_MAX_LEN.  L (optional) = the longest.
int check_pat_list(const char* who, const void* pats, const uint32_t* pat_off, u32 np, u32 max_np, const char* unit, u32* L) {
    char msg[200];
    if (np < 1 || np > max_np) {
        snprintf(msg, sizeof msg, "%s: %u patterns (1..%u are allowed)", who, np, max_np);
        set_err(msg);
        return KOLM_EARG;
    }
    if (!pats || !pat_off) return KOLM_EARG;
    u32 longest = 0;
    for (u32 i = 0; i < np; ++i) {
        if (pat_off[i + 1] <= pat_off[i]) {
            snprintf(msg, sizeof msg, "%s: pattern %u is empty", who, i);
            set_err(msg);
            return KOLM_EARG;
        }
        const u32 len = pat_off[i + 1] - pat_off[i];
        if (len > KOLM_FIND_MAX_LEN) {
            snprintf(msg, sizeof msg, "%s: pattern %u has %u %s (at most %u)", who, i, len, unit, (u32)KOLM_FIND_MAX_LEN);
            set_err(msg);
            return KOLM_EARG;
        }
        longest = std::max(longest, len);
    }
    if (L) *L = longest;
    return KOLM_OK;
}

// The three searches that share k_find.hip's tile skeleton differ, on the host, in a variant object:
//   np, L                      the patterns of the call and the longest match (the hold-back)
//   count_name, emit_name      the kernels' names for the timing scopes
//   upload(c)                  the call's tables to the device, on c->stream
//   count(buf, n, lo, shi, cnt, s), emit(buf, n, lo, shi, t0, t1, tscan, dpos, dwhich, slots, s)
//                              the two launches around launch_find_scan
// Each is filled by its own check (find_check_pats, findcls_check_pats, findrx_check), which launches nothing.

// np patterns, pattern i = pats[pat_off[i], pat_off[i + 1])
struct LitSearch {
    static constexpr const char *count_name = "k_find_count", *emit_name = "k_find_emit";
    const uint8_t* pats = nullptr;
    const uint32_t* pat_off = nullptr;
    u32 np = 0, L = 0;
    fnd::Pats hp;
    const fnd::Pats* dP = nullptr;
    void upload(kolm_ctx* c) {
        fnd::make_pats(pats, pat_off, np, hp);
        fnd::Pats* d = c->get<fnd::Pats>("fd_pats", 1);
        KOLM_HIP_CHECK(hipMemcpyAsync(d, &hp, sizeof hp, hipMemcpyHostToDevice, c->stream));
        dP = d;
    }
    void count(const u8* buf, u32 n, u32 lo, u32 shi, u32* cnt, hipStream_t s) const {
        launch_find_count(buf, n, lo, shi, dP, np, cnt, s);
    }
    void emit(const u8* buf, u32 n, u32 lo, u32 shi, u32 t0, u32 t1, const u64* tscan, u32* dpos, u8* dwhich, u32 slots,
              hipStream_t s) const {
        launch_find_emit(buf, n, lo, shi, dP, np, t0, t1, tscan, dpos, dwhich, slots, s);
    }
};

int find_check_pats(const char* who, const uint8_t* pats, const uint32_t* pat_off, u32 np, LitSearch& v) {
    v.pats = pats, v.pat_off = pat_off, v.np = np;
    return check_pat_list(who, pats, pat_off, np, KOLM_FIND_MAX_PATTERNS, "bytes", &v.L);
}

// The emit half of a search of one scan buffer, behind its count, scan and totals round trip
// (tscan [ntiles + 1] on the device, `total` records in all): up to `limit` results are held, `held`
// of them already.  more_than (optional): when the buffer would return more than *more_than
// results, nothing is emitted and it is set to that number.  cap: the records one launch may hold.
//   stage(slots)               allocates the device staging of `slots` records, once, before the
//                              first timed launch (an allocation may wait for the device: it stays
//                              outside the event pairs, so ms never covers one)
//   emit(t0, t1, recs, slots)  launches the emit kernel for tiles [t0, t1) (recs records) into it
//   take(n)                    downloads the first n records of the staging, waits for the stream
//                              (c->sync()) and appends them to the call's results
template <class Stage, class Emit, class Take>
void emit_matches(kolm_ctx* c, u32 ntiles, const u64* tscan, u64 total, u64 held, u64 limit, u64 cap, u64* more_than,
                  u32& launches, double& ms, Stage&& stage, Emit&& emit, Take&& take) {
    const u64 want = std::min<u64>(total, limit > held ? limit - held : 0);
    if (more_than && want > *more_than) {
        *more_than = want;
        return;
    }
    if (!want) return;
    hipStream_t s = c->stream;
    const u64 slots = std::min<u64>(cap, total);  // no launch holds more than either
    stage(slots);
    // everything fits one launch and all of it is wanted: the tile scan stays on the device
    const bool one = want == total && total <= cap;
    std::vector<u64> hscan;
    if (!one) {
        hscan.resize((size_t)ntiles + 1);
        KOLM_HIP_CHECK(hipMemcpyAsync(hscan.data(), tscan, sizeof(u64) * hscan.size(), hipMemcpyDeviceToHost, s));
        c->sync();
    }
    u64 got = 0;
    for (u32 t0 = 0; got < want;) {
        u32 t1 = ntiles;
        u64 recs = total;
        if (!one) {
            while (hscan[t0 + 1] == hscan[t0]) ++t0;
            t1 = fnd::emit_cut(hscan.data(), ntiles, t0, cap, want);
            recs = hscan[t1] - hscan[t0];
        }
        KOLM_HIP_CHECK(hipEventRecord(c->ev[6], s));
        emit(t0, t1, recs, (u32)slots);
        KOLM_HIP_CHECK(hipEventRecord(c->ev[7], s));
        const u64 n = std::min<u64>(recs, want - got);
        take(n);
        ms += ev_ms(c->ev[6], c->ev[7]);  // retired: take waited for the stream
        got += n;
        t0 = t1;
        ++launches;
    }
}

// One scan buffer buf [0, n) on c->stream, for every variant: count, scan, one round trip for the totals,
// then the emit launches (none when nothing is to be returned).  counts [np] accumulate; (base + position,
// pattern) are appended to offs / which until `limit` results are held.  more_than: as emit_matches.
template <class V>
void find_group(kolm_ctx* c, const V& v, const u8* buf, u32 n, u32 lo, u32 shi, u64 base, u64 limit, u64* counts,
                std::vector<u64>& offs, std::vector<u8>& which, u32& launches, double& ms, u64* more_than = nullptr) {
    const u32 ntiles = fnd::tiles(n), np = v.np;
    if (!ntiles) return;
    hipStream_t s = c->stream;
    u32* cnt = c->get<u32>("fd_cnt", (size_t)(np + 1) * ntiles);
    u64* tot = c->get<u64>("fd_tot", fnd::MAX_PATTERNS + 1);
    u64* tscan = c->get<u64>("fd_scan", (size_t)ntiles + 1);
    KOLM_HIP_CHECK(hipEventRecord(c->ev[6], s));
    {
        TScope t(c, KOLM_KT_EMIT, V::count_name, n);
        v.count(buf, n, lo, shi, cnt, s);
    }
    {
        TScope t(c, KOLM_KT_EMIT, "k_find_scan", sizeof(u32) * (u64)(np + 1) * ntiles);
        launch_find_scan(cnt, ntiles, np, tot, tscan, s);
    }
    KOLM_HIP_CHECK(hipEventRecord(c->ev[7], s));
    u64 htot[fnd::MAX_PATTERNS + 1] = {};
    KOLM_HIP_CHECK(hipMemcpyAsync(htot, tot, sizeof(u64) * (np + 1), hipMemcpyDeviceToHost, s));
    c->sync();
    ms += ev_ms(c->ev[6], c->ev[7]);
    for (u32 i = 0; i < np; ++i) counts[i] += htot[i];
    const u64 cap = std::min<u64>(fnd::stage_records(find_stage_bytes(), np), 0xFFFFFFFFull);
    u32* dpos = nullptr;
    u8* dwhich = nullptr;
    std::vector<u32> hpos;
    std::vector<u8> hwhich;
    emit_matches(
        c, ntiles, tscan, htot[np], offs.size(), limit, cap, more_than, launches, ms,
        [&](u64 slots) {
            dpos = c->get<u32>("fd_pos", slots);
            dwhich = c->get<u8>("fd_which", slots);
        },
        [&](u32 t0, u32 t1, u64 recs, u32 slots) {
            TScope t(c, KOLM_KT_EMIT, V::emit_name, (u64)(t1 - t0) * fnd::TILE + fnd::REC_BYTES * recs);
            v.emit(buf, n, lo, shi, t0, t1, tscan, dpos, dwhich, slots, s);
        },
        [&](u64 take) {
            hpos.resize(take), hwhich.resize(take);
            KOLM_HIP_CHECK(hipMemcpyAsync(hpos.data(), dpos, sizeof(u32) * take, hipMemcpyDeviceToHost, s));
            KOLM_HIP_CHECK(hipMemcpyAsync(hwhich.data(), dwhich, take, hipMemcpyDeviceToHost, s));
            c->sync();
            for (u64 k = 0; k < take; ++k) offs.push_back(base + hpos[k]);
            which.insert(which.end(), hwhich.begin(), hwhich.end());
        });
}

// The checks of a reader's search that precede every launch: the window, and that the device
// decodes every block that holds a byte of it.  Fills the plan and the stats' block figures.
int find_plan(const char* who, kolm_reader* r, u64 lo, u64 hi, RangePlan& p, kolm_find_stats& st) {
    if (lo > hi || hi > r->total) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: the window [%llu, %llu) is not inside the container's %llu bytes", who,
                 (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)r->total);
        set_err(msg);
        return KOLM_EARG;
    }
    const u64 wlen = hi - lo;
    if (int rc = range_plan(r->lens.data(), r->starts.data(), r->nb, &lo, &wlen, 1, 0, p)) return rc;
    return reader_check_blocks(r, p, st);
}

// The group loop of a reader's search (the caller holds the context's lock and has selected the
// device): the plan's blocks are decoded group by group (reader_decode_group), each group's bytes
// behind the carry of the groups before it, and search(scan buffer, its fnd::GroupScan) runs on
// every scan buffer in stream order.  L: the longest pattern (the hold-back).
template <class F>
int find_over_groups(kolm_reader* r, const RangePlan& p, u64 lo, u64 hi, u32 L, kolm_find_stats& st, F&& search) {
    kolm_ctx* c = r->c;
    hipStream_t s = c->stream;
    u8* keep = c->get<u8>("fd_carry", fnd::MAX_LEN);  // the carry between two groups' scan buffers
    GroupDecode w;
    u64 S = lo;
    u32 carry = 0;
    const u32 ng = (u32)p.group_first.size() - 1;
    for (u32 g = 0; g < ng; ++g) {
        // the scan buffer: room for the carry (it ends at a 256-byte boundary), the group's
        // decoded bytes there
        const int e = reader_decode_group(r, p, g, "fd_buf", fnd::MAX_LEN, w);
        st.ms_decode += w.ms_decode;
        if (e) return e;
        if (carry) KOLM_HIP_CHECK(hipMemcpyAsync(w.dec - carry, keep, carry, hipMemcpyDeviceToDevice, s));
        const u64 a = r->starts[p.sel[w.i0]], b = r->starts[p.sel[w.i0 + w.n - 1] + 1];
        const fnd::GroupScan gs = fnd::group_scan(S, a, b, L, g + 1 == ng, hi);
        st.bytes_scanned += gs.n;
        search(w.dec - gs.carry, gs);
        S = gs.S_next;
        carry = (u32)(b - S);  // < L: the bytes [S, b) end the scan buffer
        if (g + 1 < ng && carry) {
            KOLM_HIP_CHECK(hipMemcpyAsync(keep, w.dec + w.tot - carry, carry, hipMemcpyDeviceToDevice, s));
            c->sync();  // the next group may move the scan buffer
        }
    }
    return KOLM_OK;
}

// ---- class patterns (findcls_core.h, k_findcls.hip) ----

// np class patterns, pattern i = the 32-byte bitmaps [pat_off[i], pat_off[i + 1])
struct ClsSearch {
    static constexpr const char *count_name = "k_findcls_count", *emit_name = "k_findcls_emit";
    u32 np = 0, L = 0;
    fcl::Pats hp;
    const fcl::Pats* dP = nullptr;
    void upload(kolm_ctx* c) {
        fcl::Pats* d = c->get<fcl::Pats>("fc_pats", 1);
        KOLM_HIP_CHECK(hipMemcpyAsync(d, &hp, sizeof hp, hipMemcpyHostToDevice, c->stream));
        dP = d;
    }
    void count(const u8* buf, u32 n, u32 lo, u32 shi, u32* cnt, hipStream_t s) const {
        launch_findcls_count(buf, n, lo, shi, dP, np, cnt, s);
    }
    void emit(const u8* buf, u32 n, u32 lo, u32 shi, u32 t0, u32 t1, const u64* tscan, u32* dpos, u8* dwhich, u32 slots,
              hipStream_t s) const {
        launch_findcls_emit(buf, n, lo, shi, dP, np, t0, t1, tscan, dpos, dwhich, slots, s);
    }
};

// Classifies and deduplicates the classes into v.hp (no launch yet).
int findcls_check_pats(const char* who, const uint8_t* bitmaps, const uint32_t* pat_off, u32 np, ClsSearch& v) {
    v.np = np;
    if (int rc = check_pat_list(who, bitmaps, pat_off, np, KOLM_FIND_MAX_PATTERNS, "positions", &v.L)) return rc;
    u32 ntab = 0, bad_pat = 0, bad_pos = 0;
    if (!fcl::make_pats(bitmaps, pat_off, np, v.hp, &ntab, &bad_pat, &bad_pos)) {
        char msg[200];
        snprintf(msg, sizeof msg,
                 "%s: position %u of pattern %u is distinct table class %u of the call (at most %u classes that are no "
                 "masked equality)",
                 who, bad_pos, bad_pat, fcl::MAX_TABLES + 1, fcl::MAX_TABLES);
        set_err(msg);
        return KOLM_EARG;
    }
    return KOLM_OK;
}

// ---- regular expressions (findrx_core.h, k_findrx.hip) ----

// The automaton of a call, checked (frx::validate) and laid out as the kernels read it.
struct RxSearch {
    static constexpr const char *count_name = "k_findrx_count", *emit_name = "k_findrx_emit";
    std::vector<u8> img;  // the class map, then the table in whole 16-byte words
    frx::Starts st{};
    u32 nstates = 0, ncls = 0, np = 0;
    u32 L = 0;  // the hold-back, from the table itself
    const u8* dimg = nullptr;
    void upload(kolm_ctx* c) {
        u8* d = c->get<u8>("rx_img", img.size());
        KOLM_HIP_CHECK(hipMemcpyAsync(d, img.data(), img.size(), hipMemcpyHostToDevice, c->stream));
        dimg = d;
    }
    void count(const u8* buf, u32 n, u32 lo, u32 shi, u32* cnt, hipStream_t s) const {
        launch_findrx_count(buf, n, lo, shi, dimg, nstates, ncls, st, np, cnt, s);
    }
    void emit(const u8* buf, u32 n, u32 lo, u32 shi, u32 t0, u32 t1, const u64* tscan, u32* dpos, u8* dwhich, u32 slots,
              hipStream_t s) const {
        launch_findrx_emit(buf, n, lo, shi, dimg, nstates, ncls, st, np, t0, t1, tscan, dpos, dwhich, slots, s);
    }
};

int findrx_check(const char* who, const uint8_t* cls_map, const uint16_t* table, u32 nstates, u32 ncls, const uint16_t* starts,
                 u32 np, RxSearch& rx) {
    char why[200], msg[280];
    if (frx::validate(cls_map, table, nstates, ncls, starts, np, why, sizeof why)) {
        snprintf(msg, sizeof msg, "%s: %s", who, why);
        set_err(msg);
        return KOLM_EARG;
    }
    rx.nstates = nstates, rx.ncls = ncls, rx.np = np;
    rx.img.assign(frx::MAP + sizeof(uint16_t) * (size_t)frx::padded_entries(nstates, ncls), 0);
    memcpy(rx.img.data(), cls_map, frx::MAP);
    memcpy(rx.img.data() + frx::MAP, table, sizeof(uint16_t) * (size_t)nstates * ncls);
    for (u32 i = 0; i < np; ++i) rx.st.s[i] = starts[i];
    std::vector<u8> scratch(2 * (size_t)nstates);
    rx.L = frx::hold_back(table, nstates, ncls, starts, np, scratch.data());
    return KOLM_OK;
}

// The body of kolm_find_device, kolm_find_classes_device and kolm_find_dfa_device behind the
// variant's own check: one resident buffer, one find_group.  A refused call launches nothing.
template <class V>
int find_device_call(const char* who, kolm_ctx* c, V& v, const void* d_data, u64 n, u64 max_results, u64* counts, u64* offs,
                     u8* which, u64 cap, u64* nfound, double* ms) {
    const u32 np = v.np;
    if (n >= (1ull << 31)) {
        set_err(std::string(who) + ": the buffer must be smaller than 2^31 bytes");
        return KOLM_EARG;
    }
    if ((n && !d_data) || (cap && (!offs || (!which && np > 1)))) return KOLM_EARG;
    for (u32 i = 0; i < np; ++i) counts[i] = 0;
    if (n == 0) return KOLM_OK;
    return guarded([&] {
        std::lock_guard<std::mutex> g(c->mu);
        KOLM_HIP_CHECK(hipSetDevice(c->device));
        c->timing_reset();
        c->active = c->stream;
        v.upload(c);
        std::vector<u64> o;
        std::vector<u8> w;
        u32 launches = 0;
        double t = 0.0;
        u64 more = cap;
        find_group(c, v, static_cast<const u8*>(d_data), (u32)n, 0, (u32)n, 0, max_results, counts, o, w, launches, t, &more);
        if (c->timing) c->timing_collect_tail(0, nullptr);
        if (ms) *ms = t;
        if (more > cap) {
            *nfound = more;
            set_err(std::string(who) + ": result capacity too small");
            return KOLM_ECAP;
        }
        *nfound = o.size();
        std::copy(o.begin(), o.end(), offs);
        if (which) std::copy(w.begin(), w.end(), which);
        return KOLM_OK;
    });
}

// The body of kolm_reader_find, kolm_reader_find_classes and kolm_reader_find_dfa behind the
// variant's own check.  Every remaining check (the window, the selected blocks) precedes the first
// launch; no results leave a failed call.
template <class V>
int reader_find_call(const char* who, kolm_reader* r, V& v, u64 lo, u64 hi, u64 max_results, u64* counts, u64* nfound,
                     kolm_find_stats* stats) {
    const u32 np = v.np;
    RangePlan p;
    kolm_find_stats st{};
    st.patterns = np;
    if (int rc = find_plan(who, r, lo, hi, p, st)) return rc;
    for (u32 i = 0; i < np; ++i) counts[i] = 0;
    kolm_ctx* c = r->c;
    std::vector<u64> offs;
    std::vector<u8> which;
    int rc = guarded([&] {
        std::lock_guard<std::mutex> g(c->mu);
        r->f_offs.clear(), r->f_which.clear(), r->fs_offs.clear(), r->fs_which.clear();
        if (p.sel.empty()) return KOLM_OK;
        ReaderCall::enter(c);
        v.upload(c);
        if (int e = find_over_groups(r, p, lo, hi, v.L, st, [&](const u8* buf, const fnd::GroupScan& gs) {
                find_group(c, v, buf, gs.n, gs.lo, gs.shi, gs.start, max_results, counts, offs, which, st.emit_launches,
                           st.ms_find);
            }))
            return e;
        if (c->timing) c->timing_collect_tail(0, nullptr);
        return KOLM_OK;
    });
    if (rc) {
        for (u32 i = 0; i < np; ++i) counts[i] = 0;
        if (stats) *stats = st;
        return rc;
    }
    for (u32 i = 0; i < np; ++i) st.matches += counts[i];
    st.returned = offs.size();
    *nfound = offs.size();
    {
        std::lock_guard<std::mutex> g(c->mu);
        r->f_offs.swap(offs), r->f_which.swap(which);
    }
    if (stats) *stats = st;
    return KOLM_OK;
}

}  // namespace

extern "C" {

int kolm_find_device(kolm_ctx* c, const void* d_data, uint64_t n, const uint8_t* pats, const uint32_t* pat_off, uint32_t np,
                     uint64_t max_results, uint64_t* counts, uint64_t* offs, uint8_t* which, uint64_t cap,
                     uint64_t* nfound, double* ms) {
    if (ms) *ms = 0.0;
    if (nfound) *nfound = 0;
    if (!c || !counts || !nfound) return KOLM_EARG;
    LitSearch v;
    if (int rc = find_check_pats("kolm_find_device", pats, pat_off, np, v)) return rc;
    return find_device_call("kolm_find_device", c, v, d_data, n, max_results, counts, offs, which, cap, nfound, ms);
}

int kolm_reader_find(kolm_reader* r, const uint8_t* pats, const uint32_t* pat_off, uint32_t np, uint64_t lo, uint64_t hi,
                     uint64_t max_results, uint64_t* counts, uint64_t* nfound, kolm_find_stats* stats) {
    if (stats) *stats = kolm_find_stats{};
    if (nfound) *nfound = 0;
    if (!r || !r->c || !counts || !nfound) return KOLM_EARG;
    LitSearch v;
    if (int rc = find_check_pats("kolm_reader_find", pats, pat_off, np, v)) return rc;
    return reader_find_call("kolm_reader_find", r, v, lo, hi, max_results, counts, nfound, stats);
}

int kolm_reader_find_copy(kolm_reader* r, uint64_t first, uint64_t n, uint64_t* offs, uint8_t* which) {
    if (!r || !r->c) return KOLM_EARG;
    std::lock_guard<std::mutex> g(r->c->mu);
    if (first > r->f_offs.size() || n > r->f_offs.size() - first) {
        set_err("kolm_reader_find_copy: more results than the last find holds");
        return KOLM_EARG;
    }
    if (n && !offs) return KOLM_EARG;
    std::copy(r->f_offs.begin() + first, r->f_offs.begin() + first + n, offs);
    if (which) std::copy(r->f_which.begin() + first, r->f_which.begin() + first + n, which);
    return KOLM_OK;
}

int kolm_find_classes_device(kolm_ctx* c, const void* d_data, uint64_t n, const uint8_t* bitmaps, const uint32_t* pat_off,
                             uint32_t np, uint64_t max_results, uint64_t* counts, uint64_t* offs, uint8_t* which,
                             uint64_t cap, uint64_t* nfound, double* ms) {
    if (ms) *ms = 0.0;
    if (nfound) *nfound = 0;
    if (!c || !counts || !nfound) return KOLM_EARG;
    ClsSearch v;
    if (int rc = findcls_check_pats("kolm_find_classes_device", bitmaps, pat_off, np, v)) return rc;
    return find_device_call("kolm_find_classes_device", c, v, d_data, n, max_results, counts, offs, which, cap, nfound, ms);
}

int kolm_reader_find_classes(kolm_reader* r, const uint8_t* bitmaps, const uint32_t* pat_off, uint32_t np, uint64_t lo,
                             uint64_t hi, uint64_t max_results, uint64_t* counts, uint64_t* nfound, kolm_find_stats* stats) {
    if (stats) *stats = kolm_find_stats{};
    if (nfound) *nfound = 0;
    if (!r || !r->c || !counts || !nfound) return KOLM_EARG;
    ClsSearch v;
    if (int rc = findcls_check_pats("kolm_reader_find_classes", bitmaps, pat_off, np, v)) return rc;
    return reader_find_call("kolm_reader_find_classes", r, v, lo, hi, max_results, counts, nfound, stats);
}

int kolm_find_dfa_device(kolm_ctx* c, const void* d_data, uint64_t n, const uint8_t* cls_map, const uint16_t* table,
                         uint32_t nstates, uint32_t ncls, const uint16_t* starts, uint32_t np, uint64_t max_results,
                         uint64_t* counts, uint64_t* offs, uint8_t* which, uint64_t cap, uint64_t* nfound, double* ms) {
    if (ms) *ms = 0.0;
    if (nfound) *nfound = 0;
    if (!c || !counts || !nfound) return KOLM_EARG;
    RxSearch v;
    if (int rc = findrx_check("kolm_find_dfa_device", cls_map, table, nstates, ncls, starts, np, v)) return rc;
    return find_device_call("kolm_find_dfa_device", c, v, d_data, n, max_results, counts, offs, which, cap, nfound, ms);
}

int kolm_reader_find_dfa(kolm_reader* r, const uint8_t* cls_map, const uint16_t* table, uint32_t nstates, uint32_t ncls,
                         const uint16_t* starts, uint32_t np, uint64_t lo, uint64_t hi, uint64_t max_results,
                         uint64_t* counts, uint64_t* nfound, kolm_find_stats* stats) {
    if (stats) *stats = kolm_find_stats{};
    if (nfound) *nfound = 0;
    if (!r || !r->c || !counts || !nfound) return KOLM_EARG;
    RxSearch v;
    if (int rc = findrx_check("kolm_reader_find_dfa", cls_map, table, nstates, ncls, starts, np, v)) return rc;
    return reader_find_call("kolm_reader_find_dfa", r, v, lo, hi, max_results, counts, nfound, stats);
}

}  // extern "C"

// ---- search for a prepared pattern set (findset_core.h, k_findset.hip) ----
// The set owns its device tables (its own allocations: the context's named scratch may move with
// the next call) and the per-pattern counters of a call.
struct kolm_patset {
    kolm_ctx* c = nullptr;
    fst::Info info{};
    fst::Set dev{};  // the tables on the device
    u32 *d_filter = nullptr;
    fst::Slot* d_slots = nullptr;
    fst::Entry* d_entries = nullptr;
    u64 *d_blob = nullptr, *d_pcnt = nullptr;
};

namespace {

void patset_release(kolm_patset* ps) {
    for (void* q : {(void*)ps->d_filter, (void*)ps->d_slots, (void*)ps->d_entries, (void*)ps->d_blob, (void*)ps->d_pcnt})
        if (q) (void)hipFree(q);
}

// find_group for a set.  which: the pattern indices, 32 bits each; the per-pattern counters stay
// on the device (ps->d_pcnt) until the call ends.
void findset_group(kolm_ctx* c, const kolm_patset* ps, const u8* buf, u32 n, u32 lo, u32 shi, u64 base, u64 limit,
                   u64& matches, std::vector<u64>& offs, std::vector<u32>& which, u32& launches, double& ms,
                   u64* more_than = nullptr) {
    const u32 ntiles = fnd::tiles(n);
    if (!ntiles) return;
    hipStream_t s = c->stream;
    u32* cnt = c->get<u32>("fs_cnt", ntiles);
    u64* tot = c->get<u64>("fs_tot", 1);
    u64* tscan = c->get<u64>("fs_scan", (size_t)ntiles + 1);
    KOLM_HIP_CHECK(hipEventRecord(c->ev[6], s));
    {
        TScope t(c, KOLM_KT_EMIT, "k_findset_count", n);
        launch_findset_count(buf, n, lo, shi, ps->dev, cnt, ps->d_pcnt, s);
    }
    {
        TScope t(c, KOLM_KT_EMIT, "k_find_scan", sizeof(u32) * (u64)ntiles);
        launch_find_scan(cnt, ntiles, 0, tot, tscan, s);
    }
    KOLM_HIP_CHECK(hipEventRecord(c->ev[7], s));
    u64 total = 0;
    KOLM_HIP_CHECK(hipMemcpyAsync(&total, tot, sizeof(u64), hipMemcpyDeviceToHost, s));
    c->sync();
    ms += ev_ms(c->ev[6], c->ev[7]);
    matches += total;
    const u64 cap = std::min<u64>(fst::stage_records(find_stage_bytes(), ps->info.np), 0xFFFFFFFFull);
    uint2* drec = nullptr;
    std::vector<uint2> hrec;
    emit_matches(
        c, ntiles, tscan, total, offs.size(), limit, cap, more_than, launches, ms,
        [&](u64 slots) { drec = c->get<uint2>("fs_rec", slots); },
        [&](u32 t0, u32 t1, u64 recs, u32 slots) {
            TScope t(c, KOLM_KT_EMIT, "k_findset_emit", (u64)(t1 - t0) * fnd::TILE + fst::REC_BYTES * recs);
            launch_findset_emit(buf, n, lo, shi, ps->dev, t0, t1, tscan, drec, slots, s);
        },
        [&](u64 take) {
            hrec.resize(take);
            KOLM_HIP_CHECK(hipMemcpyAsync(hrec.data(), drec, sizeof(uint2) * take, hipMemcpyDeviceToHost, s));
            c->sync();
            for (u64 k = 0; k < take; ++k) offs.push_back(base + hrec[k].x), which.push_back(hrec[k].y);
        });
}

void findset_zero_counts(kolm_ctx* c, const kolm_patset* ps) {
    KOLM_HIP_CHECK(hipMemsetAsync(ps->d_pcnt, 0, sizeof(u64) * ps->info.np, c->stream));
}

// the counters back once, at the end of a call (counts may be NULL)
void findset_read_counts(kolm_ctx* c, const kolm_patset* ps, u64* counts) {
    if (!counts) return;
    KOLM_HIP_CHECK(hipMemcpyAsync(counts, ps->d_pcnt, sizeof(u64) * ps->info.np, hipMemcpyDeviceToHost, c->stream));
    c->sync();
}

}  // namespace

extern "C" {

int kolm_patset_create(kolm_ctx* c, const uint8_t* pats, const uint32_t* pat_off, uint32_t np, kolm_patset** out) {
    if (!out) return KOLM_EARG;
    *out = nullptr;
    if (!c) c = need_default();
    if (!c) return KOLM_ENOINIT;
    if (int rc = check_pat_list("kolm_patset_create", pats, pat_off, np, KOLM_FIND_SET_MAX_PATTERNS, "bytes", nullptr))
        return rc;
    char msg[160];
    fst::Tables T;
    u32 dup[2] = {0, 0};
    if (!fst::build(pats, pat_off, np, T, dup)) {
        snprintf(msg, sizeof msg, "kolm_patset_create: patterns %u and %u are equal (a set holds distinct patterns)", dup[0],
                 dup[1]);
        set_err(msg);
        return KOLM_EARG;
    }
    std::unique_ptr<kolm_patset> ps(new kolm_patset);
    ps->c = c;
    ps->info = T.info;
    int rc = guarded([&] {
        std::lock_guard<std::mutex> g(c->mu);
        KOLM_HIP_CHECK(hipSetDevice(c->device));
        c->active = c->stream;  // c->sync() below waits for the uploads
        auto up = [&](auto*& d, const auto& v) {
            KOLM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d), v.size() * sizeof(v[0])));
            KOLM_HIP_CHECK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, c->stream));
        };
        up(ps->d_filter, T.filter), up(ps->d_slots, T.slots), up(ps->d_entries, T.entries), up(ps->d_blob, T.blob);
        KOLM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ps->d_pcnt), sizeof(u64) * np));
        c->sync();  // the host tables go out of scope
        ps->dev = T.view();
        ps->dev.filter = ps->d_filter, ps->dev.slots = ps->d_slots, ps->dev.entries = ps->d_entries, ps->dev.blob = ps->d_blob;
        return KOLM_OK;
    });
    if (rc) {
        patset_release(ps.get());
        return rc;
    }
    *out = ps.release();
    return KOLM_OK;
}

void kolm_patset_free(kolm_patset* ps) {
    if (!ps) return;
    if (ps->c) {
        std::lock_guard<std::mutex> g(ps->c->mu);
        (void)hipSetDevice(ps->c->device);
        patset_release(ps);
    }
    delete ps;
}

int kolm_patset_info(const kolm_patset* ps, kolm_patset_info_t* out) {
    if (!ps || !out) return KOLM_EARG;
    *out = kolm_patset_info_t{ps->info.np,   ps->info.K, ps->info.keys,          ps->info.slots,
                              ps->info.filter_bits, ps->info.L, ps->info.longest_bucket};
    return KOLM_OK;
}

int kolm_find_set_device(kolm_ctx* c, const void* d_data, uint64_t n, const kolm_patset* ps, uint64_t max_results,
                         uint64_t* counts, uint64_t* offs, uint32_t* which, uint64_t cap, uint64_t* nfound, double* ms) {
    if (ms) *ms = 0.0;
    if (nfound) *nfound = 0;
    if (!c || !ps || !nfound) return KOLM_EARG;
    if (ps->c != c) {
        set_err("kolm_find_set_device: the pattern set belongs to another context");
        return KOLM_EARG;
    }
    if (n >= (1ull << 31)) {
        set_err("kolm_find_set_device: the buffer must be smaller than 2^31 bytes");
        return KOLM_EARG;
    }
    if ((n && !d_data) || (cap && (!offs || !which))) return KOLM_EARG;
    const u32 np = ps->info.np;
    if (counts)
        for (u32 i = 0; i < np; ++i) counts[i] = 0;
    if (n == 0) return KOLM_OK;
    return guarded([&] {
        std::lock_guard<std::mutex> g(c->mu);
        KOLM_HIP_CHECK(hipSetDevice(c->device));
        c->timing_reset();
        c->active = c->stream;
        findset_zero_counts(c, ps);
        std::vector<u64> o;
        std::vector<u32> w;
        u32 launches = 0;
        double t = 0.0;
        u64 more = cap, matches = 0;
        findset_group(c, ps, static_cast<const u8*>(d_data), (u32)n, 0, (u32)n, 0, max_results, matches, o, w, launches, t,
                      &more);
        findset_read_counts(c, ps, counts);
        if (c->timing) c->timing_collect_tail(0, nullptr);
        if (ms) *ms = t;
        if (more > cap) {
            *nfound = more;
            set_err("kolm_find_set_device: result capacity too small");
            return KOLM_ECAP;
        }
        *nfound = o.size();
        std::copy(o.begin(), o.end(), offs);
        std::copy(w.begin(), w.end(), which);
        return KOLM_OK;
    });
}

int kolm_reader_find_set(kolm_reader* r, const kolm_patset* ps, uint64_t lo, uint64_t hi, uint64_t max_results,
                         uint64_t* counts, uint64_t* nfound, kolm_find_stats* stats) {
    if (stats) *stats = kolm_find_stats{};
    if (nfound) *nfound = 0;
    if (!r || !r->c || !ps || !nfound) return KOLM_EARG;
    // every argument check before the first launch: the set's context, the window, the selected blocks
    if (ps->c != r->c) {
        set_err("kolm_reader_find_set: the pattern set and the reader belong to different contexts");
        return KOLM_EARG;
    }
    const u32 np = ps->info.np;
    RangePlan p;
    kolm_find_stats st{};
    st.patterns = np;
    if (int rc = find_plan("kolm_reader_find_set", r, lo, hi, p, st)) return rc;
    if (counts)
        for (u32 i = 0; i < np; ++i) counts[i] = 0;
    kolm_ctx* c = r->c;
    std::vector<u64> offs;
    std::vector<u32> which;
    std::vector<u64> hc(counts ? np : 0);
    u64 matches = 0;
    int rc = guarded([&] {
        std::lock_guard<std::mutex> g(c->mu);
        r->f_offs.clear(), r->f_which.clear(), r->fs_offs.clear(), r->fs_which.clear();
        if (p.sel.empty()) return KOLM_OK;
        ReaderCall::enter(c);
        findset_zero_counts(c, ps);
        if (int e = find_over_groups(r, p, lo, hi, ps->info.L, st, [&](const u8* buf, const fnd::GroupScan& gs) {
                findset_group(c, ps, buf, gs.n, gs.lo, gs.shi, gs.start, max_results, matches, offs, which, st.emit_launches,
                              st.ms_find);
            }))
            return e;
        findset_read_counts(c, ps, counts ? hc.data() : nullptr);
        if (c->timing) c->timing_collect_tail(0, nullptr);
        return KOLM_OK;
    });
    if (rc) {  // no results leave a failed call
        if (stats) *stats = st;
        return rc;
    }
    if (counts) std::copy(hc.begin(), hc.end(), counts);
    st.matches = matches;
    st.returned = offs.size();
    *nfound = offs.size();
    {
        std::lock_guard<std::mutex> g(c->mu);
        r->fs_offs.swap(offs), r->fs_which.swap(which);
    }
    if (stats) *stats = st;
    return KOLM_OK;
}

int kolm_reader_find_copy32(kolm_reader* r, uint64_t first, uint64_t n, uint64_t* offs, uint32_t* which) {
    if (!r || !r->c) return KOLM_EARG;
    std::lock_guard<std::mutex> g(r->c->mu);
    if (first > r->fs_offs.size() || n > r->fs_offs.size() - first) {
        set_err("kolm_reader_find_copy32: more results than the last find_set holds");
        return KOLM_EARG;
    }
    if (n && !offs) return KOLM_EARG;
    std::copy(r->fs_offs.begin() + first, r->fs_offs.begin() + first + n, offs);
    if (which) std::copy(r->fs_which.begin() + first, r->fs_which.begin() + first + n, which);
    return KOLM_OK;
}

// ---- open, close, read ----

int kolm_reader_open(kolm_ctx* c, const uint8_t* container, uint64_t cn, kolm_reader** out) {
    if (!out) return KOLM_EARG;
    *out = nullptr;
    if (!c) c = need_default();
    if (!c) return KOLM_ENOINIT;
    if (!container && cn) return KOLM_EARG;
    Toc t;
    if (int rc = toc_load(container, cn, t)) return rc;
    if (int rc = toc_check_length(t)) return rc;
    for (u32 i = 0; i < t.nb; ++i)
        if (t.poff[i + 1] < t.poff[i]) return KOLM_EFORMAT;
    std::unique_ptr<kolm_reader> r(new kolm_reader);
    r->c = c;
    r->mode = t.mode, r->size_field = t.size_field, r->total = t.total, r->nb = t.nb;
    r->starts.assign((size_t)r->nb + 1, 0);
    for (u32 i = 0; i < r->nb; ++i) r->starts[i + 1] = r->starts[i] + t.lens[i];
    r->methods.swap(t.methods), r->lens.swap(t.lens), r->poff.swap(t.poff);
    r->pbytes = r->nb ? r->poff[r->nb] - r->poff[0] : 0;
    int rc = guarded([&] {
        std::lock_guard<std::mutex> g(c->mu);
        KOLM_HIP_CHECK(hipSetDevice(c->device));
        KOLM_HIP_CHECK(hipMalloc((void**)&r->dpay, r->pbytes + 64 + rng::WORD));
        if (r->pbytes) {
            const hipError_t e = hipMemcpy(r->dpay, container + t.start + r->poff[0], r->pbytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(r->dpay);
                r->dpay = nullptr;
                KOLM_HIP_CHECK(e);
            }
        }
        return KOLM_OK;
    });
    if (rc) return rc;
    *out = r.release();
    return KOLM_OK;
}

int kolm_reader_close(kolm_reader* r) {
    if (!r) return KOLM_EARG;
    kolm_ctx* c = r->c;
    int rc = guarded([&] {
        std::lock_guard<std::mutex> g(c->mu);
        KOLM_HIP_CHECK(hipSetDevice(c->device));
        if (r->dpay) KOLM_HIP_CHECK(hipFree(r->dpay));
        return KOLM_OK;
    });
    delete r;
    return rc;
}

int kolm_reader_info(kolm_reader* r, uint64_t* info, uint32_t* methods, uint32_t* orig_lens, uint32_t cap) {
    if (!r || !info) return KOLM_EARG;
    info[0] = r->mode, info[1] = r->size_field, info[2] = r->total, info[3] = r->nb, info[4] = r->pbytes;
    if ((methods || orig_lens) && cap < r->nb) {
        set_err("kolm_reader_info: capacity too small");
        return KOLM_ECAP;
    }
    if (methods) std::copy(r->methods.begin(), r->methods.end(), methods);
    if (orig_lens) std::copy(r->lens.begin(), r->lens.end(), orig_lens);
    return KOLM_OK;
}

int kolm_reader_read(kolm_reader* r, const uint64_t* offs, const uint64_t* lens, uint32_t nranges, uint8_t* out,
                     uint64_t out_cap, kolm_read_stats* stats) {
    return reader_read(r, offs, lens, nranges, out, nullptr, out_cap, stats);
}

int kolm_reader_read_device(kolm_reader* r, const uint64_t* offs, const uint64_t* lens, uint32_t nranges, void* d_out,
                            uint64_t out_cap, kolm_read_stats* stats) {
    if (!d_out && nranges) {
        u64 want = 0;
        for (u32 i = 0; offs && lens && i < nranges; ++i) want += lens[i];
        if (want) return KOLM_EARG;
    }
    return reader_read(r, offs, lens, nranges, nullptr, d_out, out_cap, stats);
}

int kolm_reader_set_checksums(kolm_reader* r, const uint32_t* crc_in, uint32_t nblocks) {
    if (!r || !r->c) return KOLM_EARG;
    std::lock_guard<std::mutex> g(r->c->mu);
    if (!crc_in) {
        r->crcs.clear();
        return KOLM_OK;
    }
    if (nblocks != r->nb) {
        set_err("kolm_reader_set_checksums: the block count differs from the container's");
        return KOLM_EARG;
    }
    r->crcs.assign(crc_in, crc_in + nblocks);
    return KOLM_OK;
}

}  // extern "C"

// ---- line index: lines of a container on the device (lines_core.h, k_lines.hip, kolm_lines.cpp) ----
namespace {

void lines_message(u32 block, u32 expected, u32 got) {
    char msg[160];
    snprintf(msg, sizeof msg, "line index: block %u: expected %u delimiters, got %u", block, expected, got);
    set_err(msg);
}

// The plan whose selected blocks are `blocks` (ascending, distinct, none empty), grouped as a
// read's blocks are: one 1-byte range at each block's start.
int lines_plan(kolm_reader* r, const std::vector<u32>& blocks, RangePlan& p) {
    std::vector<u64> offs(blocks.size()), lens(blocks.size(), 1);
    for (size_t i = 0; i < blocks.size(); ++i) offs[i] = r->starts[blocks[i]];
    return range_plan(r->lens.data(), r->starts.data(), r->nb, offs.data(), lens.data(), (u32)blocks.size(), 0, p);
}

// The queries q (sorted by block; q[i].block = the container's block, never an empty one) answered
// group by group: res[i].  Each group's real counts are compared with the attached index first.
int lines_run(kolm_reader* r, std::vector<lin::Query>& q, std::vector<u32>& res, kolm_lines_stats& st) {
    st.queries = (u32)q.size();
    res.assign(q.size(), 0);
    if (q.empty()) return KOLM_OK;
    std::vector<u32> blocks, cb(q.size());  // cb: the queries' container block numbers
    for (size_t i = 0; i < q.size(); ++i) {
        cb[i] = q[i].block;
        if (blocks.empty() || blocks.back() != cb[i]) blocks.push_back(cb[i]);
    }
    RangePlan p;
    if (int rc = lines_plan(r, blocks, p)) return rc;
    if (int rc = reader_check_blocks(r, p, st)) return rc;
    kolm_ctx* c = r->c;
    return guarded([&] {
        ReaderCall call(c);
        GroupDecode w;
        std::vector<u32> hb, cnt;
        size_t q0 = 0;
        for (u32 gi = 0; gi + 1 < p.group_first.size(); ++gi) {
            const int e = reader_decode_group(r, p, gi, "rd_dec", 0, w);
            st.ms_decode += w.ms_decode;
            if (e) return e;
            const u32 i0 = w.i0, n = w.n, i1 = i0 + n;
            // the group's queries: q[q0, q1), their blocks renumbered to the group's slots
            size_t q1 = q0;
            u32 slot = 0;
            while (q1 < q.size() && cb[q1] <= p.sel[i1 - 1]) {
                while (p.sel[i0 + slot] != cb[q1]) ++slot;
                q[q1++].block = slot;
            }
            hb.assign((size_t)n + 1, 0);
            for (u32 i = 0; i < n; ++i) hb[i + 1] = hb[i] + w.gl[i];
            cnt.resize(n);
            lines_prepare(c, w.dec, w.tot, 0, hb.data(), n, r->ldelim, true, q.data() + q0, (u32)(q1 - q0));
            lines_launch(c, c->stream);
            st.ms_lines += lines_collect(c, cnt.data(), res.data() + q0);
            for (u32 i = 0; i < n; ++i)
                if (cnt[i] != r->lcounts[p.sel[i0 + i]]) {
                    lines_message(p.sel[i0 + i], r->lcounts[p.sel[i0 + i]], cnt[i]);
                    return KOLM_ELINES;
                }
            for (size_t i = q0; i < q1; ++i)
                if (res[i] == lin::NONE) {
                    lines_message(cb[i], r->lcounts[cb[i]], cnt[q[i].block]);
                    return KOLM_ELINES;
                }
            q0 = q1;
        }
        if (c->timing) c->timing_collect_tail(0, nullptr);
        return KOLM_OK;
    });
}

int lines_need_index(const char* who, kolm_reader* r) {
    if (r->has_lines) return KOLM_OK;
    set_err(std::string(who) + ": no line index is attached (kolm_reader_set_lines / kolm_reader_index_lines)");
    return KOLM_EARG;
}

}  // namespace

extern "C" {

int kolm_reader_set_lines(kolm_reader* r, uint32_t delim, const uint32_t* counts, uint32_t nblocks) {
    if (!r || !r->c) return KOLM_EARG;
    std::lock_guard<std::mutex> g(r->c->mu);
    if (!counts) {
        r->has_lines = false;
        r->lcounts.clear();
        return KOLM_OK;
    }
    if (delim > 0xFFu) {
        set_err("kolm_reader_set_lines: the delimiter is one byte value");
        return KOLM_EARG;
    }
    if (nblocks != r->nb) {
        set_err("kolm_reader_set_lines: the block count differs from the container's");
        return KOLM_EARG;
    }
    r->lcounts.assign(counts, counts + nblocks);
    r->ldelim = delim;
    r->has_lines = true;
    return KOLM_OK;
}

int kolm_reader_index_lines(kolm_reader* r, uint32_t delim, uint32_t* counts, uint32_t cap, kolm_lines_stats* stats) {
    if (stats) *stats = kolm_lines_stats{};
    if (!r || !r->c) return KOLM_EARG;
    if (delim > 0xFFu) {
        set_err("kolm_reader_index_lines: the delimiter is one byte value");
        return KOLM_EARG;
    }
    if (counts && cap < r->nb) {
        set_err("kolm_reader_index_lines: capacity too small");
        return KOLM_ECAP;
    }
    kolm_lines_stats st{};
    RangePlan p;
    const u64 lo = 0, len = r->total;
    if (int rc = range_plan(r->lens.data(), r->starts.data(), r->nb, &lo, &len, 1, 0, p)) return rc;
    if (int rc = reader_check_blocks(r, p, st)) return rc;
    std::vector<u32> all(r->nb, 0);
    kolm_ctx* c = r->c;
    int rc = guarded([&] {
        std::lock_guard<std::mutex> g(c->mu);
        if (p.sel.empty()) return KOLM_OK;
        ReaderCall::enter(c);
        GroupDecode w;
        std::vector<u32> hb, cnt;
        for (u32 gi = 0; gi + 1 < p.group_first.size(); ++gi) {
            const int e = reader_decode_group(r, p, gi, "rd_dec", 0, w);
            st.ms_decode += w.ms_decode;
            if (e) return e;
            const u32 i0 = w.i0, n = w.n;
            hb.assign((size_t)n + 1, 0);
            for (u32 i = 0; i < n; ++i) hb[i + 1] = hb[i] + w.gl[i];
            cnt.resize(n);
            lines_prepare(c, w.dec, w.tot, 0, hb.data(), n, delim, false);
            lines_launch(c, c->stream);
            st.ms_lines += lines_collect(c, cnt.data());
            for (u32 i = 0; i < n; ++i) all[p.sel[i0 + i]] = cnt[i];
        }
        if (c->timing) c->timing_collect_tail(0, nullptr);
        return KOLM_OK;
    });
    if (stats) *stats = st;
    if (rc) return rc;
    {
        std::lock_guard<std::mutex> g(c->mu);
        r->lcounts = all;
        r->ldelim = delim;
        r->has_lines = true;
    }
    if (counts) std::copy(all.begin(), all.end(), counts);
    return KOLM_OK;
}

int kolm_reader_line_spans(kolm_reader* r, const uint64_t* lines, uint32_t n, uint64_t* starts, uint64_t* ends,
                           kolm_lines_stats* stats) {
    if (stats) *stats = kolm_lines_stats{};
    if (!r || !r->c || (n && (!lines || !starts || !ends))) return KOLM_EARG;
    if (int rc = lines_need_index("kolm_reader_line_spans", r)) return rc;
    // every argument check before the first launch: the lines, the selected blocks
    std::vector<u64> prefix;
    lines_prefix(r->lcounts.data(), r->nb, prefix);
    const u64 D = prefix[r->nb];
    std::vector<u64> need;  // the delimiters whose positions the spans are made of, each once
    for (u32 i = 0; i < n; ++i) {
        if (lines[i] > D) {
            char msg[160];
            snprintf(msg, sizeof msg, "kolm_reader_line_spans: entry %u: line %llu of %llu", i, (unsigned long long)lines[i],
                     (unsigned long long)(D + 1));
            set_err(msg);
            return KOLM_EARG;
        }
        if (lines[i] > 0) need.push_back(lines[i] - 1);
        if (lines[i] < D) need.push_back(lines[i]);
    }
    std::sort(need.begin(), need.end());
    need.erase(std::unique(need.begin(), need.end()), need.end());
    std::vector<lin::Query> q(need.size());  // ascending delimiter numbers: sorted by block
    for (size_t i = 0; i < need.size(); ++i) {
        const u32 b = lines_block_of(prefix, need[i]);
        q[i] = lin::Query{b, (u32)(need[i] - prefix[b]), lin::OP_SELECT};
    }
    const std::vector<lin::Query> asked = q;
    kolm_lines_stats st{};
    std::vector<u32> res;
    const int rc = lines_run(r, q, res, st);
    if (stats) *stats = st;
    if (rc) return rc;  // no results leave a failed call
    auto pos = [&](u64 k) {
        const size_t i = (size_t)(std::lower_bound(need.begin(), need.end(), k) - need.begin());
        return r->starts[asked[i].block] + res[i];
    };
    for (u32 i = 0; i < n; ++i) {
        starts[i] = lines[i] ? pos(lines[i] - 1) + 1 : 0;
        ends[i] = lines[i] < D ? pos(lines[i]) : r->total;
    }
    return KOLM_OK;
}

int kolm_reader_line_of(kolm_reader* r, const uint64_t* offs, uint32_t n, uint64_t* lines, kolm_lines_stats* stats) {
    if (stats) *stats = kolm_lines_stats{};
    if (!r || !r->c || (n && (!offs || !lines))) return KOLM_EARG;
    if (int rc = lines_need_index("kolm_reader_line_of", r)) return rc;
    std::vector<u64> prefix;
    lines_prefix(r->lcounts.data(), r->nb, prefix);
    // (block, offset in it) of every offset that needs a decode, each once, sorted by block
    std::vector<std::pair<u32, u32>> at(n), need;
    for (u32 i = 0; i < n; ++i) {
        if (offs[i] > r->total) {
            char msg[160];
            snprintf(msg, sizeof msg, "kolm_reader_line_of: entry %u: offset %llu is not inside the container's %llu bytes", i,
                     (unsigned long long)offs[i], (unsigned long long)r->total);
            set_err(msg);
            return KOLM_EARG;
        }
        const u32 b = offs[i] == r->total
                          ? r->nb
                          : (u32)(std::upper_bound(r->starts.begin(), r->starts.end(), offs[i]) - r->starts.begin()) - 1;
        at[i] = {b, (u32)(offs[i] - r->starts[b])};
        if (at[i].second) need.push_back(at[i]);  // a block's start, the stream's end: the prefix sum alone
    }
    std::sort(need.begin(), need.end());
    need.erase(std::unique(need.begin(), need.end()), need.end());
    std::vector<lin::Query> q(need.size());
    for (size_t i = 0; i < need.size(); ++i) q[i] = lin::Query{need[i].first, need[i].second, lin::OP_RANK};
    kolm_lines_stats st{};
    std::vector<u32> res;
    const int rc = lines_run(r, q, res, st);
    if (stats) *stats = st;
    if (rc) return rc;
    for (u32 i = 0; i < n; ++i) {
        lines[i] = prefix[at[i].first];
        if (at[i].second) lines[i] += res[(size_t)(std::lower_bound(need.begin(), need.end(), at[i]) - need.begin())];
    }
    return KOLM_OK;
}

}  // extern "C"
