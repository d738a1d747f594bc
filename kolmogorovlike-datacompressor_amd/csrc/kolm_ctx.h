// struct kolm_ctx and what the host files that drive it share: kolm_api.cpp (encode, decode,
// verify, dedup, checksums, line counts) and kolm_reader.cpp (readers, searches, pattern sets).
// Private to those two files; everything else sees kolm_ctx as an opaque type.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/kolm.h"
#include "kolm_internal.h"

using namespace kolm;  // kolm_ctx is the C ABI's type (global scope) and speaks the internal names

namespace kolm {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

// Host-side copy workers for the pinned staging buffers: a host buffer of the caller
// (pageable) is copied into pinned memory by several threads at once, so the DMA engine
// sees pinned memory and the host side keeps up with PCIe (one thread's memcpy does not).
class CopyPool {
  public:
    explicit CopyPool(unsigned n) {
        for (unsigned i = 0; i < n; ++i) th_.emplace_back([this] { loop(); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    // dst[0, n) = src[0, n), split over the workers and the calling thread
    void copy(void* dst, const void* src, size_t n) {
        const size_t parts = th_.size() + 1, piece = ((n + parts - 1) / parts + 4095) & ~(size_t)4095;
        std::vector<Job> jobs;
        for (size_t o = piece; o < n; o += piece)
            jobs.push_back({(char*)dst + o, (const char*)src + o, std::min(piece, n - o)});
        {
            std::lock_guard<std::mutex> g(mu_);
            for (auto& j : jobs) q_.push_back(j);
            pending_ += jobs.size();
        }
        cv_.notify_all();
        std::memcpy(dst, src, std::min(piece, n));
        std::unique_lock<std::mutex> g(mu_);
        done_cv_.wait(g, [this] { return pending_ == 0; });
    }

  private:
    struct Job {
        char* d;
        const char* s;
        size_t n;
    };
    void loop() {
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [this] { return stop_ || !q_.empty(); });
                if (stop_ && q_.empty()) return;
                j = q_.back();
                q_.pop_back();
            }
            std::memcpy(j.d, j.s, j.n);
            std::lock_guard<std::mutex> g(mu_);
            if (--pending_ == 0) done_cv_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::vector<Job> q_;
    size_t pending_ = 0;
    bool stop_ = false;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
};

// counter slots in the device counter array
enum : int {
    C_CLS = 0,       // 12 slots
    C_NEXT = 12,
    C_EQ = 13,
    C_ACTIVE = 14,
    C_ALPHA = 15,    // round 0: max code width of the batch
    C_L0SEG = 16,
    C_L0TILE = 17,
    C_L1SEG = 18,
    C_L1TILE = 19,
    C_STATUS = 20,
    C_NLONG = 21,
    C_RICE = 22,
    C_NFIX = 23,     // LZ77 stitch fix-up tokens (statistics)
    C_CLSE = 24,     // 12 slots: elements per small class
    C_L0ELEM = 36,
    C_L1ELEM = 37,
    C_LMAX = 38,     // the round's longest large segment
    C_CDC = 40,      // FastCDC cut count
    C_N = 48,
    H_RSUM = C_N,    // host mirror only (2 words): summed per-block cyclic rounds
    H_ALPHA = C_N + 4,  // host mirror only: the batch's code width from the early alphabet pass
    H_N = C_N + 16
};

// Milliseconds between two recorded events the device has already passed.  A batch's results
// reach the host through coherent host words (read_spans), which the host can see before the
// runtime has retired the events of the same stream: on hipErrorNotReady wait for the runtime
// (no device wait is left) and ask again.  The usual case costs nothing extra.
inline float event_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    hipError_t e = hipEventElapsedTime(&ms, a, b);
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        KOLM_HIP_CHECK(hipEventSynchronize(a));
        KOLM_HIP_CHECK(hipEventSynchronize(b));
        e = hipEventElapsedTime(&ms, a, b);
    }
    KOLM_HIP_CHECK(e);
    return ms;
}

// Records a HIP event pair around the launches in its scope (timing enabled only).
struct TScope {
    kolm_ctx* c;
    int fam;
    const char* name;  // kernel symbol (as rocprof shows it, namespaces stripped)
    u64 bytes;
    hipEvent_t a = nullptr;
    TScope(kolm_ctx* c_, int fam_, const char* name_, u64 bytes_);
    ~TScope() noexcept(false);
};

}  // namespace kolm

struct kolm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  // main stream
    hipStream_t aux = nullptr;     // second stream: Lyndon + cyclic sort chain runs beside LZ77
    hipStream_t active = nullptr;  // stream used by launches / TScope / sync()
    hipStream_t rp = nullptr;      // third stream: Re-Pair (candidate 9), one workgroup per block
    bool serial = false;           // every launch of a batch on one stream (kolm_ctx_set_serial; KOLM_SERIAL=1)
    // verify-after-encode (kolm_ctx_set_verify; KOLM_VERIFY=1): every encode batch is decoded and
    // compared with its text before the call returns; vrep accumulates over the batches of one
    // call (vrep.blocks = blocks checked so far), vshard = the call's first block within a
    // multi-device encode
    bool verify = false;
    kolm_verify_report vrep{};
    u32 vshard = 0;
    // dedup (kolm_ctx_set_dedup; KOLM_DEDUP=1): every encode batch encodes each distinct block
    // once (encode_batch in kolm_api.cpp); drep accumulates over the batches of one call
    bool dedup = false;
    kolm_dedup_report drep{};
    hipEvent_t evd[2] = {};        // dedup: the event pair around its kernels
    // checksums (kolm_ctx_set_checksums; KOLM_CHECKSUMS=1): every encode batch takes the CRC-32 of
    // its blocks on the resident text (crc_enqueue / crc_collect in kolm_api.cpp); ccrc accumulates
    // over the batches of one call.  The rest is the state of one CRC pass, used by every caller of
    // the pair under the context lock: the table words on the device (an allocation of its own, made
    // at the first pass: the per-batch clean-up of the named buffers never touches it), the host
    // arrays the pass's uploads read (alive until the pass is collected), the pinned landing
    // buffer of the raw words and the events around the kernel and behind the read-back
    bool checksums = false;
    std::vector<u32> ccrc;
    struct CrcPass {
        u32* d_tab = nullptr;
        u32* h_raw = nullptr;
        size_t h_cap = 0;
        std::vector<u32> hb, scan;  // block bounds (nb + 1) and the scan of the run counts
        u32 nb = 0;
        // what crc_prepare leaves for crc_launch: the text, its geometry and the raw words' buffer
        const u8* text = nullptr;
        u64 N = 0;
        u32 bs = 0;
        bool var = false;
        u32* draw = nullptr;
        bool armed = false;     // prepared, not launched yet
        bool launched = false;
        hipEvent_t ev[3] = {};  // kernel start, kernel end, words on the host
    } crc;
    // line index (kolm_ctx_set_lines; KOLM_LINES=1, KOLM_LINES_DELIM): every encode batch counts the
    // bytes equal to lines_delim in its blocks on the resident text (lines_prepare / lines_launch /
    // lines_collect in kolm_api.cpp: the CRC pass's shape, launched where that pass is); clines accumulates
    // over the batches of one call.  The rest is the state of one counting pass, used by every
    // caller under the context lock.
    bool lines = false;
    u32 lines_delim = 0x0A;
    std::vector<u32> clines;
    struct LinePass {
        u32* h_cnt = nullptr;  // pinned landing buffer of the counts
        size_t h_cap = 0;
        std::vector<u32> hb, scan, pbase;  // block bounds, the scans of the run and of the piece counts (nb + 1 each)
        u32 nb = 0;
        const u8* text = nullptr;
        u64 N = 0;
        u32 bs = 0, delim = 0;
        bool var = false;
        bool pieces = false;    // also the 4 KiB pieces' counts ("lin_pcnt", at "lin_pbase") and their scan
        const lin::Query* q = nullptr;  // with pieces: the queries answered behind the scan
        u32 nq = 0;
        u32* dcnt = nullptr;
        bool armed = false;     // prepared, not launched yet
        bool launched = false;
        hipEvent_t ev[3] = {};  // kernel start, kernel end, counts on the host
    } lin;
    // Lyndon fast route (kolm_ctx_lyndon_report): the last batch's block count, whether the fast
    // route ran and the stream it ran on; the route words stay in the "lyn_route" buffer
    u32 lyn_nb = 0;
    bool lyn_fast = false;
    hipStream_t lyn_stream = nullptr;
    // pinned host staging: an upload ring (input chunks) and the result buffer of
    // kolm_compress_fixed (container bytes, valid until the next call on this context)
    static constexpr int NSTAGE = 4;
    u8* stage[NSTAGE] = {};
    hipEvent_t stage_ev[NSTAGE] = {};
    u8* h_res = nullptr;
    size_t h_res_cap = 0, h_res_len = 0, h_res_off = 0;  // the container is h_res[off, off + len)
    hipStream_t up = nullptr, dl = nullptr;  // kolm_compress_fixed: upload / download streams
    hipEvent_t up_ev = nullptr;
    std::unique_ptr<CopyPool> pool;
    hipEvent_t evj[4] = {};        // join events
    hipEvent_t evr[2] = {};        // Re-Pair start / done
    hipEvent_t evg[2] = {};        // early BBWT gather: slots marked / gathered
    hipEvent_t eva = nullptr;      // the early alphabet pass's width copied to the host
    std::mutex mu;
    std::map<std::string, DevBuf> bufs;
    u32* h_cnt = nullptr;  // pinned mirror of the counters
    // fine-grained (coherent) host words small device results are stored into by k_spans_to_host
    // (read_spans below): RT_WORDS result words, then one sequence word per wave
    u32* h_rt = nullptr;
    u32* d_rt = nullptr;  // the same buffer as the device addresses it
    u32 rt_seq = 0;
    // pinned landing buffer of a batch's packed small results (one device-to-host copy per
    // host round trip instead of one per array: each copy is a blit launch of ~15-25 us)
    u32* h_tail = nullptr;
    size_t h_tail_cap = 0;
    u32* tail_host(size_t words) {
        if (words > h_tail_cap) {
            if (h_tail) KOLM_HIP_CHECK(hipHostFree(h_tail));
            h_tail = nullptr;
            h_tail_cap = 0;
            const size_t cap = std::max<size_t>(words + (words >> 2), 4096);
            KOLM_HIP_CHECK(hipHostMalloc((void**)&h_tail, cap * sizeof(u32), hipHostMallocDefault));
            h_tail_cap = cap;
        }
        return h_tail;
    }
    hipEvent_t ev[8] = {};
    // per-launch timing of kernel families (kolm_ctx_set_timing)
    bool timing = false;
    std::vector<hipEvent_t> evpool;
    size_t evused = 0;
    struct Pend {
        int fam;
        const char* name;
        hipEvent_t a, b;
        u64 bytes;
        int strm;  // 0 index stream, 1 sort stream, 2 Re-Pair stream
    };
    int strm_of(hipStream_t s) const { return s == aux ? 1 : s == rp ? 2 : 0; }
    std::vector<Pend> pend;
    struct Acc {
        double ms = 0;
        u64 launches = 0, bytes = 0;
        int fam = 0;   // KOLM_KT_* family of the kernel
        int strm = 0;  // stream of its last launch (Pend::strm)
    };
    std::map<std::string, Acc> kacc;  // per kernel, accumulated while timing is enabled
    // KTimer for multi-kernel launchers: events on the active stream, nested scopes allowed
    struct Hook : KTimer {
        kolm_ctx* c = nullptr;
        struct Open {
            int fam;
            const char* name;
            u64 bytes;
            hipEvent_t a;
        };
        std::vector<Open> open;
        void begin(int fam, const char* name, u64 bytes) override {
            hipEvent_t a = c->ev_take();
            KOLM_HIP_CHECK(hipEventRecord(a, c->active));
            open.push_back({fam, name, bytes, a});
        }
        void end() override {
            Open o = open.back();
            open.pop_back();
            hipEvent_t b = c->ev_take();
            KOLM_HIP_CHECK(hipEventRecord(b, c->active));
            c->pend.push_back({o.fam, o.name, o.a, b, o.bytes, c->strm_of(c->active)});
        }
    } hook;
    KTimer* kt() {
        hook.c = this;
        return timing ? &hook : nullptr;
    }
    hipEvent_t ev_take() {
        if (evused == evpool.size()) {
            hipEvent_t e;
            KOLM_HIP_CHECK(hipEventCreate(&e));
            evpool.push_back(e);
        }
        return evpool[evused++];
    }
    void timing_reset() {
        pend.clear();
        evused = 0;
    }
    void timing_add(const Pend& p, kolm_stats* st) {
        const float ms = event_ms(p.a, p.b);
        if (st) {
            st->kt[p.fam].ms += ms;
            st->kt[p.fam].launches += 1;
            st->kt[p.fam].bytes += p.bytes;
        }
        Acc& a = kacc[p.name];
        a.fam = p.fam;
        a.strm = p.strm;
        a.ms += ms;
        a.launches += 1;
        a.bytes += p.bytes;
    }
    void timing_collect(kolm_stats* st) {
        for (auto& p : pend) timing_add(p, st);
        timing_reset();
    }
    // only the launches recorded since pend held p0 entries (the verify step, which runs after
    // a batch's own collection or without one); st optional
    void timing_collect_tail(size_t p0, kolm_stats* st) {
        for (size_t i = p0; i < pend.size(); ++i) timing_add(pend[i], st);
        pend.resize(p0);
    }

    void* raw(const char* name, size_t bytes) {
        DevBuf& b = bufs[name];
        if (bytes == 0) bytes = 16;
        if (b.cap < bytes) {
            if (b.p) KOLM_HIP_CHECK(hipFree(b.p));
            b.p = nullptr;
            const size_t cap = (bytes + 255) & ~(size_t)255;
            KOLM_HIP_CHECK(hipMalloc(&b.p, cap));
            b.cap = cap;
        }
        return b.p;
    }
    template <class T>
    T* get(const char* name, size_t count) {
        return static_cast<T*>(raw(name, count * sizeof(T)));
    }
    u64 bytes_held(const char* name) const {
        const auto it = bufs.find(name);
        return it == bufs.end() ? 0 : it->second.cap;
    }
    // Small device results back to the host (the doubling rounds' counters, the batch's
    // offsets / winners / sizes): k_spans_to_host stores the spans into coherent host memory
    // and then each wave's sequence word (system-scope release), and the host spins on those
    // words — no blit dispatch and no stream query between the last kernel and the host's next
    // launch.  A stream error, or a finished stream without the words, ends the wait with an
    // error.  Returns the spans' words (h_rt[o[k] + j]).
    static constexpr u32 RT_WORDS = 16384;  // h_rt: RT_WORDS result words, then 4 sequence words
    const u32* read_spans(const kolm::PackSpans& ps, hipStream_t s) {
        const u32 seq = ++rt_seq;
        const u32 waves = kolm::launch_spans_to_host(ps, d_rt, d_rt + RT_WORDS, seq, s);
        volatile u32* f = h_rt + RT_WORDS;
        for (u32 w = 0, it = 1; w < waves; ++it) {
            if (f[w] == seq) {
                ++w;
                continue;
            }
            if (it % 1024 == 0) {
                const hipError_t e = hipStreamQuery(s);
                if (e != hipErrorNotReady) {
                    KOLM_HIP_CHECK(e);
                    if (f[w] != seq)
                        throw kolm::HipError(hipErrorUnknown, "result words not seen after the stream finished", __LINE__);
                }
            }
            __builtin_ia32_pause();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        return h_rt;
    }
    static bool fits_rt(const kolm::PackSpans& ps) {
        u64 end = 0;
        for (int k = 0; k < 6; ++k)
            if (ps.p[k]) end = std::max<u64>(end, (u64)ps.o[k] + ps.n[k]);
        return end <= RT_WORDS;
    }
    void read_counts(u32* h, const u32* cnt, u32 n, hipStream_t s) {
        kolm::PackSpans ps{};
        ps.p[0] = cnt, ps.n[0] = n, ps.o[0] = 0;
        const volatile u32* r = read_spans(ps, s);
        for (u32 i = 0; i < n; ++i) h[i] = r[i];
    }
    // Host round trips (per-round counters) spin on the stream instead of sleeping in
    // hipStreamSynchronize: the sort stream idles for the host's wake-up otherwise.
    void sync() {
        static const bool block = getenv("KOLM_SYNC_BLOCK") && atoi(getenv("KOLM_SYNC_BLOCK"));
        if (block) {
            KOLM_HIP_CHECK(hipStreamSynchronize(active));
            return;
        }
        hipError_t e;
        while ((e = hipStreamQuery(active)) == hipErrorNotReady) {
        }
        KOLM_HIP_CHECK(e);
    }
};

namespace kolm {

inline TScope::TScope(kolm_ctx* c_, int fam_, const char* name_, u64 bytes_) : c(c_), fam(fam_), name(name_), bytes(bytes_) {
    if (c->timing) {
        a = c->ev_take();
        KOLM_HIP_CHECK(hipEventRecord(a, c->active));
    }
}
inline TScope::~TScope() noexcept(false) {
    if (c->timing) {
        hipEvent_t b = c->ev_take();
        KOLM_HIP_CHECK(hipEventRecord(b, c->active));
        c->pend.push_back({fam, name, a, b, bytes, c->strm_of(c->active)});
    }
}

// The message's text is part of the library's behaviour and says "kolm_api line": the line is one
// of kolm_api.cpp, kolm_reader.cpp or this header, wherever the failing HIP call stands.
template <class F>
int guarded(F&& f) {
    try {
        return f();
    } catch (const HipError& e) {
        char buf[256];
        snprintf(buf, sizeof buf, "HIP error %d (%s) at kolm_api line %d: %s", (int)e.err,
                 hipGetErrorString(e.err), e.line, e.what);
        set_err(buf);
        return KOLM_EHIP;
    } catch (const std::bad_alloc&) {
        set_err("host allocation failed");
        return KOLM_EHIP;
    }
}

// ---- defined in kolm_api.cpp, used by the reader as well ----
kolm_ctx* need_default();  // the context of kolm_init, or null
float ev_ms(hipEvent_t a, hipEvent_t b);
// Decodes nb blocks whose payloads are resident at dpay (+ payload_off[i] - payload_off[0]) into
// dout (device), every kernel on the context stream; returns with the stream drained.
int decode_batch(kolm_ctx* c, const u8* dpay, const uint64_t* payload_off, const uint32_t* methods,
                 const uint32_t* orig_lens, u32 nb, u64 total, u8* dout, double* ms,
                 std::vector<u32>* status_out = nullptr, const u32** d_obase = nullptr);
// the CRC-32 of the blocks of lengths lens[0, n) that lie back to back at d: out[0, n)
double crc_blocks_at(kolm_ctx* c, const u8* d, const u32* lens, u32 n, u32* out);
void checksum_message(u32 block, u32 method, u32 expected, u32 got);
// one delimiter-counting pass (and its queries) over resident blocks
void lines_prepare(kolm_ctx* c, const u8* d_text, u64 N, u32 bs, const u32* hb, u32 nb, u32 delim, bool pieces,
                   const lin::Query* q = nullptr, u32 nq = 0);
void lines_launch(kolm_ctx* c, hipStream_t s);
double lines_collect(kolm_ctx* c, u32* out, u32* res = nullptr);

// ---- defined in kolm_reader.cpp, used by dedup's compaction as well ----
// Uploads a segment table with the exclusive scan of its item counts and launches k_range_gather
// on c->stream between the event pair (e0, e1).  Scratch: "<name>_seg", "<name>_scan".
void gather_segments(kolm_ctx* c, const char* name, const u8* src, u8* dst, const rng::Seg* segs, u32 nseg,
                     std::vector<u32>& scan, hipEvent_t e0, hipEvent_t e1);

// ---- kolm_api.cpp: a container's table of contents on the host (kolm_toc_read) ----
struct Toc {
    u32 mode = 0, size_field = 0, nb = 0;
    u64 total = 0;  // the header's total_len
    u64 start = 0;  // the payload area's offset in the container
    u64 sum = 0;    // what the blocks' lengths add up to
    std::vector<u32> methods, lens;  // nb entries each
    std::vector<u64> poff;           // nb + 1 payload offsets
};
int toc_load(const uint8_t* container, uint64_t cn, Toc& t);
// KOLM_EFORMAT ("Length mismatch: ...") unless the lengths add up to total_len
int toc_check_length(const Toc& t);

}  // namespace kolm
