/* kolm.h — C ABI of libkolm_hip.so, the MI355X (gfx950) block-transform hot path of
 * KolmogorovLike-DataCompressor v2-2.
 *
 * Reference interfaces replaced (PY = final_researched/kolm_final_researched_v2-2.py):
 *   kolm_bbwt_forward      <- bbwt_forward(bytes)->bytes                PY:351-423
 *   kolm_mtf_encode        <- mtf_encode(bytes)->List[int]              PY:460-468
 *   kolm_rice_encode       <- rice_encode(seq, k)->bytes                PY:1413-1421
 *   kolm_lz77_encode       <- encode_lz77(bytes)->(bytes, {})           PY:1686-1763
 *   kolm_bbwt_mtf_rice     <- encode_bbwt_mtf_rice(block, flags, k=2)   PY:2028-2073
 *   kolm_encode_blocks     <- the per-block MDL loop of compress_blocks_fixed
 *                             (candidates 0..9 of _select_encoders, argmin with
 *                             ties -> lowest id)                        PY:2152-2178, 2332-2369
 *                             candidate 9 = repair_compress            PY:1817-1911
 *   kolm_encode_blocks_device: same, input already resident in device memory
 *                             (bench / multi-GPU path; PY has no equivalent).
 *   kolm_encode_blocks_multi: same as kolm_encode_blocks over several devices of one
 *                             process (contiguous block shards, one host thread and
 *                             context per device).
 *   kolm_toc_write / kolm_toc_read: the KOLR container's header + TOC on the host
 *                             (PY:2375-2445 writer, PY:2451-2530 reader; kolm_toc.cpp).
 *   kolm_find_device / kolm_reader_find: search of decoded bytes on the device (PY has none)
 *   kolm_patset_create / kolm_find_set_device / kolm_reader_find_set: the same for a prepared set of
 *     up to 65 536 patterns in one pass (PY has none)
 *   kolm_reader_* / kolm_range_plan: random-access reads of a container (PY has no
 *                             equivalent: decompress, PY:2451-2550, decodes every block): only
 *                             the blocks a byte range touches are decoded, the ranges are packed
 *                             on the device (k_range.hip, kolm_range.cpp).
 *   kolm_*_dedup* / kolm_dedup_plan: encode the repeated blocks of a batch once (PY has no
 *                             equivalent: the loop at PY:2350-2369 encodes every block); opt-in,
 *                             outputs byte-identical (k_dedup.hip, kolm_dedup.cpp).
 *   kolm_comm_* / kolm_gather_payloads: RCCL over xGMI (kolm_comm.cpp) — the reassembly
 *                             of independently encoded block shards (PY:2350-2369 blocks,
 *                             PY:2375-2445 the container they feed) onto one rank.
 *
 * Conventions: plain pointers and sizes; caller-allocated buffers with explicit
 * capacities; every function returns 0 (KOLM_OK) or a negative code; no exception
 * crosses the ABI.  One context per device; calls on one context are serialised
 * (internally locked).  The free functions (kolm_bbwt_forward, ...) use the default
 * context created by kolm_init().
 */
#ifndef KOLM_H
#define KOLM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KOLM_OK 0
#define KOLM_EARG (-1)     /* bad argument */
#define KOLM_ECAP (-2)     /* output capacity too small */
#define KOLM_EHIP (-3)     /* HIP runtime error (message: kolm_last_error) */
#define KOLM_ERCCL (-4)    /* RCCL (collective) error (message: kolm_last_error) */
#define KOLM_ENOINIT (-5)  /* kolm_init not called */
#define KOLM_EFORMAT (-6)  /* malformed container (message: PY's ValueError text) */
#define KOLM_ERANGE (-7)   /* a container field overflows (PY: struct.error) */
#define KOLM_EVERIFY (-8)  /* verify on: an encode entry point produced a payload that does not
                              decode to its input (message names block, method, offset) */
#define KOLM_ECHECKSUM (-9) /* decoded bytes do not match the expected CRC-32 (message: block,
                              method, expected, got) */
#define KOLM_ELINES (-10)   /* the attached line index does not describe the decoded bytes (message:
                              block, expected count, actual count) */

/* Candidate method ids (index into PY _select_encoders(), PY:2152-2165). */
#define KOLM_M_RAW 0
#define KOLM_M_XOR 1
#define KOLM_M_BBWT 2
#define KOLM_M_BBWT_BP 3
#define KOLM_M_BBWT_NIB 4
#define KOLM_M_BBWT_BR 5
#define KOLM_M_BBWT_GRAY 6
#define KOLM_M_LZ77 7
#define KOLM_M_LFSR 8
#define KOLM_M_REPAIR 9
#define KOLM_M_V2NEW 10
#define KOLM_NCAND 11          /* ids 0..10 are computed on the GPU */
#define KOLM_DEFAULT_MASK 0x3FFu  /* the reference's candidate set as shipped, ids 0..9 (v2_new raises in PY) */
#define KOLM_FULL_MASK 0x7FFu     /* + v2_new (id 10) with the automaton evaluated serially (opt-in) */
#define KOLM_HOTPATH_MASK 0x1FFu  /* BBWT / MTF+Rice / LZ77 path of the north star, ids 0..8 */
#define KOLM_REPAIR_MAX_BLOCK (1u << 22)  /* candidate 9 handles blocks up to 4 MiB */

typedef struct kolm_ctx kolm_ctx;

/* Kernel families timed with HIP events when timing is enabled (kolm_ctx_set_timing). */
#define KOLM_KT_CLASSIFY 0   /* k_classify */
#define KOLM_KT_KEYGEN 1     /* k_keypos, k_keygen_small, k_keygen_large */
#define KOLM_KT_MSD 2        /* k_msd_hist, k_msd_scan, k_msd_scatter, k_copy_back */
#define KOLM_KT_SMALLSORT 3  /* k_small_sort<1..11>, k_single, k_finalize_eq */
#define KOLM_KT_LSD 4        /* per-block LSD radix passes of the cyclic round 0: k_lsd_*, k_r0_* */
#define KOLM_KT_LZPARSE 5    /* k_lz_local (LDS 3-gram index + speculative parse), k_lz_stitch */
#define KOLM_KT_MTF 6        /* k_mtf_summary, k_mtf_compose, k_mtf_replay */
#define KOLM_KT_SIZES 7      /* k_sizes, k_mdl, k_offsets */
#define KOLM_KT_EMIT 8       /* emission kernels */
#define KOLM_KT_LYNDON 9     /* k_duval_*, Lyndon scans, k_prevc, k_bbwt_gather */
#define KOLM_KT_REPAIR 10    /* k_repair (one workgroup per block), k_rp_emit */
#define KOLM_KT_CDC 11       /* k_cdc_flags, k_cdc_spec, k_cdc_stitch, k_cdc_count/scan/emit */
#define KOLM_NKT 12

typedef struct kolm_ktime {
    double ms;          /* summed launch durations (HIP events on the library stream) */
    uint64_t launches;
    uint64_t bytes;     /* algorithmic HBM bytes of those launches */
} kolm_ktime;

/* Per-batch statistics reported by the encode entry points. */
typedef struct kolm_stats {
    uint32_t lin_rounds;      /* linear suffix-order rounds: 0 (Lyndon factors by Duval, LZ77 index in LDS) */
    uint32_t cyc_rounds;      /* prefix-doubling rounds, cyclic omega-order (max over blocks) */
    uint64_t lin_active;      /* 0 (kept for ABI stability) */
    uint64_t cyc_active;      /* same, cyclic */
    uint64_t lz_tokens;       /* LZ77 tokens over all blocks */
    uint64_t lz_long;         /* LZ77 parse positions that needed exact long-match resolution */
    double ms_total;          /* device time of the whole batch (HIP events) */
    double ms_sa;             /* of which: linear + cyclic suffix sorting */
    double ms_lz;             /* of which: LZ77 match + parse */
    double ms_entropy;        /* of which: BBWT gather + MTF + Rice sizes */
    double ms_emit;           /* of which: MDL + payload emission */
    kolm_ktime kt[KOLM_NKT];  /* per kernel family, filled when timing is enabled */
    double ms_repair;         /* Re-Pair (candidate 9) on its own stream, overlapping the rest */
    uint64_t rp_rules;        /* Re-Pair rules over all blocks */
    uint64_t rp_batches;      /* Re-Pair batches (sequential depth) summed over blocks */
    uint64_t rp_final;        /* Re-Pair final sequence symbols over all blocks */
    uint64_t lz_fix;          /* LZ77 tokens the stitch computed off the speculative paths */
    uint64_t cyc_rounds_sum;  /* sum over blocks of the rounds each block needed: round 0 through
                                 the last round that split one of its groups (>= 1; independent of
                                 how blocks are batched; SURVEY §8d's per-block R, used for the
                                 byte contract) */
} kolm_stats;

/* ---- library / default context ------------------------------------------------ */
int kolm_init(int device);
int kolm_shutdown(void);
const char* kolm_last_error(void);
int kolm_device_count(int* count);

/* ---- single-block kernels on the default context (host buffers) --------------- */
/* out: n bytes. */
int kolm_bbwt_forward(const uint8_t* in, size_t n, uint8_t* out);
/* out: n bytes (MTF indices 0..255). */
int kolm_mtf_encode(const uint8_t* in, size_t n, uint8_t* out);
/* Rice code of the byte sequence, parameter k in [0, 15]; worst case
 * n*(255/2^k + 1 + k)/8 + 1 bytes.  A code of 2^32 bits or more (possible from n = 2^24
 * at k = 0) is refused with KOLM_ERANGE, *out_len = 0 and nothing written to out; the same
 * holds for kolm_bbwt_mtf_rice with flags 0. */
int kolm_rice_encode(const uint8_t* in, size_t n, int k, uint8_t* out, size_t cap, size_t* out_len);
/* LZ77 stream (worst case 2n bytes). */
int kolm_lz77_encode(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len);
/* BBWT -> MTF -> bitwise map -> Rice k (flags: 0, 1 bit-plane, 4 nibble, 8 bitrev, 16 gray). */
int kolm_bbwt_mtf_rice(const uint8_t* in, size_t n, int flags, int k, uint8_t* out, size_t cap,
                       size_t* out_len);

/* ---- content-defined chunking (FastCDC) ------------------------------------------ */
/* Chunk boundaries of data[0, n) exactly as cdc_fast_boundaries_strict (PY:210-309,
 * replaces the loop at PY:247-298 + the orphan-tail merge PY:300-306): starts[0 ..
 * *nchunks] receives the chunk starts followed by n (chunk i = [starts[i], starts[i+1])).
 * cap = entries available in starts (n / min_size + 2 always suffices).  KOLM_EARG with
 * PY's messages for the parameters it rejects (0 < min <= avg <= max, avg >= 64). */
int kolm_cdc_boundaries(const uint8_t* data, uint64_t n, uint32_t min_size, uint32_t avg_size,
                        uint32_t max_size, int merge_orphan_tail, uint64_t* starts, uint64_t cap,
                        uint64_t* nchunks);

/* ---- decode side (host buffers, default context) -------------------------------- */
/* Decodes nblocks payloads of a container on the device (the decoder registry
 * _select_decoders, PY:2194-2207): block i = payloads[payload_off[i], payload_off[i+1]),
 * method id methods[i], original length orig_lens[i]; the blocks are written back to back
 * into out (sum of orig_lens bytes, out_cap available).  Method ids outside
 * KOLM_DECODE_MASK return KOLM_EARG; so do malformed payloads (message names the block).
 * v2_new (id 10, decode_new_pipeline PY:1578-1648): Rice parameters k = 0..15 are decoded,
 * every value an encoder writes (PY:1489 tries 0..15).  PY's decoder accepts any k byte; here
 * a block whose k list holds a byte above 15 is a malformed payload (decode it on the host).
 * id-10 blocks of 2^28 bytes or more return KOLM_EARG. */
#define KOLM_DECODE_MASK 0x7FFu  /* every candidate id 0..10 (raw, xor, bbwt family 2..6, lz77, lfsr_pred, repair, v2_new) */
int kolm_decode_blocks(const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* methods,
                       const uint32_t* orig_lens, uint32_t nblocks, uint8_t* out, uint64_t out_cap);

/* ---- container (host only: no device call, usable without a GPU) ---------------- */
/* Header + TOC of a KOLR container (PY:2213-2326 CDC, PY:2332-2445 fixed): mode 0 fixed /
 * 1 CDC, size_field = block size (fixed) or avg_size (CDC), nblocks entries of method id,
 * original length and payload length.  Writes every byte that precedes the payload area
 * (the payloads follow back to back) into out[0, cap); *out_len receives the count (out
 * may be NULL to query it).  KOLM_ERANGE when nblocks > 65535 or total_len >= 2^32. */
int kolm_toc_write(int mode, uint32_t size_field, uint64_t total_len, uint32_t nblocks,
                   const uint32_t* methods, const uint32_t* orig_lens, const uint64_t* payload_lens,
                   uint8_t* out, uint64_t cap, uint64_t* out_len);
/* Parses a whole container buf[0, n): fields[4] = {mode, size_field, total_len, nblocks},
 * *payload_start = offset of the payload area, methods / orig_lens (cap >= nblocks
 * entries) and payload_off (nblocks + 1 entries, relative to the payload area).  Checks
 * exactly what PY's decompress checks before decoding (magic, truncations, RLE size, EF
 * sum, trailing bytes): KOLM_EFORMAT with PY's message otherwise; KOLM_ECAP (fields and
 * *payload_start filled) when cap < nblocks. */
int kolm_toc_read(const uint8_t* buf, uint64_t n, uint32_t* fields, uint64_t* payload_start,
                  uint32_t* methods, uint32_t* orig_lens, uint64_t* payload_off, uint32_t cap);

/* ---- batched hot entry (host buffers, default context) ------------------------- */
/* Encodes nblocks blocks of `data` (block i = data[starts[i] .. starts[i]+lens[i]);
 * blocks contiguous and non-empty: fixed chunking when all lens are equal except a
 * shorter last one, otherwise content-defined chunks, e.g. kolm_cdc_boundaries' output
 * for compress_blocks_cdc, PY:2213-2326).
 * sizes[i*KOLM_NCAND + m] receives the payload size of candidate m (UINT32_MAX if the
 * candidate is disabled by cand_mask).  method[i] receives the MDL winner, or the
 * forced method when force_method != NULL and force_method[i] >= 0.  The winners'
 * payloads are written back to back into payload_arena in block order;
 * payload_off[i] / payload_off[i+1] delimit block i (nblocks+1 entries). */
int kolm_encode_blocks(const uint8_t* data, const uint64_t* starts, const uint32_t* lens,
                       uint32_t nblocks, uint32_t cand_mask, const int32_t* force_method,
                       uint32_t* sizes, uint32_t* method, uint8_t* payload_arena,
                       uint64_t arena_cap, uint64_t* payload_off, kolm_stats* stats);

/* compress_blocks_fixed (PY:2332-2445) in one call on the default context: the host
 * buffer data[0, n) goes up through a ring of pinned staging chunks (parallel host copies
 * beside the DMA), every block of block_size bytes is encoded (candidates cand_mask, MDL),
 * and the KOLR container (header + TOC by kolm_toc_write, then the winners' payloads copied
 * straight from device memory) is assembled in a pinned host buffer owned by the context:
 * *out / *out_len describe it until the next call on the default context: callers on
 * several threads must serialise the call AND their read of *out (the Python binding holds
 * one lock across both), since the next call reuses the buffer.  Inputs above
 * 2^31 bytes run as several device batches.  KOLM_ERANGE when the block count exceeds
 * 65535 or n >= 2^32 (PY's struct.error). */
int kolm_compress_fixed(const uint8_t* data, uint64_t n, uint32_t block_size, uint32_t cand_mask,
                        const uint8_t** out, uint64_t* out_len, kolm_stats* stats);

/* Second phase of kolm_compress_fixed: copy the container it described (*out, *out_len)
 * into the caller's buffer dst[0, n) (n <= *out_len) with the context's host copy
 * threads (page faults of a fresh destination and the memcpy itself spread over them).
 * Same serialisation rule as kolm_compress_fixed's *out.  KOLM_ECAP when n exceeds the
 * container. */
int kolm_result_copy(uint8_t* dst, uint64_t n);

/* kolm_encode_blocks over ngpu devices (0..ngpu-1, clamped to the device count and the
 * block count) of this process: fixed blocks of block_size over data[0, total), block i
 * of shard r lives on device r, shards are contiguous block ranges, one host thread and
 * context per device.  The shards' payloads are reassembled with RCCL: one
 * ncclCommInitAll communicator over the devices (created on first use, kept until
 * kolm_shutdown), every device's payload arena received into device 0 in one group over
 * xGMI, then one copy into payload_arena (KOLM_MULTI_GATHER=host: each device copies its
 * own payloads to the host instead).  Outputs exactly as kolm_encode_blocks (block order;
 * sizes [nblocks*KOLM_NCAND], method [nblocks], payload_off [nblocks+1]).  stats
 * (optional) sums counts and takes the max of times over devices.  KOLM_ERCCL on a
 * collective error. */
int kolm_encode_blocks_multi(int ngpu, const uint8_t* data, uint64_t total, uint32_t block_size,
                             uint32_t cand_mask, const int32_t* force_method, uint32_t* sizes,
                             uint32_t* method, uint8_t* payload_arena, uint64_t arena_cap,
                             uint64_t* payload_off, kolm_stats* stats);

/* ---- explicit contexts and device-resident batches ------------------------------ */
int kolm_ctx_create(int device, kolm_ctx** out);
int kolm_ctx_destroy(kolm_ctx* ctx);
/* Pre-allocates device scratch for batches of up to total_bytes with blocks of up to
 * max_block bytes (optional: buffers grow on demand otherwise). */
int kolm_ctx_reserve(kolm_ctx* ctx, uint64_t total_bytes, uint32_t max_block);
/* Allocate / free / copy device memory through the context's HIP runtime. */
int kolm_dev_alloc(kolm_ctx* ctx, uint64_t bytes, void** dptr);
int kolm_dev_free(kolm_ctx* ctx, void* dptr);
int kolm_memcpy_h2d(kolm_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int kolm_memcpy_d2h(kolm_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int kolm_ctx_sync(kolm_ctx* ctx);
/* Enable (1) / disable (0) per-launch HIP-event timing of the kernel families. */
int kolm_ctx_set_timing(kolm_ctx* ctx, int enable);
/* 1: run every launch of the next batches on one stream (kernels serialised: each kernel's
 * solo duration, for profiling); 0 (default, or KOLM_SERIAL=1 at context creation): the
 * sort chain, the LZ77 parse and Re-Pair overlap on their own streams. */
int kolm_ctx_set_serial(kolm_ctx* ctx, int serial);
/* Per-kernel timing accumulated since timing was enabled, as JSON text
 * {"k_name": {"ms": .., "launches": .., "bytes": .., "family": KOLM_KT_*, "stream":
 * "sort"|"index"|"repair"}, ...} (bytes = algorithmic HBM bytes; stream = the
 * HIP stream the kernel ran on).  *len receives the length; buf may be NULL to query it. */
int kolm_ctx_kernel_times(kolm_ctx* ctx, char* buf, size_t cap, size_t* len);
/* Fixed-size blocks of d_data (device pointer, total bytes, block_size).  Payloads go
 * to the device arena d_arena (cap bytes); h_sizes / h_method / h_off are host arrays
 * as in kolm_encode_blocks.  Blocks until the batch is complete. */
int kolm_encode_blocks_device(kolm_ctx* ctx, const uint8_t* d_data, uint64_t total,
                              uint32_t block_size, uint32_t cand_mask,
                              const int32_t* force_method, uint8_t* d_arena, uint64_t arena_cap,
                              uint32_t* h_sizes, uint32_t* h_method, uint64_t* h_off,
                              kolm_stats* stats);
/* Content-defined blocks of d_data: block i = [h_bounds[i], h_bounds[i+1]), h_bounds[0] = 0,
 * strictly increasing, nblocks + 1 entries (PY:2213-2326).  Outputs as
 * kolm_encode_blocks_device. */
int kolm_encode_blocks_device_var(kolm_ctx* ctx, const uint8_t* d_data, const uint32_t* h_bounds,
                                  uint32_t nblocks, uint32_t cand_mask, const int32_t* force_method,
                                  uint8_t* d_arena, uint64_t arena_cap, uint32_t* h_sizes,
                                  uint32_t* h_method, uint64_t* h_off, kolm_stats* stats);
/* kolm_cdc_boundaries over a device-resident buffer; h_starts are host u32 entries. */
int kolm_cdc_boundaries_device(kolm_ctx* ctx, const uint8_t* d_data, uint64_t n, uint32_t min_size,
                               uint32_t avg_size, uint32_t max_size, int merge_orphan_tail,
                               uint32_t* h_starts, uint64_t cap, uint64_t* nchunks);
/* kolm_decode_blocks over device-resident payloads (e.g. an encode arena): block i =
 * d_payloads[payload_off[i], payload_off[i+1]) with payload_off / methods / orig_lens on
 * the host; the blocks are written back to back into d_out (device, out_cap bytes).
 * ms (optional) receives the device time of the decode kernels (HIP events). */
int kolm_decode_blocks_device(kolm_ctx* ctx, const void* d_payloads, const uint64_t* payload_off,
                              const uint32_t* methods, const uint32_t* orig_lens, uint32_t nblocks,
                              void* d_out, uint64_t out_cap, double* ms);

/* ---- verify: decode the payloads where they lie and compare with the input --------- */
/* The KOLR container carries no checksum; this is the check that payloads decode back to
 * their input, made on the device: the payloads are decoded (the decoders of
 * kolm_decode_blocks) into scratch, k_verify_cmp compares the scratch with the original
 * (both resident), and one word per block comes back. */
#define KOLM_VERIFY_EQUAL 0xFFFFFFFFu     /* per-block word: the block decodes to its input */
#define KOLM_VERIFY_REJECTED 0xFFFFFFFEu  /* per-block word: the decoder rejected the payload */
#define KOLM_VR_NONE 0      /* kolm_verify_report.first_bad_reason */
#define KOLM_VR_DIFFER 1    /* bytes differ: first_bad_offset = first differing byte of the block */
#define KOLM_VR_REJECTED 2  /* the decoder rejected the payload */
#define KOLM_VR_LENGTH 3    /* kolm_verify_container only: total_len differs from the data's length */
typedef struct kolm_verify_report {
    uint32_t blocks;            /* blocks checked */
    uint32_t bad_blocks;        /* of which: differing or rejected */
    uint32_t first_bad_block;   /* the lowest-numbered bad block, its method id, the offset of */
    uint32_t first_bad_method;  /* its first differing byte (0 when rejected) and the reason */
    uint32_t first_bad_offset;
    uint32_t first_bad_reason;  /* KOLM_VR_* */
    uint64_t bytes;             /* decoded bytes compared */
    double ms_decode;           /* device time of the decode kernels (HIP events) */
    double ms_compare;          /* device time of k_verify_cmp */
} kolm_verify_report;
/* Original d_data (block i = [h_bounds[i], h_bounds[i+1]), h_bounds[0] = 0, nblocks + 1 host
 * entries; any alignment) and payloads d_payloads (block i = [payload_off[i],
 * payload_off[i+1]), method methods[i]; host arrays) are both device-resident.  h_first_bad
 * (optional, nblocks host words) receives per block the offset of its first differing byte,
 * KOLM_VERIFY_EQUAL or KOLM_VERIFY_REJECTED; *rep (optional) the summary.  KOLM_OK whenever
 * the check ran, whether or not blocks differ; argument errors as kolm_decode_blocks_device
 * (method ids outside KOLM_DECODE_MASK: KOLM_EARG, the block named).  The blocks are checked
 * in groups whose decoded bytes stay under min(2^31 - 1, $KOLM_VERIFY_BYTES (default 1 GiB,
 * read per call)); a single block always forms a group: the decode scratch is bounded and
 * inputs of 2 GiB and more can be checked. */
int kolm_verify_blocks_device(kolm_ctx* ctx, const void* d_data, const uint64_t* h_bounds, uint32_t nblocks,
                              const void* d_payloads, const uint64_t* payload_off, const uint32_t* methods,
                              uint32_t* h_first_bad, kolm_verify_report* rep);
/* A whole container against the data it should hold (host buffers, default context): the
 * TOC by kolm_toc_read (KOLM_EFORMAT as there); total_len != n is reported as KOLM_VR_LENGTH
 * without decoding (first_bad untouched); otherwise payloads and data go up, the grouped check
 * runs and only the per-block words come down: first_bad[0, cap) (optional; KOLM_ECAP when
 * cap < the block count), *rep the summary. */
int kolm_verify_container(const uint8_t* container, uint64_t cn, const uint8_t* data, uint64_t n,
                          uint32_t* first_bad, uint32_t cap, kolm_verify_report* rep);
/* Verify-after-encode (default off, or KOLM_VERIFY=1 at context creation): when enabled,
 * kolm_encode_blocks, kolm_encode_blocks_device, kolm_encode_blocks_device_var,
 * kolm_compress_fixed (every device batch) and kolm_encode_blocks_multi (its per-device
 * contexts take the default context's setting) check every batch on the resident text and
 * arena before they return, after the emission kernels and under the context lock the call
 * holds.  A bad block makes the call return KOLM_EVERIFY (kolm_last_error names the block, the
 * method and the offset or "decoder rejected the payload"); kolm_compress_fixed then hands
 * out no container (*out_len = 0), the other entry points still fill their outputs.
 * Disabled: no extra launch, allocation or synchronisation.  $KOLM_VERIFY_INJECT=<block>
 * (test switch, read per call, verify on only) xors 0x80 into the first payload byte of that
 * block in the device arena before the check. */
int kolm_ctx_set_verify(kolm_ctx* ctx, int enable);
int kolm_set_verify(int enable);  /* default context */
/* The report accumulated over the batches of the last encode call of ctx (NULL: the default
 * context) that ran with verify enabled. */
int kolm_ctx_verify_report(kolm_ctx* ctx, kolm_verify_report* rep);

/* ---- random-access reads: decode only the blocks a byte range touches --------------- */
/* A KOLR container's blocks are coded independently and its TOC gives every block's geometry,
 * method and payload offset, so a byte range of the decoded stream needs only the blocks it
 * touches: they are decoded into scratch on the device (the decoders of kolm_decode_blocks) and
 * k_range_gather packs the requested bytes, back to back in request order, into the output. */
typedef struct kolm_range_seg {
    uint64_t src;  /* offset in the group's decoded scratch (its selected blocks back to back) */
    uint64_t dst;  /* offset in the packed output */
    uint64_t len;
} kolm_range_seg;
/* The plan of a read (host only: no device call, usable without a GPU): blocks of orig_lens[i]
 * decoded bytes each, nranges ranges [offs[r], offs[r] + lens[r]) of the decoded stream.
 *   sel          the blocks that hold a byte of a range, ascending, each once
 *   group_first  [ngroups + 1]: group g = sel[group_first[g], group_first[g + 1]).  Consecutive
 *                selected blocks share a group while their decoded bytes stay at or under
 *                min(2^31 - 1, group_limit); group_limit 0 = $KOLM_READ_BYTES (read per call), else
 *                1 GiB.  A single block always forms a group.
 *   run_first    [nruns + 1]: run r = sel[run_first[r], run_first[r + 1]), blocks consecutive in
 *                the container (contiguous payloads); a run lies inside one group
 *   group_seg    [ngroups + 1]: group g's copy segments = segs[group_seg[g], group_seg[g + 1]),
 *                in request order; a range that has bytes in several groups has one segment in
 *                each, an empty range none.  The output is the ranges back to back.
 * caps[4] = entries available: sel, groups (group_first and group_seg hold one more), runs
 * (run_first holds one more), segs; counts[4] receives what the plan needs, in that order.
 * KOLM_EARG (message names the range) when a range does not lie inside [0, total_len], before
 * anything else; KOLM_ECAP (counts filled) when an array is too small or caps is NULL. */
int kolm_range_plan(const uint32_t* orig_lens, uint32_t nblocks, const uint64_t* offs, const uint64_t* lens,
                    uint32_t nranges, uint64_t group_limit, uint32_t* sel, uint32_t* group_first,
                    uint32_t* run_first, uint32_t* group_seg, kolm_range_seg* segs, const uint64_t* caps,
                    uint64_t* counts);

typedef struct kolm_reader kolm_reader;
typedef struct kolm_read_stats {
    uint32_t ranges;          /* ranges of the call */
    uint32_t blocks_decoded;  /* selected blocks */
    uint32_t groups;          /* decode batches */
    uint32_t compactions;     /* groups whose payload runs were gathered into a staging buffer first */
    uint64_t bytes_returned;  /* the packed output */
    uint64_t bytes_decoded;   /* decoded bytes of the selected blocks */
    double ms_decode;         /* device time of the decode kernels (HIP events) */
    double ms_gather;         /* device time of k_range_gather, both uses */
} kolm_read_stats;
/* Opens container[0, cn) for reading on ctx (NULL: the default context): kolm_toc_read first
 * (KOLM_EFORMAT / KOLM_ERANGE with PY's message, as there), then the payload area goes up once
 * and stays resident until kolm_reader_close; the container's bytes are not needed afterwards.
 * Blocks the device does not decode (method ids outside KOLM_DECODE_MASK, id-10 blocks of 2^28
 * bytes or more) do not fail the open: they matter when a read selects them.  Close every
 * reader before its context is destroyed.  Several readers may share a context; every call
 * holds the context's lock. */
int kolm_reader_open(kolm_ctx* ctx, const uint8_t* container, uint64_t cn, kolm_reader** out);
int kolm_reader_close(kolm_reader* r);
/* info[5] = {mode, size_field, total_len, nblocks, payload bytes}; methods / orig_lens (optional,
 * cap entries each; KOLM_ECAP when cap < nblocks and either is given). */
int kolm_reader_info(kolm_reader* r, uint64_t* info, uint32_t* methods, uint32_t* orig_lens, uint32_t cap);
/* Reads nranges byte ranges of the decoded stream into out[0, out_cap) (host), back to back in
 * request order (range r at the sum of lens[0, r)): plan (kolm_range_plan), then per group the
 * payload runs are compacted into a staging buffer when there are several (one run is decoded
 * where it lies), the group's blocks are decoded into scratch and k_range_gather packs the
 * group's segments into a device buffer; one copy brings the packed bytes to the host.  The
 * decoded scratch never leaves the device.  Every argument is checked before the first launch:
 * KOLM_EARG for a range outside [0, total_len] (message names the range) and for a selected
 * block the device does not decode (message names the container's block number and method);
 * KOLM_ECAP when the ranges' bytes exceed out_cap.  A selected block whose decoder rejects its
 * payload: KOLM_EARG, the block and method named.  Blocks no range touches do not matter.
 * stats optional. */
int kolm_reader_read(kolm_reader* r, const uint64_t* offs, const uint64_t* lens, uint32_t nranges, uint8_t* out,
                     uint64_t out_cap, kolm_read_stats* stats);
/* The same with the packed output left in device memory d_out[0, out_cap) (any alignment; only
 * the ranges' bytes are written). */
int kolm_reader_read_device(kolm_reader* r, const uint64_t* offs, const uint64_t* lens, uint32_t nranges,
                            void* d_out, uint64_t out_cap, kolm_read_stats* stats);

/* ---- search: where do byte strings occur in decoded data? ---------------------------------- */
/* A call takes np patterns (1..KOLM_FIND_MAX_PATTERNS), pattern i = pats[pat_off[i], pat_off[i + 1])
 * of 1..KOLM_FIND_MAX_LEN bytes, and a window [lo, hi) of the data.  (o, i) is a match iff
 * lo <= o, o + len_i <= hi and data[o, o + len_i) == pattern i: every match counts, overlapping
 * ones and those of identical patterns included.  The matches are listed in (offset, pattern
 * index) order; with max_results the first max_results of that order.  counts [np] are the exact
 * totals per pattern whatever max_results is.  Results are the same from run to run and do not
 * depend on KOLM_READ_BYTES or KOLM_FIND_STAGE.
 * On the device (csrc/find_core.h, k_find.hip): k_find_count (a workgroup per 4 KiB tile; a masked
 * 64-bit compare of every position with every pattern's first 8 bytes, the rest only for
 * candidates), a scan of the tile totals, one round trip for the totals, and k_find_emit writing
 * (position, pattern) records at the scanned slots of a staging buffer of at most
 * $KOLM_FIND_STAGE bytes (default 64 MiB, read per call, never less than one tile's records);
 * a buffer with more matches is emitted in several launches over consecutive tile ranges.  No
 * emit launch when nothing is to be returned (max_results = 0, or no match).
 * KOLM_EARG before any launch, the message naming the pattern: np = 0 or np > 16, an empty pattern,
 * a pattern of more than 256 bytes. */
#define KOLM_FIND_MAX_PATTERNS 16
#define KOLM_FIND_MAX_LEN 256
/* The search of a resident buffer d_data[0, n) (device memory of any alignment, n < 2^31; the
 * aligned 16-byte words that hold its first and last byte are read whole).  offs / which [cap]
 * receive the first min(total, max_results) matches, nfound their number; which may be NULL when
 * np == 1.  KOLM_ECAP when cap < min(total, max_results): counts are filled, nfound = the
 * capacity needed, nothing is emitted.  ms (optional): device time of the kernels. */
int kolm_find_device(kolm_ctx* ctx, const void* d_data, uint64_t n, const uint8_t* pats, const uint32_t* pat_off,
                     uint32_t np, uint64_t max_results, uint64_t* counts, uint64_t* offs, uint8_t* which, uint64_t cap,
                     uint64_t* nfound, double* ms);
typedef struct kolm_find_stats {
    uint32_t patterns;
    uint32_t blocks_decoded;  /* blocks that hold a byte of the window */
    uint32_t groups;          /* decode batches */
    uint32_t emit_launches;   /* k_find_emit launches (0: a count-only call, or no match) */
    uint64_t matches;         /* total over the patterns, whatever max_results is */
    uint64_t returned;        /* min(matches, max_results) */
    uint64_t bytes_decoded;
    uint64_t bytes_scanned;   /* the groups' scan buffers: the window's bytes plus the carries */
    double ms_decode;         /* device time of the decode kernels */
    double ms_find;           /* device time of the search kernels */
} kolm_find_stats;
/* The search of the window [lo, hi) of a reader's decoded stream.  The blocks that hold a byte of
 * the window are decoded group by group as kolm_reader_read decodes them (KOLM_READ_BYTES; payload
 * runs compacted; a rejected payload: KOLM_EARG, block and method named; with
 * kolm_reader_set_checksums in force every decoded block's CRC-32 is checked before any result
 * leaves: KOLM_ECHECKSUM and no results).  Group g reports the matches that start in
 * [S_g, S_g+1): S_0 = lo, S_g+1 = max(S_g, the group's end - (L - 1)) with L the longest pattern,
 * hi after the last group; the bytes [S_g+1, group end), fewer than L, are copied in front of the
 * next group's decoded bytes, so every start is examined once, in ascending order, and a match may
 * span any number of blocks and groups.  The decoded bytes never leave the device; per group the
 * totals make one round trip, and each emit launch one copy of its records.
 * The result (absolute offsets, pattern indices) stays in the reader until its next find or its
 * close: nfound entries, copied out by kolm_reader_find_copy (the two-call pattern of
 * kolm_compress_fixed / kolm_result_copy).  KOLM_EARG before any launch also for lo > hi or
 * hi > total_len and for a selected block the device does not decode (block and method named).
 * stats optional. */
int kolm_reader_find(kolm_reader* r, const uint8_t* pats, const uint32_t* pat_off, uint32_t np, uint64_t lo, uint64_t hi,
                     uint64_t max_results, uint64_t* counts, uint64_t* nfound, kolm_find_stats* stats);
/* Results [first, first + n) of the reader's last find to offs / which (which optional). */
int kolm_reader_find_copy(kolm_reader* r, uint64_t first, uint64_t n, uint64_t* offs, uint8_t* which);

/* ---- class patterns: ignore case, wildcards and byte sets ------------------------------------- */
/* A class pattern is a sequence of 1..KOLM_FIND_MAX_LEN byte classes, each a subset of 0..255
 * passed as a 32-byte bitmap (bit b & 7 of byte b >> 3 is byte value b); pattern i takes the
 * bitmaps [pat_off[i], pat_off[i + 1]) of `bitmaps`.  (o, i) is a match iff lo <= o,
 * o + len_i <= hi and data[o + j] is in class j of pattern i for every j; a pattern that holds an
 * empty class has no match.  Counting, order, max_results, the exact totals and the independence
 * of KOLM_READ_BYTES / KOLM_FIND_STAGE are those of the search above, as are the tile geometry, the
 * scan, the staged emit, the hold-back between groups and the checksum rule.
 * The library classifies and deduplicates the classes (csrc/findcls_core.h): a class equal to
 * {b : (b & mask) == value} (a single byte, every byte, an ASCII case pair, [0-7] ...) counts against
 * no limit; of all others, the table classes, a call holds at most KOLM_FIND_MAX_TABLE_CLASSES
 * distinct ones.  k_findcls_count / k_findcls_emit (k_findcls.hip) filter every position with one
 * masked 64-bit compare on the first 8 classes and look at the table and the later positions
 * only for candidates.
 * KOLM_EARG before any launch, the message naming the pattern: np = 0 or np > 16, a pattern of 0
 * or more than 256 positions, and the position at which a 65th distinct table class appears. */
#define KOLM_FIND_MAX_TABLE_CLASSES 64
/* kolm_find_device for class patterns (KOLM_ECAP included). */
int kolm_find_classes_device(kolm_ctx* ctx, const void* d_data, uint64_t n, const uint8_t* bitmaps,
                             const uint32_t* pat_off, uint32_t np, uint64_t max_results, uint64_t* counts, uint64_t* offs,
                             uint8_t* which, uint64_t cap, uint64_t* nfound, double* ms);
/* kolm_reader_find for class patterns: the result stays in the reader until its next find of any
 * kind and is copied out by kolm_reader_find_copy. */
int kolm_reader_find_classes(kolm_reader* r, const uint8_t* bitmaps, const uint32_t* pat_off, uint32_t np, uint64_t lo,
                             uint64_t hi, uint64_t max_results, uint64_t* counts, uint64_t* nfound, kolm_find_stats* stats);

/* ---- regular expressions: one automaton for up to 16 expressions ------------------------------- */
/* The np expressions (1..KOLM_FIND_MAX_PATTERNS) of a call are passed compiled, as one deterministic
 * automaton (kolm/regex.py builds it; csrc/findrx_core.h walks it):
 *   cls_map  256 bytes: the class of every byte value, each < ncls (1..256)
 *   table    nstates x ncls transitions, row-major: table[s * ncls + c] is the state after state s
 *            reads a byte of class c.  State 0 is dead and state 1 accepts; both are absorbing and
 *            their rows are all zero.  nstates * ncls <= KOLM_RX_MAX_ENTRIES (32 KiB of LDS).
 *   starts   the start state of every expression, each in [2, nstates): no expression matches the
 *            empty string
 * (o, i) is a match iff lo <= o and there is a k in 1..KOLM_FIND_MAX_LEN with o + k <= hi such that
 * the walk from starts[i] over data[o .. o + k) ends in state 1: expression i matches data[o:o + k]
 * exactly.  For the syntax of kolm.regex.compile that is
 *   re.compile(b"(?:" + expr + b")", re.DOTALL [| re.IGNORECASE]).match(data, o, min(hi, o + 256)) is not None.
 * Every such start is reported, overlapping ones and those of identical expressions included, sorted
 * by (offset, expression).  Only starts are reported: a match has no length here (greedy, lazy
 * and leftmost-longest differ, and none of them is decided per start).  The witness cap of
 * KOLM_FIND_MAX_LEN = 256 bytes is the hold-back the group loop supports: a start whose shortest
 * match is longer is not a match.  The walk takes at most 256 steps whatever the table holds.
 * Counting, max_results, the exact totals under a limit and the independence of KOLM_READ_BYTES /
 * KOLM_FIND_STAGE are those of the search above, as are the tile geometry, the scan, the staged
 * emit, the hold-back between groups (its length derived from the table by the library) and the
 * checksum rule.
 * KOLM_EARG before any launch, the message naming what is wrong: np = 0 or np > 16, ncls = 0 or
 * > 256, fewer than 3 states, more than KOLM_RX_MAX_ENTRIES entries, a class id >= ncls, an entry
 * >= nstates, a non-zero entry in row 0 or 1, a start outside [2, nstates). */
#define KOLM_RX_MAX_ENTRIES 16384
/* kolm_find_device for an automaton (KOLM_ECAP included). */
int kolm_find_dfa_device(kolm_ctx* ctx, const void* d_data, uint64_t n, const uint8_t* cls_map, const uint16_t* table,
                         uint32_t nstates, uint32_t ncls, const uint16_t* starts, uint32_t np, uint64_t max_results,
                         uint64_t* counts, uint64_t* offs, uint8_t* which, uint64_t cap, uint64_t* nfound, double* ms);
/* kolm_reader_find for an automaton: the result stays in the reader until its next find of any
 * kind and is copied out by kolm_reader_find_copy. */
int kolm_reader_find_dfa(kolm_reader* r, const uint8_t* cls_map, const uint16_t* table, uint32_t nstates, uint32_t ncls,
                         const uint16_t* starts, uint32_t np, uint64_t lo, uint64_t hi, uint64_t max_results,
                         uint64_t* counts, uint64_t* nfound, kolm_find_stats* stats);

/* ---- pattern sets: up to 65 536 patterns in one pass ----------------------------------------- */
/* A set holds np patterns (1..KOLM_FIND_SET_MAX_PATTERNS) of 1..KOLM_FIND_MAX_LEN bytes each,
 * pairwise distinct: two equal patterns are refused with KOLM_EARG, the message naming both
 * indices.  The match rule, the order of the results, the exact per-pattern totals and the
 * independence of KOLM_READ_BYTES / KOLM_FIND_STAGE are those of the search above; distinctness
 * bounds the matches of one position (prefixes of one another: at most min(np, 256)).
 * On the device (csrc/findset_core.h, k_findset.hip): the key of a pattern is its first
 * K = min(8, shortest pattern) bytes; the patterns of one key form a bucket (ascending index) behind
 * an open-addressing table of the keys and a bitmap filter of 1..32 KiB that the kernels keep in
 * LDS.  k_findset_count tests each position's key against the filter, probes the table on a hit and
 * verifies the bucket's patterns in full; the cost of a position does not grow with the set while
 * few positions pass the filter.  Scan, round trip, staging (8-byte records) and emit launches as
 * above.  A set owns its device tables and is bound to the context it was made in (NULL: the
 * default context); it is used with readers and buffers of that context and must be freed before
 * that context is destroyed.  The per-pattern counters of a call live in the set: calls that use
 * one set are serialised by its context's lock, and a set is shared between threads only that way. */
#define KOLM_FIND_SET_MAX_PATTERNS 65536
typedef struct kolm_patset kolm_patset;
typedef struct kolm_patset_info_t {
    uint32_t np;              /* patterns */
    uint32_t key_bytes;       /* K */
    uint32_t keys;            /* distinct keys = buckets */
    uint32_t slots;           /* of the key table: a power of two >= 2 * keys */
    uint32_t filter_bits;     /* a power of two >= 16 * keys within [2^13, 2^18] */
    uint32_t longest;         /* L, the longest pattern: the hold-back between decode groups */
    uint32_t longest_bucket;  /* patterns that share one key, at most (they are verified one by one) */
} kolm_patset_info_t;
int kolm_patset_create(kolm_ctx* ctx, const uint8_t* pats, const uint32_t* pat_off, uint32_t np, kolm_patset** out);
void kolm_patset_free(kolm_patset* ps);
int kolm_patset_info(const kolm_patset* ps, kolm_patset_info_t* out);
/* kolm_find_device for a set: counts [np] may be NULL; which holds 32-bit pattern indices.
 * KOLM_ECAP as there (counts filled, nfound = the capacity needed, nothing emitted). */
int kolm_find_set_device(kolm_ctx* ctx, const void* d_data, uint64_t n, const kolm_patset* ps, uint64_t max_results,
                         uint64_t* counts, uint64_t* offs, uint32_t* which, uint64_t cap, uint64_t* nfound, double* ms);
/* kolm_reader_find for a set: one decode of the window's blocks serves the whole set (the hold-back
 * uses the set's longest pattern).  counts [np] may be NULL.  The per-pattern counters are zeroed
 * once per call and read back once at its end; per group only the grand total makes the round
 * trip.  KOLM_EARG before any launch also for a set of another context than the reader's.  The
 * result stays in the reader until its next find / find_set or its close and is copied out by
 * kolm_reader_find_copy32; stats->patterns = np. */
int kolm_reader_find_set(kolm_reader* r, const kolm_patset* ps, uint64_t lo, uint64_t hi, uint64_t max_results,
                         uint64_t* counts, uint64_t* nfound, kolm_find_stats* stats);
/* Results [first, first + n) of the reader's last find_set to offs / which (which optional). */
int kolm_reader_find_copy32(kolm_reader* r, uint64_t first, uint64_t n, uint64_t* offs, uint32_t* which);

/* ---- dedup: encode repeated blocks once ---------------------------------------------- */
/* A block's payload depends on its bytes, the candidate mask and its forced method and on
 * nothing else (PY:2350-2369 loops over the blocks independently), so a batch can encode each
 * distinct block once and copy that payload to every repeat: the outputs are byte for byte those
 * of a call without dedup (the KOLR format cannot reference an earlier block: the saving is time,
 * not bytes).  Default off, or KOLM_DEDUP=1 at context creation.  When enabled, every device
 * batch of kolm_encode_blocks, kolm_encode_blocks_device, kolm_encode_blocks_device_var,
 * kolm_compress_fixed (each piece on its own) and kolm_encode_blocks_multi (each shard on its
 * own; the per-device contexts take the default context's setting) first fingerprints its blocks
 * on the device (k_block_fp: one streaming read, 16 bytes per block come back), groups them on
 * the host by (length, forced method, fingerprint), compares every group member with the group's
 * lowest-numbered block byte for byte (k_dedup_cmp) and, when that confirms duplicates, packs the
 * distinct blocks into a scratch text, encodes those into a scratch arena and copies every
 * block's payload from its representative's into the caller's arena (k_range_gather).  Blocks
 * with different forced methods are never duplicates of each other.  kolm_stats of such a call
 * describes the work that ran: the distinct blocks.  Verify, when also on, checks the expanded
 * arena against the original text: block numbers are container numbers.  Without a confirmed
 * duplicate the original buffer is encoded exactly as with dedup off.  Disabled: no extra
 * launch, allocation or synchronisation.
 * With dedup on, up to 15 bytes on either side of d_data[0, total) may be read (and dropped) by
 * the packing copy: they lie inside the aligned 16-byte word of a valid byte, hence inside any
 * allocation that holds the data.  The fingerprint and compare kernels read [0, total) only.
 * $KOLM_DEDUP_BITS=<0..128> (test switch, read per call, dedup on only) keeps that many low bits
 * of the fingerprint for the grouping, so that the collision path runs. */
typedef struct kolm_dedup_report {
    uint32_t blocks;           /* blocks of the call's batches */
    uint32_t blocks_encoded;   /* of which: distinct, encoded */
    uint32_t candidate_pairs;  /* (block, representative) pairs compared byte for byte */
    uint32_t collisions;       /* of which: different bytes under one fingerprint */
    uint64_t bytes;            /* bytes of the batches */
    uint64_t bytes_encoded;    /* bytes of the distinct blocks */
    double ms_hash;            /* device time of k_block_fp (HIP events) */
    double ms_compare;         /* of k_dedup_cmp */
    double ms_compact;         /* of the gather that packs the distinct blocks */
    double ms_expand;          /* of the gather that spreads the payloads */
} kolm_dedup_report;
int kolm_ctx_set_dedup(kolm_ctx* ctx, int enable);
int kolm_set_dedup(int enable);  /* default context */
/* The report accumulated over the batches of the last encode call of ctx (NULL: the default
 * context); all zero when that call ran with dedup off. */
int kolm_ctx_dedup_report(kolm_ctx* ctx, kolm_dedup_report* rep);
/* Lyndon factorisation routes of the last batch ctx (NULL: the default context) factorised: the
 * blocks whose factor starts came from the prefix-minimum candidates (accepted) and the blocks
 * left to the parallel Duval kernels (fallback: periodic data that exceeds the candidate or
 * common-prefix budget, or every block with $KOLM_LYN_FAST=0).  Both routes give the same factors.
 * $KOLM_LYN_FAST=<0|1> (default 1), $KOLM_LYN_CAND_MAX=<1..1024> and $KOLM_LYN_LCP_MAX=<0..65536>
 * (test switches that move the budgets) are read per call.  Waits for the batch. */
int kolm_ctx_lyndon_report(kolm_ctx* ctx, uint32_t* accepted, uint32_t* fallback);
/* The fingerprints of the blocks of d_data (device; block i = [h_bounds[i], h_bounds[i+1]),
 * h_bounds[0] = 0, non-empty blocks, nblocks + 1 host entries, total < 2^31; any alignment):
 * h_fp[2 i], h_fp[2 i + 1] = block i's 128 bits.  A function of the block's bytes alone; it may
 * change between versions of the library and must not be persisted. */
int kolm_block_fingerprints_device(kolm_ctx* ctx, const void* d_data, const uint64_t* h_bounds, uint32_t nblocks,
                                   uint64_t* h_fp);
/* The confirmed duplicate map of the same blocks without encoding anything: h_rep[i] = i for a
 * distinct block, else the lowest-numbered block with the same bytes that the plan paired it with
 * (kolm_dedup_plan); *rep (optional) the counts and times. */
int kolm_find_duplicates_device(kolm_ctx* ctx, const void* d_data, const uint64_t* h_bounds, uint32_t nblocks,
                                uint32_t* h_rep, kolm_dedup_report* rep);
/* The host plan (no device call, usable without a GPU).  lens / fps (2 words per block) /
 * force_method (optional; entries < 0 = not forced) describe nblocks blocks; fp_bits (0..128) =
 * low fingerprint bits that count.
 * Phase A: blocks are grouped by (length, forced id or -1, fingerprint); a group's representative
 * is its lowest-numbered block; every other member gives a pair (member, representative):
 * pairs[2 p], pairs[2 p + 1], ascending by member; counts[0] = the pairs.  With differ == NULL
 * and at least one pair the call ends here (counts[1] = counts[2] = 0).
 * Phase B (differ[p] != 0: pair p's blocks differ): rep[i] = i for distinct blocks and the
 * representative for confirmed duplicates; a member that differs from its representative is
 * encoded itself and is nobody's representative.  distinct = the blocks with rep[i] = i,
 * ascending (counts[1] of them; counts[2] = the collisions); compact[q] = the copy of distinct
 * block q from the batch (src) into the dense text (dst).  Given distinct_off (counts[1] + 1
 * payload offsets of the distinct blocks): payload_off (nblocks + 1, a prefix sum in block order)
 * and expand[i] = the copy of block i's payload from its representative's (src relative to
 * distinct_off[0]) to payload_off[i].
 * Every output array holds nblocks entries (pairs 2 * nblocks, payload_off nblocks + 1); each
 * may be NULL (payload_off not when distinct_off is given). */
int kolm_dedup_plan(const uint32_t* lens, const uint64_t* fps, const int32_t* force_method, uint32_t nblocks,
                    uint32_t fp_bits, const uint32_t* differ, uint32_t* pairs, uint32_t* rep, uint32_t* distinct,
                    kolm_range_seg* compact, const uint64_t* distinct_off, uint64_t* payload_off,
                    kolm_range_seg* expand, uint32_t* counts);

/* ---- checksums: block and stream CRC-32 of resident bytes (crc_core.h, k_crc.hip) --- */
/* The container carries no checksum and does not grow one.  These calls compute the standard
 * CRC-32 (zlib / gzip / PNG: zlib.crc32) of every block on the device while the bytes are
 * resident there (k_crc32: one streaming read, one word per block comes back; the length term and
 * every combine are host arithmetic).  The words can be persisted (kolm.checksums: a sidecar
 * file) and reproduced with standard tools. */
#define KOLM_CR_NONE 0      /* kolm_check_report.first_bad_reason */
#define KOLM_CR_MISMATCH 1  /* the block decodes to bytes with another CRC-32 */
#define KOLM_CR_REJECTED 2  /* the decoder rejected the payload */
typedef struct kolm_check_report {
    uint32_t blocks;              /* blocks checked */
    uint32_t bad_blocks;          /* of which: mismatching or rejected (0 without an expectation) */
    uint32_t first_bad_block;     /* the lowest-numbered bad block, its method id, the expected and */
    uint32_t first_bad_method;    /* the computed CRC-32 and the reason */
    uint32_t first_bad_expected;
    uint32_t first_bad_got;
    uint32_t first_bad_reason;    /* KOLM_CR_* */
    uint32_t stream_crc;          /* CRC-32 of the decoded stream: the blocks' words combined */
    uint64_t bytes;               /* decoded bytes checked */
    double ms_decode;             /* device time of the decode kernels (HIP events) */
    double ms_crc;                /* device time of k_crc32 */
} kolm_check_report;
/* CRC-32 of the blocks of d_data (device; block i = [h_bounds[i], h_bounds[i+1]), h_bounds[0] = 0,
 * non-decreasing: empty blocks are allowed and give 0, nblocks + 1 host entries, total < 2^31;
 * any alignment): h_crc[i].  *ms (optional): device time of k_crc32. */
int kolm_crc32_blocks_device(kolm_ctx* ctx, const void* d_data, const uint64_t* h_bounds, uint32_t nblocks,
                             uint32_t* h_crc, double* ms);
/* CRC-32 of A || B from crc_a = CRC-32(A), crc_b = CRC-32(B) and len_b = |B| (host only, usable
 * without a GPU; zlib's crc32_combine). */
uint32_t kolm_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* Checksums while encoding (default off, or KOLM_CHECKSUMS=1 at context creation): when enabled,
 * kolm_encode_blocks, kolm_encode_blocks_device, kolm_encode_blocks_device_var and every device
 * batch of kolm_compress_fixed run k_crc32 once over the batch's resident input, on the index
 * stream behind the event the sort stream (the critical path) starts from, so the pass runs beside
 * that chain; the words come back behind the batch's own final synchronisation.
 * Block numbers are container numbers, with dedup on too; independent of verify.  The contexts of
 * kolm_encode_blocks_multi ignore the switch.  Disabled: no extra launch, allocation or
 * synchronisation.  The container's bytes do not depend on the switch. */
int kolm_ctx_set_checksums(kolm_ctx* ctx, int enable);
int kolm_set_checksums(int enable);  /* default context */
/* The CRC-32 words of the last encode call of ctx (NULL: the default context), in container block
 * order, summed over its device batches: *nblocks (optional) their count (0 when the call ran with
 * checksums disabled), crc[0, cap) (optional; KOLM_ECAP when cap < the count). */
int kolm_ctx_checksums(kolm_ctx* ctx, uint32_t* crc, uint32_t cap, uint32_t* nblocks);
/* kolm_decode_blocks, and the CRC-32 of every decoded block taken on the device while the output
 * is resident: got[i] (optional).  With expect (optional, nblocks words) a block whose word
 * differs makes the call return KOLM_ECHECKSUM (kolm_last_error names the lowest-numbered such
 * block, its method, the expected and the computed word); out is still filled. */
int kolm_decode_blocks_crc(const uint8_t* payloads, const uint64_t* payload_off, const uint32_t* methods,
                           const uint32_t* orig_lens, uint32_t nblocks, uint8_t* out, uint64_t out_cap,
                           const uint32_t* expect, uint32_t* got);
/* A whole container against its blocks' CRC-32 words without the original data (host buffers,
 * default context): the TOC by kolm_toc_read (KOLM_EFORMAT as there), the payloads go up, the
 * blocks are decoded in the groups of kolm_verify_blocks_device ($KOLM_VERIFY_BYTES) and k_crc32
 * runs over each group's scratch; only the words come down: got[0, cap) (optional; KOLM_ECAP
 * when cap < the block count), *rep the summary.  expect (nblocks words) == NULL only computes:
 * the manifest of an existing container.  KOLM_OK whenever the check ran. */
int kolm_check_container(const uint8_t* container, uint64_t cn, const uint32_t* expect, uint32_t* got, uint32_t cap,
                         kolm_check_report* rep);
/* The expected CRC-32 of every block of the reader's container (nblocks = its block count; crc ==
 * NULL clears).  Once set, every group decode of kolm_reader_read / kolm_reader_read_device takes
 * the CRC-32 of the group's decoded blocks in the scratch and compares the words on the host
 * before anything is gathered (one more round trip per group): a mismatch makes the call return
 * KOLM_ECHECKSUM, and nothing is written to the output. */
int kolm_reader_set_checksums(kolm_reader* r, const uint32_t* crc, uint32_t nblocks);

/* ---- line index: count, locate and read a container's lines (lines_core.h, k_lines.hip) --- */
/* delim is one byte value.  D = the bytes of the decoded stream equal to delim, pos(k) the offset
 * of the k-th (0 <= k < D).  The stream's lines are what splitting at every delimiter gives: D + 1
 * lines, line k = [start_k, end_k) with start_0 = 0, start_k = pos(k - 1) + 1, end_k = pos(k) for
 * k < D and end_D = total_len; delimiters belong to no line, empty lines exist, an empty stream
 * has one empty line.  line_of(o), 0 <= o <= total_len, = the delimiters in [0, o).
 * The line index is one u32 per block: the block's delimiter count.  The container does not carry
 * it and does not change (kolm.lines: a sidecar).  With it every line question is block-local:
 * delimiter k lies in the one block a search of the counts' prefix sums names. */
/* Delimiter counts of the blocks of d_data (device; bounds as kolm_crc32_blocks_device: h_bounds[0]
 * = 0, non-decreasing, nblocks + 1 host entries, total < 2^31; any alignment): counts[i].  One
 * streaming read (k_delim_count).  *ms (optional): its device time. */
int kolm_delim_count_device(kolm_ctx* ctx, const void* d_data, const uint64_t* h_bounds, uint32_t nblocks, uint32_t delim,
                            uint32_t* counts, double* ms);
/* The same, and the counts of the blocks' 4 KiB pieces (block i's ceil(len / 4096) pieces behind
 * those of the blocks before it): piece_counts[0, cap) (KOLM_ECAP when cap < their number).  This
 * is the pass the line queries run on a decoded group; *ms covers k_delim_count and the scan of the
 * piece counts behind it. */
int kolm_delim_count_pieces_device(kolm_ctx* ctx, const void* d_data, const uint64_t* h_bounds, uint32_t nblocks,
                                   uint32_t delim, uint32_t* counts, uint32_t* piece_counts, uint64_t cap, double* ms);
/* Host only, usable without a GPU.  Delimiter numbers idx[0, n) -> the block that holds each and its
 * number inside that block (never a block without delimiters).  KOLM_EARG, the message naming the
 * entry, for a number at or above D = the sum of counts. */
int kolm_lines_locate(const uint32_t* counts, uint32_t nblocks, const uint64_t* idx, uint32_t n, uint32_t* block,
                      uint32_t* j);
/* Host only.  Stream offsets offs[0, n) -> the block that holds the byte (never an empty one; nblocks
 * for offs = total_len), the offset inside it and the delimiters in front of the block.  KOLM_EARG,
 * the message naming the entry, for an offset above total_len = the sum of orig_lens. */
int kolm_lines_locate_offsets(const uint32_t* orig_lens, const uint32_t* counts, uint32_t nblocks, const uint64_t* offs,
                              uint32_t n, uint32_t* block, uint32_t* in_block, uint64_t* before);
typedef struct kolm_lines_stats {
    uint32_t queries;         /* rank / select queries answered on the device */
    uint32_t blocks_decoded;
    uint32_t groups;          /* decode groups (bounded scratch: KOLM_READ_BYTES) */
    uint32_t reserved;
    uint64_t bytes_decoded;
    double ms_decode;         /* device time of the decode kernels (HIP events) */
    double ms_lines;          /* device time of k_delim_count, the scan and k_delim_query */
} kolm_lines_stats;
/* Attaches a line index to the reader: counts[nblocks] for delim (nblocks = the reader's block
 * count, KOLM_EARG otherwise; counts == NULL detaches). */
int kolm_reader_set_lines(kolm_reader* r, uint32_t delim, const uint32_t* counts, uint32_t nblocks);
/* Builds the index and attaches it: every block is decoded in the groups of kolm_range_plan
 * (KOLM_READ_BYTES), k_delim_count runs on each group's scratch and only the counts come back:
 * counts[0, cap) (optional; KOLM_ECAP when cap < the block count).  With checksums set each group is
 * checked first.  KOLM_EARG for a block the device does not decode. */
int kolm_reader_index_lines(kolm_reader* r, uint32_t delim, uint32_t* counts, uint32_t cap, kolm_lines_stats* stats);
/* starts[i], ends[i] of lines[i], i < n.  Every delimiter needed is located once (lines k and k + 1
 * share pos(k); line 0's start and line D's end need none), only the blocks that hold one are
 * decoded, grouped as a read's blocks are; per group: decode, k_delim_count with piece counts, their
 * scan, k_delim_query (one SELECT per delimiter), one copy of the results.
 * Every argument is checked before the first launch: KOLM_EARG without an attached index, for a
 * line above D (the message names the entry) and for a selected block the device does not decode.
 * With checksums set each decoded group is checked before any result leaves (KOLM_ECHECKSUM).
 * A block whose real count differs from the index, or a SELECT that finds no delimiter, gives
 * KOLM_ELINES (the message names the block, the expected and the actual count).  A failed call
 * writes no result.  The results do not depend on KOLM_READ_BYTES. */
int kolm_reader_line_spans(kolm_reader* r, const uint64_t* lines, uint32_t n, uint64_t* starts, uint64_t* ends,
                           kolm_lines_stats* stats);
/* lines[i] = line_of(offs[i]), i < n: the same group loop with one RANK per offset.  An offset at a
 * block's start, or equal to total_len, needs no decode.  Errors as kolm_reader_line_spans (an
 * offset above total_len: KOLM_EARG, the message naming the entry). */
int kolm_reader_line_of(kolm_reader* r, const uint64_t* offs, uint32_t n, uint64_t* lines, kolm_lines_stats* stats);
/* The line index while encoding (default off, or KOLM_LINES=1 at context creation with
 * KOLM_LINES_DELIM = the delimiter as a decimal byte value, default 10): when enabled,
 * kolm_encode_blocks, kolm_encode_blocks_device, kolm_encode_blocks_device_var and every device
 * batch of kolm_compress_fixed run k_delim_count once over the batch's resident input, where the
 * CRC pass of kolm_ctx_set_checksums is launched; the counts come back behind the batch's own final
 * synchronisation.  The contexts of kolm_encode_blocks_multi ignore the switch.  Disabled: no extra
 * launch, allocation or synchronisation.  The container's bytes do not depend on the switch. */
int kolm_ctx_set_lines(kolm_ctx* ctx, int enable, uint32_t delim);
int kolm_set_lines(int enable, uint32_t delim);  /* default context */
/* The counts of the last encode call of ctx (NULL: the default context), in container block order:
 * *nblocks (optional) their count (0 when the call ran with the switch off), *delim (optional) the
 * delimiter, counts[0, cap) (optional; KOLM_ECAP when cap < the count). */
int kolm_ctx_lines(kolm_ctx* ctx, uint32_t* counts, uint32_t cap, uint32_t* nblocks, uint32_t* delim);

/* ---- collectives: RCCL over xGMI, one process per GPU (kolm_comm.cpp) ------------- */
/* The only data exchange of the multi-GPU path: blocks are independent (PY:2350-2369), so
 * each rank encodes its block shard alone and the payloads are gathered onto one rank to
 * write the container (PY:2375-2445).  Every function returns KOLM_ERCCL on an RCCL error
 * (message: kolm_last_error).  Calls on one communicator are serialised. */
#define KOLM_COMM_ID_BYTES 128
typedef struct kolm_comm kolm_comm;
/* A fresh communicator id (ncclGetUniqueId): one rank creates it, every rank passes the
 * same KOLM_COMM_ID_BYTES bytes to kolm_comm_init (the caller moves them between the
 * processes: kolm.parallel does it over a TCP socket at MASTER_ADDR). */
int kolm_comm_unique_id(uint8_t* id);
/* Rank `rank` of an nranks-rank communicator on ctx's device (ncclCommInitRank: returns
 * when every rank has joined).  One rank per device. */
int kolm_comm_init(kolm_ctx* ctx, int nranks, int rank, const uint8_t* id, kolm_comm** out);
int kolm_comm_destroy(kolm_comm* comm);
int kolm_comm_rank(kolm_comm* comm, int* rank, int* nranks);
/* values[0, count) (host memory, 8-byte elements: dtype 0 uint64, 1 double) reduced over
 * every rank in place (op 0 sum, 1 max); synchronous.  kolm_comm_barrier: an all-reduce of
 * one word. */
int kolm_comm_allreduce(kolm_comm* comm, void* values, uint32_t count, int dtype, int op);
int kolm_comm_barrier(kolm_comm* comm);
/* Gathers every rank's payloads onto rank dst.  Each rank passes its payload arena
 * d_arena[0, nbytes) (device memory of its context, complete — e.g. as
 * kolm_encode_blocks_device returned it) and its nblocks method ids / nblocks + 1 payload
 * offsets (host arrays, as kolm_encode_blocks_device returned them).  On dst, d_dst
 * (device, dst_cap bytes) receives the ranks' payloads back to back in rank order,
 * method_all / off_all (host, dst_cap_blocks / dst_cap_blocks + 1 entries; either may be
 * NULL) the ranks' ids in rank order and their offsets into d_dst (off_all[total blocks] =
 * total bytes).  On every rank rank_bytes / rank_blocks (nranks entries, optional)
 * receive each rank's sizes.  When the payloads or ids do not fit dst's capacities every
 * rank returns KOLM_ECAP (sizes filled) and nothing is transferred.  async_op != 0:
 * returns once the transfers are queued on the communicator's stream; d_arena must stay
 * unmodified and the outputs are valid only after kolm_comm_wait (or the next call on the
 * communicator) — the transfer of one batch then runs while the next one encodes. */
int kolm_gather_payloads(kolm_comm* comm, const void* d_arena, uint64_t nbytes, const uint32_t* method,
                         const uint64_t* payload_off, uint32_t nblocks, int dst, void* d_dst, uint64_t dst_cap,
                         uint32_t dst_cap_blocks, uint64_t* rank_bytes, uint32_t* rank_blocks,
                         uint32_t* method_all, uint64_t* off_all, int async_op);
/* Completes the communicator's asynchronous gather, if any (every rank). */
int kolm_comm_wait(kolm_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* KOLM_H */
