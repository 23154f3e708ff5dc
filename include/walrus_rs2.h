/*
 * walrus_rs2.h -- C ABI of the MI355X-native Red Stuff (RS2) engine.
 *
 * This is the drop-in boundary for the Red Stuff hot path of MystenLabs/walrus
 * (crates/walrus-core/src/encoding).  Every entry point below names the reference
 * interface it replaces (paths relative to the reference checkout).  The Rust side
 * would bind these through a thin `extern "C"` block; see INTEGRATION.md.
 *
 * Conventions
 *  - Plain pointers and sizes only.  No torch / HIP types in signatures; device
 *    streams are passed as an opaque `void*` (a hipStream_t).  For plans and verifiers
 *    NULL selects the object's own stream and RS2_STREAM_LEGACY the HIP null stream.  The
 *    codec / hashing primitives take the stream as given (NULL = null stream).
 *  - Caller-allocated outputs.  The engine never frees caller memory.
 *  - Every call is synchronous (blocks until the results are in the caller's buffers)
 *    unless its name ends in `_async`.  Calls are re-entrant: one plan per thread, or
 *    serialise use of a plan (the reference call sites are rayon / tokio blocking
 *    threads, walrus-sdk/src/node_client.rs:3182, walrus-service/src/node.rs:2615).
 *  - Return value: RS2_OK or a negative error code mapping 1:1 onto the reference
 *    error enums (encoding/errors.rs:34-66, encoding/basic_encoding.rs:148-150).
 *  - Byte layouts are exactly the reference's: a symbol is `symbol_size` bytes, a
 *    sliver is its symbols concatenated, slivers are indexed by sliver index (primary
 *    sliver i = row i of the expanded matrix, secondary sliver j = column j); sliver
 *    pair i = (primary i, secondary n-1-i) (lib.rs:485-491).
 *  - Metadata layout: `hashes` is n_shards x {primary_hash[32], secondary_hash[32]}
 *    ordered by sliver-pair index (metadata.rs:611-643); `blob_id` is 32 bytes
 *    (lib.rs:159-176).
 *  - Device pointers (every `d_*` argument and `void*` buffer of the `_device` / `_async`
 *    calls).  Each call states the exact extent of every buffer; ALIGNMENT is by kind:
 *      symbol-carrying buffers -- blobs, slivers, decoded blobs, recovery symbols, codec
 *        sources and destinations -- are 2-byte aligned, and so is every byte offset
 *        (sliver_off[i], sym_off[i]) and stride (blob / sliver / symbol / line strides) that
 *        places a symbol;
 *      digest, proof and node buffers -- d_hashes, d_blob_id(s), d_leaves, d_roots, d_proofs,
 *        d_nodes -- are 16-byte aligned, their strides multiples of 16.
 *    A violating pointer, offset or stride is refused on the host with RS2_E_INVALID_ARGUMENT
 *    before anything is enqueued.  No slack beyond the stated extent is required: nothing
 *    outside the stated extent of an output is written (stride gaps and bytes at or past an
 *    out_limit / blob_len included), and no result depends on a byte outside the stated extent
 *    of an input (tests/test_gpu_guard_*.py hold every call to this inside guard bands, at
 *    every even placement mod 16).
 */
#ifndef WALRUS_RS2_H
#define WALRUS_RS2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (encoding/errors.rs) --------------------------------------------------- */
#define RS2_OK 0
#define RS2_E_DATA_TOO_LARGE (-1)          /* DataTooLargeError / DecodeError::DataTooLarge     */
#define RS2_E_EMPTY_DATA (-2)              /* InvalidDataSizeError::EmptyData                    */
#define RS2_E_INCORRECT_DATA_LENGTH (-3)   /* EncodeError::IncorrectDataLength(expected)         */
#define RS2_E_INCOMPATIBLE_PARAMETERS (-4) /* EncodeError/DecodeError::IncompatibleParameters    */
#define RS2_E_NOT_ENOUGH_SHARDS (-5)       /* DecodeError::DecoderError(NotEnoughShards)         */
#define RS2_E_DECODING_UNSUCCESSFUL (-6)   /* DecodeError::DecodingUnsuccessful                  */
#define RS2_E_VERIFICATION (-7)            /* DecodeError::VerificationError                     */
#define RS2_E_INVALID_ARGUMENT (-8)        /* null pointer, index out of range (a panic in Rust) */
#define RS2_E_UNSUPPORTED (-9)             /* shape outside this build's kernels                 */
#define RS2_E_DEVICE (-10)                 /* HIP runtime failure / no GPU                       */
#define RS2_E_INTERNAL (-11)               /* an `expect` in the reference                        */

#define RS2_AXIS_PRIMARY 0   /* common.rs:11-25 Primary   */
#define RS2_AXIS_SECONDARY 1 /* common.rs:11-25 Secondary */

#define RS2_CHECK_SKIP 0    /* ConsistencyCheckType::Skip    (common.rs:47-56) */
#define RS2_CHECK_DEFAULT 1 /* ConsistencyCheckType::Default */
#define RS2_CHECK_STRICT 2  /* ConsistencyCheckType::Strict  */

/* Stream argument of the plan / verifier calls: NULL selects the object's own stream; this
 * value selects the HIP null stream (the legacy default stream, e.g. torch's default). */
#define RS2_STREAM_LEGACY ((void*)1)

#define RS2_DIGEST_LEN 32
#define RS2_ENCODING_TYPE_RS2 1

/* ---- parameters (pure functions, no device needed) -------------------------------------- */

/* ReedSolomonEncodingConfig::new -> (source_symbols_primary, source_symbols_secondary);
 * encoding/config.rs:446-460,717-725 and bft.rs:12-25. */
int rs2_source_symbols_for_n_shards(uint16_t n_shards, uint16_t* n_primary, uint16_t* n_secondary);

/* utils::compute_symbol_size (encoding/utils.rs:10-25) for the blob of `blob_len` bytes. */
int rs2_symbol_size_for_blob(uint16_t n_shards, uint64_t blob_len, uint16_t* symbol_size);

/* EncodingFactory::encoded_blob_length (config.rs:791-826): slivers + metadata bytes. */
int rs2_encoded_blob_length(uint16_t n_shards, uint64_t blob_len, uint64_t* encoded_len);

/* ---- device context ---------------------------------------------------------------------- */

/* Select the HIP device used by plans created afterwards on this thread (default 0). */
int rs2_set_device(int device);
/* Human-readable message for the last error on this thread (never NULL). */
const char* rs2_last_error(void);
/* 1 when the HIP engine is usable (a GPU is visible and the kernels load), else 0. */
int rs2_device_available(void);

/* Engine tuning (no reference counterpart): largest transform block a codec workgroup holds
 * on chip (a power of two <= 512, default 512 or $RS2_BLOCK_MAX).  Larger transforms are split
 * into blocks with block-level mixing; outputs are identical for every setting.  Applies to
 * plans created afterwards. */
int rs2_set_block_limit(uint32_t max_block);

/* ---- blob plans ---------------------------------------------------------------------------
 * A plan binds (n_shards, blob_len): it derives K_p, K_s and the symbol size
 * (BlobEncoder::new, blob_encoding.rs:239-264) and owns device scratch, constant
 * tables and a HIP stream.  Creating it returns RS2_E_DATA_TOO_LARGE like
 * BlobEncoder::new does.                                                                     */
typedef struct rs2_plan rs2_plan;

typedef struct rs2_plan_info {
  uint16_t n_shards;
  uint16_t n_primary;   /* K_p: rows of the message matrix, symbols per secondary sliver */
  uint16_t n_secondary; /* K_s: columns, symbols per primary sliver                      */
  uint16_t symbol_size;
  uint64_t blob_len;
  uint64_t primary_sliver_len;   /* K_s * symbol_size */
  uint64_t secondary_sliver_len; /* K_p * symbol_size */
} rs2_plan_info;

int rs2_plan_create(uint16_t n_shards, uint64_t blob_len, rs2_plan** out);
int rs2_plan_info_get(const rs2_plan* plan, rs2_plan_info* info);
/* Drains the plan's streams and returns its device buffers to the device's arena (below). */
void rs2_plan_destroy(rs2_plan* plan);

/* Re-points a plan at another blob length of the same symbol size (K_p, K_s, s unchanged):
 * its tables and buffers are kept, so one plan per (n_shards, symbol size) serves every blob
 * of that size class.  The reference builds a BlobEncoder / BlobDecoder per call
 * (config.rs:545-567, 591-603); a cache keyed by (n_shards, symbol_size) plus this call is
 * the bounded equivalent.  RS2_E_INCOMPATIBLE_PARAMETERS if the length needs another symbol
 * size, RS2_E_DATA_TOO_LARGE if it fits none.  Not concurrent with other calls on the plan.  */
int rs2_plan_rebind(rs2_plan* plan, uint64_t blob_len);

/* Device memory accounting.  Every device buffer of plans, codecs, verifiers and contexts is a
 * range of a per-device arena: a few large hipMalloc'd segments, best fit over coalesced free
 * ranges.  A segment is added only when nothing fits (max(request, reserve / 2, 256 MiB)), so
 * plan churn stops calling hipMalloc once the reserve covers its peak; RS2_ARENA_RESERVE_MIB
 * reserves a first segment up front (a fixed device-memory budget), RS2_ARENA_CACHE_MIB
 * (default 8192) caps the reserve kept when segments fall wholly free.  stats_out[7]:
 *   0 hipMalloc calls (segments)   1 hipFree calls   2 live bytes   3 reserved bytes
 *   4 peak live bytes   5 device synchronizes for quarantined ranges
 *   6 pinned host allocations (the host-buffer ABI's staging rings, pooled per device)      */
int rs2_device_memory_stats(int device, uint64_t* stats_out);

/* Counters of the small per-call uploads (a decode's position offsets and multiplier logs,
 * verifier targets, large codec jobs), which travel through a ring of pinned, device-mapped
 * slots and a copy kernel.  stats_out[3]:
 *   0 uploads through the slot ring   1 codec jobs through the job ring
 *   2 slot reuses that had to wait for the slot's previous copy (a completion word the copy
 *     kernel stores; no event and no device-wide synchronize is ever taken for a slot)
 * Device-wide synchronizes the engine takes are rs2_device_memory_stats slot 5.
 * No reference counterpart (the reference computes on the host).                            */
int rs2_upload_stats(uint64_t* stats_out);

/* Hand every wholly free arena segment of `device` back to hipFree (after a device synchronize
 * when ranges wait in quarantine), e.g. after a transient large blob, so the memory is the
 * process's other allocators' again (torch's caching allocator).  *released_bytes (may be
 * NULL) = the bytes returned.  No reference counterpart (the reference's buffers are Vec<u8>). */
int rs2_device_memory_trim(int device, uint64_t* released_bytes);

/* ---- 2D Red Stuff: host buffers ------------------------------------------------------------ */

/* Caller-owned host buffers registered with the engine (page-locked in place, hipHostRegister):
 * a host-buffer call's transfer whose host range lies wholly inside a registered range skips the
 * pinned staging ring and its host copies and moves by DMA straight between the caller's memory
 * and the device.  For callers that reuse long-lived buffers (a node's or publisher's sliver
 * and blob buffers); page-locking costs about as much as one staged transfer of the range, so
 * it does not pay for one-shot buffers.  The range must stay allocated, and no host-buffer call
 * may be using it, until rs2_host_unregister(ptr) with the same start.  Process-wide (every
 * device).  RS2_E_INVALID_ARGUMENT on an empty range, an overlap with a registered range or an
 * unregistered pointer.  Extension: the reference has no counterpart (its CPU path has no
 * staging). */
int rs2_host_register(void* ptr, uint64_t len);
int rs2_host_unregister(void* ptr);

/* BlobEncoder::encode_with_metadata (blob_encoding.rs:277-368) /
 * EncodingFactory::encode_with_metadata (config.rs:591-596).
 * primary_out[i]   : n_shards pointers, primary sliver i (K_s*s bytes) by sliver index
 * secondary_out[j] : n_shards pointers, secondary sliver j (K_p*s bytes) by sliver index
 * hashes_out       : n_shards*64 bytes (may be NULL), blob_id_out: 32 bytes (may be NULL).
 * primary_out / secondary_out (or single entries) may be NULL to skip those slivers.
 * Host buffers move through a per-plan pinned staging ring (host copies on worker threads
 * under the DMA); the primary slivers leave while the secondary codecs and hashing run. */
int rs2_encode_with_metadata(rs2_plan* plan, const uint8_t* blob, uint8_t* const* primary_out,
                             uint8_t* const* secondary_out, uint8_t* hashes_out,
                             uint8_t* blob_id_out);

/* BlobEncoder::compute_metadata (blob_encoding.rs:406-486) / config.rs:598-603. */
int rs2_compute_metadata(rs2_plan* plan, const uint8_t* blob, uint8_t* hashes_out,
                         uint8_t* blob_id_out);

/* ---- blob batches ---------------------------------------------------------------------------
 * Many blobs of the plan's symbol size encoded together (the upload relay's server-side encode,
 * walrus-upload-relay/src/controller.rs:177, and the client's per-blob encode loop
 * encode_blobs_as, walrus-sdk/src/node_client.rs:3156-3221, each blob a
 * BlobEncoder::encode_with_metadata, blob_encoding.rs:277-368): every stage is one launch over
 * the whole batch.  Blob b has blob_lens[b] bytes (blob_lens NULL = the plan's blob_len for
 * every blob); each length must give the plan's symbol size (rs2_symbol_size_for_blob), else
 * RS2_E_INVALID_ARGUMENT.  At most 65535 blobs.
 *
 * Device form: blob b at d_blobs + b*blob_stride; its slivers in the single-blob layouts at
 * d_primary + b*primary_stride (>= n*primary_sliver_len) and d_secondary + b*secondary_stride;
 * its n pair hashes at d_hashes + b*64*n, its BlobId at d_blob_ids + b*32.  Same stream rules
 * as rs2_encode_device_async.  Extents: d_blobs (n_blobs-1)*blob_stride + the last blob's
 * length; d_primary (n_blobs-1)*primary_stride + n*K_s*s, d_secondary likewise with n*K_p*s
 * (the stride padding between two blobs' slivers is not written); d_hashes n_blobs*64*n;
 * d_blob_ids n_blobs*32.  d_blobs, d_primary, d_secondary and the three strides 2-byte
 * aligned, d_hashes and d_blob_ids 16-byte aligned. */
int rs2_encode_batch_device_async(rs2_plan* plan, uint32_t n_blobs, const void* d_blobs,
                                  uint64_t blob_stride, const uint64_t* blob_lens, void* d_primary,
                                  uint64_t primary_stride, void* d_secondary,
                                  uint64_t secondary_stride, void* d_hashes, void* d_blob_ids,
                                  void* stream);
/* Host form: blobs[b] (blob_lens[b] bytes); primary_out / secondary_out hold n_blobs*n sliver
 * pointers, blob-major (either array, or any entry, may be NULL: not returned); hashes_out
 * n_blobs*n*64 bytes and blob_ids_out n_blobs*32 bytes (either may be NULL).  Blocking. */
int rs2_encode_batch_with_metadata(rs2_plan* plan, uint32_t n_blobs, const uint8_t* const* blobs,
                                   const uint64_t* blob_lens, uint8_t* const* primary_out,
                                   uint8_t* const* secondary_out, uint8_t* hashes_out,
                                   uint8_t* blob_ids_out);

/* ---- blob encode across sizes: a symbol size per blob ---------------------------------------
 * The symbol size is a function of a blob's length, so an upload relay (walrus-upload-relay/src/
 * controller.rs:177) or a client encoding a queue of blobs (encode_blobs_as, node_client.rs:
 * 3156-3221) has about as many sizes as blobs, and rs2_encode_batch_* -- bound to one plan, one
 * size -- would take a call per size.  An encoder is bound to n_shards only; one call takes
 * n_blobs blobs, each with its own length.  Blob b is blob_lens[b] bytes at d_blobs_base +
 * blob_off[b]; its symbol size is s_b = rs2_symbol_size_for_blob(n_shards, blob_lens[b]); its
 * primary slivers lie in the single-blob layout (n*K_s*s_b bytes) at d_primary_base +
 * primary_off[b], its secondary slivers (n*K_p*s_b bytes) at d_secondary_base + secondary_off[b],
 * its n pair hashes at d_hashes + b*64*n and its BlobId at d_blob_ids + b*32 -- for every blob bit
 * for bit what rs2_encode_device_async writes for that blob alone.  Nothing outside these extents
 * is read or written; in particular no byte at or past blob_off[b] + blob_lens[b] is read.
 * d_blobs_base, d_primary_base, d_secondary_base and every offset are 2-byte aligned, d_hashes
 * and d_blob_ids 16-byte aligned.  THE OUTPUT EXTENTS OF DIFFERENT BLOBS MUST NOT OVERLAP EACH
 * OTHER OR THE BLOBS: that is the caller's duty, nothing checks it.
 * Metadata only (BlobEncoder::compute_metadata, blob_encoding.rs:406-486): d_primary_base and
 * d_secondary_base NULL together; the two offset arrays are then ignored, the slivers go to the
 * window's scratch and count toward its budget.  One of them NULL without the other:
 * RS2_E_INVALID_ARGUMENT for the whole call.
 * Per blob, decided on the host before anything is enqueued: the codes rs2_plan_create and
 * rs2_encode_device_async give for that length (RS2_E_DATA_TOO_LARGE, RS2_E_INCOMPATIBLE_PARAMETERS
 * for an n_shards without a recovery code); an odd blob_off[b], primary_off[b] or
 * secondary_off[b] RS2_E_INVALID_ARGUMENT; host form only: a NULL blob of non-zero length
 * RS2_E_INVALID_ARGUMENT.  status_out NULL: the first failing blob's code is returned and nothing
 * is enqueued; non-NULL: failing blobs get their code and are skipped (none of their output slots
 * is touched), the rest run, RS2_OK.  Whole-call refusals (RS2_E_INVALID_ARGUMENT): a NULL
 * encoder or needed array, a base that is not 2-byte or a d_hashes / d_blob_ids that is not
 * 16-byte aligned, more than 65535 blobs.  n_blobs 0: RS2_OK, nothing enqueued.
 *
 * How it runs.  Blobs are taken, in the caller's order, in windows: a blob of symbol size s holds
 * (n-K_p)*(n-K_s)*s + 32*n*n bytes of scratch (its repair-repair quadrant and its n*n leaf
 * digests; metadata only: n*(K_p+K_s)*s more for its slivers; the zero-padded message is staged
 * in the blob's own systematic primary slivers and takes nothing more).  A window closes before the
 * blob that would take it past the budget (rs2_set_encode_mixed_budget; at least one blob per
 * window) or past RS2_ENCODE_MIXED_WINDOW_BLOBS blobs (what keeps a window's job and offset tables
 * within a third of the pinned upload ring), so scratch does not grow with n_blobs.  The default
 * budget is 4 GiB: at n_shards = 1000 a blob's leaves alone are 32 MB, so 256 MiB -- the other
 * mixed calls' default -- would cut windows at 8 small blobs and pay the window's launches for
 * each; 4 GiB holds about a hundred of them, and a blob of the largest symbol size (s = 65534: a
 * 14.5 GB quadrant) still runs as a window of its own.  Per window: one staging launch copies every
 * message into its primary slivers and zero-fills its padding; three codec launches, one per
 * stage (systematic columns with the systematic secondary slivers written from the same loads,
 * rows, repair columns), each a job per blob found from a tile prefix array; one leaf-hash launch
 * over a blob table; one tree launch and one root launch over all blobs of the window; and, when
 * the window's blobs are not consecutive in the caller's arrays from its first blob on (a refused
 * or per-blob one lies between), one launch that moves hashes and ids to the caller's slots.  That
 * is at most RS2_ENCODE_MIXED_WINDOW_LAUNCHES compute launches per window, however many blobs and
 * sizes it holds.  (Where the column code is not a single shared-input block -- n_shards = 13,
 * or above 1534 at the default block limit -- its codec has no fused copy-out and the staging
 * launch writes the systematic secondary slivers instead.)  A blob runs there iff its symbol
 * size is >= 4, n_shards <= 4096, all three stages have 1..8 transform blocks on each side
 * (n_shards = 10 .. 4096 have at most 3 at the default block limit) and the tiles of each stage launch stay below
 * 2^31.  Every other blob (a 2-byte symbol,
 * wider n_shards) runs inside the same call and window through the single-blob encode, a blob at a
 * time on an internally cached plan per size, on the same stream; only that path may wait for the
 * device (a plan re-bound to other buffers waits for its previous encode).  All blobs of at most
 * 2*K_p*K_s bytes share s = 2: a batch of those should keep rs2_encode_batch_*.
 * Measured (tools/encode_mixed_probe.py, MI355X, n_shards = 1000, device-resident; DESIGN.md
 * §22): 32 symbol sizes 4 .. 66, two blobs each: 15.1 ms against 21.5 ms for 32
 * rs2_encode_batch_device_async calls (1.43x); 64 blobs uniform at s = 20: 12.9 ms against 12.0 ms
 * for the one rs2_encode_batch_device_async call (1.08x slower: its leaf kernel is specialised per
 * message length), so a batch uniform in size should keep that call.
 * The call is enqueued on `stream` and never waits for the device on the group path; the host
 * arrays may be reused as soon as it returns (the tables go through the pinned upload ring).
 * Stream conventions and the `done` event as the checker's; one encoder per thread, or serialise
 * its use; destroy waits for pending work. */
#define RS2_ENCODE_MIXED_WINDOW_LAUNCHES 8
#define RS2_ENCODE_MIXED_WINDOW_BLOBS 256
typedef struct rs2_blob_encoder rs2_blob_encoder;
int rs2_blob_encoder_create(uint16_t n_shards, rs2_blob_encoder** out);
void rs2_blob_encoder_destroy(rs2_blob_encoder* e);
int rs2_blob_encoder_encode_device_async(
    rs2_blob_encoder* e, uint32_t n_blobs, const uint64_t* blob_lens, const void* d_blobs_base,
    const uint64_t* blob_off, void* d_primary_base, const uint64_t* primary_off,
    void* d_secondary_base, const uint64_t* secondary_off, void* d_hashes, void* d_blob_ids,
    int* status_out, void* stream);
/* Host form (blocking): blobs[b] is blob b (blob_lens[b] bytes); primary_out / secondary_out hold
 * n_blobs*n sliver pointers, blob-major (either array, or any entry, may be NULL: not returned);
 * hashes_out n_blobs*n*64 bytes and blob_ids_out n_blobs*32 bytes (either may be NULL).  Output
 * slots of skipped blobs are not written. */
int rs2_encode_blobs_with_metadata(uint16_t n_shards, uint32_t n_blobs, const uint8_t* const* blobs,
                                   const uint64_t* blob_lens, uint8_t* const* primary_out,
                                   uint8_t* const* secondary_out, uint8_t* hashes_out,
                                   uint8_t* blob_ids_out, int* status_out);
/* Window scratch of the mixed encode in bytes (default 4 GiB; 0 restores it).  Process-wide. */
int rs2_set_encode_mixed_budget(uint64_t bytes);
/* Process-wide counters, stats_out[5]: windows; blobs encoded inside group launches; blobs that
 * took the per-blob path; distinct symbol sizes inside windows; compute launches of the group
 * path (staging, codecs, leaf hash, trees, roots, scatter; table uploads and the per-blob path's
 * own launches are not counted).  No reference counterpart. */
int rs2_encode_mixed_stats(uint64_t* stats_out);

/* BlobDecoder::decode (blob_encoding.rs:888-993) / EncodingFactory::decode (config.rs:605-611).
 * `count` slivers of axis `axis`, sliver i at slivers[i] with index sliver_idx[i], length
 * sliver_len[i] bytes and symbol size sliver_symbol_size[i] (NULL: all equal to the plan's).
 * As check_and_write_slivers_to_workspace (blob_encoding.rs:904-951): a repeated index is
 * skipped, a sliver of the wrong length or symbol size dropped, the surplus beyond K
 * dropped; too few -> RS2_E_DECODING_UNSUCCESSFUL.  An index >= n_shards is taken like the
 * reference takes it and then fails the column decodes -> RS2_E_NOT_ENOUGH_SHARDS
 * (DecodeError::DecoderError).  blob_out: blob_len bytes. */
int rs2_decode_blob(rs2_plan* plan, int axis, uint32_t count, const uint16_t* sliver_idx,
                    const uint8_t* const* slivers, const uint64_t* sliver_len,
                    const uint16_t* sliver_symbol_size, uint8_t* blob_out);

/* EncodingFactory::decode_and_verify (config.rs:613-658).  `hashes` / `blob_id` are the
 * metadata being verified against (n_shards*64 and 32 bytes).
 *   RS2_CHECK_DEFAULT: BlobEncoder::default_consistency_check (blob_encoding.rs:579-612) --
 *     with primary slivers, every systematic index (< K_p) the decoder pulled from the input
 *     counts as already verified (config.rs:621-640) and only the other systematic primary
 *     slivers are re-encoded and Merkle-checked (on the device); with secondary slivers all
 *     K_p are checked.
 *   RS2_CHECK_STRICT: the decoded blob's metadata is re-derived and its blob id compared
 *     (config.rs:164-172).
 * A failed check -> RS2_E_VERIFICATION (blob_out then unspecified). */
int rs2_decode_and_verify(rs2_plan* plan, int axis, uint32_t count, const uint16_t* sliver_idx,
                          const uint8_t* const* slivers, const uint64_t* sliver_len,
                          const uint16_t* sliver_symbol_size, const uint8_t* hashes,
                          const uint8_t* blob_id, int consistency_check, uint8_t* blob_out);

/* ---- 2D Red Stuff: device-resident (the measured path) ----------------------------------------
 * Same semantics with device buffers: d_blob (blob_len bytes); d_primary n*K_s*s bytes
 * (primary sliver i at i*K_s*s); d_secondary n*K_p*s bytes (secondary sliver j at j*K_p*s);
 * d_hashes n*64; d_blob_id 32.  Work is enqueued on `stream` (hipStream_t, NULL = the
 * plan's stream); the call returns after enqueueing.  d_blob, d_primary and d_secondary are
 * 2-byte aligned, d_hashes and d_blob_id 16-byte aligned (all calls of this section).         */
int rs2_encode_device_async(rs2_plan* plan, const void* d_blob, void* d_primary, void* d_secondary,
                            void* d_hashes, void* d_blob_id, void* stream);

/* BlobEncoder::compute_metadata (blob_encoding.rs:406-486) on a device-resident blob: every
 * symbol is expanded and hashed, only d_hashes (n*64) and d_blob_id (32) are written (the
 * slivers go to the plan's own scratch).  The upload relay's call (walrus-upload-relay/src/
 * controller.rs:177) when the blob is already in HBM. */
int rs2_compute_metadata_device_async(rs2_plan* plan, const void* d_blob, void* d_hashes,
                                      void* d_blob_id, void* stream);

/* rs2_encode_device_async with an early hand-off of the primary slivers: `primary_stream`
 * (non-NULL, not `stream`) is made to wait only until every primary sliver is written, so
 * work queued on it next (a decode from primary slivers, their D2H to the storage backend)
 * runs beside the secondary codecs and the hashing still in flight on `stream`.  Outputs are
 * identical to rs2_encode_device_async.  The caller must order `stream` after its
 * primary_stream work before the next encode rewrites those buffers.  No reference
 * counterpart: the reference returns all slivers at once (blob_encoding.rs:277-368). */
int rs2_encode_device_split_async(rs2_plan* plan, const void* d_blob, void* d_primary,
                                  void* d_secondary, void* d_hashes, void* d_blob_id, void* stream,
                                  void* primary_stream);

/* Decode from `count` device slivers of `axis`: sliver i lives at d_slivers_base +
 * sliver_off[i] (bytes) and has index sliver_idx[i].  Host-side validation as in
 * rs2_decode_blob (all given slivers must have the correct length).  Each sliver is
 * K_s*s (primary) or K_p*s (secondary) bytes; d_blob_out: blob_len bytes, and nothing at or
 * past blob_len is written (the last symbols are cut, blob_encoding.rs:970-993).
 * d_slivers_base, every sliver_off[i] and d_blob_out are 2-byte aligned. */
int rs2_decode_device_async(rs2_plan* plan, int axis, uint32_t count, const uint16_t* sliver_idx,
                            const void* d_slivers_base, const uint64_t* sliver_off,
                            void* d_blob_out, void* stream);

/* ---- decode batches -------------------------------------------------------------------------
 * Many blobs of the plan's symbol size decoded together, each from its own set of slivers (an
 * aggregator's or client's read of many small blobs, each a BlobDecoder::decode,
 * blob_encoding.rs:888-993): the blobs' decode jobs are planned on the host's worker threads and
 * run as one launch per chunk of a few hundred blobs.  A blob whose decode does not fit a batch
 * job (no erased original, a 2-byte symbol, more than 8 transform blocks) is decoded like
 * rs2_decode_device_async on the same stream, so the call serves every n_shards.
 *
 * Blob b: counts[b] slivers of `axis`, their indices / byte offsets consecutive in sliver_idx /
 * sliver_off (relative to d_slivers_base); length blob_lens[b] (NULL: the plan's), which must
 * give the plan's symbol size; decoded to d_blobs_out + b*out_stride, nothing at or past its
 * length written, the stride padding not written.  Per-blob rules as rs2_decode_device_async.
 * status_out NULL: the first failing blob's code is returned and nothing is enqueued;
 * non-NULL: failing blobs get their code and are skipped, the rest are decoded, RS2_OK.
 * n_blobs 0: RS2_OK, nothing enqueued.  At most 65535 blobs.  Alignment as the decode's
 * (d_slivers_base, every offset, d_blobs_out and out_stride 2-byte aligned; a misaligned base
 * or stride fails the call, a misaligned offset its blob). */
int rs2_decode_batch_device_async(rs2_plan* plan, int axis, uint32_t n_blobs,
                                  const uint64_t* blob_lens, const uint32_t* counts,
                                  const uint16_t* sliver_idx, const void* d_slivers_base,
                                  const uint64_t* sliver_off, void* d_blobs_out,
                                  uint64_t out_stride, int* status_out, void* stream);
/* Host form (blocking): slivers[] / sliver_len[] / sliver_symbol_size[] concatenated likewise
 * (per-sliver rules as rs2_decode_blob), blobs_out[b] receives blob b (blob_lens[b] bytes). */
int rs2_decode_batch(rs2_plan* plan, int axis, uint32_t n_blobs, const uint64_t* blob_lens,
                     const uint32_t* counts, const uint16_t* sliver_idx,
                     const uint8_t* const* slivers, const uint64_t* sliver_len,
                     const uint16_t* sliver_symbol_size, uint8_t* const* blobs_out,
                     int* status_out);
/* Process-wide counters, stats_out[3]: batched launches, blobs decoded inside them, blobs that
 * took the per-blob path.  No reference counterpart. */
int rs2_decode_batch_stats(uint64_t* stats_out);

/* ---- verified decode batches ------------------------------------------------------------------
 * The read path's call, EncodingFactory::decode_and_verify (config.rs:613-658), for many blobs of
 * the plan's symbol size at once: each blob decoded from its own slivers as in a decode batch and
 * checked against its own metadata, with a verdict per blob.  The blob, sliver, length and stride
 * arguments, the per-blob rules, the alignment rules, the status_out contract and the 65535-blob
 * limit are those of rs2_decode_batch_device_async / rs2_decode_batch; n_blobs 0: RS2_OK.
 *
 * Device form: the metadata is device-resident in the layout rs2_encode_batch_device_async
 * writes -- blob b's pair hashes at d_hashes + b*64*n, its id at d_blob_ids + b*32, both 16-byte
 * aligned.  RS2_CHECK_DEFAULT reads only the primary hash of pairs < K_p (d_blob_ids may be
 * NULL), RS2_CHECK_STRICT only the blob ids (d_hashes may be NULL), RS2_CHECK_SKIP neither.  A
 * NULL pointer the check needs, a misaligned one or a bad check value: RS2_E_INVALID_ARGUMENT
 * before anything is enqueued.  d_verdict (n_blobs int32, 16-byte aligned) receives one of the
 * constants below in every slot.  The checks are those of rs2_decode_and_verify_device: on the
 * primary axis every systematic index among the input slivers the decoder pulled counts as
 * verified, a blob with nothing left to check is a match; rows at or past blob_lens[b] are the
 * message's zero padding and hashed as zeros, no byte at or past blob_lens[b] of an output slot
 * is read or written.  A mismatching blob's decoded bytes stay in its slot.  With status_out
 * NULL and a failing blob the first code is returned and neither outputs nor verdicts are
 * touched.  All work is enqueued on the one stream (decodes, checks and verdicts of a window of
 * blobs, window after window); the call never synchronizes and reads no result back, and its
 * device scratch is bounded by the window budget below, not by n_blobs. */
#define RS2_BLOB_MISMATCH 0  /* decoded, the check failed                         */
#define RS2_BLOB_MATCH    1  /* decoded and the check passed (always, under SKIP) */
#define RS2_BLOB_SKIPPED  2  /* refused on the host (status_out[b] != RS2_OK)     */
int rs2_decode_and_verify_batch_device_async(
    rs2_plan* plan, int axis, uint32_t n_blobs, const uint64_t* blob_lens, const uint32_t* counts,
    const uint16_t* sliver_idx, const void* d_slivers_base, const uint64_t* sliver_off,
    const void* d_hashes, const void* d_blob_ids, int consistency_check, void* d_blobs_out,
    uint64_t out_stride, void* d_verdict, int* status_out, void* stream);
/* Host form (blocking): slivers as rs2_decode_batch (per-sliver rules as rs2_decode_and_verify),
 * hashes n_blobs*n*64 and blob_ids n_blobs*32 host bytes in the same layout (NULL as above).
 * blobs_out[b] receives blob b whatever its verdict; verdict_out (n_blobs values, required) is
 * written whenever the call returns RS2_OK. */
int rs2_decode_and_verify_batch(rs2_plan* plan, int axis, uint32_t n_blobs,
                                const uint64_t* blob_lens, const uint32_t* counts,
                                const uint16_t* sliver_idx, const uint8_t* const* slivers,
                                const uint64_t* sliver_len, const uint16_t* sliver_symbol_size,
                                const uint8_t* hashes, const uint8_t* blob_ids,
                                int consistency_check, uint8_t* const* blobs_out,
                                int32_t* verdict_out, int* status_out);
/* A window holds at most a decode chunk's blobs (a few hundred) and at most `bytes` of check
 * scratch (Default: gathered rows, their leaves and repair symbols; Strict: the re-encoded
 * slivers, repair quadrant and leaves), but always one blob.  Default 256 MiB; 0 restores it.
 * Process-wide, applies to calls made afterwards.  No reference counterpart. */
int rs2_set_verify_batch_budget(uint64_t bytes);
/* Process-wide counters, stats_out[4]: check windows, blobs checked (Default or Strict), rows
 * hashed by Default, blobs re-encoded by Strict.  No reference counterpart. */
int rs2_verify_batch_stats(uint64_t* stats_out);

/* EncodingFactory::decode_and_verify (config.rs:613-658) on device-resident slivers (as
 * rs2_decode_device_async) into the device buffer d_blob_out (blob_len bytes); `hashes` /
 * `blob_id` are host copies of the metadata.  The checks are those of rs2_decode_and_verify and
 * run on the device; the call returns once the verdict is known (RS2_E_VERIFICATION on a
 * failed check). */
int rs2_decode_and_verify_device(rs2_plan* plan, int axis, uint32_t count,
                                 const uint16_t* sliver_idx, const void* d_slivers_base,
                                 const uint64_t* sliver_off, const uint8_t* hashes,
                                 const uint8_t* blob_id, int consistency_check, void* d_blob_out,
                                 void* stream);

/* Wait for the plan's outstanding work on `stream` (NULL = plan stream). */
int rs2_sync(rs2_plan* plan, void* stream);

/* Stage profiler (no reference counterpart; the reference uses tracing spans,
 * blob_encoding.rs:261).  When enabled, the plan records a HIP event between consecutive
 * kernel launches on the stream; rs2_profile_read synchronises, returns per-stage totals
 * (names: 32-byte NUL-padded slots) and resets the totals. */
int rs2_profile_enable(rs2_plan* plan, int enable);
int rs2_profile_read(rs2_plan* plan, uint32_t max_stages, char* names, double* total_ms,
                     uint32_t* launches, uint32_t* n_stages);

/* ---- 1D codec (basic_encoding.rs) and sliver helpers ------------------------------------------ */

/* ReedSolomonEncoder::encode_all (basic_encoding.rs:195-211): `k*symbol_size` bytes of data ->
 * all n_shards symbols (source || repair), n_shards*symbol_size bytes.  `batch` independent
 * codewords laid out back to back (data stride k*s, output stride n*s). */
int rs2_encode_1d(uint16_t k, uint16_t n_shards, uint16_t symbol_size, uint32_t batch,
                  const uint8_t* data, uint8_t* out_all);

/* ReedSolomonDecoder::decode (basic_encoding.rs:387-429): `count` symbols with indices idx[]
 * (index < k: source symbol, else repair symbol index-k) -> the k source symbols.
 * Wrong-size symbols cannot occur at this ABI (fixed symbol_size); duplicates are ignored;
 * fewer than k distinct -> RS2_E_NOT_ENOUGH_SHARDS. */
int rs2_decode_1d(uint16_t k, uint16_t n_shards, uint16_t symbol_size, uint32_t count,
                  const uint16_t* idx, const uint8_t* const* symbols, uint8_t* out_source);

/* SliverData::get_merkle_root (slivers.rs:387-392): expand a sliver of `axis` on the
 * orthogonal axis and return the Merkle root over the n_shards symbols (the value
 * SliverData::verify / check_hash compares with the metadata, slivers.rs:100-135). */
int rs2_sliver_merkle_root(uint16_t n_shards, uint16_t symbol_size, int axis,
                           const uint8_t* sliver, uint64_t sliver_len, uint8_t root_out[32]);

/* Batched form of the above for `count` slivers of one axis and symbol size (the storage
 * node's verify_sliver_against_metadata, walrus-service/src/node.rs:2615-2633, and the
 * recovery-symbol service's per-sliver Merkle trees, node/recovery_symbol_service.rs:132-159).
 * A sliver of the wrong length -> RS2_E_INCORRECT_DATA_LENGTH.  roots_out: count*32 bytes. */
int rs2_sliver_merkle_roots(uint16_t n_shards, uint16_t symbol_size, int axis, uint32_t count,
                            const uint8_t* const* slivers, const uint64_t* sliver_len,
                            uint8_t* roots_out);

/* Device-resident batched sliver verification: a verifier binds (n_shards, symbol_size,
 * axis) and owns scratch + a stream; d_slivers holds `count` slivers back to back
 * (K*symbol_size bytes each, K = source symbols of the orthogonal axis' code), d_roots
 * receives count*32 bytes.  Same stream conventions as the plan API.  d_slivers 2-byte
 * aligned (count*K*symbol_size bytes), d_roots 16-byte aligned. */
typedef struct rs2_verifier rs2_verifier;
int rs2_verifier_create(uint16_t n_shards, uint16_t symbol_size, int axis, rs2_verifier** out);
int rs2_verifier_roots_device_async(rs2_verifier* v, uint32_t count, const void* d_slivers,
                                    void* d_roots, void* stream);
void rs2_verifier_destroy(rs2_verifier* v);

/* ---- recovery symbols with Merkle proofs ------------------------------------------------------
 * SliverData::recovery_symbol_for_sliver (slivers.rs:180-213), batched as the storage node's
 * recovery-symbol service runs it (walrus-service/src/node/recovery_symbol_service.rs:161-235):
 * request i expands source sliver i (of `axis`) on the orthogonal axis to n_shards symbols,
 * builds the MerkleTree over them (merkle.rs:216-266) and returns
 *   symbols_out + i*symbol_size : expanded symbol target_sliver_index[i] (the recovery symbol's
 *                                 data; its DecodingSymbol index is the source sliver's index)
 *   proofs_out + i*path_len*32  : MerkleTree::get_proof(target) (merkle.rs:281-309), the sibling
 *                                 path leaf -> root, path_len = rs2_merkle_tree_shape(n_shards).
 * target_sliver_index[i] is the index on the orthogonal axis (SliverPairIndex::to_sliver_index,
 * lib.rs:485-491); >= n_shards -> RS2_E_INVALID_ARGUMENT (RecoverySymbolError::IndexTooLarge).
 * A sliver of the wrong length -> RS2_E_INCORRECT_DATA_LENGTH. */
int rs2_recovery_symbols(uint16_t n_shards, uint16_t symbol_size, int axis, uint32_t count,
                         const uint8_t* const* slivers, const uint64_t* sliver_len,
                         const uint16_t* target_sliver_index, uint8_t* symbols_out,
                         uint8_t* proofs_out);

/* Device form on a verifier (slivers back to back as for rs2_verifier_roots_device_async;
 * target_sliver_index is a HOST array of `count` entries).  d_nodes (may be NULL) receives each
 * tree's full node array (count * n_nodes * 32 bytes, MerkleTree::nodes order: levels from the
 * leaves, each padded to even with the zero node, root last) -- what the service caches per
 * (blob, source sliver) (recovery_symbol_service.rs:132-159).  d_symbols: count*symbol_size
 * bytes, 2-byte aligned like d_slivers; d_proofs: count*path_len*32 bytes and d_nodes, both
 * 16-byte aligned. */
int rs2_verifier_recovery_symbols_device_async(rs2_verifier* v, uint32_t count,
                                               const void* d_slivers,
                                               const uint16_t* target_sliver_index,
                                               void* d_symbols, void* d_proofs, void* d_nodes,
                                               void* stream);

/* ---- recovery symbols in bulk: a target list per sliver, cached trees -------------------------
 * The serving side of a sliver recovery as the node's recovery-symbol service runs it: the
 * service keeps the MerkleTree per (blob, source sliver) (recovery_symbol_service.rs:132-159)
 * because one source sliver is asked for many targets -- a recovering peer that holds several
 * shards asks for one symbol per shard, and after an epoch change the same slivers are asked
 * again.  One call takes n_slivers source slivers of the verifier's axis (back to back in
 * d_slivers, as for rs2_verifier_roots_device_async) and a list of targets per sliver:
 * target_counts[i] (HOST, 0 allowed) targets of sliver i, consecutive in target_sliver_index
 * (HOST, orthogonal-axis indices, any order, repeats allowed).  Request j is a position in that
 * concatenated list; with path_len and n_nodes from rs2_merkle_tree_shape(n_shards) and
 * k = the verifier's symbols per sliver:
 *   d_slivers  n_slivers*k*symbol_size bytes, 2-byte aligned, read only
 *   d_symbols  request j's expanded symbol (slivers.rs:180-213) at + j*symbol_size; 2-byte aligned
 *   d_proofs   request j's MerkleTree::get_proof(target) (merkle.rs:281-309) at + j*path_len*32;
 *              16-byte aligned
 *   d_nodes    sliver i's tree at + i*n_nodes*32 in MerkleTree::nodes order (as the call above
 *              writes it); 16-byte aligned
 * Nothing outside these extents is read or written.  Each sliver is expanded and hashed once,
 * however many targets it has.  trees selects where the trees come from: */
#define RS2_TREES_BUILD  0  /* hash every sliver's n leaves, build its tree (d_nodes: optional output) */
#define RS2_TREES_CACHED 1  /* d_nodes holds the trees already (required, read only): no hashing     */
/* BUILD: a sliver with targets, and with a non-NULL d_nodes every sliver (a call whose counts are
 * all zero warms the cache), is expanded, hashed and its tree built; a sliver with no target and
 * no d_nodes does no work.  CACHED: d_nodes is never written, nothing is hashed, and the codec
 * runs only for slivers with a repair target (>= k) -- the expanded sliver is not kept, recompute
 * is the reference's own trade (slivers.rs:180-213); a call whose targets are all systematic
 * launches no codec, its symbols are copies out of the slivers.
 * Checked on the host before anything is enqueued (outputs untouched on failure):
 * RS2_E_INVALID_ARGUMENT for a NULL v or needed buffer, trees not one of the two values, CACHED
 * with a NULL d_nodes, a misaligned pointer, n_slivers > 65535, more than 2^31-1 requests, a
 * target >= n_shards (RecoverySymbolError::IndexTooLarge).  n_slivers 0: RS2_OK, nothing
 * enqueued.  The host arrays may be reused as soon as the call returns.  Stream conventions as
 * the other verifier calls; the call never synchronizes and reads nothing back.  Slivers are
 * taken in windows whose device scratch (leaves, repair symbols, node arrays the caller does not
 * take) stays within the budget below, one sliver at least: scratch does not grow with
 * n_slivers. */
int rs2_verifier_recovery_symbols_multi_device_async(
    rs2_verifier* v, uint32_t n_slivers, const void* d_slivers, const uint32_t* target_counts,
    const uint16_t* target_sliver_index, int trees, void* d_nodes, void* d_symbols, void* d_proofs,
    void* stream);
/* Host form (blocking, BUILD, pooled verifier and pinned staging like rs2_recovery_symbols):
 * slivers[i] of sliver_len[i] bytes; a NULL or wrong-length sliver ->
 * RS2_E_INCORRECT_DATA_LENGTH.  symbols_out / proofs_out laid out as d_symbols / d_proofs. */
int rs2_recovery_symbols_multi(uint16_t n_shards, uint16_t symbol_size, int axis,
                               uint32_t n_slivers, const uint8_t* const* slivers,
                               const uint64_t* sliver_len, const uint32_t* target_counts,
                               const uint16_t* target_sliver_index, uint8_t* symbols_out,
                               uint8_t* proofs_out);
/* Window scratch of the bulk call, process-wide, for calls made afterwards.  Default 256 MiB; 0
 * restores it.  No reference counterpart. */
int rs2_set_recovery_symbols_budget(uint64_t bytes);
/* Process-wide counters of the bulk calls, stats_out[5]: windows, slivers expanded (codec lines
 * launched), trees built, trees taken from the caller's cache (slivers of CACHED calls with at
 * least one target), requests served.  No reference counterpart. */
int rs2_recovery_symbols_stats(uint64_t* stats_out);

/* ---- sliver recovery in bulk ------------------------------------------------------------------
 * SliverData::recover_sliver_or_generate_inconsistency_proof (slivers.rs:341-379, called per
 * missing sliver from walrus-service's request_futures.rs:436-497) for many slivers of the
 * verifier's axis in one call, each from its own set of received recovery symbols: the 1D
 * decodes (slivers.rs:246-289) run as jobs of one launch per chunk of a few hundred slivers,
 * then each recovered sliver's Merkle root is formed and compared with the expected one.  A
 * sliver whose decode does not fit a batch job (every original received, a 2-byte symbol, more
 * than 8 transform blocks) is decoded on its own on the same stream.
 *
 * Sliver i: counts[i] received symbols, their DecodingSymbol indices (symbols.rs; the source
 * sliver's index) consecutive in symbol_idx (HOST), their data consecutive in d_symbols (sum of
 * counts symbols of symbol_size bytes back to back, 2-byte aligned).  It is written whole to
 * d_slivers_out + i*k*symbol_size (k = the verifier's symbols per sliver; 2-byte aligned):
 * received originals copied, erased ones decoded.  d_roots (may be NULL; n_slivers*32 bytes,
 * 16-byte aligned) receives the recovered slivers' roots as rs2_verifier_roots_device_async
 * computes them.  expected_roots (HOST, n_slivers*32 bytes, may be NULL): the target slivers'
 * hashes from their blobs' metadata; d_verdict (n_slivers int32, 16-byte aligned) then gets one
 * of the constants below in every slot.  expected_roots NULL: no verdicts, d_verdict must be
 * NULL too.
 * Per sliver, checked on the host before anything is enqueued: counts[i] < k ->
 * RS2_E_DECODING_UNSUCCESSFUL; else as rs2_decode_1d: entries in order, duplicates and indices
 * >= n_shards ignored, the first k distinct ones used, fewer -> RS2_E_NOT_ENOUGH_SHARDS.
 * status_out NULL: the first failing sliver's code is returned and nothing is enqueued;
 * non-NULL: failing slivers get their code and are skipped (output and root slot not written,
 * verdict RS2_SLIVER_SKIPPED), the rest run, RS2_OK.  n_slivers 0: RS2_OK, nothing enqueued.
 * At most 65535 slivers.  Stream conventions as the other verifier calls. */
#define RS2_SLIVER_MISMATCH 0   /* recovered, Merkle root differs from expected_roots[i]  */
#define RS2_SLIVER_MATCH    1   /* recovered and verified                                  */
#define RS2_SLIVER_SKIPPED  2   /* refused on the host (status_out[i] != RS2_OK), not decoded */
int rs2_verifier_recover_slivers_device_async(
    rs2_verifier* v, uint32_t n_slivers, const uint32_t* counts, const uint16_t* symbol_idx,
    const void* d_symbols, const uint8_t* expected_roots, void* d_slivers_out,
    void* d_roots, void* d_verdict, int* status_out, void* stream);
/* Host form (blocking): symbols[] holds one pointer per received symbol (symbol_size bytes
 * each), concatenated like symbol_idx; slivers_out[i] receives sliver i (k*symbol_size bytes),
 * roots_out (may be NULL) n_slivers*32 bytes, verdict_out n_slivers values (NULL exactly when
 * expected_roots is).  Slots of skipped slivers are not written, except verdict_out. */
int rs2_recover_slivers(uint16_t n_shards, uint16_t symbol_size, int axis, uint32_t n_slivers,
                        const uint32_t* counts, const uint16_t* symbol_idx,
                        const uint8_t* const* symbols, const uint8_t* expected_roots,
                        uint8_t* const* slivers_out, uint8_t* roots_out, int32_t* verdict_out,
                        int* status_out);
/* Process-wide counters, stats_out[3]: batched recovery launches, slivers decoded inside them,
 * slivers that took the per-sliver path.  No reference counterpart. */
int rs2_recover_stats(uint64_t* stats_out);
/* Stage profiler of a verifier's recovery calls, as rs2_profile_enable / rs2_profile_read for a
 * plan: host planning of the windows (rec_plan_host), the chunk uploads and table build
 * (dec_batch_setup), the decode launches (dec_batch_codec; dec_setup / dec_codec /
 * dec_copy_present for per-sliver decodes), the roots (rec_roots) and the verdicts
 * (rec_verdict).  No reference counterpart. */
int rs2_verifier_profile_enable(rs2_verifier* v, int enable);
int rs2_verifier_profile_read(rs2_verifier* v, uint32_t max_stages, char* names,
                              double* total_ms, uint32_t* launches, uint32_t* n_stages);

/* ---- sliver verification across blobs: a symbol size per sliver -----------------------------
 * verify_sliver_against_metadata (walrus-service node.rs:2615-2633, called from put_sliver for
 * every sliver a node receives) forms SliverData::get_merkle_root (slivers.rs:151-166) of one
 * sliver and compares it with the hash in its blob's metadata.  A node holds slivers of many
 * blobs at once, so of about as many symbol sizes, on both axes: this call takes n_slivers
 * slivers that share only n_shards.  Sliver i is K*symbol_size[i] bytes at d_slivers_base +
 * sliver_off[i] (K = K_s for axis[i] == RS2_AXIS_PRIMARY, K_p for RS2_AXIS_SECONDARY, as
 * rs2_verifier_create); nothing outside these extents is read.  d_roots (may be NULL;
 * n_slivers*32 bytes, 16-byte aligned) receives, in the caller's order, the root
 * rs2_verifier_roots_device_async gives for that sliver on a verifier of its size and axis.
 * expected_roots (HOST, n_slivers*32, may be NULL): the hashes from the slivers' metadata;
 * d_verdict (n_slivers int32, 16-byte aligned, NULL exactly when expected_roots is) then gets
 * RS2_SLIVER_MATCH / RS2_SLIVER_MISMATCH / RS2_SLIVER_SKIPPED per sliver.  Nothing but d_roots
 * and d_verdict is written.  The call never waits for the device; the host arrays may be reused
 * as soon as it returns.
 * Per sliver, decided on the host before anything is enqueued: an axis that is not one of the two
 * RS2_E_INVALID_ARGUMENT; symbol_size[i] 0 or odd RS2_E_INCOMPATIBLE_PARAMETERS; an odd
 * sliver_off[i] RS2_E_INVALID_ARGUMENT; host form only: a NULL sliver or sliver_len[i] != K*s
 * RS2_E_INCORRECT_DATA_LENGTH.  status_out NULL: the first failing sliver's code is returned and
 * nothing is enqueued; non-NULL: failing slivers get their code and are skipped (root slot not
 * written, verdict RS2_SLIVER_SKIPPED), the rest run, RS2_OK.  Whole-call refusals
 * (RS2_E_INVALID_ARGUMENT): a NULL checker or needed array, a d_slivers_base that is not 2-byte
 * or a d_roots / d_verdict that is not 16-byte aligned, more than 65535 slivers, d_verdict and
 * expected_roots not NULL together.  n_slivers 0: RS2_OK, nothing enqueued.
 *
 * How it runs.  The slivers are grouped by (axis, symbol size) and taken, in the caller's order,
 * in windows: a sliver of symbol size s holds n_shards*(s + 32) bytes of scratch (its gathered
 * copy, its repair symbols, its leaves); a window closes before the sliver that would take it past
 * the budget (rs2_set_verify_mixed_budget; at least one sliver per window), or past
 * RS2_VERIFY_MIXED_WINDOW_GROUPS groups (what keeps a window's job table in one upload chunk), so
 * scratch does not grow with n_slivers.  Per window: one gather puts every group's slivers back to
 * back; one codec launch per axis present expands all its groups, a job per group found from a
 * tile prefix array; one leaf-hash launch over a group table; one tree launch; one launch writes
 * roots and verdicts in the caller's order.  That is at most RS2_VERIFY_MIXED_WINDOW_LAUNCHES
 * compute launches per window, however many slivers and sizes it holds.  A group runs there iff its
 * symbol size is >= 4, n_shards <= 4096, and its axis' encode has 1..8 transform blocks on each side
 * (both axes of n_shards = 10 .. 4096 at the default block limit); other groups (2-byte symbols,
 * wider trees) run through a per-size verifier on the same stream, inside the same windows.
 * Measured (tools/verify_mixed_probe.py, MI355X, n_shards = 1000, 128 primary slivers; DESIGN.md
 * §19): 64 symbol sizes, two slivers each: 0.65 ms against 10.3 ms for 64
 * rs2_verifier_roots_device_async calls (15.8x); uniform at s = 1206: 0.49 ms against 0.38 ms for
 * the one rs2_verifier_roots_device_async call (1.28x slower: its leaf kernels are tuned per size
 * class and its codec runs pipelined), so a batch uniform in axis and size should keep that call.
 * Stream conventions as the verifier calls; one checker per thread, or serialise its use. */
#define RS2_VERIFY_MIXED_WINDOW_LAUNCHES 6
#define RS2_VERIFY_MIXED_WINDOW_GROUPS 256
typedef struct rs2_sliver_checker rs2_sliver_checker;
int rs2_sliver_checker_create(uint16_t n_shards, rs2_sliver_checker** out);
void rs2_sliver_checker_destroy(rs2_sliver_checker* c);
int rs2_sliver_checker_verify_device_async(
    rs2_sliver_checker* c, uint32_t n_slivers, const uint8_t* axis, const uint16_t* symbol_size,
    const void* d_slivers_base, const uint64_t* sliver_off, const uint8_t* expected_roots,
    void* d_roots, void* d_verdict, int* status_out, void* stream);
/* Host form (blocking): slivers[i] is sliver i (sliver_len[i] bytes); roots_out (may be NULL)
 * n_slivers*32 bytes, verdict_out n_slivers values (NULL exactly when expected_roots is).  Root
 * slots of skipped slivers are not written. */
int rs2_verify_slivers_mixed(uint16_t n_shards, uint32_t n_slivers, const uint8_t* axis,
                             const uint16_t* symbol_size, const uint8_t* const* slivers,
                             const uint64_t* sliver_len, const uint8_t* expected_roots,
                             uint8_t* roots_out, int32_t* verdict_out, int* status_out);
/* Window scratch of the mixed calls in bytes (default 256 MiB; 0 restores it).  Process-wide. */
int rs2_set_verify_mixed_budget(uint64_t bytes);
/* Process-wide counters, stats_out[5]: windows; slivers verified inside group launches; slivers
 * that took the per-size path; groups, i.e. distinct (axis, size) pairs inside windows; compute
 * launches of the group path (gather, codec, leaf hash, trees, roots/verdicts; table uploads and
 * the per-size path's own launches are not counted).  No reference counterpart. */
int rs2_verify_mixed_stats(uint64_t* stats_out);

/* ---- sliver recovery across blobs: a symbol size and an axis per sliver ----------------------
 * rs2_verifier_recover_slivers_device_async for slivers that share only n_shards: a node that
 * missed blobs, or takes over a shard at an epoch change, recovers one sliver per blob and axis,
 * so of about as many symbol sizes as blobs.  Sliver i (axis[i], symbol_size[i]; K = K_s / K_p as
 * above) is recovered from counts[i] received symbols whose DecodingSymbol indices are
 * consecutive in symbol_idx (HOST) and whose data lie back to back at d_symbols_base +
 * symbols_off[i]; it is written whole (K*symbol_size[i] bytes) at d_slivers_base + sliver_off[i].
 * For every accepted sliver these bytes, its root at d_roots + 32 i and its verdict at
 * d_verdict + i are bit for bit what rs2_verifier_recover_slivers_device_async writes for that
 * sliver alone on a verifier of (n_shards, symbol_size[i], axis[i]).  Nothing outside the slivers'
 * extents, d_roots and d_verdict is written; the symbol buffer is not written.  OUTPUT SLIVERS
 * MUST NOT OVERLAP EACH OTHER OR THE SYMBOLS.  expected_roots / d_roots / d_verdict as the
 * verifier call's; with d_roots and expected_roots both NULL nothing is hashed.
 * Per sliver, decided on the host before anything is enqueued, in this order: an axis that is
 * not one of the two RS2_E_INVALID_ARGUMENT; symbol_size[i] 0 or odd
 * RS2_E_INCOMPATIBLE_PARAMETERS; an odd symbols_off[i] or sliver_off[i] RS2_E_INVALID_ARGUMENT;
 * counts[i] < K RS2_E_DECODING_UNSUCCESSFUL; then rs2_decode_1d's rules
 * (RS2_E_NOT_ENOUGH_SHARDS).  status_out NULL: the first failing sliver's code is returned and
 * nothing is enqueued; non-NULL: failing slivers get their code and are skipped (output and root
 * slot not written, verdict RS2_SLIVER_SKIPPED), the rest run, RS2_OK.  Whole-call refusals,
 * alignment (bases 2-byte; d_roots and d_verdict 16-byte), the 65535 cap, n_slivers 0 and the
 * stream conventions as rs2_sliver_checker_verify_device_async.  The host arrays may be reused as
 * soon as the call returns.  The call does not wait for the device, except that a window's third
 * decode launch waits for the slot of its first (a window has at most two range launches unless
 * its multiplier tables pass 256 MiB, plus one launch per sliver on the per-sliver path).
 *
 * How it runs.  The slivers are taken in the caller's order in the windows of the mixed
 * verification (same scratch rule and budget, rs2_set_verify_mixed_budget; at most
 * RS2_VERIFY_MIXED_WINDOW_GROUPS groups and a few hundred slivers).  Per window every sliver's
 * decode is planned on the host pool; the slivers whose decode fits a batch job leave in range
 * launches -- a job per sliver with its own symbol size, found from a tile prefix array, one
 * launch per block size present (at most two: one per axis) -- and the others (every original
 * received, a 2-byte symbol, more than 8 transform blocks) are decoded on their own on the same
 * stream.  Then the recovered slivers, in place, are the sources of one window of the mixed
 * verification above: gather, group codec launches, leaf hashes, trees, roots and verdicts.
 * That half counts in rs2_verify_mixed_stats exactly as a rs2_sliver_checker_verify_device_async
 * call over the accepted slivers would; rs2_recover_stats is not touched.
 * Measured (tools/recover_mixed_probe.py, MI355X, n_shards = 1000, 128 slivers, each from a random
 * K-subset of its recovery symbols): 64 symbol sizes over 4 .. 300 alternating
 * between the axes, two slivers each: 4.02 ms (3.90 - 4.16; the call returns after 1.8 ms) against
 * 18.62 ms (18.60 - 18.69) for 64 rs2_verifier_recover_slivers_device_async calls, 4.6x; uniform,
 * primary, s = 1206: 4.44 ms (4.38 - 4.51) against 4.31 ms (4.24 - 4.34) for the one verifier
 * call, 3 % slower, so a batch uniform in axis and size should keep that call. */
int rs2_sliver_checker_recover_device_async(
    rs2_sliver_checker* c, uint32_t n_slivers, const uint8_t* axis, const uint16_t* symbol_size,
    const uint32_t* counts, const uint16_t* symbol_idx, const void* d_symbols_base,
    const uint64_t* symbols_off, const uint8_t* expected_roots, void* d_slivers_base,
    const uint64_t* sliver_off, void* d_roots, void* d_verdict, int* status_out, void* stream);
/* Host form (blocking): symbols[] holds one pointer per received symbol (symbol_size[i] bytes
 * each for sliver i's), concatenated like symbol_idx; slivers_out[i] receives sliver i; roots_out
 * and verdict_out as rs2_recover_slivers.  Slots of skipped slivers are not written, except
 * verdict_out. */
int rs2_recover_slivers_mixed(uint16_t n_shards, uint32_t n_slivers, const uint8_t* axis,
                              const uint16_t* symbol_size, const uint32_t* counts,
                              const uint16_t* symbol_idx, const uint8_t* const* symbols,
                              const uint8_t* expected_roots, uint8_t* const* slivers_out,
                              uint8_t* roots_out, int32_t* verdict_out, int* status_out);
/* Process-wide counters of the mixed recovery calls, stats_out[5]: windows; decode range
 * launches; slivers decoded inside them; slivers that took the per-sliver decode path; groups,
 * i.e. distinct (axis, size) pairs inside windows.  No reference counterpart. */
int rs2_recover_mixed_stats(uint64_t* stats_out);

/* rs2_verifier_check_recovery_symbols_device_async with a symbol size and a byte offset per
 * sliver: sliver i's counts[i] received symbols of symbol_size[i] bytes lie back to back at
 * d_symbols_base + symbols_off[i] (2-byte aligned) and all authenticate leaf target_index[i] of
 * their own source sliver's tree.  Proofs, expected roots and d_ok are indexed by the symbol's
 * position j in the concatenated list, as there.  No axis is needed: a source sliver's tree has
 * n_shards leaves on either axis.  Whole-call refusals before anything is enqueued: a target
 * index >= n_shards, an odd offset or misaligned pointer RS2_E_INVALID_ARGUMENT; a symbol size of
 * 0 or odd RS2_E_INCOMPATIBLE_PARAMETERS.  Only d_ok is written. */
int rs2_sliver_checker_check_recovery_symbols_device_async(
    rs2_sliver_checker* c, uint32_t n_slivers, const uint16_t* symbol_size, const uint32_t* counts,
    const uint16_t* target_index, const void* d_symbols_base, const uint64_t* symbols_off,
    const void* d_proofs, const void* d_expected_roots, void* d_ok, void* stream);
/* Host form (blocking): symbols[] holds one pointer per received symbol; proofs and
 * expected_roots are contiguous host arrays laid out as the device form's, ok_out one byte per
 * symbol. */
int rs2_check_recovery_symbols_mixed(uint16_t n_shards, uint32_t n_slivers,
                                     const uint16_t* symbol_size, const uint32_t* counts,
                                     const uint16_t* target_index, const uint8_t* const* symbols,
                                     const uint8_t* proofs, const uint8_t* expected_roots,
                                     uint8_t* ok_out);

/* ---- recovery symbols across blobs: a symbol size, an axis and a target list per sliver --------
 * rs2_verifier_recovery_symbols_multi_device_async for source slivers that share only n_shards:
 * the serving half of a recovery.  A node that is asked for recovery symbols after an epoch
 * change holds source slivers of about as many symbol sizes as blobs, on both axes.  Source sliver
 * i (axis[i], symbol_size[i]; K = K_s / K_p as above) is K*symbol_size[i] bytes at d_slivers_base +
 * sliver_off[i], read only.  Its target_counts[i] targets (orthogonal-axis indices, any order,
 * repeats allowed, a count of 0 allowed) are consecutive in target_sliver_index; both are HOST
 * arrays.  Target t of sliver i is request j = (sum of earlier counts, refused slivers' included)
 * + t: its symbol goes to d_symbols_base + symbols_off[i] + t*symbol_size[i] -- a sliver's symbols
 * back to back, the layout rs2_sliver_checker_check_recovery_symbols_device_async reads -- and its
 * proof to d_proofs + j*path_len*32.  Sliver i's tree is at d_nodes + i*n_nodes*32 in
 * MerkleTree::nodes order (path_len, n_nodes: rs2_merkle_tree_shape(n_shards)).  trees is
 * RS2_TREES_BUILD or RS2_TREES_CACHED with the meaning given above: BUILD expands and hashes a
 * sliver with targets and builds its tree once (with d_nodes non-NULL every accepted sliver, so
 * all-zero counts warm the cache); CACHED requires d_nodes, never writes it, hashes nothing,
 * expands only slivers with a repair target (>= K) and serves an all-systematic sliver by a copy
 * out of the caller's sliver.  For every accepted sliver the symbol, proof and node bytes are bit
 * for bit what rs2_verifier_recovery_symbols_multi_device_async writes for that sliver alone with
 * the same targets on a verifier of (n_shards, symbol_size[i], axis[i]).  Nothing outside those
 * extents is written, nothing outside the slivers (CACHED: and the accepted slivers' trees) is
 * read.  Base pointers and offsets are 2-byte aligned, d_proofs and d_nodes 16-byte aligned.
 * Per sliver, decided on the host before anything is enqueued, in this order: an axis that is
 * not one of the two RS2_E_INVALID_ARGUMENT; symbol_size[i] 0 or odd
 * RS2_E_INCOMPATIBLE_PARAMETERS; an odd sliver_off[i] or symbols_off[i] RS2_E_INVALID_ARGUMENT; a
 * target >= n_shards RS2_E_INVALID_ARGUMENT (RecoverySymbolError::IndexTooLarge); host form only: a
 * NULL or wrong-length sliver RS2_E_INCORRECT_DATA_LENGTH.  status_out NULL: the first failing
 * sliver's code is returned and nothing is enqueued; non-NULL: failing slivers get their code and
 * are skipped (their symbol extent, proof slots and node slot keep their bytes), the rest run,
 * RS2_OK.  Whole-call refusals (RS2_E_INVALID_ARGUMENT): a NULL checker or needed array
 * (target_sliver_index may be NULL when every count is 0), trees not one of the two values, CACHED
 * with a NULL d_nodes, a misaligned pointer, more than 65535 slivers, more than 2^31-1 requests
 * (summed in 64 bits).  n_slivers 0: RS2_OK, nothing enqueued.  The call never waits for the
 * device and reads nothing back; the host arrays may be reused as soon as it returns.  Stream
 * conventions as rs2_sliver_checker_verify_device_async.
 *
 * How it runs.  The slivers are taken in the caller's order in the windows of the mixed
 * verification (budget: rs2_set_verify_mixed_budget; a sliver holds n*(s+32) bytes and with BUILD
 * n_nodes*32 for its tree; at most RS2_VERIFY_MIXED_WINDOW_GROUPS groups).  Per window: one table
 * upload; the slivers to expand are gathered and expanded by at most two group codec launches;
 * with BUILD their leaves are hashed in one launch and their trees built in one, slot after slot
 * into scratch, and one scatter launch moves them to the caller's order when d_nodes is given;
 * one launch per 2^20 requests gathers each request's symbol (a systematic one from the caller's
 * sliver in place) and sibling path through a per-slot record that names the sliver's own
 * addresses, symbol size and K.  So a window makes at most RS2_SYMBOLS_MIXED_WINDOW_LAUNCHES
 * compute launches however many sizes it holds.  Groups the group launch cannot take (s = 2,
 * n_shards > 4096, more than 8 transform blocks) are expanded and hashed per size on the same
 * stream; the same tree and request launches serve them.  rs2_verify_mixed_stats and
 * rs2_recovery_symbols_stats are not touched.
 * Measured (tools/symbols_mixed_probe.py, MI355X, n_shards = 1000, 128 slivers, 10 targets each,
 * half of them systematic): 64 symbol sizes over 4 .. 300 alternating between the
 * axes, two slivers each, BUILD into d_nodes: 0.792 ms (0.765 - 0.946; the call returns after
 * 0.22 ms) against 11.310 ms (11.233 - 11.348) for 64
 * rs2_verifier_recovery_symbols_multi_device_async calls, 14.3x (1 window, 128 slivers expanded,
 * 128 trees built, 1280 requests, 7 launches); CACHED: 0.641 ms (0.620 - 0.653) against 5.100 ms
 * (5.070 - 5.118), 8.0x (128 expanded, 128 trees from the cache, 4 launches).  Uniform, primary,
 * s = 1206: 0.527 ms (0.514 - 0.547) against 0.430 ms (0.409 - 0.472) for the one verifier call
 * with BUILD, 0.241 ms (0.240 - 0.242) against 0.223 ms (0.221 - 0.225) with CACHED: 22 % and 8 %
 * slower, so a batch uniform in axis and size should keep that call. */
#define RS2_SYMBOLS_MIXED_WINDOW_LAUNCHES 7
int rs2_sliver_checker_recovery_symbols_device_async(
    rs2_sliver_checker* c, uint32_t n_slivers, const uint8_t* axis, const uint16_t* symbol_size,
    const void* d_slivers_base, const uint64_t* sliver_off, const uint32_t* target_counts,
    const uint16_t* target_sliver_index, int trees, void* d_nodes, void* d_symbols_base,
    const uint64_t* symbols_off, void* d_proofs, int* status_out, void* stream);
/* Host form (blocking, RS2_TREES_BUILD, no trees handed out): slivers[i] / sliver_len[i] as
 * rs2_verify_slivers_mixed; symbols_out[i] receives sliver i's target_counts[i] symbols back to
 * back (may be NULL for a count of 0), proofs_out request j's path at j*path_len*32.  Slots of
 * skipped slivers are not written. */
int rs2_recovery_symbols_mixed(uint16_t n_shards, uint32_t n_slivers, const uint8_t* axis,
                               const uint16_t* symbol_size, const uint8_t* const* slivers,
                               const uint64_t* sliver_len, const uint32_t* target_counts,
                               const uint16_t* target_sliver_index, uint8_t* const* symbols_out,
                               uint8_t* proofs_out, int* status_out);
/* Process-wide counters of the mixed recovery-symbol calls, stats_out[6]: windows; slivers
 * expanded; trees built; trees served from the caller's cache (CACHED: accepted slivers with a
 * request); requests served; compute launches of the group path (the per-size path's own launches
 * are not counted).  No reference counterpart. */
int rs2_symbols_mixed_stats(uint64_t* stats_out);

/* RecoverySymbol::verify's proof step (symbols.rs:617-642; merkle.rs:78-99,150-169) for every
 * received symbol of a recovery call, grouped and laid out as above: sliver i's counts[i]
 * symbols all authenticate leaf target_index[i] (HOST; the target sliver's index on the
 * orthogonal axis; >= n_shards -> RS2_E_INVALID_ARGUMENT before anything is enqueued) of their
 * own source sliver's tree.  Symbol j (position in d_symbols, 2-byte aligned): its proof is
 * path_len = rs2_merkle_tree_shape(n_shards) nodes at d_proofs + j*path_len*32, its expected
 * root (the source sliver's hash, gathered by the caller) 32 bytes at d_expected_roots + j*32;
 * d_ok + j (sum of counts bytes) receives 1 if the proof's root equals it, else 0.  d_proofs,
 * d_expected_roots and d_ok are 16-byte aligned.  The length and index-bound checks of
 * verify_proof stay with the caller, as for rs2_merkle_proof_roots.  At most 65535 slivers. */
int rs2_verifier_check_recovery_symbols_device_async(
    rs2_verifier* v, uint32_t n_slivers, const uint32_t* counts, const uint16_t* target_index,
    const void* d_symbols, const void* d_proofs, const void* d_expected_roots,
    void* d_ok, void* stream);
/* Host form (blocking): symbols, proofs and expected_roots are contiguous host arrays laid out
 * as the device form's, ok_out one byte per symbol. */
int rs2_check_recovery_symbols(uint16_t n_shards, uint16_t symbol_size, int axis,
                               uint32_t n_slivers, const uint32_t* counts,
                               const uint16_t* target_index, const uint8_t* symbols,
                               const uint8_t* proofs, const uint8_t* expected_roots,
                               uint8_t* ok_out);

/* Path length (merkle.rs path_length) and node count (n_nodes) of a tree over n_leaves. */
int rs2_merkle_tree_shape(uint32_t n_leaves, uint32_t* path_len, uint64_t* n_nodes);

/* MerkleProof::compute_root (merkle.rs:150-169) for `count` proofs, on the device: leaf r is
 * leaf_len bytes (even) at leaves + r*leaf_len (leaf_hash'ed, merkle.rs:313-321), its index
 * leaf_index[r], its path path_len nodes at paths + r*path_len*32.  roots_out: count*32.  The
 * checks of MerkleAuth::verify_proof (path length, index bound, merkle.rs:78-99,150-156) are the
 * caller's (they need no data). */
int rs2_merkle_proof_roots(uint32_t count, const uint8_t* leaves, uint32_t leaf_len,
                           const uint32_t* leaf_index, const uint8_t* paths, uint32_t path_len,
                           uint8_t* roots_out);

/* ---- device 1D codec over strided lines (partitioned 2D code, batched recovery) --------------
 * A codec binds one 1D Reed-Solomon code (k source symbols -> n_shards, symbol_size bytes):
 * the device form of ReedSolomonEncoder / ReedSolomonDecoder (basic_encoding.rs:107-429)
 * applied to `lines` independent codewords per call.  Codeword `l`'s source symbol i lives at
 * d_src + l*src_line_stride + i*src_sym_stride; repair symbol j (shard index k+j) is written
 * to d_repair + l*repair_line_stride + j*repair_sym_stride.  This is what the reference runs
 * once per row / column inside BlobEncoder (blob_encoding.rs:309-354) and once per sliver in
 * SliverData::recovery_symbols (slivers.rs:100-118); the multi-GPU partitioned encode calls it
 * on a rank's row / column range.  Same stream conventions as the plan API (NULL = default
 * stream); one codec per thread, or serialise its use.  Symbol strides are >= symbol_size;
 * only the symbols themselves are read and written, never the gaps a larger symbol or line
 * stride leaves between them, so a buffer's extent ends with its last line's last symbol:
 * (lines-1)*line_stride + (symbols-1)*sym_stride + symbol_size.  d_src, d_repair and the
 * four strides are 2-byte aligned.  Supported range (encode and decode calls alike): every
 * stride and every sym_off[i] is below 2^47 bytes; a larger one is RS2_E_INVALID_ARGUMENT,
 * checked with the alignment before anything is enqueued (also when lines == 0).  Line strides
 * from (2^31 - 65536) / 64 = 33,553,408 bytes on put every 64-pair tile inside one line. */
typedef struct rs2_codec rs2_codec;
int rs2_codec_create(uint16_t k, uint16_t n_shards, uint16_t symbol_size, rs2_codec** out);
void rs2_codec_destroy(rs2_codec* codec);
int rs2_codec_encode_device_async(rs2_codec* codec, uint32_t lines, const void* d_src,
                                  uint64_t src_sym_stride, uint64_t src_line_stride,
                                  void* d_repair, uint64_t repair_sym_stride,
                                  uint64_t repair_line_stride, void* stream);

/* ReedSolomonDecoder::decode (basic_encoding.rs:387-429) for `lines` codewords sharing one
 * erasure pattern: `count` shard indices idx[] (index < k: source symbol, else repair index-k;
 * duplicates and indices >= n_shards ignored, the first k distinct used), shard idx[i] of line
 * l at d_base + sym_off[i] + l*line_stride.  All k source symbols of line l are written to
 * d_out + l*out_line_stride + i*out_sym_stride (present ones copied, missing ones decoded);
 * bytes at offsets >= out_limit (relative to d_out) are not written (the BlobDecoder's
 * truncation to the blob length, blob_encoding.rs:970-993).  Fewer than k distinct shards ->
 * RS2_E_NOT_ENOUGH_SHARDS.  Column-partitioned multi-GPU decode runs it on a rank's columns.
 * d_base, d_out, every sym_off[i] (ignored entries included), line_stride, out_sym_stride
 * and out_line_stride are 2-byte aligned; out_limit is any byte count (odd ones cut inside
 * an element). */
int rs2_codec_decode_device_async(rs2_codec* codec, uint32_t lines, uint32_t count,
                                  const uint16_t* idx, const void* d_base, const uint64_t* sym_off,
                                  uint64_t line_stride, void* d_out, uint64_t out_sym_stride,
                                  uint64_t out_line_stride, uint64_t out_limit, void* stream);

/* Segment copies: the exchange packing of the partitioned encode / decode (walrus_amd/
 * partition.py), i.e. the row -> column transposition of blob_encoding.rs:309-324 split by
 * rank.  Segment (a, b), a < count_a, b < count_b, is seg_len bytes from
 * d_src + d_src_a[a] + b*src_b_stride to d_dst + d_dst_a[a] + b*dst_b_stride; d_src_a / d_dst_a
 * are device arrays of count_a int64 byte offsets.  `unit` (1, 2, 4, 8 or 16) is the copy
 * width: seg_len, the strides and the bases must be multiples of it, else
 * RS2_E_INVALID_ARGUMENT.  Every offset in d_src_a / d_dst_a must be a multiple of it too:
 * those live in device memory and are NOT checked (an unaligned one makes misaligned wide
 * accesses -- a fault or wrong bytes); walrus_amd/partition.py passes the gcd of each table.
 * Segments must not overlap their sources. */
int rs2_copy_segments_device_async(const void* d_src, void* d_dst, uint32_t count_a,
                                   const int64_t* d_src_a, const int64_t* d_dst_a, uint32_t count_b,
                                   int64_t src_b_stride, int64_t dst_b_stride, uint32_t seg_len,
                                   uint32_t unit, void* stream);

/* leaf_hash (merkle.rs:313-321) of `count` contiguous symbols of symbol_size bytes ->
 * count*32 bytes of digests (blob_encoding.rs:161-196 hashes every expanded symbol).
 * d_symbols (count*symbol_size bytes) 2-byte aligned, d_leaves 16-byte aligned. */
int rs2_leaf_hashes_device_async(const void* d_symbols, uint64_t count, uint16_t symbol_size,
                                 void* d_leaves, void* stream);

/* MerkleTree::build_from_leaf_hashes(..).root() (merkle.rs:216-266, inner_hash :323-332) of
 * `n_trees` trees of `n_leaves` (1..65535; above 4,096 through a device scratch buffer) leaf
 * digests: leaf i of tree t at d_leaves + t*tree_stride + i*leaf_stride, root t (32 bytes)
 * written to d_roots + t*root_stride; the gaps a larger root_stride leaves are not written.
 * d_leaves, d_roots and the three strides are multiples of 16. */
int rs2_merkle_roots_device_async(const void* d_leaves, uint32_t n_trees, uint32_t n_leaves,
                                  uint64_t tree_stride, uint64_t leaf_stride, void* d_roots,
                                  uint64_t root_stride, void* stream);

/* Device form of rs2_blob_id_from_hashes (metadata.rs:571-578, lib.rs:159-176): d_hashes
 * n_shards*64 bytes, d_blob_id 32 bytes, both 16-byte aligned. */
int rs2_blob_id_device_async(const void* d_hashes, uint16_t n_shards, uint64_t blob_len,
                             void* d_blob_id, void* stream);

/* MerkleTree::build(..).root() over `n_leaves` leaves of `leaf_len` bytes each
 * (merkle.rs:216-266, leaf_hash :313-321, inner_hash :323-332).  Hashed on the device. */
int rs2_merkle_root(const uint8_t* leaves, uint32_t n_leaves, uint32_t leaf_len,
                    uint8_t root_out[32]);

/* BlobId::from_sliver_pair_metadata (lib.rs:147-157 via metadata.rs:571-578).  Hashed on the
 * device. */
int rs2_blob_id_from_hashes(const uint8_t* hashes, uint16_t n_shards, uint64_t blob_len,
                            uint8_t blob_id_out[32]);

/* QuiltEncoderV1::construct_quilt's column fill (quilt_encoding.rs:1447-1528, 1530-1646) on the
 * device: the quilt is n_rows x n_cols symbols of symbol_size bytes, row-major, and column c
 * holds bytes [0, d_col_len[c]) of the payload starting at d_payload + d_col_off[c], laid
 * down symbol by symbol from row 0 (the rest of the column is zero).  Each blob's serialized
 * bytes (header, identifier, tags, data) fill whole consecutive columns: column j of a blob
 * starting at payload offset P is d_col_off = P + j*n_rows*symbol_size.  Offsets even,
 * d_col_len[c] <= n_rows*symbol_size; d_quilt: n_rows*n_cols*symbol_size bytes, 16-byte
 * aligned.  The column
 * tables (int64 / uint32, n_cols entries) are device arrays built by the host layout plan. */
int rs2_quilt_layout_device_async(uint16_t n_rows, uint16_t n_cols, uint16_t symbol_size,
                                  const void* d_payload, const int64_t* d_col_off,
                                  const uint32_t* d_col_len, void* d_quilt, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WALRUS_RS2_H */
