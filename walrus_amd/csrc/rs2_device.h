// Device-side job descriptors shared by the HIP kernels (rs2_codec.hip, rs2_hash.hip,
// rs2_copy.hip) and the host planner (rs2_planner.cpp).  Plain structs, no HIP types, so both
// sides agree on layout.
#pragma once
#include <stdint.h>

namespace rs2 {

constexpr int kMaxBlocks = 64;  // input / output blocks of a job passed by value (W <= 32768)
// Jobs with more blocks (n_shards above about 24,580: W = 65536 = 128 blocks of 512) live in
// device memory and reach the kernel by pointer (CodecJobBig, C = 512 only); their block arrays
// and mixing kinds would not fit the kernel argument.
constexpr int kMaxBlocksBig = 128;
// Jobs of a decode batch (one job per blob, a table of them in device memory, CodecJobBatch):
// 8 blocks cover every decode up to n_shards of about 3100 at C = 512 and n_shards = 1000 at a
// block limit of 256, and keep a job near 1.5 KiB, so a few hundred fit one upload slot.
constexpr int kBatchBlocks = 8;
constexpr int kMaxC = 512;      // largest transform block held on chip (positions)
constexpr int kTabU16 = 128;    // one multiplier table: u16 sub-tables of 64 + 32 + 32 entries
                                // for operand bits 0-5, 6-10, 11-15 (rs2_planner.cpp nib_table)
// Codeword positions one wave holds in VGPRs; a size-C transform uses C / PPW waves.  The
// kernel's table consumption order and the host's sd_stream order both derive from it.
constexpr int kPpwTarget = 32;

// One input block of a codec job: up to C codeword positions, loaded from symbols in HBM,
// optionally pre-multiplied per position, then inverse-transformed (IFFT) with skew offset
// `sd` (the tables in `sd_tab` are that transform's constants in consumption order).
struct InBlock {
  const uint8_t* base;       // symbol (pos, line) lives at base + pos_off[pos] + line*line_stride
  const int64_t* pos_off;    // [C]; -1 = position absent (zero)
  const uint16_t* pre_tab;   // [C][64] per-position multiplier tables, or null
  const uint16_t* sd_tab;    // [C-1][64] IFFT constant tables
  int64_t line_stride;
  // fused copy-out of the loaded symbols (systematic secondary slivers on encode, present
  // originals on decode): symbol (pos, line) -> copy_base + copy_off[pos] + line*copy_stride,
  // bytes at offset >= copy_limit not written.  copy_off null = no copy.
  uint8_t* copy_base;
  const int64_t* copy_off;   // [C]; -1 = not copied
  int64_t copy_line_stride;
  int64_t copy_limit;
  int32_t count;             // positions >= count are zero
  int32_t zero_first;        // 1: group 0 of every cross-wave layer multiplies by zero (sd = 0)
  // split input: positions >= alt_from read from alt_base instead of base (same offsets); the
  // encode reads the blob's whole rows in place and its zero-padded last row from a small
  // buffer.  alt_base null = unused.
  const uint8_t* alt_base;
  int32_t alt_from;
  // second fused copy-out at the input's own layout: symbol (pos, line) is also written to
  // copy2_base + pos_off[pos] + line*line_stride (the encode's systematic primary slivers, so
  // no separate blob copy).  Null = none.
  uint8_t* copy2_base;
};

// codec kernel variants (one __global__ each, so profiles attribute time per stage)
// kModeColsPipe / kModeRowsPipe: the shared-input / mixing encode as a persistent,
// tile-pipelined kernel (launch_codec_c picks them when the last output block's active waves fit
// below the head input block's); kModeDecodePersist: the decode with one persistent workgroup
// per CU walking an XCD-interleaved tile range (CodecJob::n_tiles tiles)
enum CodecMode : int {
  kModeRows = 0, kModeCols = 1, kModeDecode = 2, kModeColsPipe = 3, kModeRowsPipe = 4,
  kModeDecodePersist = 5
};

// One output block: FFT with skew offset `sd`, optional per-position post-multiply,
// store of positions < trunc whose pos_off >= 0; bytes at offset >= limit are not stored.
struct OutBlock {
  uint8_t* base;
  const int64_t* pos_off;
  const uint16_t* post_tab;
  const uint16_t* sd_tab;
  int64_t line_stride;
  int64_t limit;
  int32_t trunc;
  int32_t zero_first;        // as InBlock::zero_first
};

// The scalar fields of a codec job (CodecJobT below derives from it, so they are read as
// job.n_in etc.).  Kept in a base of their own so that narrowing a planned CodecJobBig to the
// by-value CodecJob (rs2_engine.cpp narrow_job) copies them all at once: a field added here can
// not be left at its default in the kernel argument.
struct CodecScalars {
  const uint16_t* mix_tab;
  int32_t n_in;
  int32_t n_out;
  int32_t symbol_size;
  int32_t n_pairs;           // element pairs per symbol = ceil(symbol_size / 4)
  int32_t shared_in;         // 1: single input, every output = FFT_o(X_0) (low-rate encode)
  int32_t line_base;         // line of blockIdx.y == 0 (launches are split at 65535 lines)
  // decode: the pre-multiplier tables of output block z start at in[b].pre_tab + z * pre_z_stride
  // (u16 elements), because each output folds its own mixing coefficient into them
  int64_t pre_z_stride;
  // lanes walk a flattened (line, pair) space: pairs_span (even, >= n_pairs) pairs per line,
  // n_lines lines from line_base (set per launch)
  int32_t pairs_span;
  int32_t n_lines;
  // diagnostics (RS2_STAMP_FILE): wave 0 of every workgroup records s_memtime at its phase
  // boundaries into stamps[blockIdx.x * kStamps + k]; null = off
  uint64_t* stamps;
  // blob batches (rs2_encode_batch_*): tile t (after the XCD order) belongs to blob
  // t / tiles_per_blob, whose symbols lie in_blob_stride / out_blob_stride / copy_blob_stride
  // bytes past blob 0's for every input / output / copy base; tiles_per_blob 0 = one blob
  int32_t tiles_per_blob;
  int64_t in_blob_stride, out_blob_stride, copy_blob_stride;
  // pipelined kernels: tiles of the whole launch (gridDim.x workgroups each walk a contiguous
  // range); kModeRowsPipe: the input block loaded beside the previous tile's tail
  int32_t n_tiles;
  int32_t pipe_head;
  // pipelined kernels, dynamic tile order (null = static XCD-interleaved ranges): kTileCtrWords
  // zeroed words of device memory; word x < 8 counts the tiles taken from XCD x's contiguous
  // range, word 8 the workgroups that have finished (the last one zeroes them all again, so the
  // next launch on the same words starts from zero).  A workgroup takes its XCD's next tile,
  // then the other XCDs' leftovers, so a workgroup that got its CU late (another kernel held
  // it) takes fewer tiles instead of finishing its fixed range late.
  uint32_t* tile_ctr;
};

// out_o = FFT_o( sum_b  M1[o][b] * Dw(X_b)  +  M2[o][b] * X_b ),  X_b = IFFT_b(in_b)
// where Dw is the in-block formal derivative.  Coefficient kinds: 0 zero, 1 one, 2 table
// (mix_tab + ((o*MB + b)*2 + {0:M1, 1:M2}) * 64).  MB = kMaxBlocks (CodecJob, the kernel
// argument) or kMaxBlocksBig (CodecJobBig, by pointer); the host plans in CodecJobBig and
// narrows jobs of <= kMaxBlocks blocks to CodecJob at launch.  Every per-block array is listed
// in kArrayBytes, so a new array field that narrow_job does not copy breaks the build.
template <int MB>
struct CodecJobT : CodecScalars {
  static constexpr int kBlocks = MB;
  InBlock in[MB];
  OutBlock out[MB];
  uint8_t m1_kind[MB][MB];
  uint8_t m2_kind[MB][MB];
  // decode, output block z: two input blocks whose active waves fit one workgroup together are
  // loaded and run their in-wave IFFT layers side by side (rs2_codec.hip load_ifft): block
  // pair_p[z] on waves [0, pair_nw[z]), block pair_q[z] (no formal derivative) on the rest.
  // pair_q is always the last input block; pair_nw 0 = no pair.
  int8_t pair_p[MB], pair_q[MB], pair_nw[MB];
  static constexpr size_t kArrayBytes =
      MB * (sizeof(InBlock) + sizeof(OutBlock)) + 2 * MB * MB + 3 * MB;
};
using CodecJob = CodecJobT<kMaxBlocks>;
using CodecJobBig = CodecJobT<kMaxBlocksBig>;
// One blob's job in a decode batch's device job table (rs2_decode_batch_kernel): every pointer,
// the absolute bases of that blob's buffers included, is its own; tiles_per_blob is 0.
using CodecJobBatch = CodecJobT<kBatchBlocks>;
static_assert(sizeof(CodecJob) ==
                  (sizeof(CodecScalars) + CodecJob::kArrayBytes + 7) / 8 * 8 &&
              sizeof(CodecJobBig) ==
                  (sizeof(CodecScalars) + CodecJobBig::kArrayBytes + 7) / 8 * 8 &&
              sizeof(CodecJobBatch) ==
                  (sizeof(CodecScalars) + CodecJobBatch::kArrayBytes + 7) / 8 * 8,
              "a CodecJobT field outside CodecScalars and kArrayBytes: narrow_job would drop it");
constexpr int kTileCtrWords = 16;
constexpr int kStamps = 64;
// CodecJob travels by value as the codec kernels' argument.  tools/micro/kernarg20.hip probed a
// 20 KiB by-value argument on the box (gfx950, ROCm 7.2); keep the job (plus the few hidden
// arguments) below that instead of relying on an untested larger limit.
static_assert(sizeof(CodecJob) <= 19 * 1024 + 512, "CodecJob outgrows the probed kernel-argument size");

// Where the n x n expanded-matrix symbol (r, c) lives after an encode (leaf hashing).
struct SymbolMap {
  const uint8_t* primary;    // [n][K_s][s]  rows, columns < K_s
  const uint8_t* secondary;  // [n][K_p][s]  columns >= K_s hold rows < K_p
  const uint8_t* both;       // [n-K_p][n-K_s][s]  rows >= K_p, columns >= K_s
  int32_t n, kp, ks, s;
  // blob batches: blob y (grid.y) at these byte offsets from blob 0 (leaves: out + y*leaf_stride)
  int64_t primary_stride, secondary_stride, both_stride, leaf_stride;
};

// A verified decode batch's check tables (rs2_decode_and_verify_batch_*), one window at a time.
// A row the Default check hashes: where it starts in its decoded blob, how many of its bytes lie
// inside the blob (the rest is hashed as zeros, never read) and its sliver-pair index.
struct CheckRow {
  const uint8_t* src;
  uint32_t valid;
  uint32_t pair;
};
// A slot of the window: its rows in the window's row table (Default; none: nothing to check),
// or kCheckSkipped in `rows` for a blob that was refused on the host.
struct CheckSlot {
  uint32_t first;
  uint32_t rows;
};
constexpr uint32_t kCheckSkipped = 0xFFFFFFFFu;
static_assert(sizeof(CheckRow) == 16 && sizeof(CheckSlot) == 8, "check tables are packed");

// Mixed sliver verification (rs2_sliver_checker_*): one window's device tables.
// A slot of the window (an accepted sliver, slots sorted by group): its bytes in the caller's
// memory, where its copy goes in the window's gathered buffer (groups back to back, a group's
// slivers back to back) and its first 4 KiB chunk of the gather launch (sliver_gather_kernel
// searches these; the entry after the last slot holds the launch's chunk count).
struct SliverSlot {
  const uint8_t* src;
  uint64_t dst_off;
  uint32_t len;     // K * s, even
  uint32_t chunk0;
};
// A group of the leaf launch (leaf_hash_groups_kernel): `count` slivers of k symbols of s bytes
// from slot `first_slot` on, their systematic symbols back to back at sys, their n - k repair
// symbols back to back at rep.  The table is searched by first_slot; the entry after the last
// group holds the launch's slot count.
struct SliverLeafGroup {
  const uint8_t* sys;
  const uint8_t* rep;
  uint32_t first_slot, count, k, s;
};
static_assert(sizeof(SliverSlot) == 24 && sizeof(SliverLeafGroup) == 32, "sliver tables are packed");
// The received symbols of one sliver of a mixed proof check (leaf_hash_runs_kernel): `count`
// symbols of s bytes back to back at sym; symbol w's digest goes to digest first + w of the call.
struct SymbolRun {
  const uint8_t* sym;
  uint32_t first, count, s, pad;
};
static_assert(sizeof(SymbolRun) == 24, "symbol runs are packed");
// caller index -> slot table entry of a sliver refused on the host (sliver_finish_kernel)
constexpr uint32_t kSliverSkipped = 0xFFFFFFFFu;

// Mixed blob encode (rs2_blob_encoder_*): one window's device tables.
// An eligible blob of the leaf launch (leaf_hash_blobs_kernel): where its n x n expanded symbols
// lie (the three runs of SymbolMap: primary [n][K_s][s], secondary [n][K_p][s], both
// [n-K_p][n-K_s][s]), where its 32 n^2 bytes of leaves go, its symbol size and its first tile of
// the launch.  The table is searched by first_tile; the entry after the last blob holds the
// launch's tile count.
struct BlobLeaves {
  const uint8_t* primary;
  const uint8_t* secondary;
  const uint8_t* both;
  uint8_t* leaves;
  uint32_t s;
  uint32_t first_tile;
};
// A blob of the staging launch (blob_stage_kernel): `len` bytes at src go to dst, followed by
// zeros up to `msg` bytes (the zero-padded message K_p K_s s: the systematic primary slivers);
// chunk0 is its first 4 KiB chunk of the launch, and the entry after the last blob holds the
// launch's chunk count.  sec: where the systematic secondary slivers go as well (secondary c, row
// r = primary r, column c; s: the blob's symbol size), or null when the systematic-column codec
// writes them from its own loads.
struct BlobStage {
  const uint8_t* src;
  uint8_t* dst;
  uint8_t* sec;
  uint64_t len;
  uint64_t msg;
  uint32_t chunk0;
  uint32_t s;
};
static_assert(sizeof(BlobLeaves) == 40 && sizeof(BlobStage) == 48, "blob tables are packed");

// Bulk recovery symbols (symbol_requests_kernel): where each level of a sliver's MerkleTree::nodes
// array starts, in nodes -- a path has at most kSymbolLevels siblings for n <= 65535 leaves.  By
// value in the launch arguments (wave-uniform, read once per wave).
constexpr int kSymbolLevels = 16;
struct SymbolLevels {
  uint32_t base[kSymbolLevels];
};

// Mixed recovery symbols (symbol_requests_slots_kernel): a slot of the window, i.e. a source sliver
// with its own symbol size and axis.  sys: its K systematic symbols (the caller's sliver, in
// place); rep: its n - K repair symbols (null when the sliver was not expanded: no request of it
// asks for one); nodes: its tree in MerkleTree::nodes order (the window's scratch, or the caller's
// cached slot); sym: where its first request's symbol goes, the others behind it back to back;
// first_request: that request's index in the call.  Read wave-uniformly, once per request.
struct SymbolSlot {
  const uint8_t* sys;
  const uint8_t* rep;
  const uint8_t* nodes;
  uint8_t* sym;
  uint32_t first_request;
  uint16_t s, k;
};
static_assert(sizeof(SymbolSlot) == 40, "symbol slots are packed");
// request table entry of a sliver refused on the host: the wave that draws it leaves
constexpr uint32_t kRequestSkipped = 0xFFFFFFFFu;

}  // namespace rs2
