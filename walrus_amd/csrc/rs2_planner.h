// The codec job planner: GF(2^16) constant tables and the plans of encode / decode jobs, i.e.
// every offset, table and mixing coefficient the codec kernels consume.  Pure host arithmetic:
// this unit includes no device runtime header and calls no device function, so it builds with a
// plain host compiler and is checked without a GPU (tests/capi/planner_check.cpp).
// rs2_engine.cpp uploads a planned job's arrays (bind_job) and launches it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/walrus_rs2.h"
#include "rs2_device.h"

namespace rs2 {

// ---------------------------------------------------------------------------------------------
// errors: the calling thread's last message (rs2_last_error).  The string itself stays local to
// rs2_planner.cpp: a thread_local std::string declared extern would make the library export its
// initialisation function, a name outside the prefixes the ABI allows.
// ---------------------------------------------------------------------------------------------
int fail(int code, const std::string& msg);
const char* last_error();

// Return the first failing status of a chain of engine calls.
#define RS2_TRY(expr)                   \
  do {                                  \
    int rc_ = (expr);                   \
    if (rc_ != RS2_OK) return rc_;      \
  } while (0)

// An integer A/B knob from the environment (`dflt` when unset).  Callers keep the value in a
// function-local static, so every knob is read once per process.
int env_int(const char* name, int dflt);

// ---------------------------------------------------------------------------------------------
// GF(2^16) tables (reed-solomon-simd engine/tables.rs restated; see oracle/rs2_oracle.py)
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kOrder = 65536, kModulus = 65535;

struct Gf {
  std::vector<uint16_t> exp, log, skew;
  Gf();
  static uint32_t add_mod(uint32_t a, uint32_t b) {
    const uint32_t s = a + b;
    return (s + (s >> 16)) & 0xFFFFu;
  }
  // x * exp(log_m) with the generic semantics (log_m == 65535 is log 0, i.e. times one)
  uint32_t mul(uint32_t x, uint32_t log_m) const {
    return x == 0 ? 0 : exp[add_mod(log[x], log_m)];
  }
};

const Gf& gf();

// 256-byte multiplier table of exp(log_m), one sub-table per bit field of the operand
// (rs2_device.h kTabU16): out[f] = f * m (bits 0-5, 64 entries), out[64 + f] = (f << 6) * m
// (bits 6-10), out[96 + f] = (f << 11) * m (bits 11-15).  Multiplication by a constant is
// GF(2)-linear, so x * m is the XOR of the three entries its fields select.  Each sub-table
// spans at most 32 dwords, so a wave's lookups into it never bank-conflict.
// fft_zero: a butterfly constant log_m == 65535 means multiply by ZERO (engine special case).
void nib_table(uint32_t log_m, bool fft_zero, uint16_t* out);

// Constant tables of a size-C transform with skew offset sd, in kernel consumption order
// (rs2_codec.hip: A slots PPW - PPW/d + g per wave, then B slots NW - C/d + g).
std::vector<uint16_t> sd_stream(int C, int sd, int ppw = kPpwTarget);

// 1 when group 0 of every cross-wave layer of a size-C transform with skew offset sd multiplies
// by zero (skew[d + sd - 1] is log 0, which holds for sd = 0): the kernel then skips those
// multiplies (rs2_codec.hip phase_b).
int group0_zero(int C, int sd, int ppw = kPpwTarget);

uint32_t next_pow2(uint32_t x);
// reed-solomon-simd DefaultRate: high rate iff pow2(recovery) <= pow2(original)
bool use_high_rate(uint32_t k, uint32_t r);
bool rate_supported(uint32_t k, uint32_t r);

// Largest transform block held on chip.  RS2_BLOCK_MAX (a power of two <= kMaxC) lowers it for
// experiments: smaller blocks mean smaller workgroups (C/32 waves) and more of them per CU, at
// the price of more block-level mixing.
uint32_t block_max();
void set_block_max(uint32_t max_block);  // rs2_set_block_limit: overrides RS2_BLOCK_MAX

// Blocks a job of block size C may have: jobs beyond kMaxBlocks run from device memory
// (CodecJobBig), for which only C = 512 kernels are built.
int max_blocks(int C);

// ---------------------------------------------------------------------------------------------
// codec job planning
// ---------------------------------------------------------------------------------------------
// A planned job: the CodecJob plus host copies of its per-position offset arrays.  Pointer
// fields that reference per-job device arrays are filled by bind_job (rs2_engine.cpp) once those
// are uploaded.
struct PlannedJob {
  CodecJobBig job{};                 // narrowed to CodecJob at launch when it has <= 64 blocks
  int mix_stride = kMaxBlocks;       // mixing-table row length (kMaxBlocksBig for big jobs)
  int C = 1;
  int n_z = 1;
  int mode = kModeRows;              // kernel variant (rs2_device.h CodecMode)
  int ppw = kPpwTarget;              // positions per wave of the variant's table stream
  std::vector<int64_t> offs;         // (n_in + n_out) blocks x C
  std::vector<int64_t> copy_offs;    // n_in blocks x C fused copy-out offsets, or empty
  uint8_t* copy_base = nullptr;
  int64_t copy_ls = 0, copy_limit = INT64_MAX;
  std::vector<uint16_t> pre_logs;    // per in-block C logs (decode), empty if none
  std::vector<uint16_t> post_logs;   // per out-block C logs (decode)
  std::vector<uint16_t> mix;         // mix_stride^2 * 2 tables (block mixing tables)
  std::vector<uint16_t> logs;        // pre ++ post logs as uploaded (kept alive for async H2D)
  std::vector<int> in_sd, out_sd;    // skew offset of each block's in-block transform
  std::vector<uint32_t> in_first;    // code position (source index) of each in-block's slot 0
  bool has_pre = false, has_post = false, has_mix = false;

  size_t in_off(int b) const { return size_t(b) * C; }
  size_t out_off(int o) const { return size_t(job.n_in + o) * C; }
};

// Symbolic block-level transform layers.  A "slot" is one block of C positions; its value is a
// linear combination (GF(2^16) coefficients) of the jobs' input blocks after their in-block
// IFFTs.  Layers whose butterfly distance is >= C have one constant per block pair, so on whole
// blocks they are scalar operations (same constants as the element-level transforms).
using Coef = std::vector<uint32_t>;
void coef_xor(Coef& y, const Coef& x);
// IFFT layers d = C .. span/2 of a size-`span` transform with skew offset sd
void sym_ifft_top(std::vector<Coef>& V, uint32_t C, uint32_t span, uint32_t sd);
// FFT layers d = span/2 .. C of a size-`span` transform with skew offset sd
void sym_fft_top(std::vector<Coef>& V, uint32_t C, uint32_t span, uint32_t sd);
// Mixing kinds and tables of output block oi from its coefficient vectors (M1 may be empty).
void set_mixing(PlannedJob& pj, int oi, const Coef* m1, const Coef& m2);

// Encode K source symbols into R recovery symbols for every line (reed-solomon-simd encoders,
// oracle rs_encode_elems).  src(i) / dst(j): byte offsets relative to the base (before the line
// stride).  Transforms larger than the block size C are split into blocks of C with the
// top layers applied as block mixing.
template <class SrcF, class DstF>
int plan_encode(uint32_t K, uint32_t R, int symbol_size, const uint8_t* src_base,
                int64_t src_ls, SrcF src, uint8_t* dst_base, int64_t dst_ls, DstF dst,
                int64_t dst_limit, PlannedJob& pj) {
  if (!rate_supported(K, R)) return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "unsupported shard count");
  CodecJobBig& j = pj.job;
  j = CodecJobBig{};
  pj.mix.clear();
  pj.has_mix = false;
  pj.in_sd.clear();
  pj.out_sd.clear();
  pj.in_first.clear();
  j.symbol_size = symbol_size;
  j.n_pairs = (symbol_size + 3) / 4;
  const bool high = use_high_rate(K, R);
  const uint32_t cs = high ? next_pow2(R) : next_pow2(K);
  const uint32_t C = std::min(cs, block_max());
  const uint32_t nb = cs / C;
  pj.C = int(C);
  // input blocks
  struct Blk { uint32_t first, count; int sd; };
  std::vector<Blk> in, out;
  if (high) {
    for (uint32_t k = 0; k * cs < K; ++k)
      for (uint32_t b = 0; b < nb && k * cs + b * C < K; ++b)
        in.push_back({k * cs + b * C, std::min(C, K - k * cs - b * C), int((k + 1) * cs + b * C)});
  } else {
    for (uint32_t b = 0; b < nb && b * C < K; ++b)
      in.push_back({b * C, std::min(C, K - b * C), int(b * C)});
  }
  if (in.size() > size_t(max_blocks(C))) return fail(RS2_E_UNSUPPORTED, "too many input blocks");
  j.n_in = int(in.size());
  // block mixing: coefficient vectors of each output block's pre-FFT slot
  std::vector<Coef> outs;
  const size_t ni = in.size();
  if (high) {
    std::vector<Coef> acc(nb, Coef(ni, 0));
    size_t bi = 0;
    for (uint32_t k = 0; k * cs < K; ++k) {
      std::vector<Coef> V(nb, Coef(ni, 0));
      for (uint32_t b = 0; b < nb && k * cs + b * C < K; ++b) V[b][bi++] = 1;
      sym_ifft_top(V, C, cs, (k + 1) * cs);
      for (uint32_t b = 0; b < nb; ++b) coef_xor(acc[b], V[b]);
    }
    sym_fft_top(acc, C, cs, 0);
    for (uint32_t b = 0; b < nb && b * C < R; ++b) {
      out.push_back({b * C, std::min(C, R - b * C), int(b * C)});
      outs.push_back(acc[b]);
    }
  } else {
    std::vector<Coef> V(nb, Coef(ni, 0));
    for (size_t bi = 0; bi < ni; ++bi) V[bi][bi] = 1;
    sym_ifft_top(V, C, cs, 0);
    for (uint32_t k = 0; k * cs < R; ++k) {
      std::vector<Coef> Wk = V;
      sym_fft_top(Wk, C, cs, (k + 1) * cs);
      for (uint32_t b = 0; b < nb && k * cs + b * C < R; ++b) {
        out.push_back({k * cs + b * C, std::min(C, R - k * cs - b * C), int((k + 1) * cs + b * C)});
        outs.push_back(Wk[b]);
      }
    }
  }
  if (out.size() > size_t(max_blocks(C))) return fail(RS2_E_UNSUPPORTED, "too many output blocks");
  j.n_out = int(out.size());
  pj.mix_stride = std::max(in.size(), out.size()) > size_t(kMaxBlocks) ? kMaxBlocksBig : kMaxBlocks;
  // one shared IFFT when a single input block feeds every output unmixed (low rate, C == cs)
  j.shared_in = (!high && nb == 1) ? 1 : 0;
  pj.n_z = j.shared_in ? 1 : j.n_out;
  pj.mode = j.shared_in ? kModeCols : kModeRows;
  pj.ppw = kPpwTarget;
  pj.copy_offs.clear();
  pj.offs.assign(size_t(j.n_in + j.n_out) * C, -1);
  for (int bi = 0; bi < j.n_in; ++bi) {
    InBlock& ib = j.in[bi];
    ib.base = src_base;
    ib.line_stride = src_ls;
    ib.count = int(in[bi].count);
    for (uint32_t p = 0; p < in[bi].count; ++p) pj.offs[pj.in_off(bi) + p] = src(in[bi].first + p);
    pj.in_sd.push_back(in[bi].sd);
    pj.in_first.push_back(in[bi].first);
  }
  for (int oi = 0; oi < j.n_out; ++oi) {
    OutBlock& ob = j.out[oi];
    ob.base = dst_base;
    ob.line_stride = dst_ls;
    ob.trunc = int(out[oi].count);
    ob.limit = dst_limit;
    for (uint32_t p = 0; p < out[oi].count; ++p) pj.offs[pj.out_off(oi) + p] = dst(out[oi].first + p);
    pj.out_sd.push_back(out[oi].sd);
    if (!j.shared_in) set_mixing(pj, oi, nullptr, outs[oi]);
  }
  return RS2_OK;
}

// Fused copy-out of a job's loaded source symbols: source index q (a loaded position) is
// also written to base + line*ls + f(q) (f(q) < 0: not copied).  Needs whole-dword symbol
// I/O (s >= 4); the caller keeps a separate copy pass otherwise.
template <class F>
void set_copy(PlannedJob& pj, uint8_t* base, int64_t ls, int64_t limit, F f) {
  pj.copy_base = base;
  pj.copy_ls = ls;
  pj.copy_limit = limit;
  pj.copy_offs.assign(size_t(pj.job.n_in) * pj.C, -1);
  for (int b = 0; b < pj.job.n_in; ++b)
    for (int p = 0; p < pj.job.in[b].count; ++p)
      pj.copy_offs[size_t(b) * pj.C + p] = f(pj.in_first[b] + uint32_t(p));
}

// True when every in-block that carries copy positions is loaded by at least one output
// block (the kernel skips in-blocks whose mixing coefficients are all zero); otherwise the
// copy is dropped and the caller falls back to a separate copy pass.
bool copy_covered(PlannedJob& pj);

// The last planning step, after plan_encode / plan_decode (and set_copy / copy_covered): the
// job's flattened lane space (CodecScalars::pairs_span, from its largest line stride) and the
// fused copy-out offsets appended to the position offsets, so both go up in one upload.
// Returns the number of position offsets, i.e. where the copy offsets start in pj.offs.
size_t finish_plan(PlannedJob& pj);

// Symbols of a 1D decode: present[q] = source offset (or -1) for shard index q < n;
// dst(i) = destination offset of source symbol i (only erased originals are written here).
struct DecodeSpec {
  uint32_t K = 0, R = 0;
  std::vector<int64_t> present;        // size K + R
  const uint8_t* src_base = nullptr;
  int64_t src_ls = 0;
  uint8_t* dst_base = nullptr;
  int64_t dst_ls = 0;
  std::vector<int64_t> dst;            // size K: destination offset of source symbol i
  int64_t dst_limit = INT64_MAX;
  int symbol_size = 0;
  bool copy_present = false;           // also write present originals to dst (fused copy)
};

int plan_decode(const DecodeSpec& sp, PlannedJob& pj);

// ---------------------------------------------------------------------------------------------
// decode batches (rs2_decode_batch_*): one CodecJobBatch per blob in a device job table
// ---------------------------------------------------------------------------------------------
// True when a decode planned into a fresh PlannedJob can run as one job of a batch launch: a
// decode of at most kBatchBlocks input and output blocks (and at least one of each), whole-dword
// symbol I/O (s >= 4), and either nothing to copy -- the plan was made without copy_present,
// because no original is among its inputs -- or a fused copy-out that is covered (`fused`:
// sp.copy_present && copy_covered(pj)).  The batch launch has no separate copy pass.
bool batch_eligible(const PlannedJob& pj, bool fused);

// Narrow a planned decode to the batch job, like the launch's narrowing to CodecJob: every
// CodecScalars field, the block arrays, mixing kinds and pair arrays below kBatchBlocks.  `mix`
// receives the mixing tables of output blocks o < n_out re-strided to rows of kBatchBlocks
// (table (o, b, k) at ((o * kBatchBlocks + b) * 2 + k) * kTabU16), or nothing when the plan has
// none.  The caller checked batch_eligible.
void pack_batch_job(const PlannedJob& pj, CodecJobBatch& out, std::vector<uint16_t>& mix);

// What the chunk cut rule reads of a planned job of a window, and its result: chunk c is the jobs
// members[ends[c - 1] .. ends[c]) (ends[-1] = 0), each an index into the window, in order.
struct ChunkJob {
  bool eligible;
  int C;
  int64_t pairs_span;
  size_t n_logs;  // multiplier logs: kTabU16 * 2 table bytes each
};
struct ChunkCut {
  std::vector<uint32_t> members, ends, demoted;
};
// Pack a window's eligible jobs into launches, in order.  A chunk's jobs share the C and
// pairs_span of its first job (the launch geometry): a job that differs from them is demoted to
// the per-item path and starts no chunk.  A chunk is cut before the job whose tables would take
// it past table_budget bytes, so a job larger than the budget still forms a chunk of its own.
void cut_batch_chunks(const std::vector<ChunkJob>& jobs, size_t table_budget, ChunkCut& cut);

// ---------------------------------------------------------------------------------------------
// sliver recovery (rs2_recover_slivers, rs2_verifier_recover_slivers_device_async): a sliver is
// one line of a 1D code, K = its symbols, recovered from `count` received symbols
// ---------------------------------------------------------------------------------------------
// The symbols a recovery uses, as (index, position in idx) in the caller's order.  Fewer than k
// entries: RS2_E_DECODING_UNSUCCESSFUL (slivers.rs:246-289).  Otherwise rs2_decode_1d's rules:
// entries are taken in order, duplicates and indices >= n are ignored, the first k distinct ones
// are used; fewer than k distinct: RS2_E_NOT_ENOUGH_SHARDS.
int select_recovery_symbols(uint32_t k, uint32_t n, uint32_t count, const uint16_t* idx,
                            std::vector<std::pair<uint16_t, uint32_t>>& chosen);

// The decode of one sliver from its chosen symbols: the received symbols are back to back from
// `src` (symbol at position p at p * s), the sliver's k symbols back to back from `dst`, bytes
// from k * s on never written.  copy_present: an original is among the chosen symbols, s >= 4
// and the fused copy-out is allowed (`may_fuse`), as for a blob of a decode batch.
void sliver_recover_spec(uint32_t k, uint32_t n, int symbol_size,
                         const std::vector<std::pair<uint16_t, uint32_t>>& chosen,
                         const uint8_t* src, uint8_t* dst, bool may_fuse, DecodeSpec& sp);

// ---------------------------------------------------------------------------------------------
// verified decode batches (rs2_decode_and_verify_batch_*): the rows the Default check hashes and
// the windows a call's checks run in
// ---------------------------------------------------------------------------------------------
// A systematic primary row the Default check re-expands: row index i < K_p (also its sliver-pair
// index) and how many of its K_s * s bytes lie inside the blob; the rest is the message's zero
// padding (0 valid bytes: the row is all padding).
struct VerifyRow {
  uint32_t row = 0;
  uint32_t valid = 0;
};
inline bool operator==(const VerifyRow& a, const VerifyRow& b) {
  return a.row == b.row && a.valid == b.valid;
}

// The rows of the Default check of a blob of blob_len bytes decoded from slivers of `axis`
// (config.rs:621-640), ascending: with primary slivers every row whose index is not among the
// `pulled` input indices the decoder consumed (select_slivers' prefix of the caller's list, the
// surplus item that found the workspace full included), with secondary slivers all K_p rows.
void verify_rows(uint32_t kp, uint32_t ks, uint32_t s, int axis, const uint16_t* pulled_idx,
                 uint32_t pulled, uint64_t blob_len, std::vector<VerifyRow>& rows);

// Windows of a verified batch over slots 0 .. need.size(): need[b] is the check scratch of slot b
// in bytes (0: nothing to check, or a refused blob).  Slots are taken in order; a window closes
// before the slot that would make it hold more than max_blobs slots or more than `budget` bytes,
// and always holds at least one slot.  ends[w] = one past window w's last slot.
void verify_windows(const std::vector<uint64_t>& need, uint64_t budget, size_t max_blobs,
                    std::vector<uint32_t>& ends);

// ---------------------------------------------------------------------------------------------
// recovery symbols in bulk (rs2_verifier_recovery_symbols_multi_device_async): a list of targets
// per source sliver, the slivers taken in windows of bounded scratch
// ---------------------------------------------------------------------------------------------
// Level l of a MerkleTree over n leaves starts at node level_base[l] of MerkleTree::nodes
// (merkle.rs:216-266: levels from the leaves, each but the root padded to even with the zero
// node).  Returns the path length (merkle.rs path_length; at most 16 for n <= 65535); level_base
// has kSymbolLevels entries, those from the path length on hold the root's index.  n_nodes (may be
// null) receives the node count.
int merkle_level_bases(uint32_t n, uint32_t* level_base, uint64_t* n_nodes);

// One window of a bulk recovery-symbol call: slivers first_sliver .. + n_slivers (its slots
// 0 .. n_slivers) and their requests first_request .. + n_requests of the concatenated list.
// runs: the slots whose slivers are expanded, as maximal (first slot, count) runs in order --
// BUILD: every sliver with a request, and every sliver when the trees go to the caller (warming);
// CACHED: the slivers with a repair target (>= k).  BUILD also hashes the leaves of those runs and
// builds their trees.
struct SymbolWindow {
  uint32_t first_sliver = 0, n_slivers = 0;
  uint64_t first_request = 0;
  uint32_t n_requests = 0;
  bool needs_codec = false;  // some run launches the codec (runs not empty and n > k)
  std::vector<std::pair<uint32_t, uint32_t>> runs;
};

struct SymbolRequestPlan {
  std::vector<SymbolWindow> windows;
  std::vector<uint32_t> table;       // per request: slot in its window << 16 | target
  uint32_t level_base[kSymbolLevels] = {};
  int path_len = 0;
  uint64_t n_nodes = 0;
  uint64_t total = 0;                // requests of the call
  uint64_t per_sliver = 0;           // scratch bytes a sliver of a window holds
};

// Validate and plan a bulk call over slivers of k symbols of s bytes expanded to n: the refusals
// of include/walrus_rs2.h that need no pointer (trees not one of the two modes, CACHED without
// nodes, more than 65535 slivers, more than 2^31-1 requests summed in 64 bits, a target >= n:
// RS2_E_INVALID_ARGUMENT, as are null arrays), then the windows.  A sliver's scratch is
// (n - k) * s of repair symbols, with BUILD n * 32 of leaves and, when the trees stay inside
// (have_nodes false), n_nodes * 32; a window takes budget / that many slivers, at least one and at
// most 65535 (the slot is 16 bits of a table entry), so every window but the last has the same
// count.  targets may be null when every count is zero.
int plan_symbol_requests(uint32_t n, uint32_t k, uint32_t s, uint32_t n_slivers,
                         const uint32_t* target_counts, const uint16_t* targets, int trees,
                         bool have_nodes, uint64_t budget, SymbolRequestPlan& plan);

// ---------------------------------------------------------------------------------------------
// mixed sliver verification (rs2_sliver_checker_verify_device_async): slivers that share only
// n_shards, each with its own axis and symbol size, grouped by (axis, symbol size) and taken in
// windows of bounded scratch
// ---------------------------------------------------------------------------------------------
// The 1D code a sliver of one axis expands with (a primary sliver: K_s -> n, a secondary one:
// K_p -> n), planned once: everything of plan_encode that depends on (K, R) only -- the blocks,
// their skew offsets, the mixing kinds and tables.  tmpl.offs holds symbol indices (the offsets
// of a unit symbol size), so a group's position offsets are those times its s.
struct SliverAxisCode {
  uint32_t n = 0, k = 0;
  uint32_t block_max = 0;         // block_max() the template was planned under
  bool planned = false;           // plan_encode accepted the code (n > k, rate supported)
  // the group launch can run it: at least one and at most kBatchBlocks input and output blocks,
  // and trees of at most kGroupMaxLeaves leaves
  bool batchable = false;
  PlannedJob tmpl;
  CodecJobBatch job{};            // tmpl narrowed (pack_batch_job); pointers and s-fields unset
  std::vector<uint16_t> mix;      // mixing tables in rows of kBatchBlocks, or empty
};
constexpr uint32_t kGroupMaxLeaves = 4096;  // rs2_hash.hip kMerkleMax: trees without scratch
// RS2_E_INVALID_ARGUMENT for an axis that is not one of the two or an n_shards without a code;
// a code plan_encode refuses leaves planned = false (its groups take the per-size path, which
// reports the refusal).
int plan_sliver_axis(uint32_t n_shards, int axis, SliverAxisCode& code);

// pairs_span of a job of n_pairs pairs per symbol whose largest line stride is max_ls bytes
// (finish_plan's rule)
int32_t sliver_pairs_span(int32_t n_pairs, int64_t max_ls);

// Scratch bytes a sliver of symbol size s holds in a window: its gathered copy (K * s), its
// repair symbols ((n - K) * s) and its leaves (n * 32).
inline uint64_t sliver_scratch_bytes(uint32_t n, uint32_t s) { return uint64_t(n) * (uint64_t(s) + 32); }

// ELIGIBILITY.  A group (axis, s) runs inside the window's group launches iff
//   s >= 4 (whole-dword symbol I/O, as the decode batch), and
//   its axis' code is batchable (1 .. kBatchBlocks input and output blocks at the current block
//   limit, n_shards <= kGroupMaxLeaves, n_shards > K), and
//   the codec tiles of its axis' launch stay below 2^31.
// Every other group (s = 2, n_shards above 4096, K = n_shards) goes through a per-size verifier
// on the same stream.
struct SliverGroup {
  uint32_t first_slot = 0, count = 0;  // its slots of the window
  uint32_t k = 0, s = 0;
  uint8_t axis = 0;
  bool eligible = false;
  uint32_t first_tile = 0;             // eligible: its first tile of its axis' codec launch
  int32_t pairs_span = 0;              // eligible: lanes per line of its codec job
  uint64_t gather_off = 0;             // its first sliver in the window's gathered buffer
  uint64_t repair_off = 0;             // eligible: its first repair run in the repair buffer
};

// One window: the caller's slivers first .. first + count.  Accepted slivers get slots
// 0 .. n_slots, sorted stably by group; the groups are ordered eligible primary, eligible
// secondary, then ineligible ones, each class in the order of first appearance, so the eligible
// slots are 0 .. n_eligible_slots and an axis' jobs are neighbours in the group table.
struct SliverWindow {
  uint32_t first = 0, count = 0;
  uint32_t n_slots = 0, n_eligible_slots = 0;
  std::vector<SliverGroup> groups;
  uint32_t axis_first[2] = {0, 0};     // eligible groups of an axis: groups[axis_first ..
  uint32_t axis_groups[2] = {0, 0};    //   + axis_groups)
  // per axis: first tile of each of its eligible groups, then the launch's tile count (what the
  // codec kernel searches); tiles[a][g + 1] - tiles[a][g] = ceil(count * pairs_span / 64)
  std::vector<uint32_t> tiles[2];
  std::vector<uint32_t> perm;          // slot -> caller index
  uint64_t gather_bytes = 0, repair_bytes = 0;  // of all slots / of the eligible ones
};

struct SliverGroupsPlan {
  std::vector<SliverWindow> windows;
  uint32_t accepted = 0;
};

// Validate and plan a mixed call.  Per sliver, in this order: an axis that is not one of the two
// RS2_E_INVALID_ARGUMENT; a symbol size of 0 or odd RS2_E_INCOMPATIBLE_PARAMETERS; device form
// (sliver_off given) an odd offset RS2_E_INVALID_ARGUMENT; host form (slivers and sliver_len given)
// a null sliver or sliver_len[i] != K * s RS2_E_INCORRECT_DATA_LENGTH.  status_out null: the first
// failing sliver's code is returned; else every sliver's code is stored and refused slivers get no
// slot.  Windows: slivers are taken in the caller's order; a window closes before the sliver that
// would take its scratch (sliver_scratch_bytes summed) past `budget`, or its groups past
// max_groups, and always holds at least one sliver.  More than 65535 slivers, null arrays or
// max_groups 0: RS2_E_INVALID_ARGUMENT.
int plan_sliver_groups(const SliverAxisCode (&codes)[2], uint32_t n_slivers, const uint8_t* axis,
                       const uint16_t* symbol_size, const uint64_t* sliver_off,
                       const uint8_t* const* slivers, const uint64_t* sliver_len, uint64_t budget,
                       uint32_t max_groups, int* status_out, SliverGroupsPlan& plan);

// ---------------------------------------------------------------------------------------------
// mixed sliver recovery (rs2_sliver_checker_recover_device_async): slivers that share only
// n_shards, each recovered from its own received symbols, with its own axis and symbol size
// ---------------------------------------------------------------------------------------------
// One launch of the range cut: its jobs (indices into the window, in order), their C and the tile
// prefix array rs2_decode_ranges_kernel searches -- job j of the chunk owns the tiles
// [tiles[j], tiles[j + 1]), ceil(lines * pairs_span_j / 64) of them, and tiles.back() is the
// launch's tile count.
struct RangeChunk {
  int C = 0;
  std::vector<uint32_t> members, tiles;
};
// Pack a window's eligible jobs into range launches.  The jobs are partitioned by C (the block
// size: a function of the axis' (K, n) and the block limit, so a checker's window has at most two
// classes), the classes in the order of first appearance; each class is cut, in order, before the
// job whose tables would take the chunk past table_budget bytes or whose tiles would take the
// launch past 2^31 - 1 (a job larger than the budget still forms a chunk of its own).  Nothing is
// demoted for its pairs_span.  `demoted` receives only jobs whose own tiles exceed a launch grid.
void cut_range_chunks(const std::vector<ChunkJob>& jobs, int64_t lines, size_t table_budget,
                      std::vector<RangeChunk>& chunks, std::vector<uint32_t>& demoted);

// One validated sliver of a mixed recovery call: its index in the call, its first entry of
// symbol_idx and the symbols it is recovered from (select_recovery_symbols).
struct MixedRecoverItem {
  uint32_t slot = 0;
  uint64_t first = 0;
  std::vector<std::pair<uint16_t, uint32_t>> chosen;
};

// Validate and plan a mixed recovery call.  Per sliver, in this order: an axis that is not one of
// the two RS2_E_INVALID_ARGUMENT; a symbol size of 0 or odd RS2_E_INCOMPATIBLE_PARAMETERS; an odd
// symbols_off[i] or sliver_off[i] (either may be null: the host form has none)
// RS2_E_INVALID_ARGUMENT; counts[i] < K RS2_E_DECODING_UNSUCCESSFUL; then
// select_recovery_symbols' rules (RS2_E_NOT_ENOUGH_SHARDS).  status_out as plan_sliver_groups.
// items: the accepted slivers in the caller's order.  plan: the windows of the recovered slivers'
// verification, plan_sliver_groups' rule (budget, max_groups) and also closed before the sliver
// that would take a window past max_slivers accepted slivers.  More than 65535 slivers, null
// arrays, max_groups or max_slivers 0, or a code without repair symbols: whole-call refusals.
int plan_recover_mixed(const SliverAxisCode (&codes)[2], uint32_t n_slivers, const uint8_t* axis,
                       const uint16_t* symbol_size, const uint32_t* counts,
                       const uint16_t* symbol_idx, const uint64_t* symbols_off,
                       const uint64_t* sliver_off, uint64_t budget, uint32_t max_groups,
                       uint32_t max_slivers, int* status_out, std::vector<MixedRecoverItem>& items,
                       SliverGroupsPlan& plan);

// ---------------------------------------------------------------------------------------------
// mixed recovery symbols (rs2_sliver_checker_recovery_symbols_device_async): source slivers that
// share only n_shards, each with its own axis, symbol size and list of targets
// ---------------------------------------------------------------------------------------------
// One window: the caller's slivers first .. first + count and their requests first_request ..
// + n_requests of the concatenated list (those of refused slivers included).  Accepted slivers
// get slots 0 .. n_slots: first the slivers that are expanded, laid out as a SliverWindow of
// their own (`ex`: slots sorted by group, tiles, gather and repair offsets; ex.perm holds caller
// indices), then the others in the caller's order.
//   BUILD expands every accepted sliver with a target, and every accepted sliver when the trees
//   go to the caller; CACHED the accepted slivers with a repair target (>= K).
struct SymbolsMixedWindow {
  uint32_t first = 0, count = 0;
  uint32_t n_slots = 0;
  SliverWindow ex;
  std::vector<uint32_t> perm;           // slot -> caller index
  std::vector<uint32_t> slot_request;   // slot -> its first request of the call
  std::vector<uint32_t> slot_requests;  // slot -> its requests
  uint64_t first_request = 0;
  uint32_t n_requests = 0;
  uint32_t served = 0;                  // requests of accepted slivers
  uint32_t with_requests = 0;           // accepted slivers with a request
};

struct SymbolsMixedPlan {
  std::vector<SymbolsMixedWindow> windows;
  // per request of the call: slot of its window << 16 | target, or kRequestSkipped for a request
  // of a refused sliver (no real entry equals it: a slot is at most 65534)
  std::vector<uint32_t> table;
  uint32_t level_base[kSymbolLevels] = {};
  int path_len = 0;
  uint64_t n_nodes = 0;
  uint64_t total = 0;           // requests of the call, refused slivers' included
  uint32_t accepted = 0;
};

// Validate and plan a mixed recovery-symbol call.  Whole-call refusals (RS2_E_INVALID_ARGUMENT):
// trees not one of the two modes, CACHED without nodes, more than 65535 slivers, null arrays
// (targets may be null when every count is zero), more than 2^31-1 requests summed in 64 bits --
// all before a target is read.  Per sliver, in this order: an axis that is not one of the two
// RS2_E_INVALID_ARGUMENT; a symbol size of 0 or odd RS2_E_INCOMPATIBLE_PARAMETERS; an odd
// sliver_off[i] or symbols_off[i] (either array may be null: the host form has none)
// RS2_E_INVALID_ARGUMENT; a target >= n_shards RS2_E_INVALID_ARGUMENT; host form (slivers and
// sliver_len given) a null sliver or sliver_len[i] != K * s RS2_E_INCORRECT_DATA_LENGTH.
// status_out as plan_sliver_groups.  Windows: plan_sliver_groups' rule over the accepted slivers
// (budget, max_groups), a sliver's scratch being sliver_scratch_bytes plus, with BUILD,
// n_nodes * 32 for its slot-ordered tree.
int plan_symbols_mixed(const SliverAxisCode (&codes)[2], uint32_t n_slivers, const uint8_t* axis,
                       const uint16_t* symbol_size, const uint64_t* sliver_off,
                       const uint64_t* symbols_off, const uint8_t* const* slivers,
                       const uint64_t* sliver_len, const uint32_t* target_counts,
                       const uint16_t* targets, int trees, bool have_nodes, uint64_t budget,
                       uint32_t max_groups, int* status_out, SymbolsMixedPlan& plan);

// ---------------------------------------------------------------------------------------------
// mixed blob encode (rs2_blob_encoder_*): blobs that share only n_shards, each with its own length
// and therefore its own symbol size, taken in windows of bounded scratch
// ---------------------------------------------------------------------------------------------
// The three 1D stages of a blob's encode, in launch order.  Each uses one of the two codes
// plan_sliver_axis plans per n_shards:
//   cols_sys  K_s lines (columns c < K_s), K_p -> n - K_p: primary rows r < K_p of column c to the
//             primary repair rows; its fused copy-out writes the systematic secondary slivers
//   rows      K_p lines (rows r < K_p), K_s -> n - K_s: primary sliver r to the secondary repair
//             slivers' row r
//   cols_rep  n - K_s lines (columns c >= K_s), K_p -> n - K_p: secondary repair sliver c to column
//             c - K_s of the repair-repair quadrant
enum BlobStageId : int { kStageColsSys = 0, kStageRows = 1, kStageColsRep = 2, kBlobStages = 3 };

// One stage planned once per encoder with unit symbol offsets: tmpl.offs (position offsets, then
// the fused copy-out offsets from n_off on), the line strides and the extents are in symbols, so
// a blob's job is the template with everything times its symbol size.
struct BlobStageCode {
  PlannedJob tmpl;
  CodecJobBatch job{};            // tmpl narrowed (pack_batch_job); pointers and s-fields unset
  std::vector<uint16_t> mix;      // mixing tables in rows of kBatchBlocks, or empty
  size_t n_off = 0;               // position offsets of tmpl.offs; copy offsets follow (cols_sys)
  uint32_t n_lines = 0;
  int64_t in_ls = 0, out_ls = 0, copy_ls = 0;   // line strides in symbols
  int64_t max_ls = 0;                           // the largest of them (pairs_span's rule)
  // where the stage stores: symbols of the output buffer / of the copy-out buffer it may touch
  int64_t out_extent = 0, copy_extent = 0;
};

struct BlobStages {
  uint32_t n = 0, kp = 0, ks = 0;
  uint32_t block_max = 0;         // block_max() the templates were planned under
  bool planned = false;           // plan_encode accepted all three stages
  // the group launches can run them: 1 .. kBatchBlocks blocks per side in every stage and
  // n_shards <= kGroupMaxLeaves
  bool batchable = false;
  // cols_sys writes the systematic secondary slivers from its own loads (a shared-input code);
  // else the staging launch writes them (a mixing code has no copy-out: n_shards = 13, or above
  // 1534 at the default block limit) and cols_sys has no copy offsets
  bool sys_fused = false;
  BlobStageCode stage[kBlobStages];
};
// RS2_E_INVALID_ARGUMENT for n_shards 0; a code plan_encode refuses (n_shards too small for a
// recovery code, an unsupported rate) leaves planned = false, and every blob takes the per-blob
// path, which reports the refusal.
int plan_blob_stages(uint32_t n_shards, BlobStages& st);

// Scratch bytes a blob of symbol size s holds in a window: its repair-repair quadrant
// ((n - K_p)(n - K_s) s) and its leaves (32 n^2); a metadata-only call keeps the slivers there too
// (n (K_p + K_s) s).  The zero-padded message is staged in the primary slivers' own systematic
// rows, so staging takes nothing more.
inline uint64_t blob_scratch_bytes(uint32_t n, uint32_t kp, uint32_t ks, uint32_t s, bool meta_only) {
  const uint64_t n64 = n;
  return (n64 - kp) * (n64 - ks) * s + 32 * n64 * n64 + (meta_only ? n64 * (uint64_t(kp) + ks) * s : 0);
}

// One accepted blob of a window.
struct BlobSlot {
  uint32_t blob = 0;              // caller index
  uint32_t s = 0;
  bool eligible = false;
  uint32_t size_class = 0;        // eligible: index into BlobWindow::sizes
  int32_t pairs_span[kBlobStages] = {0, 0, 0};
  uint64_t both_off = 0;          // eligible: its quadrant in the window's quadrant scratch
  uint64_t primary_off = 0, secondary_off = 0;  // metadata-only: its slivers in the window scratch
};

// One window: the caller's blobs first .. first + count.  Accepted blobs get slots in the caller's
// order, the eligible ones first (slots 0 .. n_eligible), then the ineligible ones.
//   ELIGIBILITY.  A blob runs inside the window's group launches iff s >= 4, the stages are
//   batchable, and every stage launch's tiles stay below 2^31.  Every other blob (s = 2, n_shards
//   above 4096) goes through the single-blob encode on the same stream.
struct BlobWindow {
  uint32_t first = 0, count = 0;
  uint32_t n_eligible = 0;
  std::vector<BlobSlot> slots;
  std::vector<uint32_t> sizes;    // distinct symbol sizes of the eligible slots, by appearance
  // per stage: first tile of each eligible slot, then the launch's tile count;
  // tiles[g][q + 1] - tiles[g][q] = ceil(n_lines * pairs_span / 64)
  std::vector<uint32_t> tiles[kBlobStages];
  uint64_t both_bytes = 0, primary_bytes = 0, secondary_bytes = 0;  // window scratch (the last
                                                                    // two: metadata-only)
};

struct BlobsMixedPlan {
  std::vector<BlobWindow> windows;
  uint32_t accepted = 0;
};

// Validate and plan a mixed encode.  Per blob, in this order: the codes rs2_plan_create gives for
// its length (RS2_E_DATA_TOO_LARGE; RS2_E_INCOMPATIBLE_PARAMETERS for an n_shards without a
// recovery code); device form (blob_off given) an odd blob_off[b], primary_off[b] or
// secondary_off[b] (the latter two may be null: metadata only) RS2_E_INVALID_ARGUMENT; host form
// (blobs given) a null blob of non-zero length RS2_E_INVALID_ARGUMENT.  status_out as
// plan_sliver_groups.  Windows: blobs are taken in the caller's order; a window closes before the
// blob that would take its scratch (blob_scratch_bytes summed) past `budget`, or its eligible
// blobs past max_blobs (what a window's tables hold), and always holds at least one blob.  More
// than 65535 blobs, null arrays or max_blobs 0: RS2_E_INVALID_ARGUMENT.
int plan_blobs_mixed(const BlobStages& st, uint32_t n_blobs, const uint64_t* blob_lens,
                     const uint64_t* blob_off, const uint64_t* primary_off,
                     const uint64_t* secondary_off, const uint8_t* const* blobs, bool meta_only,
                     uint64_t budget, uint32_t max_blobs, int* status_out, BlobsMixedPlan& plan);

}  // namespace rs2
