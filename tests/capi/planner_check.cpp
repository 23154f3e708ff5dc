// CPU check of the codec job planner (walrus_amd/csrc/rs2_planner.h): plans encodes and decodes
// over a fixed list of shard counts with fake base pointers, asserts properties every correct
// planner has, and prints one line per plan -- its return code, scalars and an FNV-1a-64 digest
// of every array the kernels would consume.  tests/test_planner.py compares the output with
// tests/golden/planner_digests.txt.  Built from the planner sources only, with the host compiler:
// no device runtime is linked.
//
//   planner_check          the digest lines
//   planner_check --time   host time of plan_decode at n = 1000 (primary axis, 200 subsets)
#ifndef RS2_PLANNER_CHECK_SHIM  // a shim that has the planner in its own translation unit
#include "../../walrus_amd/csrc/rs2_planner.h"
#endif

#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <vector>

namespace {

using namespace rs2;

uint8_t* const kSrcBase = reinterpret_cast<uint8_t*>(0x1000);
uint8_t* const kDstBase = reinterpret_cast<uint8_t*>(0x2000);
// Factor on every line stride.  Above 1, the lines lie so far apart that lines can no longer
// share a workgroup's 32-bit offsets (the other pairs_span of finish_plan).
int64_t g_line_scale = 1;

struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void bytes(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  }
  template <class T>
  void val(T v) { bytes(&v, sizeof v); }
  template <class T>
  void vec(const std::vector<T>& v) {
    val(uint64_t(v.size()));
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
};

[[noreturn]] void breach(const char* what, const char* label) {
  std::fprintf(stderr, "planner_check: %s: %s\n", label, what);
  std::exit(1);
}
#define CHECK(cond) \
  do {              \
    if (!(cond)) breach(#cond, label); \
  } while (0)

// digest of the constant tables of one transform, computed once per (C, sd, ppw)
uint64_t stream_digest(int C, int sd, int ppw) {
  static std::map<std::tuple<int, int, int>, uint64_t> cache;
  const auto key = std::make_tuple(C, sd, ppw);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  Fnv f;
  f.vec(sd_stream(C, sd, ppw));
  f.val(int32_t(group0_zero(C, sd, ppw)));
  return cache.emplace(key, f.h).first->second;
}

// What a plan was asked for: the offsets of the symbols it must load and store.
struct Want {
  std::vector<int64_t> in;    // one in-block slot each
  std::vector<int64_t> out;   // one out-block slot each, below the block's trunc
  std::vector<int64_t> copy;  // fused copy-out offsets given (may be empty)
};

// every offset in `given` exactly once among slots [first, first + blocks) x C of pj.offs, no
// other non-negative offset there; `limit(b, p)` says whether slot p of block b may hold one
void check_slots(const PlannedJob& pj, const std::vector<int64_t>& given, int first, int blocks,
                 bool out_side, const char* label) {
  std::multiset<int64_t> left(given.begin(), given.end());
  for (int b = 0; b < blocks; ++b)
    for (int p = 0; p < pj.C; ++p) {
      const int64_t v = pj.offs[size_t(first + b) * pj.C + p];
      if (v < 0) {
        CHECK(v == -1);
        continue;
      }
      auto it = left.find(v);
      CHECK(it != left.end());  // an offset nobody gave, or one used twice
      left.erase(it);
      CHECK(p < (out_side ? pj.job.out[b].trunc : pj.job.in[b].count));
    }
  CHECK(left.empty());
}

void check_plan(const PlannedJob& pj, const Want& w, bool covered, const char* label) {
  const CodecJobBig& j = pj.job;
  CHECK(j.n_in >= 1);  // (n_out is 0 when no original is erased)
  CHECK(j.n_in <= max_blocks(pj.C) && j.n_out <= max_blocks(pj.C));
  const bool big = j.n_in > kMaxBlocks || j.n_out > kMaxBlocks;
  CHECK(pj.mix_stride == (big ? kMaxBlocksBig : kMaxBlocks));
  const size_t n_pos = size_t(j.n_in + j.n_out) * pj.C;
  CHECK(pj.offs.size() == n_pos + pj.copy_offs.size());
  check_slots(pj, w.in, 0, j.n_in, false, label);
  check_slots(pj, w.out, j.n_in, j.n_out, true, label);
  int64_t max_given = -1;
  for (const auto* v : {&w.in, &w.out, &w.copy})
    for (int64_t x : *v) max_given = std::max(max_given, x);
  for (int64_t x : pj.offs) CHECK(x >= -1 && x <= max_given);
  for (int64_t x : pj.copy_offs) CHECK(x >= -1 && x <= max_given);
  const int ppw = std::min(pj.C, pj.ppw), nw = pj.C / ppw;
  auto waves = [&](int b) { return (j.in[b].count + ppw - 1) / ppw; };
  for (int z = 0; z < kMaxBlocksBig; ++z) {
    if (j.pair_nw[z] == 0) continue;
    CHECK(z < j.n_out);
    CHECK(j.pair_nw[z] >= 1 && j.pair_q[z] == j.n_in - 1);
    CHECK(j.pair_p[z] >= 0 && j.pair_p[z] < j.pair_q[z]);
    CHECK(waves(j.pair_p[z]) + waves(j.pair_q[z]) <= nw);
  }
  if (covered) {
    CHECK(!pj.copy_offs.empty());
    for (int b = 0; b < j.n_in && !j.shared_in; ++b) {
      bool any_copy = false, loaded = false;
      for (int p = 0; p < pj.C; ++p) any_copy |= pj.copy_offs[size_t(b) * pj.C + p] >= 0;
      for (int o = 0; o < j.n_out; ++o) loaded |= j.m1_kind[o][b] != 0 || j.m2_kind[o][b] != 0;
      CHECK(!any_copy || loaded);
    }
  }
}

void print_plan(const char* label, int rc, const PlannedJob& pj, bool covered) {
  if (rc != RS2_OK) {
    std::printf("%s rc=%d\n", label, rc);
    return;
  }
  const CodecJobBig& j = pj.job;
  Fnv f;
  f.vec(pj.offs);
  f.vec(pj.copy_offs);
  f.vec(pj.pre_logs);
  f.vec(pj.post_logs);
  f.vec(pj.mix);
  f.vec(pj.in_sd);
  f.vec(pj.out_sd);
  f.vec(pj.in_first);
  for (int o = 0; o < j.n_out; ++o) {
    f.bytes(j.m1_kind[o], size_t(j.n_in));
    f.bytes(j.m2_kind[o], size_t(j.n_in));
  }
  f.bytes(j.pair_p, sizeof j.pair_p);
  f.bytes(j.pair_q, sizeof j.pair_q);
  f.bytes(j.pair_nw, sizeof j.pair_nw);
  for (int b = 0; b < j.n_in; ++b) {
    f.val(j.in[b].count);
    f.val(j.in[b].line_stride);
    f.val(uint64_t(reinterpret_cast<uintptr_t>(j.in[b].base)));
    f.val(stream_digest(pj.C, pj.in_sd[size_t(b)], pj.ppw));
  }
  for (int o = 0; o < j.n_out; ++o) {
    f.val(j.out[o].trunc);
    f.val(j.out[o].line_stride);
    f.val(j.out[o].limit);
    f.val(uint64_t(reinterpret_cast<uintptr_t>(j.out[o].base)));
    f.val(stream_digest(pj.C, pj.out_sd[size_t(o)], pj.ppw));
  }
  if (!pj.copy_offs.empty()) {
    f.val(uint64_t(reinterpret_cast<uintptr_t>(pj.copy_base)));
    f.val(pj.copy_ls);
    f.val(pj.copy_limit);
  }
  std::printf("%s rc=0 C=%d n_z=%d mode=%d ppw=%d mix_stride=%d n_in=%d n_out=%d shared_in=%d "
              "n_pairs=%d pairs_span=%d has_pre=%d has_post=%d has_mix=%d covered=%d "
              "digest=%016" PRIx64 "\n",
              label, pj.C, pj.n_z, pj.mode, pj.ppw, pj.mix_stride, j.n_in, j.n_out, j.shared_in,
              j.n_pairs, j.pairs_span, int(pj.has_pre), int(pj.has_post), int(pj.has_mix),
              int(covered), f.h);
}

struct Lcg {
  uint64_t x;
  uint32_t next(uint32_t bound) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t((x >> 33) % bound);
  }
};

// K of the n shards, by pattern
std::vector<uint32_t> pattern(int which, uint32_t n, uint32_t K, uint64_t seed) {
  std::vector<uint32_t> q;
  switch (which) {
    case 0:  // the last K shards
      for (uint32_t i = n - K; i < n; ++i) q.push_back(i);
      break;
    case 1:  // the first K, original 0 swapped for the last recovery shard
      for (uint32_t i = 1; i < K; ++i) q.push_back(i);
      q.push_back(n - 1);
      break;
    case 2:  // every other shard until K (the even ones, then the odd ones from the start)
      for (uint32_t i = 0; i < n && q.size() < K; i += 2) q.push_back(i);
      for (uint32_t i = 1; i < n && q.size() < K; i += 2) q.push_back(i);
      break;
    default: {  // a K-subset from the LCG (partial Fisher-Yates)
      std::vector<uint32_t> all(n);
      for (uint32_t i = 0; i < n; ++i) all[i] = i;
      Lcg g{seed};
      for (uint32_t i = 0; i < K; ++i) std::swap(all[i], all[i + g.next(n - i)]);
      q.assign(all.begin(), all.begin() + K);
    }
  }
  return q;
}

// The decode of one line of n symbols of s bytes at q * s, originals written 3 * s apart.
DecodeSpec decode_spec(uint32_t n, uint32_t K, int s, const std::vector<uint32_t>& have,
                       bool copy_present) {
  DecodeSpec sp;
  sp.K = K;
  sp.R = n - K;
  sp.symbol_size = s;
  sp.present.assign(n, -1);
  for (uint32_t q : have) sp.present[q] = int64_t(q) * s;
  sp.src_base = kSrcBase;
  sp.src_ls = int64_t(n) * s * g_line_scale;
  sp.dst_base = kDstBase;
  sp.dst_ls = int64_t(K) * 3 * s * g_line_scale;
  sp.dst.resize(K);
  for (uint32_t i = 0; i < K; ++i) sp.dst[i] = int64_t(i) * 3 * s;
  sp.dst_limit = int64_t(K) * 3 * s - 1;
  sp.copy_present = copy_present;
  return sp;
}

void run_case(uint32_t n, uint32_t K, int s, uint32_t bm) {
  const uint32_t R = n - K;
  const char* far = g_line_scale > 1 ? " far" : "";
  char label[128];
  {
    std::snprintf(label, sizeof label, "enc n=%u K=%u R=%u s=%d bm=%u%s", n, K, R, s, bm, far);
    PlannedJob pj;
    Want w;
    const int rc = plan_encode(
        K, R, s, kSrcBase, int64_t(K) * s * g_line_scale,
        [&](uint32_t i) { return int64_t(i) * s; }, kDstBase, int64_t(n) * s * g_line_scale, [&](uint32_t jj) { return (int64_t(K) + jj) * s; }, INT64_MAX, pj);
    bool covered = false;
    if (rc == RS2_OK) {
      for (uint32_t i = 0; i < K; ++i) w.in.push_back(int64_t(i) * s);
      for (uint32_t jj = 0; jj < R; ++jj) w.out.push_back((int64_t(K) + jj) * s);
      if (s >= 4) {  // the fused copy-out of the loaded symbols (the systematic columns')
        set_copy(pj, kDstBase, int64_t(K) * s, INT64_MAX,
                 [&](uint32_t r) { return int64_t(r) * 2 * s; });
        for (uint32_t r = 0; r < K; ++r) w.copy.push_back(int64_t(r) * 2 * s);
        covered = copy_covered(pj);
      }
      finish_plan(pj);
      check_plan(pj, w, covered, label);
    }
    print_plan(label, rc, pj, covered);
  }
  for (int pat = 0; pat < 4; ++pat)
    for (int cp = 0; cp < 2; ++cp) {
      std::snprintf(label, sizeof label, "dec n=%u K=%u R=%u s=%d bm=%u%s pat=%d copy=%d", n, K,
                    R, s, bm, far, pat, cp);
      PlannedJob pj;
      if (R == 0) {  // no recovery code: nothing to leave out
        print_plan(label, plan_decode(decode_spec(n, K, s, {}, cp != 0), pj), pj, false);
        continue;
      }
      const std::vector<uint32_t> have = pattern(pat, n, K, 0x9E3779B97F4A7C15ull ^ n);
      const DecodeSpec sp = decode_spec(n, K, s, have, cp != 0);
      const int rc = plan_decode(sp, pj);
      bool covered = false;
      if (rc == RS2_OK) {
        Want w;
        for (uint32_t q : have) w.in.push_back(sp.present[q]);
        for (uint32_t i = 0; i < K; ++i) {
          if (sp.present[i] < 0) w.out.push_back(sp.dst[i]);
          else if (cp) w.copy.push_back(sp.dst[i]);
        }
        if (cp) covered = copy_covered(pj);
        finish_plan(pj);
        check_plan(pj, w, covered, label);
      }
      print_plan(label, rc, pj, covered);
    }
}

int time_decode() {
  const uint32_t n = 1000, K = 334;
  set_block_max(uint32_t(kMaxC));
  PlannedJob pj;
  uint64_t sink = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint64_t k = 0; k < 200; ++k) {
    const DecodeSpec sp = decode_spec(n, K, 6, pattern(3, n, K, k + 1), true);
    if (plan_decode(sp, pj) != RS2_OK) return 1;
    sink += uint64_t(copy_covered(pj)) + finish_plan(pj) + pj.pre_logs.back();
  }
  const double ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::printf("plan_decode n=1000 K=334 copy_present=1: %.4f ms per plan (200 plans, sink %" PRIu64
              ")\n", ms / 200, sink);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--time") == 0) return time_decode();
  const uint32_t ns[] = {1,    2,    3,    4,    7,    10,    31,    100,  301, 1000,
                         3067, 3070, 3073, 6139, 6143, 6145,  24580, 24600, 49155};
  for (uint32_t n : ns) {
    const uint32_t f = (n - 1) / 3, kp = n - 2 * f, ks = n - f;  // rs2_source_symbols_for_n_shards
    for (uint32_t bm : {uint32_t(kMaxC), 256u}) {
      if (bm != uint32_t(kMaxC) && n != 1000) continue;
      set_block_max(bm);
      for (int axis = 0; axis < (kp == ks ? 1 : 2); ++axis)  // n <= 3: both codes are the same
        for (int s : {2, 6}) run_case(n, axis == 0 ? kp : ks, s, bm);
    }
    if (n == 1000) {  // once more with lines 2^20 times as far apart
      g_line_scale = int64_t(1) << 20;
      set_block_max(uint32_t(kMaxC));
      for (uint32_t K : {kp, ks}) run_case(n, K, 6, uint32_t(kMaxC));
      g_line_scale = 1;
    }
  }
  return 0;
}
