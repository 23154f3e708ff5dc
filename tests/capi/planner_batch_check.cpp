// CPU check of the decode-batch half of the planner (walrus_amd/csrc/rs2_planner.h:
// batch_eligible, pack_batch_job), built from the planner sources alone with the host compiler
// by tests/test_planner_batch.py.  For every case it plans a decode into a fresh PlannedJob,
// states the eligibility rule independently, and compares the packed CodecJobBatch and its
// re-strided mixing tables with the planned job.  One line per case; a breach exits non-zero.
// With a file argument (lines `k n limit s q0 q1 ...`, the k present shards of an n-shard code)
// the cases are the file's patterns instead of the built-in ones, through the same checks, and
// each line also reports how many output blocks the planner paired.  With `--chunks` it checks
// the chunk cut rule (cut_batch_chunks) on a fixed list of small windows instead.
#include "../../walrus_amd/csrc/rs2_planner.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

using namespace rs2;

uint8_t* const kSrcBase = reinterpret_cast<uint8_t*>(0x10000);
uint8_t* const kDstBase = reinterpret_cast<uint8_t*>(0x900000);

[[noreturn]] void breach(const char* what, const char* label) {
  std::fprintf(stderr, "planner_batch_check: %s: %s\n", label, what);
  std::exit(1);
}
#define CHECK(cond)                    \
  do {                                 \
    if (!(cond)) breach(#cond, label); \
  } while (0)

struct Lcg {
  uint64_t x;
  uint32_t next(uint32_t bound) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t((x >> 33) % bound);
  }
};

enum Pattern { kRandom = 0, kAllRepair = 1, kAllSystematic = 2, kOneErasure = 3 };
const char* const kPatternName[] = {"random", "all_repair", "all_systematic", "one_erasure"};

// K of the n shards
std::vector<uint32_t> pattern(int which, uint32_t n, uint32_t K, uint64_t seed) {
  std::vector<uint32_t> q;
  switch (which) {
    case kAllRepair:  // as many repair shards as there are, topped up with the last originals
      for (uint32_t i = n; i-- > 0 && q.size() < K;) q.push_back(i);
      break;
    case kAllSystematic:
      for (uint32_t i = 0; i < K; ++i) q.push_back(i);
      break;
    case kOneErasure: {  // one original (picked by the seed) replaced by one repair shard
      const uint32_t gone = uint32_t(seed % K);
      for (uint32_t i = 0; i < K; ++i)
        if (i != gone) q.push_back(i);
      q.push_back(K + uint32_t(seed % (n - K)));
      break;
    }
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

void same_scalars(const CodecScalars& a, const CodecScalars& b, const char* label) {
  CHECK(a.mix_tab == b.mix_tab && a.n_in == b.n_in && a.n_out == b.n_out);
  CHECK(a.symbol_size == b.symbol_size && a.n_pairs == b.n_pairs && a.shared_in == b.shared_in);
  CHECK(a.line_base == b.line_base && a.pre_z_stride == b.pre_z_stride);
  CHECK(a.pairs_span == b.pairs_span && a.n_lines == b.n_lines && a.stamps == b.stamps);
  CHECK(a.tiles_per_blob == b.tiles_per_blob && a.in_blob_stride == b.in_blob_stride);
  CHECK(a.out_blob_stride == b.out_blob_stride && a.copy_blob_stride == b.copy_blob_stride);
  CHECK(a.n_tiles == b.n_tiles && a.pipe_head == b.pipe_head && a.tile_ctr == b.tile_ctr);
}

void same_in(const InBlock& a, const InBlock& b, const char* label) {
  CHECK(a.base == b.base && a.pos_off == b.pos_off && a.pre_tab == b.pre_tab);
  CHECK(a.sd_tab == b.sd_tab && a.line_stride == b.line_stride && a.copy_base == b.copy_base);
  CHECK(a.copy_off == b.copy_off && a.copy_line_stride == b.copy_line_stride);
  CHECK(a.copy_limit == b.copy_limit && a.count == b.count && a.zero_first == b.zero_first);
  CHECK(a.alt_base == b.alt_base && a.alt_from == b.alt_from && a.copy2_base == b.copy2_base);
}

void same_out(const OutBlock& a, const OutBlock& b, const char* label) {
  CHECK(a.base == b.base && a.pos_off == b.pos_off && a.post_tab == b.post_tab);
  CHECK(a.sd_tab == b.sd_tab && a.line_stride == b.line_stride && a.limit == b.limit);
  CHECK(a.trunc == b.trunc && a.zero_first == b.zero_first);
}

int g_cases = 0;

// One decode of K of n shards from the shards `have` at block limit bm and symbol size s: plan,
// rule, packed job.  `paired` adds the number of output blocks with a P/Q pair to the line.
void check_pattern(const char* label, uint32_t n, uint32_t K, uint32_t bm, int s,
                   const std::vector<uint32_t>& have, bool paired) {
  set_block_max(bm);
  CHECK(have.size() == K);
  DecodeSpec sp;
  sp.K = K;
  sp.R = n - K;
  sp.symbol_size = s;
  sp.present.assign(n, -1);
  uint32_t originals = 0;
  for (uint32_t q : have) {
    sp.present[q] = int64_t(q) * 64 * s;
    originals += q < K;
  }
  sp.src_base = kSrcBase;
  sp.src_ls = s;
  sp.dst_base = kDstBase;
  sp.dst_ls = int64_t(K) * s;
  sp.dst.resize(K);
  for (uint32_t i = 0; i < K; ++i) sp.dst[i] = int64_t(i) * s;
  sp.dst_limit = int64_t(K) * 40 * s - 3;
  sp.copy_present = originals > 0 && s >= 4;
  PlannedJob pj;  // fresh: batch_eligible reads copy_base, which only plan_decode sets
  CHECK(plan_decode(sp, pj) == RS2_OK);
  const bool fused = sp.copy_present && copy_covered(pj);
  finish_plan(pj);
  const CodecJobBig& j = pj.job;
  // the rule, stated from the plan's inputs: a decode with something to reconstruct, at most
  // kBatchBlocks blocks each way, whole-dword symbols, and no copy pass of its own needed
  const bool want = pj.mode == kModeDecode && j.n_in >= 1 && j.n_out >= 1 &&
                    j.n_in <= kBatchBlocks && j.n_out <= kBatchBlocks && s >= 4 &&
                    (originals == 0 || fused);
  const bool got = batch_eligible(pj, fused);
  CHECK(got == want);
  if (got) {
    // pointer fields the engine fills at bind time: distinct fakes, so a dropped one shows
    CodecJobBig& jw = pj.job;
    jw.mix_tab = reinterpret_cast<const uint16_t*>(0x7000);
    jw.pre_z_stride = 12345;
    jw.n_lines = int(K);
    for (int b = 0; b < j.n_in; ++b) {
      jw.in[b].pos_off = reinterpret_cast<const int64_t*>(0x100000 + 8 * b);
      jw.in[b].pre_tab = reinterpret_cast<const uint16_t*>(0x200000 + 8 * b);
      jw.in[b].sd_tab = reinterpret_cast<const uint16_t*>(0x300000 + 8 * b);
      jw.in[b].copy_off = reinterpret_cast<const int64_t*>(0x400000 + 8 * b);
      jw.in[b].copy_base = kDstBase + b;
      jw.in[b].copy_limit = 1000 + b;
      jw.in[b].copy_line_stride = 2000 + b;
      jw.in[b].zero_first = b & 1;
    }
    for (int o = 0; o < j.n_out; ++o) {
      jw.out[o].pos_off = reinterpret_cast<const int64_t*>(0x500000 + 8 * o);
      jw.out[o].post_tab = reinterpret_cast<const uint16_t*>(0x600000 + 8 * o);
      jw.out[o].sd_tab = reinterpret_cast<const uint16_t*>(0x700000 + 8 * o);
      jw.out[o].zero_first = (o + 1) & 1;
    }
    CodecJobBatch bj;
    std::memset(static_cast<void*>(&bj), 0xA5, sizeof bj);
    std::vector<uint16_t> mix(7, 9);
    pack_batch_job(pj, bj, mix);
    same_scalars(bj, j, label);
    for (int b = 0; b < j.n_in; ++b) same_in(bj.in[b], j.in[b], label);
    for (int o = 0; o < j.n_out; ++o) same_out(bj.out[o], j.out[o], label);
    for (int o = 0; o < j.n_out; ++o)
      for (int b = 0; b < j.n_in; ++b) {
        CHECK(bj.m1_kind[o][b] == j.m1_kind[o][b]);
        CHECK(bj.m2_kind[o][b] == j.m2_kind[o][b]);
      }
    for (int z = 0; z < kBatchBlocks; ++z) {
      CHECK(bj.pair_p[z] == j.pair_p[z] && bj.pair_q[z] == j.pair_q[z]);
      CHECK(bj.pair_nw[z] == j.pair_nw[z]);
    }
    if (!pj.has_mix) {
      CHECK(mix.empty());
    } else {
      const size_t tab = kTabU16, ms = size_t(pj.mix_stride);
      CHECK(mix.size() == size_t(j.n_out) * kBatchBlocks * 2 * tab);
      for (int o = 0; o < j.n_out; ++o)
        for (int b = 0; b < j.n_in; ++b)
          for (int k = 0; k < 2; ++k) {
            const uint16_t* src = pj.mix.data() + ((size_t(o) * ms + b) * 2 + k) * tab;
            const uint16_t* dst = mix.data() + ((size_t(o) * kBatchBlocks + b) * 2 + k) * tab;
            CHECK(std::memcmp(src, dst, tab * 2) == 0);
          }
    }
  }
  std::printf("%s n_in=%d n_out=%d originals=%u fused=%d eligible=%d", label, j.n_in, j.n_out,
              originals, int(fused), int(got));
  if (paired) {
    int pairs = 0;
    for (int o = 0; o < j.n_out; ++o) pairs += j.pair_nw[o] != 0;
    std::printf(" paired=%d", pairs);
  }
  std::printf("\n");
  ++g_cases;
}

void run_case(uint32_t n, int axis, uint32_t bm, int pat, uint64_t seed, int s) {
  const uint32_t f = (n - 1) / 3, kp = n - 2 * f, ks = n - f, K = axis == 0 ? kp : ks;
  char label[160];
  std::snprintf(label, sizeof label, "n=%u axis=%d bm=%u s=%d pat=%s seed=%llu", n, axis, bm, s,
                kPatternName[pat], static_cast<unsigned long long>(seed));
  check_pattern(label, n, K, bm, s, pattern(pat, n, K, seed), false);
}

// A file of explicit patterns, one per line: k n limit s q0 q1 ... (the k present shards).
int run_file(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) {
    std::fprintf(stderr, "planner_batch_check: cannot open %s\n", path);
    return 2;
  }
  std::vector<char> buf(1 << 20);
  for (int line = 1; std::fgets(buf.data(), int(buf.size()), f); ++line) {
    char label[160];
    std::snprintf(label, sizeof label, "line=%d", line);
    CHECK(std::strchr(buf.data(), '\n') != nullptr);  // a whole line was read
    std::vector<unsigned long> v;
    char* at = buf.data();
    for (;;) {
      char* end = nullptr;
      const unsigned long x = std::strtoul(at, &end, 10);
      if (end == at) break;
      v.push_back(x);
      at = end;
    }
    while (*at == ' ' || *at == '\n' || *at == '\r') ++at;
    CHECK(*at == 0);  // numbers only
    if (v.empty()) continue;
    CHECK(v.size() >= 4);
    const uint32_t k = uint32_t(v[0]), n = uint32_t(v[1]), bm = uint32_t(v[2]);
    const int s = int(v[3]);
    CHECK(k >= 1 && k < n && n <= 65535 && v.size() == size_t(4) + k);
    CHECK(bm >= 1 && bm <= uint32_t(kMaxC) && (bm & (bm - 1)) == 0 && s >= 2 && s % 2 == 0);
    std::vector<uint32_t> have;
    std::vector<uint8_t> seen(n, 0);
    for (size_t i = 4; i < v.size(); ++i) {
      CHECK(v[i] < n && !seen[v[i]]);
      seen[v[i]] = 1;
      have.push_back(uint32_t(v[i]));
    }
    std::snprintf(label, sizeof label, "line=%d k=%u n=%u bm=%u s=%d", line, k, n, bm, s);
    check_pattern(label, n, k, bm, s, have, true);
  }
  std::fclose(f);
  return 0;
}

// The chunk cut rule (cut_batch_chunks) on one window: prints `label chunks=a,b|c demoted=d`
// (job indices; "-" for none) after the properties any cut satisfies.
void check_cut(const char* label, const std::vector<ChunkJob>& jobs, size_t budget) {
  ChunkCut cut;
  cut.members.assign(3, 99);  // stale contents must not survive
  cut.ends.assign(2, 99);
  cut.demoted.assign(1, 99);
  cut_batch_chunks(jobs, budget, cut);
  // every eligible job is in exactly one chunk or demoted, never both; no other job is in either
  std::vector<int> in_chunk(jobs.size(), 0), is_demoted(jobs.size(), 0);
  for (uint32_t m : cut.members) {
    CHECK(m < jobs.size());
    ++in_chunk[m];
  }
  for (uint32_t d : cut.demoted) {
    CHECK(d < jobs.size());
    ++is_demoted[d];
  }
  for (size_t i = 0; i < jobs.size(); ++i)
    CHECK(in_chunk[i] + is_demoted[i] == (jobs[i].eligible ? 1 : 0));
  // the ranges are half-open, in order, non-empty and cover the members
  CHECK(cut.ends.empty() ? cut.members.empty() : cut.ends.back() == cut.members.size());
  for (size_t i = 1; i < cut.members.size(); ++i) CHECK(cut.members[i - 1] < cut.members[i]);
  for (size_t i = 1; i < cut.demoted.size(); ++i) CHECK(cut.demoted[i - 1] < cut.demoted[i]);
  size_t at = 0;
  for (uint32_t end : cut.ends) {
    CHECK(end > at);
    // one geometry per chunk; within the budget unless the chunk is a single job
    size_t bytes = 0;
    for (size_t m = at; m < end; ++m) {
      const ChunkJob& j = jobs[cut.members[m]];
      CHECK(j.C == jobs[cut.members[at]].C && j.pairs_span == jobs[cut.members[at]].pairs_span);
      bytes += j.n_logs * kTabU16 * 2;
    }
    CHECK(end - at == 1 || bytes <= budget);
    at = end;
  }
  std::printf("%s chunks=", label);
  at = 0;
  for (size_t c = 0; c < cut.ends.size(); at = cut.ends[c++]) {
    if (c) std::printf("|");
    for (size_t m = at; m < cut.ends[c]; ++m)
      std::printf("%s%u", m > at ? "," : "", unsigned(cut.members[m]));
  }
  if (cut.ends.empty()) std::printf("-");
  std::printf(" demoted=");
  for (size_t i = 0; i < cut.demoted.size(); ++i)
    std::printf("%s%u", i ? "," : "", unsigned(cut.demoted[i]));
  if (cut.demoted.empty()) std::printf("-");
  std::printf("\n");
  ++g_cases;
}

// The smallest windows at which the cut can go wrong.  A job of 3 logs has 3 * 256 = 768 table
// bytes, so a budget of 1600 fits two of them and 2400 fits three.
void run_cuts() {
  const ChunkJob a{true, 64, 10, 3}, off{false, 64, 10, 3};
  const ChunkJob other_c{true, 128, 10, 3}, other_span{true, 64, 12, 3}, big{true, 64, 10, 7};
  check_cut("empty", {}, 1600);
  check_cut("none_eligible", {off, off}, 1600);
  check_cut("three_fit", {a, a, a}, 2400);
  check_cut("three_exact", {a, a, a}, 2304);
  check_cut("two_fit", {a, a, a}, 1600);
  check_cut("one_above_budget", {big}, 1600);
  check_cut("above_budget_between", {a, big, a}, 1600);
  check_cut("other_c_between", {a, other_c, a}, 2400);
  check_cut("other_span_between", {a, other_span, a}, 2400);
  check_cut("ineligible_first", {off, other_c, a, other_c}, 2400);
  check_cut("demoted_does_not_count", {a, other_c, a, a}, 1600);
  check_cut("geometry_of_each_chunk", {a, a, a, other_c}, 1600);
  check_cut("zero_budget", {a, a}, 0);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--chunks") == 0) {
    run_cuts();
    std::fprintf(stderr, "planner_batch_check: %d cuts\n", g_cases);
    return 0;
  }
  if (argc > 1) {
    const int rc = run_file(argv[1]);
    std::fprintf(stderr, "planner_batch_check: %d cases\n", g_cases);
    return rc;
  }
  const uint32_t ns[] = {10, 13, 100, 1000, 3100, 4500};
  for (uint32_t n : ns)
    for (int axis = 0; axis < 2; ++axis)
      for (uint32_t bm : {512u, 256u, 128u}) {
        if (bm == 128u && n != 1000) continue;
        for (uint64_t seed = 1; seed <= 6; ++seed) run_case(n, axis, bm, kRandom, seed * 977 + n, 20);
        run_case(n, axis, bm, kRandom, 5, 2);  // 2-byte symbols: never eligible
        run_case(n, axis, bm, kRandom, 6, 4);
        run_case(n, axis, bm, kAllRepair, 0, 20);
        run_case(n, axis, bm, kAllSystematic, 0, 20);
        for (uint64_t seed : {0ull, 7ull, 1234567ull}) run_case(n, axis, bm, kOneErasure, seed, 20);
      }
  std::fprintf(stderr, "planner_batch_check: %d cases\n", g_cases);
  return 0;
}
