// CPU check of the sliver-recovery half of the planner (walrus_amd/csrc/rs2_planner.h:
// select_recovery_symbols, sliver_recover_spec), built from the planner sources alone with the
// host compiler by tests/test_planner_recover.py.  For every case it builds a received-symbol
// list, restates the selection rule directly, compares status and chosen list, checks every field
// of the DecodeSpec, plans it and reports whether the plan can be a job of a batch launch.  One
// line per case; a breach exits non-zero.
#include "../../walrus_amd/csrc/rs2_planner.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

using namespace rs2;

uint8_t* const kSrcBase = reinterpret_cast<uint8_t*>(0x10000);
uint8_t* const kDstBase = reinterpret_cast<uint8_t*>(0x9000000);

[[noreturn]] void breach(const char* what, const char* label) {
  std::fprintf(stderr, "planner_recover_check: %s: %s\n", label, what);
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

enum Pattern {
  kRandom = 0, kAllRepair, kAllOriginal, kOneErasure, kNoisy, kOneShort, kDuplicate
};
const char* const kPatternName[] = {"random",  "all_repair", "all_original", "one_erasure",
                                    "noisy",   "one_short",  "duplicate"};

// a K-subset of 1..n-1 (original 0 is always left out), in LCG order
std::vector<uint16_t> random_subset(uint32_t n, uint32_t K, uint64_t seed) {
  std::vector<uint16_t> all;
  for (uint32_t i = 1; i < n; ++i) all.push_back(uint16_t(i));
  Lcg g{seed};
  for (uint32_t i = 0; i < K; ++i) std::swap(all[i], all[i + g.next(uint32_t(all.size()) - i)]);
  all.resize(K);
  return all;
}

// the received-symbol index list of a case
std::vector<uint16_t> pattern(int which, uint32_t n, uint32_t K, uint64_t seed) {
  std::vector<uint16_t> q;
  switch (which) {
    case kAllRepair:  // as many repair symbols as there are, topped up with the last originals
      for (uint32_t i = n; i-- > 0 && q.size() < K;) q.push_back(uint16_t(i));
      break;
    case kAllOriginal:
      for (uint32_t i = 0; i < K; ++i) q.push_back(uint16_t(i));
      break;
    case kOneErasure: {
      const uint32_t gone = uint32_t(seed % K);
      for (uint32_t i = 0; i < K; ++i)
        if (i != gone) q.push_back(uint16_t(i));
      q.push_back(uint16_t(K + seed % (n - K)));
      break;
    }
    case kNoisy: {  // duplicates, indices >= n and a surplus tail around a random subset
      const std::vector<uint16_t> base = random_subset(n, K, seed);
      for (size_t i = 0; i < base.size(); ++i) {
        q.push_back(base[i]);
        if (i % 3 == 0) q.push_back(base[i / 2]);           // a duplicate of an earlier entry
        if (i % 5 == 0) q.push_back(uint16_t(n + i % 7));   // out of range
      }
      q.push_back(0);  // surplus: never reached
      q.push_back(uint16_t(n - 1));
      break;
    }
    case kOneShort: {
      q = random_subset(n, K, seed);
      q.pop_back();
      break;
    }
    case kDuplicate: {  // K entries, K - 1 distinct
      q = random_subset(n, K, seed);
      q.back() = q.front();
      break;
    }
    default:
      q = random_subset(n, K, seed);
  }
  return q;
}

int g_cases = 0;

void run_case(uint32_t n, int axis, int pat, uint64_t seed, int s) {
  // axis 0: a primary sliver (K_s symbols), axis 1: a secondary one (K_p symbols)
  const uint32_t f = (n - 1) / 3, kp = n - 2 * f, ks = n - f, K = axis == 0 ? ks : kp;
  char label[160];
  std::snprintf(label, sizeof label, "n=%u axis=%d s=%d pat=%s seed=%llu", n, axis, s,
                kPatternName[pat], static_cast<unsigned long long>(seed));
  set_block_max(512);
  const std::vector<uint16_t> idx = pattern(pat, n, K, seed);
  // the rule, restated: too short a list fails outright; else first K distinct in-range entries
  int want_rc = RS2_OK;
  std::vector<std::pair<uint16_t, uint32_t>> want;
  if (idx.size() < K) {
    want_rc = RS2_E_DECODING_UNSUCCESSFUL;
  } else {
    for (uint32_t i = 0; i < idx.size() && want.size() < K; ++i) {
      bool dup = idx[i] >= n;
      for (const auto& w : want) dup |= w.first == idx[i];
      if (!dup) want.emplace_back(idx[i], i);
    }
    if (want.size() < K) {
      want_rc = RS2_E_NOT_ENOUGH_SHARDS;
      want.clear();
    }
  }
  std::vector<std::pair<uint16_t, uint32_t>> chosen(3, {uint16_t(7), 7u});
  const int rc = select_recovery_symbols(K, n, uint32_t(idx.size()), idx.data(), chosen);
  CHECK(rc == want_rc);
  CHECK(chosen == want);
  CHECK((pat == kOneShort) == (rc == RS2_E_DECODING_UNSUCCESSFUL));
  CHECK((pat == kDuplicate) == (rc == RS2_E_NOT_ENOUGH_SHARDS));
  int eligible = 0, n_in = 0, n_out = 0;
  uint32_t originals = 0;
  if (rc == RS2_OK) {
    DecodeSpec sp;
    sliver_recover_spec(K, n, s, chosen, kSrcBase, kDstBase, true, sp);
    CHECK(sp.K == K && sp.R == n - K && sp.symbol_size == s);
    CHECK(sp.src_base == kSrcBase && sp.dst_base == kDstBase && sp.src_ls == 0 && sp.dst_ls == 0);
    CHECK(sp.dst_limit == int64_t(K) * s);
    CHECK(sp.present.size() == n && sp.dst.size() == K);
    std::vector<int64_t> present(n, -1);
    for (const auto& c : chosen) present[c.first] = int64_t(c.second) * s;
    CHECK(sp.present == present);
    for (uint32_t i = 0; i < K; ++i) {
      CHECK(sp.dst[i] == int64_t(i) * s);
      originals += present[i] >= 0;
    }
    CHECK(sp.copy_present == (originals > 0 && s >= 4));
    DecodeSpec nofuse;
    sliver_recover_spec(K, n, s, chosen, kSrcBase, kDstBase, false, nofuse);
    CHECK(!nofuse.copy_present && nofuse.present == sp.present);
    if (originals < K) {  // something erased: the engine plans it as a batch job candidate
      PlannedJob pj;
      CHECK(plan_decode(sp, pj) == RS2_OK);
      const bool fused = sp.copy_present && copy_covered(pj);
      finish_plan(pj);
      eligible = batch_eligible(pj, fused) && (originals == 0 || fused);
      n_in = pj.job.n_in;
      n_out = pj.job.n_out;
    }
  }
  std::printf("%s count=%zu rc=%d originals=%u n_in=%d n_out=%d eligible=%d\n", label, idx.size(),
              rc, originals, n_in, n_out, eligible);
  ++g_cases;
}

}  // namespace

int main() {
  const uint32_t ns[] = {10, 13, 100, 1000, 3100, 4500};
  for (uint32_t n : ns)
    for (int axis = 0; axis < 2; ++axis)
      for (int s : {2, 6, 20, 1206}) {
        for (uint64_t seed = 1; seed <= 3; ++seed) run_case(n, axis, kRandom, seed * 977 + n, s);
        run_case(n, axis, kAllRepair, 0, s);
        run_case(n, axis, kAllOriginal, 0, s);
        for (uint64_t seed : {0ull, 1234567ull}) run_case(n, axis, kOneErasure, seed, s);
        run_case(n, axis, kNoisy, 11 + n, s);
        run_case(n, axis, kOneShort, 12 + n, s);
        run_case(n, axis, kDuplicate, 13 + n, s);
      }
  std::fprintf(stderr, "planner_recover_check: %d cases\n", g_cases);
  return 0;
}
