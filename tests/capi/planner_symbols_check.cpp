// CPU check of the bulk recovery-symbol planner (walrus_amd/csrc/rs2_planner.h:
// plan_symbol_requests, merkle_level_bases), built from the planner sources alone with the host
// compiler by tests/test_planner_symbols.py.  Per case it restates the window rule, the request
// table and the tree's level bases directly and compares; one line per case, a breach exits
// non-zero.
#include "../../walrus_amd/csrc/rs2_planner.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

using namespace rs2;

[[noreturn]] void breach(const char* what, const char* label) {
  std::fprintf(stderr, "planner_symbols_check: %s: %s\n", label, what);
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

int g_cases = 0;

// merkle.rs:216-266 restated: the leaves, then each level half the (padded) one below; every
// level but the root is padded to an even count with the zero node
void tree_shape(uint32_t n, std::vector<uint64_t>& bases, uint64_t& n_nodes) {
  bases.clear();
  uint64_t level = n, at = 0;
  while (level > 1) {
    bases.push_back(at);
    if (level % 2) ++level;
    at += level;
    level /= 2;
  }
  n_nodes = at + level;  // the root (or a lone leaf)
}

void check_levels(uint32_t n) {
  char label[64];
  std::snprintf(label, sizeof label, "levels n=%u", n);
  std::vector<uint64_t> want;
  uint64_t want_nodes = 0;
  tree_shape(n, want, want_nodes);
  uint32_t got[kSymbolLevels];
  uint64_t nn = 0;
  const int L = merkle_level_bases(n, got, &nn);
  CHECK(L == int(want.size()) && L <= kSymbolLevels);
  CHECK(nn == want_nodes);
  for (int l = 0; l < L; ++l) CHECK(got[l] == want[l]);
  for (int l = L; l < kSymbolLevels; ++l) CHECK(got[l] == want_nodes - 1);
  std::printf("levels n=%u path_len=%d n_nodes=%llu\n", n, L, static_cast<unsigned long long>(nn));
  ++g_cases;
}

enum Targets { kMixed = 0, kSystematic, kRepair };
const char* const kTargetsName[] = {"mixed", "systematic", "repair"};

// `hold`: slivers a window is to hold (0: all of them)
void run_case(uint32_t n, int axis, uint32_t s, const std::vector<uint32_t>& counts, int trees,
              bool have_nodes, uint32_t hold, int kind, uint64_t seed) {
  const uint32_t f = (n - 1) / 3, kp = n - 2 * f, ks = n - f, k = axis == 0 ? ks : kp;
  const uint32_t m = uint32_t(counts.size());
  char label[200];
  std::snprintf(label, sizeof label, "n=%u axis=%d s=%u slivers=%u trees=%d nodes=%d hold=%u targets=%s",
                n, axis, s, m, trees, int(have_nodes), hold, kTargetsName[kind]);
  Lcg g{seed};
  std::vector<uint16_t> targets;
  for (uint32_t c : counts)
    for (uint32_t q = 0; q < c; ++q) {
      uint32_t t = kind == kSystematic ? g.next(k) : kind == kRepair ? k + g.next(n - k) : g.next(n);
      if (kind == kMixed && q == 0) t = k - 1;  // the seam
      if (kind == kMixed && q == 1) t = k;
      targets.push_back(uint16_t(t));
    }
  std::vector<uint64_t> bases;
  uint64_t n_nodes = 0;
  tree_shape(n, bases, n_nodes);
  const bool build = trees == RS2_TREES_BUILD;
  const uint64_t per = uint64_t(n - k) * s + (build ? uint64_t(n) * 32 : 0) +
                       (build && !have_nodes ? n_nodes * 32 : 0);
  // a budget that holds exactly `hold` slivers (one byte short of the next)
  const uint64_t budget = hold ? per * (hold + 1) - 1 : per * m;
  SymbolRequestPlan plan;
  const int rc = plan_symbol_requests(n, k, s, m, counts.data(), targets.data(), trees, have_nodes,
                                      budget, plan);
  CHECK(rc == RS2_OK);
  CHECK(plan.per_sliver == per && plan.n_nodes == n_nodes && plan.path_len == int(bases.size()));
  CHECK(plan.total == targets.size() && plan.table.size() == targets.size());
  const uint32_t per_window = hold ? hold : m;
  CHECK(plan.windows.size() == (m + per_window - 1) / per_window);
  uint32_t sliver = 0;
  uint64_t req = 0, expanded = 0;
  bool any_codec = false;
  for (const SymbolWindow& w : plan.windows) {
    // windows partition the slivers and the requests, in order
    CHECK(w.first_sliver == sliver && w.first_request == req);
    CHECK(w.n_slivers >= 1 && w.n_slivers <= per_window);
    CHECK(uint64_t(w.n_slivers) * per <= budget || w.n_slivers == 1);
    CHECK(&w == &plan.windows.back() || w.n_slivers == per_window);
    std::vector<uint8_t> want_expand(w.n_slivers, 0), got_expand(w.n_slivers, 0);
    uint64_t wreq = 0;
    for (uint32_t slot = 0; slot < w.n_slivers; ++slot) {
      const uint32_t c = counts[sliver + slot];
      want_expand[slot] = build && (have_nodes || c > 0);
      for (uint32_t q = 0; q < c; ++q, ++wreq) {
        // every packed entry decodes to its (slot, target)
        const uint32_t e = plan.table[size_t(req + wreq)];
        CHECK((e >> 16) == slot && (e & 0xFFFFu) == targets[size_t(req + wreq)]);
        if (targets[size_t(req + wreq)] >= k) want_expand[slot] = 1;
      }
    }
    CHECK(w.n_requests == wreq);
    uint32_t prev_end = 0;
    bool first_run = true;
    for (const auto& run : w.runs) {
      CHECK(run.second >= 1 && run.first + run.second <= w.n_slivers);
      CHECK(first_run || run.first > prev_end);  // maximal: a gap between runs
      for (uint32_t i = 0; i < run.second; ++i) got_expand[run.first + i] = 1;
      prev_end = run.first + run.second;
      first_run = false;
      expanded += run.second;
    }
    CHECK(got_expand == want_expand);
    CHECK(w.needs_codec == !w.runs.empty());  // n > k for every n here
    any_codec |= w.needs_codec;
    sliver += w.n_slivers;
    req += wreq;
  }
  CHECK(sliver == m && req == targets.size());
  if (!build && kind == kSystematic) CHECK(!any_codec && expanded == 0);
  std::printf("%s requests=%zu windows=%zu expanded=%llu codec=%d\n", label, targets.size(),
              plan.windows.size(), static_cast<unsigned long long>(expanded), int(any_codec));
  ++g_cases;
}

void refusals() {
  const char* label = "refusals";
  SymbolRequestPlan plan;
  const uint32_t counts[3] = {1, 0, 2};
  const uint16_t targets[3] = {0, 9, 6};
  const uint64_t big = uint64_t(1) << 28;
  CHECK(plan_symbol_requests(10, 7, 2, 3, counts, targets, RS2_TREES_BUILD, false, big, plan) == RS2_OK);
  CHECK(plan_symbol_requests(10, 7, 2, 3, counts, targets, 2, true, big, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_symbol_requests(10, 7, 2, 3, counts, targets, -1, true, big, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_symbol_requests(10, 7, 2, 3, counts, targets, RS2_TREES_CACHED, false, big, plan) ==
        RS2_E_INVALID_ARGUMENT);
  CHECK(plan_symbol_requests(10, 7, 2, 3, counts, targets, RS2_TREES_CACHED, true, big, plan) == RS2_OK);
  CHECK(plan_symbol_requests(10, 7, 2, 3, nullptr, targets, RS2_TREES_BUILD, false, big, plan) ==
        RS2_E_INVALID_ARGUMENT);
  CHECK(plan_symbol_requests(10, 7, 2, 3, counts, nullptr, RS2_TREES_BUILD, false, big, plan) ==
        RS2_E_INVALID_ARGUMENT);
  const uint16_t too_large[3] = {0, 10, 6};  // IndexTooLarge: n itself
  CHECK(plan_symbol_requests(10, 7, 2, 3, counts, too_large, RS2_TREES_BUILD, false, big, plan) ==
        RS2_E_INVALID_ARGUMENT);
  CHECK(plan.windows.empty() && plan.table.empty());
  // 65535 slivers pass, 65536 do not (no targets needed: all counts zero, null target list)
  std::vector<uint32_t> zeros(65536, 0);
  CHECK(plan_symbol_requests(10, 7, 2, 65535, zeros.data(), nullptr, RS2_TREES_BUILD, true, big, plan) ==
        RS2_OK);
  CHECK(plan.total == 0 && !plan.windows.empty());
  CHECK(plan_symbol_requests(10, 7, 2, 65536, zeros.data(), nullptr, RS2_TREES_BUILD, true, big, plan) ==
        RS2_E_INVALID_ARGUMENT);
  // the request sum is taken in 64 bits: two counts of 2^31 would wrap a 32-bit sum to 0, and
  // 2^31-1 + 1 is one too many; the refusal comes before any target is read
  const uint32_t wrap[2] = {0x80000000u, 0x80000000u};
  CHECK(plan_symbol_requests(10, 7, 2, 2, wrap, targets, RS2_TREES_BUILD, false, big, plan) ==
        RS2_E_INVALID_ARGUMENT);
  const uint32_t one_over[2] = {0x7FFFFFFFu, 1};
  CHECK(plan_symbol_requests(10, 7, 2, 2, one_over, targets, RS2_TREES_BUILD, false, big, plan) ==
        RS2_E_INVALID_ARGUMENT);
  // no slivers: nothing to plan
  CHECK(plan_symbol_requests(10, 7, 2, 0, nullptr, nullptr, RS2_TREES_BUILD, false, big, plan) == RS2_OK);
  CHECK(plan.windows.empty() && plan.total == 0);
  // a budget below one sliver's scratch still holds one sliver per window
  CHECK(plan_symbol_requests(10, 7, 2, 3, counts, targets, RS2_TREES_BUILD, false, 1, plan) == RS2_OK);
  CHECK(plan.windows.size() == 3);
  std::printf("refusals ok\n");
  ++g_cases;
}

}  // namespace

int main() {
  for (uint32_t n : {4u, 7u, 10u, 100u, 1000u, 4097u, 65535u}) check_levels(n);
  refusals();
  const std::vector<std::vector<uint32_t>> lists = {
      {3, 0, 5, 1, 4}, {0, 1, 100, 3, 0, 17}, {0, 0, 0, 0}, {2, 2, 2, 2, 2, 2, 2}};
  uint64_t seed = 1;
  for (uint32_t n : {10u, 100u, 1000u, 4500u})
    for (int axis = 0; axis < 2; ++axis)
      for (uint32_t s : {2u, 6u, 1206u})
        for (const auto& counts : lists)
          for (int trees : {RS2_TREES_BUILD, RS2_TREES_CACHED})
            for (int nodes = trees == RS2_TREES_CACHED ? 1 : 0; nodes < 2; ++nodes)
              for (uint32_t hold : {1u, 2u, 0u})
                for (int kind : {kMixed, kSystematic, kRepair})
                  run_case(n, axis, s, counts, trees, nodes != 0, hold, kind, ++seed);
  std::fprintf(stderr, "planner_symbols_check: %d cases\n", g_cases);
  return 0;
}
