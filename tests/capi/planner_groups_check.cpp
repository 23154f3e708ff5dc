// CPU check of the mixed sliver verification planner (walrus_amd/csrc/rs2_planner.h:
// plan_sliver_axis, plan_sliver_groups), built from the planner sources alone with the host
// compiler by tests/test_planner_groups.py.  Per case it restates the window rule, the grouping
// and the tile counts directly and compares; one line per case, a breach exits non-zero.
#include "../../walrus_amd/csrc/rs2_planner.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

namespace {

using namespace rs2;

[[noreturn]] void breach(const char* what, const char* label) {
  std::fprintf(stderr, "planner_groups_check: %s: %s\n", label, what);
  std::exit(1);
}
#define CHECK(cond)                    \
  do {                                 \
    if (!(cond)) breach(#cond, label); \
  } while (0)

const uint16_t kSizes[] = {2, 4, 6, 62, 64, 66, 126, 128, 130, 254, 256, 258};
const uint16_t kSizes1000[] = {2, 20, 66, 130, 1206};

struct Call {
  std::vector<uint8_t> axis;
  std::vector<uint16_t> size;
  std::vector<uint64_t> off;
};

uint32_t k_of(uint32_t n, int axis) {
  const uint32_t f = (n - 1) / 3;
  return axis == RS2_AXIS_PRIMARY ? n - f : n - 2 * f;
}

// every size on both axes, `per` slivers per group; order 0 interleaved (A, B, A, B ...),
// 1 sorted by group, 2 reverse of sorted
Call make_call(uint32_t n, const std::vector<uint16_t>& sizes, uint32_t per, int order) {
  std::vector<std::pair<uint8_t, uint16_t>> groups;
  for (uint16_t s : sizes)
    for (uint8_t a = 0; a < 2; ++a) groups.emplace_back(a, s);
  std::vector<std::pair<uint8_t, uint16_t>> seq;
  if (order == 0) {
    for (uint32_t q = 0; q < per; ++q)
      for (const auto& g : groups) seq.push_back(g);
  } else {
    for (const auto& g : groups)
      for (uint32_t q = 0; q < per; ++q) seq.push_back(g);
    if (order == 2) std::reverse(seq.begin(), seq.end());
  }
  Call c;
  uint64_t at = 0;
  for (const auto& g : seq) {
    c.axis.push_back(g.first);
    c.size.push_back(g.second);
    c.off.push_back(at);
    at += uint64_t(k_of(n, g.first)) * g.second + 6;  // a gap between slivers
  }
  return c;
}

// The properties of a plan over `call` (status: per-sliver codes, or null when none was refused).
// Returns the number of windows.
size_t check_plan(const char* label, uint32_t n, const SliverAxisCode (&codes)[2], const Call& call,
                  const int* status, uint64_t budget, uint32_t max_groups,
                  const SliverGroupsPlan& plan) {
  const uint32_t m = uint32_t(call.axis.size());
  // windows partition the slivers in order
  uint32_t next = 0;
  std::set<uint32_t> seen;
  uint32_t accepted = 0;
  for (uint32_t i = 0; i < m; ++i) accepted += !status || status[i] == RS2_OK;
  CHECK(plan.accepted == accepted);
  for (size_t wi = 0; wi < plan.windows.size(); ++wi) {
    const SliverWindow& w = plan.windows[wi];
    CHECK(w.first == next);
    CHECK(w.count >= 1 || m == 0);
    next += w.count;
    // the slot permutation: a bijection onto the window's accepted slivers
    CHECK(w.perm.size() == w.n_slots);
    uint32_t in_window = 0;
    for (uint32_t i = w.first; i < w.first + w.count; ++i) in_window += !status || status[i] == RS2_OK;
    CHECK(in_window == w.n_slots);
    for (uint32_t i : w.perm) {
      CHECK(i >= w.first && i < w.first + w.count);
      CHECK(!status || status[i] == RS2_OK);
      CHECK(seen.insert(i).second);
    }
    // groups: maximal per (axis, size), contiguous slots, stable inside a group
    std::set<std::pair<int, int>> keys;
    uint32_t slot = 0, eligible_slots = 0;
    uint64_t scratch = 0, gather = 0, repair = 0;
    bool past_eligible = false;
    uint32_t tiles_at[2] = {0, 0}, n_of_axis[2] = {0, 0};
    CHECK(w.groups.size() <= max_groups);
    for (size_t p = 0; p < w.groups.size(); ++p) {
      const SliverGroup& g = w.groups[p];
      CHECK(keys.insert({int(g.axis), int(g.s)}).second);
      CHECK(g.first_slot == slot && g.count >= 1);
      CHECK(g.k == k_of(n, g.axis));
      CHECK(g.gather_off == gather);
      for (uint32_t q = 0; q < g.count; ++q) {
        const uint32_t i = w.perm[slot + q];
        CHECK(call.axis[i] == g.axis && call.size[i] == g.s);
        if (q) CHECK(w.perm[slot + q - 1] < i);
      }
      slot += g.count;
      gather += uint64_t(g.count) * g.k * g.s;
      scratch += uint64_t(g.count) * sliver_scratch_bytes(n, g.s);
      // eligibility as the header states it
      const bool want = g.s >= 4 && codes[g.axis].batchable;
      CHECK(g.eligible == want);
      if (!g.eligible) {
        past_eligible = true;
        continue;
      }
      CHECK(!past_eligible);  // eligible groups first
      CHECK(p == 0 || !w.groups[p - 1].eligible || w.groups[p - 1].axis <= g.axis);
      if (n_of_axis[g.axis]++ == 0) CHECK(w.axis_first[g.axis] == p);
      // tiles: ceil(n_lines * pairs_span / 64), prefixes increasing
      const int32_t n_pairs = int32_t((g.s + 3) / 4);
      CHECK(g.pairs_span >= n_pairs && g.pairs_span % 2 == 0);
      const uint32_t t = uint32_t((uint64_t(g.count) * uint64_t(g.pairs_span) + 63) / 64);
      CHECK(t >= 1 && g.first_tile == tiles_at[g.axis]);
      const std::vector<uint32_t>& tl = w.tiles[g.axis];
      CHECK(tl.size() > n_of_axis[g.axis]);
      CHECK(tl[n_of_axis[g.axis] - 1] == g.first_tile);
      CHECK(tl[n_of_axis[g.axis]] == g.first_tile + t);
      tiles_at[g.axis] += t;
      CHECK(g.repair_off == repair);
      repair += uint64_t(g.count) * (n - g.k) * g.s;
      eligible_slots = slot;
    }
    CHECK(w.n_eligible_slots == eligible_slots);
    for (int a = 0; a < 2; ++a) {
      CHECK(w.axis_groups[a] == n_of_axis[a]);
      CHECK(w.tiles[a].size() == size_t(n_of_axis[a]) + 1 && w.tiles[a][0] == 0);
    }
    CHECK(slot == w.n_slots && gather == w.gather_bytes && repair == w.repair_bytes);
    // the budget holds, unless the window is a single sliver
    CHECK(scratch <= budget || w.n_slots == 1);
    // and the window could not have taken the next accepted sliver
    if (wi + 1 < plan.windows.size()) {
      const SliverWindow& nx = plan.windows[wi + 1];
      uint32_t i = nx.first;
      while (status && status[i] != RS2_OK) ++i;
      CHECK(i == nx.first);  // a window starts at an accepted sliver (refused ones trail)
      const bool new_group = !keys.count({int(call.axis[i]), int(call.size[i])});
      CHECK(scratch + sliver_scratch_bytes(n, call.size[i]) > budget ||
            (new_group && w.groups.size() == max_groups));
    }
  }
  CHECK(next == m);
  CHECK(seen.size() == accepted);
  return plan.windows.size();
}

void run_case(uint32_t n, const std::vector<uint16_t>& sizes, uint32_t per, int order,
              uint32_t hold) {
  char label[128];
  std::snprintf(label, sizeof label, "n=%u sizes=%zu per=%u order=%d hold=%u", n, sizes.size(), per,
                order, hold);
  SliverAxisCode codes[2];
  CHECK(plan_sliver_axis(n, 0, codes[0]) == RS2_OK && plan_sliver_axis(n, 1, codes[1]) == RS2_OK);
  const Call call = make_call(n, sizes, per, order);
  const uint32_t m = uint32_t(call.axis.size());
  uint16_t smax = 0;
  for (uint16_t s : sizes) smax = std::max(smax, s);
  const uint64_t budget = hold ? uint64_t(hold) * sliver_scratch_bytes(n, smax) : ~uint64_t(0);
  SliverGroupsPlan plan;
  CHECK(plan_sliver_groups(codes, m, call.axis.data(), call.size.data(), call.off.data(), nullptr,
                           nullptr, budget, 256, nullptr, plan) == RS2_OK);
  const size_t windows = check_plan(label, n, codes, call, nullptr, budget, 256, plan);
  uint32_t eligible = 0, groups = 0;
  for (const SliverWindow& w : plan.windows) {
    groups += uint32_t(w.groups.size());
    for (const SliverGroup& g : w.groups) eligible += g.eligible;
  }
  std::printf("n=%u sizes=%zu per=%u order=%d hold=%u slivers=%u windows=%zu groups=%u eligible=%u\n",
              n, sizes.size(), per, order, hold, m, windows, groups, eligible);
}

// one size on one axis: the window count is exact
void run_uniform(uint32_t n, uint16_t s, uint32_t m, uint32_t hold) {
  char label[128];
  std::snprintf(label, sizeof label, "uniform n=%u s=%u m=%u hold=%u", n, unsigned(s), m, hold);
  SliverAxisCode codes[2];
  CHECK(plan_sliver_axis(n, 0, codes[0]) == RS2_OK && plan_sliver_axis(n, 1, codes[1]) == RS2_OK);
  Call call;
  for (uint32_t i = 0; i < m; ++i) {
    call.axis.push_back(RS2_AXIS_PRIMARY);
    call.size.push_back(s);
    call.off.push_back(uint64_t(i) * k_of(n, 0) * s);
  }
  const uint64_t budget = hold ? uint64_t(hold) * sliver_scratch_bytes(n, s) : ~uint64_t(0);
  SliverGroupsPlan plan;
  CHECK(plan_sliver_groups(codes, m, call.axis.data(), call.size.data(), call.off.data(), nullptr,
                           nullptr, budget, 256, nullptr, plan) == RS2_OK);
  const size_t windows = check_plan(label, n, codes, call, nullptr, budget, 256, plan);
  std::printf("uniform n=%u s=%u slivers=%u hold=%u windows=%zu\n", n, unsigned(s), m, hold, windows);
}

// every (n, axis, s >= 4) of the lists is eligible; s = 2 and n = 4500 are not
void run_eligibility() {
  const char* label = "eligibility";
  for (uint32_t n : {10u, 13u, 100u, 1000u, 4500u}) {
    SliverAxisCode codes[2];
    CHECK(plan_sliver_axis(n, 0, codes[0]) == RS2_OK && plan_sliver_axis(n, 1, codes[1]) == RS2_OK);
    std::vector<uint16_t> sizes;
    if (n == 1000)
      sizes.assign(std::begin(kSizes1000), std::end(kSizes1000));
    else
      sizes.assign(std::begin(kSizes), std::end(kSizes));
    for (int a = 0; a < 2; ++a) {
      CHECK(codes[a].planned && codes[a].k == k_of(n, a));
      const CodecJobBig& j = codes[a].tmpl.job;
      CHECK(j.n_in >= 1 && j.n_out >= 1);
      CHECK(codes[a].batchable == (n <= 4096 && j.n_in <= kBatchBlocks && j.n_out <= kBatchBlocks));
      for (uint16_t s : sizes) {
        const uint8_t axis = uint8_t(a);
        const uint64_t off = 0;
        SliverGroupsPlan plan;
        CHECK(plan_sliver_groups(codes, 1, &axis, &s, &off, nullptr, nullptr, ~uint64_t(0), 256,
                                 nullptr, plan) == RS2_OK);
        CHECK(plan.windows.size() == 1 && plan.windows[0].groups.size() == 1);
        const bool el = plan.windows[0].groups[0].eligible;
        CHECK(el == (s >= 4 && n <= 4096));
        std::printf("eligible n=%u axis=%d s=%u in=%d out=%d C=%d mode=%d: %d\n", n, a, unsigned(s),
                    j.n_in, j.n_out, codes[a].tmpl.C, codes[a].tmpl.mode, int(el));
      }
    }
  }
}

void run_refusals() {
  const char* label = "refusals";
  const uint32_t n = 10;
  SliverAxisCode codes[2];
  CHECK(plan_sliver_axis(n, 0, codes[0]) == RS2_OK && plan_sliver_axis(n, 1, codes[1]) == RS2_OK);
  CHECK(plan_sliver_axis(n, 2, codes[0]) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_sliver_axis(0, 0, codes[0]) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_sliver_axis(n, 0, codes[0]) == RS2_OK);
  // device form: good, bad axis, size 0, odd size, odd offset, good
  Call c;
  c.axis = {0, 2, 1, 0, 1, 1};
  c.size = {4, 4, 0, 5, 6, 6};
  c.off = {0, 100, 200, 300, 401, 500};
  const int want[] = {RS2_OK, RS2_E_INVALID_ARGUMENT, RS2_E_INCOMPATIBLE_PARAMETERS,
                      RS2_E_INCOMPATIBLE_PARAMETERS, RS2_E_INVALID_ARGUMENT, RS2_OK};
  int status[6];
  SliverGroupsPlan plan;
  CHECK(plan_sliver_groups(codes, 6, c.axis.data(), c.size.data(), c.off.data(), nullptr, nullptr,
                           ~uint64_t(0), 256, status, plan) == RS2_OK);
  for (int i = 0; i < 6; ++i) CHECK(status[i] == want[i]);
  check_plan(label, n, codes, c, status, ~uint64_t(0), 256, plan);
  CHECK(plan.accepted == 2);
  // without status_out: the first failing sliver's code, whichever it is
  for (int first = 1; first < 5; ++first) {
    Call d;
    d.axis = {0, c.axis[size_t(first)]};
    d.size = {4, c.size[size_t(first)]};
    d.off = {0, c.off[size_t(first)]};
    CHECK(plan_sliver_groups(codes, 2, d.axis.data(), d.size.data(), d.off.data(), nullptr,
                             nullptr, ~uint64_t(0), 256, nullptr, plan) == want[first]);
  }
  // host form: a null sliver, a wrong length; the axis and size rules come first
  const uint8_t dummy[64] = {};
  const uint8_t* ptrs[] = {dummy, nullptr, dummy, dummy, dummy};
  const uint8_t ax[] = {0, 0, 1, 0, 3};
  const uint16_t sz[] = {4, 4, 6, 3, 4};
  const uint64_t len[] = {uint64_t(k_of(n, 0)) * 4, uint64_t(k_of(n, 0)) * 4,
                          uint64_t(k_of(n, 1)) * 6 + 2, 21, 28};
  const int hwant[] = {RS2_OK, RS2_E_INCORRECT_DATA_LENGTH, RS2_E_INCORRECT_DATA_LENGTH,
                       RS2_E_INCOMPATIBLE_PARAMETERS, RS2_E_INVALID_ARGUMENT};
  int hstatus[5];
  CHECK(plan_sliver_groups(codes, 5, ax, sz, nullptr, ptrs, len, ~uint64_t(0), 256, hstatus, plan) ==
        RS2_OK);
  for (int i = 0; i < 5; ++i) CHECK(hstatus[i] == hwant[i]);
  CHECK(plan.accepted == 1);
  // whole-call refusals
  CHECK(plan_sliver_groups(codes, 65536, c.axis.data(), c.size.data(), c.off.data(), nullptr,
                           nullptr, 1, 256, nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_sliver_groups(codes, 1, nullptr, c.size.data(), c.off.data(), nullptr, nullptr, 1, 256,
                           nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_sliver_groups(codes, 1, c.axis.data(), nullptr, c.off.data(), nullptr, nullptr, 1, 256,
                           nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_sliver_groups(codes, 1, c.axis.data(), c.size.data(), nullptr, nullptr, nullptr, 1, 256,
                           nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_sliver_groups(codes, 1, c.axis.data(), c.size.data(), c.off.data(), nullptr, nullptr, 1,
                           0, nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_sliver_groups(codes, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 256, nullptr,
                           plan) == RS2_OK);
  CHECK(plan.windows.empty());
  // every sliver refused: one window, no slots
  int s2[2];
  const uint8_t bad_ax[] = {7, 9};
  const uint16_t some[] = {4, 4};
  const uint64_t offs[] = {0, 64};
  CHECK(plan_sliver_groups(codes, 2, bad_ax, some, offs, nullptr, nullptr, 1, 256, s2, plan) == RS2_OK);
  CHECK(plan.windows.size() == 1 && plan.windows[0].count == 2 && plan.windows[0].n_slots == 0);
  // the group cap closes a window: 3 groups, 2 per window
  Call g3 = make_call(n, {4, 6}, 1, 1);  // (0,4) (1,4) (0,6) (1,6)
  CHECK(plan_sliver_groups(codes, 4, g3.axis.data(), g3.size.data(), g3.off.data(), nullptr, nullptr,
                           ~uint64_t(0), 3, nullptr, plan) == RS2_OK);
  CHECK(check_plan(label, n, codes, g3, nullptr, ~uint64_t(0), 3, plan) == 2);
  std::printf("refusals ok\n");
}

}  // namespace

int main() {
  for (uint32_t n : {10u, 13u, 100u, 1000u, 4500u}) {
    std::vector<uint16_t> sizes;
    if (n == 1000)
      sizes.assign(std::begin(kSizes1000), std::end(kSizes1000));
    else if (n == 4500)
      sizes = {4, 66};
    else
      sizes.assign(std::begin(kSizes), std::end(kSizes));
    for (uint32_t per : {1u, 5u})
      for (int order : {0, 1, 2})
        for (uint32_t hold : {1u, 2u, 0u}) run_case(n, sizes, per, order, hold);
    for (uint32_t hold : {1u, 2u, 0u}) run_uniform(n, 66, 7, hold);
  }
  run_eligibility();
  run_refusals();
  return 0;
}
