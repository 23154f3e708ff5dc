// CPU check of the mixed recovery-symbol planner (walrus_amd/csrc/rs2_planner.h:
// plan_symbols_mixed), built from the planner sources alone with the host compiler by
// tests/test_planner_symbols_mixed.py.  Per case it restates the window rule, the slot order's
// invariants, the expanded set and the request table directly and compares; one line per case, a
// breach exits non-zero.
#include "../../walrus_amd/csrc/rs2_planner.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

namespace {

using namespace rs2;

[[noreturn]] void breach(const char* what, const char* label) {
  std::fprintf(stderr, "planner_symbols_mixed_check: %s: %s\n", label, what);
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

struct Call {
  std::vector<uint8_t> axis;
  std::vector<uint16_t> size;
  std::vector<uint64_t> in_off, out_off;
  std::vector<uint32_t> counts;
  std::vector<uint16_t> targets;
};

enum Targets { kMixed = 0, kSystematic, kRepair };
const char* const kTargetsName[] = {"mixed", "systematic", "repair"};

uint32_t k_of(uint32_t n, int axis) {
  const uint32_t f = (n - 1) / 3;
  return axis == 0 ? n - f : n - 2 * f;
}

// m slivers over `sizes`, the axes alternating, counts cycling through `counts`
Call make_call(uint32_t n, uint32_t m, const std::vector<uint16_t>& sizes,
               const std::vector<uint32_t>& counts, int kind, uint64_t seed) {
  Call c;
  Lcg g{seed};
  uint64_t in = 0, out = 0;
  for (uint32_t i = 0; i < m; ++i) {
    const int a = int(i % 2);
    const uint16_t s = sizes[(i / 2) % sizes.size()];
    const uint32_t k = k_of(n, a), cnt = counts[i % counts.size()];
    c.axis.push_back(uint8_t(a));
    c.size.push_back(s);
    c.in_off.push_back(in);
    c.out_off.push_back(out);
    c.counts.push_back(cnt);
    in += uint64_t(k) * s + 2;
    out += uint64_t(cnt) * s + 6;
    for (uint32_t q = 0; q < cnt; ++q) {
      uint32_t t = kind == kSystematic ? g.next(k) : kind == kRepair ? k + g.next(n - k) : g.next(n);
      if (kind == kMixed && q == 0) t = k - 1;  // the seam
      if (kind == kMixed && q == 1) t = k;
      c.targets.push_back(uint16_t(t));
    }
  }
  return c;
}

// The plan of `c` under (trees, have_nodes, budget, max_groups) against the rules restated.
// refused: slivers whose status must be non-zero (the call was made invalid there by the caller).
void check_plan(const char* label, uint32_t n, const Call& c, int trees, bool have_nodes,
                uint64_t budget, uint32_t max_groups, const std::set<uint32_t>& refused,
                size_t* windows_out, uint64_t* expanded_out) {
  SliverAxisCode codes[2];
  CHECK(plan_sliver_axis(n, 0, codes[0]) == RS2_OK && plan_sliver_axis(n, 1, codes[1]) == RS2_OK);
  const uint32_t m = uint32_t(c.axis.size());
  std::vector<int> status(m, 77);
  SymbolsMixedPlan plan;
  const int rc = plan_symbols_mixed(codes, m, c.axis.data(), c.size.data(), c.in_off.data(),
                                    c.out_off.data(), nullptr, nullptr, c.counts.data(),
                                    c.targets.empty() ? nullptr : c.targets.data(), trees,
                                    have_nodes, budget, max_groups, status.data(), plan);
  CHECK(rc == RS2_OK);
  const bool build = trees == RS2_TREES_BUILD;
  uint32_t lb[kSymbolLevels];
  uint64_t nn = 0;
  const int L = merkle_level_bases(n, lb, &nn);
  CHECK(plan.path_len == L && plan.n_nodes == nn);
  for (int l = 0; l < kSymbolLevels; ++l) CHECK(plan.level_base[l] == lb[l]);
  std::vector<uint64_t> first_req(m + 1, 0);
  for (uint32_t i = 0; i < m; ++i) first_req[i + 1] = first_req[i] + c.counts[i];
  CHECK(plan.total == first_req[m] && plan.table.size() == first_req[m]);
  uint32_t accepted = 0;
  for (uint32_t i = 0; i < m; ++i) {
    CHECK((status[i] != RS2_OK) == (refused.count(i) != 0));
    accepted += status[i] == RS2_OK;
  }
  CHECK(plan.accepted == accepted);
  // the window rule restated: caller's order, budget, groups, one sliver at least
  std::vector<std::pair<uint32_t, uint32_t>> want;  // (first, count)
  {
    uint32_t first = 0, held = 0;
    uint64_t used = 0;
    std::set<uint32_t> groups;
    for (uint32_t i = 0; i < m; ++i) {
      if (status[i] != RS2_OK) continue;
      const uint64_t need = uint64_t(n) * (uint64_t(c.size[i]) + 32) + (build ? nn * 32 : 0);
      const uint32_t key = uint32_t(c.axis[i]) << 16 | c.size[i];
      if (held && (used + need > budget || (!groups.count(key) && groups.size() == max_groups))) {
        want.emplace_back(first, i - first);
        first = i;
        held = 0;
        used = 0;
        groups.clear();
      }
      ++held;
      used += need;
      groups.insert(key);
    }
    want.emplace_back(first, m - first);
  }
  CHECK(plan.windows.size() == want.size());
  uint64_t expanded = 0;
  for (size_t wi = 0; wi < want.size(); ++wi) {
    const SymbolsMixedWindow& w = plan.windows[wi];
    CHECK(w.first == want[wi].first && w.count == want[wi].second);
    CHECK(w.first_request == first_req[w.first]);
    CHECK(w.n_requests == first_req[w.first + w.count] - first_req[w.first]);
    // the slots: every accepted sliver of the window once, the expanded ones first and in
    // SliverWindow order (grouped: a group's slots are neighbours), the others in caller order
    CHECK(w.perm.size() == w.n_slots && w.slot_request.size() == w.n_slots);
    CHECK(w.ex.n_slots <= w.n_slots && w.ex.perm.size() == w.ex.n_slots);
    std::vector<int> slot_of(w.count, -1);
    for (uint32_t sl = 0; sl < w.n_slots; ++sl) {
      const uint32_t i = w.perm[sl];
      CHECK(i >= w.first && i < w.first + w.count && status[i] == RS2_OK && slot_of[i - w.first] < 0);
      slot_of[i - w.first] = int(sl);
      CHECK(w.slot_request[sl] == first_req[i] && w.slot_requests[sl] == c.counts[i]);
      if (sl < w.ex.n_slots) CHECK(w.ex.perm[sl] == i);
      if (sl > w.ex.n_slots) CHECK(w.perm[sl - 1] < i);
    }
    uint32_t served = 0, with = 0;
    for (uint32_t q = 0; q < w.count; ++q) {
      const uint32_t i = w.first + q;
      const uint32_t k = k_of(n, c.axis[i]);
      if (status[i] != RS2_OK) {
        CHECK(slot_of[q] < 0);
        for (uint64_t j = first_req[i]; j < first_req[i + 1]; ++j) CHECK(plan.table[j] == kRequestSkipped);
        continue;
      }
      CHECK(slot_of[q] >= 0);
      bool repair = false;
      for (uint64_t j = first_req[i]; j < first_req[i + 1]; ++j) {
        // every table entry decodes to its (slot, target)
        CHECK((plan.table[j] >> 16) == uint32_t(slot_of[q]) && (plan.table[j] & 0xFFFFu) == c.targets[j]);
        repair |= c.targets[j] >= k;
      }
      const bool want_expand = build ? (have_nodes || c.counts[i] > 0) : repair;
      CHECK(want_expand == (uint32_t(slot_of[q]) < w.ex.n_slots));
      served += c.counts[i];
      with += c.counts[i] > 0;
    }
    CHECK(w.served == served && w.with_requests == with);
    // the expanded slivers' groups: slots partitioned, one (axis, size) each, tiles consistent
    uint32_t slot = 0;
    std::set<uint32_t> keys;
    for (const SliverGroup& g : w.ex.groups) {
      CHECK(g.first_slot == slot && g.count >= 1);
      CHECK(keys.insert(uint32_t(g.axis) << 16 | g.s).second);
      for (uint32_t q = 0; q < g.count; ++q) {
        const uint32_t i = w.ex.perm[slot + q];
        CHECK(c.axis[i] == g.axis && c.size[i] == g.s && g.k == k_of(n, g.axis));
      }
      slot += g.count;
    }
    CHECK(slot == w.ex.n_slots && keys.size() <= max_groups);
    for (int a = 0; a < 2; ++a) {
      CHECK(w.ex.tiles[a].size() == size_t(w.ex.axis_groups[a]) + 1);
      for (uint32_t g = 0; g < w.ex.axis_groups[a]; ++g) {
        const SliverGroup& gr = w.ex.groups[w.ex.axis_first[a] + g];
        CHECK(gr.eligible && gr.axis == a && gr.first_tile == w.ex.tiles[a][g]);
        CHECK(w.ex.tiles[a][g + 1] - w.ex.tiles[a][g] ==
              (uint64_t(gr.count) * uint64_t(gr.pairs_span) + 63) / 64);
      }
    }
    expanded += w.ex.n_slots;
  }
  *windows_out = plan.windows.size();
  *expanded_out = expanded;
}

void run_case(uint32_t n, uint32_t m, const std::vector<uint16_t>& sizes,
              const std::vector<uint32_t>& counts, int trees, bool have_nodes, uint32_t hold,
              int kind, uint64_t seed) {
  char label[200];
  std::snprintf(label, sizeof label, "n=%u slivers=%u sizes=%zu trees=%d nodes=%d hold=%u targets=%s",
                n, m, sizes.size(), trees, int(have_nodes), hold, kTargetsName[kind]);
  const Call c = make_call(n, m, sizes, counts, kind, seed);
  uint64_t nn = 0;
  uint32_t lb[kSymbolLevels];
  merkle_level_bases(n, lb, &nn);
  // a budget that holds `hold` slivers of the largest size (0: every sliver)
  uint16_t smax = 0;
  for (uint16_t s : sizes) smax = std::max(smax, s);
  const uint64_t per = uint64_t(n) * (uint64_t(smax) + 32) + (trees == RS2_TREES_BUILD ? nn * 32 : 0);
  const uint64_t budget = hold ? per * hold : per * m;
  size_t windows = 0;
  uint64_t expanded = 0;
  check_plan(label, n, c, trees, have_nodes, budget, 256, {}, &windows, &expanded);
  if (hold == 0) CHECK(windows == 1);
  if (hold && sizes.size() == 1) CHECK(windows == (m + hold - 1) / hold);
  if (hold) CHECK(windows >= (m + hold - 1) / hold || sizes.size() > 1);
  uint64_t requests = 0;
  for (uint32_t x : c.counts) requests += x;
  std::printf("%s requests=%llu windows=%zu expanded=%llu\n", label,
              static_cast<unsigned long long>(requests), windows,
              static_cast<unsigned long long>(expanded));
  ++g_cases;
}

// 600 slivers of 300 sizes on both axes: 600 groups, so the 257th opens a new window
void group_cap() {
  const char* label = "group cap";
  std::vector<uint16_t> sizes;
  for (uint16_t s = 2; s <= 600; s += 2) sizes.push_back(s);
  const Call c = make_call(10, 600, sizes, {1}, kMixed, 5);
  size_t windows = 0;
  uint64_t expanded = 0;
  check_plan(label, 10, c, RS2_TREES_BUILD, false, uint64_t(1) << 40, 256, {}, &windows, &expanded);
  CHECK(windows == 3 && expanded == 600);
  std::printf("group cap windows=%zu\n", windows);
  ++g_cases;
}

void refusals() {
  const char* label = "refusals";
  SliverAxisCode codes[2];
  CHECK(plan_sliver_axis(10, 0, codes[0]) == RS2_OK && plan_sliver_axis(10, 1, codes[1]) == RS2_OK);
  const uint64_t big = uint64_t(1) << 30;
  SymbolsMixedPlan plan;
  // a valid call of five slivers, then one fault per sliver; K_s = 7, K_p = 4
  Call ok = make_call(10, 5, {4, 6}, {2, 0, 3, 1, 2}, kMixed, 9);
  auto call = [&](const Call& c, int trees, bool nodes, int* status, const uint8_t* const* sl = nullptr,
                  const uint64_t* len = nullptr) {
    return plan_symbols_mixed(codes, uint32_t(c.axis.size()), c.axis.data(), c.size.data(),
                              sl ? nullptr : c.in_off.data(), sl ? nullptr : c.out_off.data(), sl,
                              len, c.counts.data(), c.targets.data(), trees, nodes, big, 256, status,
                              plan);
  };
  int st[5];
  CHECK(call(ok, RS2_TREES_BUILD, false, nullptr) == RS2_OK && plan.accepted == 5);
  // whole-call refusals
  CHECK(call(ok, 2, true, st) == RS2_E_INVALID_ARGUMENT);
  CHECK(call(ok, -1, true, st) == RS2_E_INVALID_ARGUMENT);
  CHECK(call(ok, RS2_TREES_CACHED, false, st) == RS2_E_INVALID_ARGUMENT);
  CHECK(call(ok, RS2_TREES_CACHED, true, st) == RS2_OK);
  CHECK(plan_symbols_mixed(codes, 5, nullptr, ok.size.data(), ok.in_off.data(), ok.out_off.data(),
                           nullptr, nullptr, ok.counts.data(), ok.targets.data(), RS2_TREES_BUILD,
                           false, big, 256, st, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_symbols_mixed(codes, 5, ok.axis.data(), ok.size.data(), ok.in_off.data(),
                           ok.out_off.data(), nullptr, nullptr, nullptr, ok.targets.data(),
                           RS2_TREES_BUILD, false, big, 256, st, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_symbols_mixed(codes, 5, ok.axis.data(), ok.size.data(), ok.in_off.data(),
                           ok.out_off.data(), nullptr, nullptr, ok.counts.data(), nullptr,
                           RS2_TREES_BUILD, false, big, 256, st, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan.windows.empty() && plan.table.empty());
  // every sliver faulty in several ways at once: the first rule in the stated order decides
  Call bad = ok;
  bad.axis[0] = 2;  bad.size[0] = 3;  bad.in_off[0] = 1;  bad.targets[0] = 10;   // axis first
  bad.size[2] = 0;  bad.out_off[2] = 3;  bad.targets[2] = 11;                    // then the size
  bad.in_off[3] |= 1;  bad.targets[5] = 10;                                       // then an offset
  bad.targets[7] = 10;                                                            // then a target
  CHECK(call(bad, RS2_TREES_BUILD, false, st) == RS2_OK);
  CHECK(st[0] == RS2_E_INVALID_ARGUMENT && st[1] == RS2_OK && st[2] == RS2_E_INCOMPATIBLE_PARAMETERS &&
        st[3] == RS2_E_INVALID_ARGUMENT && st[4] == RS2_E_INVALID_ARGUMENT);
  CHECK(plan.accepted == 1 && plan.total == 8);
  for (uint32_t e : plan.table) CHECK(e == kRequestSkipped);  // sliver 1 has no targets
  // without status_out the first failing sliver's code is the call's
  CHECK(call(bad, RS2_TREES_BUILD, false, nullptr) == RS2_E_INVALID_ARGUMENT);
  Call bad2 = ok;
  bad2.size[1] = 5;
  bad2.targets[7] = 10;
  CHECK(call(bad2, RS2_TREES_BUILD, false, nullptr) == RS2_E_INCOMPATIBLE_PARAMETERS);
  Call bad3 = ok;
  bad3.out_off[4] = 7;
  CHECK(call(bad3, RS2_TREES_BUILD, false, nullptr) == RS2_E_INVALID_ARGUMENT);
  {
    size_t windows = 0;
    uint64_t expanded = 0;
    check_plan(label, 10, bad, RS2_TREES_BUILD, true, big, 256, {0, 2, 3, 4}, &windows, &expanded);
    CHECK(windows == 1 && expanded == 1);
  }
  // every sliver refused, with targets (the smallest case: one sliver, one target = n_shards):
  // RS2_OK with status_out, one window without a slot, every entry the skip mark
  {
    Call one = make_call(10, 1, {6}, {2}, kSystematic, 3);
    one.targets[1] = 10;
    int s1[1] = {0};
    CHECK(call(one, RS2_TREES_BUILD, true, s1) == RS2_OK && s1[0] == RS2_E_INVALID_ARGUMENT);
    CHECK(plan.accepted == 0 && plan.total == 2 && plan.windows.size() == 1);
    CHECK(plan.windows[0].n_slots == 0 && plan.windows[0].ex.n_slots == 0 &&
          plan.windows[0].n_requests == 2 && plan.windows[0].served == 0);
    for (uint32_t e : plan.table) CHECK(e == kRequestSkipped);
    CHECK(call(one, RS2_TREES_BUILD, true, nullptr) == RS2_E_INVALID_ARGUMENT);
    Call all = ok;
    for (auto& a : all.axis) a = 7;
    size_t windows = 0;
    uint64_t expanded = 0;
    check_plan(label, 10, all, RS2_TREES_CACHED, true, big, 256, {0, 1, 2, 3, 4}, &windows, &expanded);
    CHECK(windows == 1 && expanded == 0);
  }
  // host form: a null or wrong-length sliver comes last
  std::vector<uint8_t> bytes(7 * 6, 0);
  const uint8_t* sl[5] = {bytes.data(), bytes.data(), nullptr, bytes.data(), bytes.data()};
  uint64_t len[5];
  for (int i = 0; i < 5; ++i) len[i] = uint64_t(k_of(10, ok.axis[size_t(i)])) * ok.size[size_t(i)];
  len[4] += 2;
  Call host = ok;
  host.targets[7] = 10;  // sliver 4: the target rule comes before the length rule
  CHECK(call(host, RS2_TREES_BUILD, false, st, sl, len) == RS2_OK);
  CHECK(st[0] == RS2_OK && st[1] == RS2_OK && st[2] == RS2_E_INCORRECT_DATA_LENGTH &&
        st[3] == RS2_OK && st[4] == RS2_E_INVALID_ARGUMENT);
  host.targets[7] = 0;
  CHECK(call(host, RS2_TREES_BUILD, false, st, sl, len) == RS2_OK && st[4] == RS2_E_INCORRECT_DATA_LENGTH);
  // 65535 slivers pass, 65536 do not (all counts zero, null target list)
  {
    std::vector<uint8_t> ax(65536, 0);
    std::vector<uint16_t> sz(65536, 2);
    std::vector<uint64_t> off(65536, 0);
    std::vector<uint32_t> zeros(65536, 0);
    CHECK(plan_symbols_mixed(codes, 65535, ax.data(), sz.data(), off.data(), off.data(), nullptr,
                             nullptr, zeros.data(), nullptr, RS2_TREES_BUILD, true, big, 256, nullptr,
                             plan) == RS2_OK);
    CHECK(plan.total == 0 && plan.accepted == 65535 && !plan.windows.empty());
    CHECK(plan_symbols_mixed(codes, 65536, ax.data(), sz.data(), off.data(), off.data(), nullptr,
                             nullptr, zeros.data(), nullptr, RS2_TREES_BUILD, true, big, 256, nullptr,
                             plan) == RS2_E_INVALID_ARGUMENT);
  }
  // the request sum is taken in 64 bits and refused before any target is read (the target list
  // here is far shorter than the counts say)
  {
    const uint8_t ax[2] = {0, 1};
    const uint16_t sz[2] = {4, 4};
    const uint64_t off[2] = {0, 0};
    const uint16_t tg[1] = {0};
    const uint32_t wrap[2] = {0x80000000u, 0x80000000u}, one_over[2] = {0x7FFFFFFFu, 1};
    CHECK(plan_symbols_mixed(codes, 2, ax, sz, off, off, nullptr, nullptr, wrap, tg, RS2_TREES_BUILD,
                             false, big, 256, st, plan) == RS2_E_INVALID_ARGUMENT);
    CHECK(plan_symbols_mixed(codes, 2, ax, sz, off, off, nullptr, nullptr, one_over, tg,
                             RS2_TREES_BUILD, false, big, 256, st, plan) == RS2_E_INVALID_ARGUMENT);
  }
  // no slivers: nothing to plan
  CHECK(plan_symbols_mixed(codes, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, RS2_TREES_BUILD, false, big, 256, nullptr, plan) == RS2_OK);
  CHECK(plan.windows.empty() && plan.total == 0);
  std::printf("refusals ok\n");
  ++g_cases;
}

}  // namespace

int main() {
  refusals();
  group_cap();
  const std::vector<std::vector<uint32_t>> lists = {{3, 0, 5, 1, 4}, {0, 0, 0, 0}, {2, 2, 2}};
  const std::vector<std::vector<uint16_t>> size_sets = {{6}, {2, 4, 6, 18, 258}};
  uint64_t seed = 1;
  for (uint32_t n : {10u, 13u, 100u, 1000u, 4500u})
    for (const auto& sizes : size_sets)
      for (const auto& counts : lists)
        for (int trees : {RS2_TREES_BUILD, RS2_TREES_CACHED})
          for (int nodes = trees == RS2_TREES_CACHED ? 1 : 0; nodes < 2; ++nodes)
            for (uint32_t hold : {1u, 2u, 0u})
              for (int kind : {kMixed, kSystematic, kRepair})
                run_case(n, 11, sizes, counts, trees, nodes != 0, hold, kind, ++seed);
  std::fprintf(stderr, "planner_symbols_mixed_check: %d cases\n", g_cases);
  return 0;
}
