// CPU check of the mixed sliver recovery planner (walrus_amd/csrc/rs2_planner.h:
// cut_range_chunks, plan_recover_mixed), built from the planner sources alone with the host
// compiler by tests/test_planner_ranges.py.  One line per case, a breach exits non-zero.
#include "../../walrus_amd/csrc/rs2_planner.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

namespace {

using namespace rs2;

[[noreturn]] void breach(const char* what, const char* label) {
  std::fprintf(stderr, "planner_ranges_check: %s: %s\n", label, what);
  std::exit(1);
}
#define CHECK(cond)                    \
  do {                                 \
    if (!(cond)) breach(#cond, label); \
  } while (0)

const uint16_t kSizes[] = {4, 6, 62, 64, 66, 126, 128, 130, 254, 256, 258};

uint32_t k_of(uint32_t n, int axis) {
  const uint32_t f = (n - 1) / 3;
  return axis == RS2_AXIS_PRIMARY ? n - f : n - 2 * f;
}

// the k shards that stay when r cyclically consecutive ones from `a` on are gone
std::vector<uint16_t> burst(uint32_t k, uint32_t n, uint32_t a) {
  std::vector<uint8_t> gone(n, 0);
  for (uint32_t j = 0; j < n - k; ++j) gone[(a + j) % n] = 1;
  std::vector<uint16_t> out;
  for (uint32_t q = 0; q < n; ++q)
    if (!gone[q]) out.push_back(uint16_t(q));
  return out;
}

// A chunk list against the rule restated: classes by C in order of first appearance, each class
// in order, cut before the budget or the grid would be passed; tile prefixes exact.
void check_cut(const char* label, const std::vector<ChunkJob>& jobs, int64_t lines, size_t budget,
               const std::vector<RangeChunk>& chunks, const std::vector<uint32_t>& demoted) {
  std::set<uint32_t> seen(demoted.begin(), demoted.end());
  std::vector<int> class_order;
  for (size_t c = 0; c < chunks.size(); ++c) {
    const RangeChunk& ch = chunks[c];
    CHECK(!ch.members.empty() && ch.tiles.size() == ch.members.size() + 1 && ch.tiles[0] == 0);
    if (class_order.empty() || class_order.back() != ch.C) {
      CHECK(std::find(class_order.begin(), class_order.end(), ch.C) == class_order.end());
      class_order.push_back(ch.C);
    }
    size_t tab = 0;
    for (size_t m = 0; m < ch.members.size(); ++m) {
      const uint32_t i = ch.members[m];
      const ChunkJob& j = jobs[i];
      CHECK(j.eligible && j.C == ch.C && seen.insert(i).second);
      if (m) CHECK(ch.members[m - 1] < i);
      const uint64_t t = (uint64_t(lines) * uint64_t(j.pairs_span) + 63) / 64;
      CHECK(t >= 1 && uint64_t(ch.tiles[m + 1]) - ch.tiles[m] == t);
      tab += j.n_logs * kTabU16 * 2;
    }
    CHECK(ch.tiles.back() <= 0x7FFFFFFFu);
    CHECK(ch.members.size() == 1 || tab <= budget);
    // the next chunk of the class starts with the job this one could not take
    if (c + 1 < chunks.size() && chunks[c + 1].C == ch.C) {
      const ChunkJob& nx = jobs[chunks[c + 1].members[0]];
      const uint64_t t = (uint64_t(lines) * uint64_t(nx.pairs_span) + 63) / 64;
      CHECK(tab + nx.n_logs * kTabU16 * 2 > budget || ch.tiles.back() + t > 0x7FFFFFFFu);
      CHECK(ch.members.back() < chunks[c + 1].members[0]);
    }
  }
  std::vector<int> first_seen;
  for (const ChunkJob& j : jobs)
    if (j.eligible && std::find(first_seen.begin(), first_seen.end(), j.C) == first_seen.end())
      first_seen.push_back(j.C);
  for (int C : class_order) CHECK(std::find(first_seen.begin(), first_seen.end(), C) != first_seen.end());
  for (uint32_t i = 0; i < jobs.size(); ++i) CHECK(seen.count(i) == (jobs[i].eligible ? 1u : 0u));
}

// Real jobs: every size on both axes, `per` burst patterns per group, planned as the engine plans
// a window (sliver_recover_spec, plan_decode, batch_eligible, finish_plan, pack_batch_job).
void real_case(uint32_t n, uint32_t per) {
  char label[96];
  std::snprintf(label, sizeof label, "real n=%u per=%u", n, per);
  SliverAxisCode codes[2];
  for (int a = 0; a < 2; ++a) CHECK(plan_sliver_axis(n, a, codes[a]) == RS2_OK);
  std::vector<uint8_t> axis;
  std::vector<uint16_t> size, idx;
  std::vector<uint32_t> counts;
  std::vector<uint64_t> s_off, o_off;
  uint64_t sa = 0, oa = 0;
  uint32_t q = 0;
  for (uint32_t rep = 0; rep < per; ++rep)
    for (uint16_t s : kSizes)
      for (uint8_t a = 0; a < 2; ++a, ++q) {
        const uint32_t k = k_of(n, a);
        std::vector<uint16_t> pat = burst(k, n, (q * 7) % n);
        if (q % 2) std::reverse(pat.begin(), pat.end());
        axis.push_back(a);
        size.push_back(s);
        counts.push_back(k);
        idx.insert(idx.end(), pat.begin(), pat.end());
        s_off.push_back(sa);
        o_off.push_back(oa);
        sa += uint64_t(k) * s + 2;
        oa += uint64_t(k) * s + 6;
      }
  const uint32_t m = uint32_t(axis.size());
  std::vector<MixedRecoverItem> items;
  SliverGroupsPlan plan;
  CHECK(plan_recover_mixed(codes, m, axis.data(), size.data(), counts.data(), idx.data(),
                           s_off.data(), o_off.data(), uint64_t(256) << 20, 256, 341, nullptr, items,
                           plan) == RS2_OK);
  CHECK(items.size() == m && plan.accepted == m && plan.windows.size() == (m + 340) / 341);
  static uint8_t mem[16];
  std::vector<ChunkJob> geo(m);
  std::set<int> classes;
  uint32_t batched = 0;
  for (uint32_t i = 0; i < m; ++i) {
    CHECK(items[i].slot == i && items[i].chosen.size() == k_of(n, axis[i]));
    DecodeSpec sp;
    sliver_recover_spec(k_of(n, axis[i]), n, size[i], items[i].chosen, mem, mem, true, sp);
    uint32_t originals = 0;
    for (uint32_t x = 0; x < sp.K; ++x) originals += sp.present[x] >= 0;
    geo[i] = {false, 1, 0, 0};
    if (originals == sp.K) continue;
    PlannedJob pj;
    CHECK(plan_decode(sp, pj) == RS2_OK);
    const bool fused = sp.copy_present && copy_covered(pj);
    if (!batch_eligible(pj, fused) || (originals > 0 && !fused)) continue;
    finish_plan(pj);
    CodecJobBatch job;
    std::vector<uint16_t> mix;
    pack_batch_job(pj, job, mix);
    CHECK(job.symbol_size == size[i] && job.n_pairs == (size[i] + 3) / 4);
    CHECK(job.pairs_span == ((job.n_pairs + 1) & ~1));
    geo[i] = {true, pj.C, job.pairs_span, pj.pre_logs.size() + pj.post_logs.size()};
    classes.insert(pj.C);
    ++batched;
  }
  std::vector<RangeChunk> chunks;
  std::vector<uint32_t> demoted;
  cut_range_chunks(geo, 1, size_t(256) << 20, chunks, demoted);
  check_cut(label, geo, 1, size_t(256) << 20, chunks, demoted);
  CHECK(demoted.empty() && classes.size() <= 2 && chunks.size() == classes.size());
  // 256 bytes: one tile; 258: two; 254: one (64 pairs, the last half filled)
  for (uint32_t i = 0; i < m; ++i) {
    if (!geo[i].eligible) continue;
    const uint64_t t = (uint64_t(geo[i].pairs_span) + 63) / 64;
    CHECK(t == (size[i] > 256 ? 2u : 1u));
  }
  std::printf("real n=%u slivers=%u batched=%u classes=%zu launches=%zu\n", n, m, batched,
              classes.size(), chunks.size());
}

void synthetic_cuts() {
  const char* label = "synthetic";
  std::vector<RangeChunk> chunks;
  std::vector<uint32_t> demoted;
  // pairs_span on both sides of a tile edge, two classes interleaved, ineligible jobs between
  std::vector<ChunkJob> jobs;
  const int64_t spans[] = {2, 62, 64, 66, 126, 128, 130, 4094, 4096, 4098};
  for (int64_t sp : spans) {
    jobs.push_back({true, 64, sp, 10});
    jobs.push_back({false, 64, sp, 10});
    jobs.push_back({true, 512, sp, 10});
  }
  cut_range_chunks(jobs, 1, size_t(1) << 30, chunks, demoted);
  check_cut(label, jobs, 1, size_t(1) << 30, chunks, demoted);
  CHECK(chunks.size() == 2 && chunks[0].C == 64 && chunks[1].C == 512 && demoted.empty());
  const uint32_t want[] = {0, 1, 2, 3, 5, 7, 9, 12, 76, 140, 205};
  CHECK(chunks[0].tiles == std::vector<uint32_t>(want, want + 11) && chunks[1].tiles == chunks[0].tiles);
  std::printf("edges classes=%zu tiles=%u\n", chunks.size(), chunks[0].tiles.back());
  // several lines per job: ceil(lines * pairs_span / 64)
  cut_range_chunks(jobs, 3, size_t(1) << 30, chunks, demoted);
  check_cut(label, jobs, 3, size_t(1) << 30, chunks, demoted);
  CHECK(chunks[0].tiles[1] == 1 && chunks[0].tiles[2] - chunks[0].tiles[1] == 3 &&
        chunks[0].tiles[4] - chunks[0].tiles[3] == 4);
  // the table budget: 256 bytes per log; a job above the budget forms a chunk of its own
  jobs.clear();
  for (size_t logs : {4u, 4u, 4u, 40u, 4u, 4u, 1u, 8u}) jobs.push_back({true, 8, 8, logs});
  const size_t budget = 8 * kTabU16 * 2;
  cut_range_chunks(jobs, 1, budget, chunks, demoted);
  check_cut(label, jobs, 1, budget, chunks, demoted);
  std::vector<size_t> sizes;
  for (const RangeChunk& ch : chunks) sizes.push_back(ch.members.size());
  CHECK((sizes == std::vector<size_t>{2, 1, 1, 2, 1, 1}));
  std::printf("budget chunks=%zu\n", chunks.size());
  // the grid: 2^31 - 1 tiles per launch; a job that alone exceeds it is demoted
  jobs.clear();
  const int64_t lines = int64_t(1) << 24;  // 2^24 lines of 4096 pairs: 2^30 tiles per job
  jobs.push_back({true, 8, 4096, 1});
  jobs.push_back({true, 8, 4096 - 64, 1});  // 2^30 - 2^24 tiles: the two stay below 2^31
  jobs.push_back({true, 8, 4096, 1});       // would pass it: a new launch
  jobs.push_back({true, 8, 8192, 1});       // 2^31 tiles alone
  jobs.push_back({true, 8, 4096 - 64, 1});
  jobs.push_back({true, 8, 4096, 1});       // 2^31 with the two before it: a third launch
  cut_range_chunks(jobs, lines, size_t(1) << 30, chunks, demoted);
  check_cut(label, jobs, lines, size_t(1) << 30, chunks, demoted);
  CHECK(chunks.size() == 3 && chunks[0].members.size() == 2 && chunks[1].members.size() == 2);
  CHECK(chunks[0].tiles.back() == (1u << 31) - (1u << 24) && chunks[1].tiles.back() == chunks[0].tiles.back());
  CHECK(chunks[2].tiles.back() == 1u << 30);
  CHECK(demoted == std::vector<uint32_t>{3});
  std::printf("grid chunks=%zu demoted=%zu\n", chunks.size(), demoted.size());
}

void validation_and_windows() {
  const char* label = "validation";
  const uint32_t n = 13;
  SliverAxisCode codes[2];
  for (int a = 0; a < 2; ++a) CHECK(plan_sliver_axis(n, a, codes[a]) == RS2_OK);
  const uint32_t ks = k_of(n, 0);
  // sliver i breaks rule i and every later one it can: the order of the checks decides its code
  struct Bad {
    uint8_t axis;
    uint16_t s;
    uint64_t sym_off, out_off;
    std::vector<uint16_t> idx;
    int code;
  };
  std::vector<uint16_t> good(ks), shorter(ks - 1, 0), dup(ks + 1, 0), past(ks, uint16_t(n));
  for (uint32_t i = 0; i < ks; ++i) good[i] = uint16_t(n - 1 - i);
  const std::vector<Bad> bad = {
      {2, 5, 1, 1, shorter, RS2_E_INVALID_ARGUMENT},
      {0, 5, 1, 1, shorter, RS2_E_INCOMPATIBLE_PARAMETERS},
      {0, 0, 1, 1, shorter, RS2_E_INCOMPATIBLE_PARAMETERS},
      {0, 6, 1, 0, shorter, RS2_E_INVALID_ARGUMENT},
      {0, 6, 0, 1, shorter, RS2_E_INVALID_ARGUMENT},
      {0, 6, 0, 0, shorter, RS2_E_DECODING_UNSUCCESSFUL},
      {0, 6, 0, 0, dup, RS2_E_NOT_ENOUGH_SHARDS},
      {0, 6, 0, 0, past, RS2_E_NOT_ENOUGH_SHARDS},
  };
  std::vector<uint8_t> axis;
  std::vector<uint16_t> size, idx;
  std::vector<uint32_t> counts;
  std::vector<uint64_t> s_off, o_off;
  auto push = [&](uint8_t a, uint16_t s, uint64_t so, uint64_t oo, const std::vector<uint16_t>& ix) {
    axis.push_back(a);
    size.push_back(s);
    s_off.push_back(so);
    o_off.push_back(oo);
    counts.push_back(uint32_t(ix.size()));
    idx.insert(idx.end(), ix.begin(), ix.end());
  };
  push(0, 6, 0, 0, good);
  for (const Bad& b : bad) push(b.axis, b.s, b.sym_off, b.out_off, b.idx);
  push(0, 8, 100, 200, good);
  const uint32_t m = uint32_t(axis.size());
  std::vector<int> status(m, 99);
  std::vector<MixedRecoverItem> items;
  SliverGroupsPlan plan;
  CHECK(plan_recover_mixed(codes, m, axis.data(), size.data(), counts.data(), idx.data(),
                           s_off.data(), o_off.data(), 1 << 20, 256, 341, status.data(), items,
                           plan) == RS2_OK);
  CHECK(status[0] == RS2_OK && status[m - 1] == RS2_OK && plan.accepted == 2 && items.size() == 2);
  for (size_t i = 0; i < bad.size(); ++i) CHECK(status[i + 1] == bad[i].code);
  CHECK(items[0].slot == 0 && items[1].slot == m - 1 && items[1].first == idx.size() - ks);
  CHECK(plan.windows.size() == 1 && plan.windows[0].count == m && plan.windows[0].n_slots == 2);
  // status_out null: the first failing sliver's code
  CHECK(plan_recover_mixed(codes, m, axis.data(), size.data(), counts.data(), idx.data(),
                           s_off.data(), o_off.data(), 1 << 20, 256, 341, nullptr, items,
                           plan) == RS2_E_INVALID_ARGUMENT);
  for (size_t i = 0; i < bad.size(); ++i) {
    const size_t at = i + 1;
    size_t first = 0;
    for (size_t q = 0; q < at; ++q) first += counts[q];
    CHECK(plan_recover_mixed(codes, 1, &axis[at], &size[at], &counts[at], idx.data() + first,
                             &s_off[at], &o_off[at], 1 << 20, 256, 341, nullptr, items,
                             plan) == bad[i].code);
  }
  // whole-call refusals
  CHECK(plan_recover_mixed(codes, 65536, axis.data(), size.data(), counts.data(), idx.data(), nullptr,
                           nullptr, 1, 256, 341, nullptr, items, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_recover_mixed(codes, m, nullptr, size.data(), counts.data(), idx.data(), nullptr,
                           nullptr, 1, 256, 341, nullptr, items, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_recover_mixed(codes, m, axis.data(), size.data(), nullptr, idx.data(), nullptr, nullptr,
                           1, 256, 341, nullptr, items, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_recover_mixed(codes, m, axis.data(), size.data(), counts.data(), nullptr, nullptr,
                           nullptr, 1, 256, 341, nullptr, items, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_recover_mixed(codes, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 256,
                           341, nullptr, items, plan) == RS2_OK);
  std::printf("refusals ok\n");

  // windows: `count` slivers of sizes 2, 4, ... (all distinct up to `distinct`), one axis
  label = "windows";
  auto windows_of = [&](uint32_t count, uint32_t distinct, uint64_t budget, uint32_t max_groups,
                        uint32_t max_slivers) {
    axis.assign(count, 0);
    size.clear();
    counts.assign(count, ks);
    idx.clear();
    for (uint32_t i = 0; i < count; ++i) {
      size.push_back(uint16_t(2 * (i % distinct + 1)));
      idx.insert(idx.end(), good.begin(), good.end());
    }
    CHECK(plan_recover_mixed(codes, count, axis.data(), size.data(), counts.data(), idx.data(),
                             nullptr, nullptr, budget, max_groups, max_slivers, nullptr, items,
                             plan) == RS2_OK);
    uint32_t next = 0;
    for (const SliverWindow& w : plan.windows) {
      CHECK(w.first == next && w.count >= 1 && w.n_slots == w.count);
      CHECK(w.groups.size() <= max_groups && w.count <= max_slivers);
      next += w.count;
    }
    CHECK(next == count);
    return plan.windows.size();
  };
  CHECK(windows_of(40, 40, 1, 256, 341) == 40);                       // a budget of one sliver
  CHECK(windows_of(40, 1, 2 * sliver_scratch_bytes(n, 2), 256, 341) == 20);
  CHECK(windows_of(300, 300, uint64_t(1) << 40, 256, 341) == 2);      // the 257th group
  CHECK(plan.windows[0].count == 256 && plan.windows[0].groups.size() == 256);
  CHECK(windows_of(700, 5, uint64_t(1) << 40, 256, 341) == 3);        // the 342nd sliver
  CHECK(plan.windows[0].count == 341 && plan.windows[1].count == 341 && plan.windows[2].count == 18);
  std::printf("windows ok\n");
}

}  // namespace

int main() {
  for (uint32_t n : {10u, 13u, 100u, 1000u}) real_case(n, n == 1000 ? 1 : 3);
  real_case(100, 20);  // 440 slivers: two windows
  synthetic_cuts();
  validation_and_windows();
  return 0;
}
