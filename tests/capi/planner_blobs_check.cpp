// CPU check of the mixed blob encode planner (walrus_amd/csrc/rs2_planner.h: plan_blob_stages,
// plan_blobs_mixed), built from the planner sources alone with the host compiler by
// tests/test_planner_blobs.py.  Per case it restates the window rule, the eligibility rule, the
// tile counts and a blob's documented extents directly and compares; one line per case, a breach
// exits non-zero.
#include "../../walrus_amd/csrc/rs2_planner.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

namespace {

using namespace rs2;

[[noreturn]] void breach(const char* what, const char* label) {
  std::fprintf(stderr, "planner_blobs_check: %s: %s\n", label, what);
  std::exit(1);
}
#define CHECK(cond)                    \
  do {                                 \
    if (!(cond)) breach(#cond, label); \
  } while (0)

const uint32_t kSizes[] = {2, 4, 6, 62, 64, 66, 126, 128, 130, 254, 256, 258};
const uint32_t kSizes1000[] = {2, 20, 66, 130};
constexpr uint32_t kWindowBlobs = RS2_ENCODE_MIXED_WINDOW_BLOBS;

struct Shape {
  uint64_t n, kp, ks;
};
Shape shape(uint32_t n) {
  const uint64_t f = (n - 1) / 3;
  return {n, n - 2 * f, n - f};
}
uint32_t symbol_size(const Shape& sh, uint64_t len) {
  const uint64_t ns = sh.kp * sh.ks;
  uint64_t sz = ((len ? len : 1) + ns - 1) / ns;
  return uint32_t((sz + 1) / 2 * 2);
}
// a length of symbol size s that ends inside a row and inside a symbol
uint64_t mid_len(const Shape& sh, uint32_t s) {
  const uint64_t lo = uint64_t(s - 2) * sh.kp * sh.ks + 1, hi = uint64_t(s) * sh.kp * sh.ks;
  uint64_t len = lo + (hi - lo) / 2;
  while (len % s == 0 || (len / s) % sh.ks == 0) ++len;
  return len;
}
std::vector<uint64_t> lengths(const Shape& sh, uint32_t s) {
  const uint64_t full = uint64_t(s) * sh.kp * sh.ks;
  std::vector<uint64_t> v = {full, full - 1, uint64_t(s - 2) * sh.kp * sh.ks + 1, mid_len(sh, s)};
  if (sh.n == 10 && s == 2) v.push_back(1);
  return v;
}

struct Call {
  std::vector<uint64_t> len, off, poff, soff;
};
// every size x its lengths, `per` blobs each; order 0 interleaved, 1 sorted by size, 2 reversed
Call make_call(const Shape& sh, const std::vector<uint32_t>& sizes, uint32_t per, int order) {
  std::vector<uint64_t> kinds;
  for (uint32_t s : sizes)
    for (uint64_t l : lengths(sh, s)) kinds.push_back(l);
  std::vector<uint64_t> seq;
  if (order == 0) {
    for (uint32_t q = 0; q < per; ++q)
      for (uint64_t l : kinds) seq.push_back(l);
  } else {
    for (uint64_t l : kinds)
      for (uint32_t q = 0; q < per; ++q) seq.push_back(l);
    if (order == 2) std::reverse(seq.begin(), seq.end());
  }
  Call c;
  uint64_t at = 0, pat = 0, sat = 0;
  for (uint64_t l : seq) {
    const uint64_t s = symbol_size(sh, l);
    c.len.push_back(l);
    c.off.push_back(at);
    c.poff.push_back(pat);
    c.soff.push_back(sat);
    at += (l + 1) / 2 * 2;  // packed back to back at 2-byte steps
    pat += sh.n * sh.ks * s + 6;
    sat += sh.n * sh.kp * s + 2;
  }
  return c;
}

int32_t span_of(uint32_t s, int64_t max_ls) {
  const int32_t np = int32_t((s + 3) / 4);
  if (64 * max_ls * int64_t(s) + 65536 >= (int64_t(1) << 31)) return (np + 63) & ~63;
  return (np + 1) & ~1;
}

// The stage templates against the documented layout of a blob's buffers, in symbols: what each
// stage reads and every symbol it can store to.
void check_stages(const char* label, const Shape& sh, const BlobStages& st) {
  const int64_t n = int64_t(sh.n), kp = int64_t(sh.kp), ks = int64_t(sh.ks);
  CHECK(st.planned);
  const int64_t want_lines[3] = {ks, kp, n - ks};
  // where a stage's outputs must land: the buffer's extent and the exact symbol set
  const int64_t out_ext[3] = {n * ks, n * kp, (n - kp) * (n - ks)};
  for (int g = 0; g < kBlobStages; ++g) {
    const BlobStageCode& c = st.stage[g];
    const PlannedJob& t = c.tmpl;
    const CodecJobBig& j = t.job;
    CHECK(int64_t(c.n_lines) == want_lines[g]);
    CHECK(c.out_extent == out_ext[g]);
    CHECK(c.max_ls == std::max(std::max(c.in_ls, c.out_ls), c.copy_ls));
    CHECK(c.n_off == size_t(j.n_in + j.n_out) * size_t(t.C));
    CHECK(t.offs.size() == c.n_off + (g == kStageColsSys && st.sys_fused ? size_t(j.n_in) * t.C : 0));
    std::set<int64_t> in_set, out_set, cp_set;
    const bool exact = n <= 100;  // the full symbol sets at the small shapes, bounds at all
    for (int64_t line = 0; line < int64_t(c.n_lines); ++line) {
      for (int b = 0; b < j.n_in; ++b)
        for (int p = 0; p < t.C; ++p) {
          const int64_t o = t.offs[t.in_off(b) + size_t(p)];
          if (p >= j.in[b].count) {
            CHECK(o < 0);
            continue;
          }
          CHECK(o >= 0);
          const int64_t at = o + line * c.in_ls;
          // cols_sys and rows read the message (primary rows < K_p), cols_rep the secondary
          // repair slivers (relative to secondary + K_s K_p)
          CHECK(at < (g == kStageColsRep ? (n - ks) * kp : kp * ks));
          if (exact) CHECK(in_set.insert(at).second);
          if (g == kStageColsSys && st.sys_fused) {
            const int64_t co = t.offs[c.n_off + size_t(b) * t.C + size_t(p)];
            CHECK(co >= 0);
            const int64_t cat = co + line * c.copy_ls;
            CHECK(cat < c.copy_extent && c.copy_extent == ks * kp);
            if (exact) CHECK(cp_set.insert(cat).second);
            // secondary sliver c, row r = primary r, column c
            CHECK(cat == (at % ks) * kp + at / ks);
          }
        }
      for (int o2 = 0; o2 < j.n_out; ++o2)
        for (int p = 0; p < t.C; ++p) {
          const int64_t o = t.offs[t.out_off(o2) + size_t(p)];
          if (p >= j.out[o2].trunc) continue;  // never stored
          if (o < 0) continue;
          const int64_t at = o + line * c.out_ls;
          CHECK(at < c.out_extent);
          // cols_sys stores primary repair rows only, rows secondary repair slivers only
          if (g == kStageColsSys) CHECK(at >= kp * ks);
          if (g == kStageRows) CHECK(at >= ks * kp);
          if (exact) CHECK(out_set.insert(at).second);
        }
    }
    if (exact) {
      const int64_t want_in[3] = {kp * ks, kp * ks, (n - ks) * kp};
      const int64_t want_out[3] = {(n - kp) * ks, (n - ks) * kp, (n - kp) * (n - ks)};
      CHECK(int64_t(in_set.size()) == want_in[g]);
      CHECK(int64_t(out_set.size()) == want_out[g]);
      if (g == kStageColsSys && st.sys_fused) CHECK(int64_t(cp_set.size()) == ks * kp);
    }
  }
}

// The properties of a plan over `call` (status: per-blob codes, or null when none was refused).
size_t check_plan(const char* label, const Shape& sh, const BlobStages& st, const Call& call,
                  const int* status, bool meta_only, uint64_t budget, uint32_t max_blobs,
                  const BlobsMixedPlan& plan, uint32_t* eligible_out) {
  const uint32_t m = uint32_t(call.len.size());
  uint32_t accepted = 0;
  for (uint32_t i = 0; i < m; ++i) accepted += !status || status[i] == RS2_OK;
  CHECK(plan.accepted == accepted);
  // the window rule restated: blobs in order, closed before the blob that would pass the budget
  // or the eligible-blob cap; refused blobs hold nothing
  std::vector<uint32_t> want_first;  // first accepted blob of each window after the first
  {
    uint64_t used = 0;
    uint32_t held = 0, held_eligible = 0;
    uint64_t tsum[3] = {0, 0, 0};
    for (uint32_t i = 0; i < m; ++i) {
      if (status && status[i] != RS2_OK) continue;
      const uint32_t s = symbol_size(sh, call.len[i]);
      const uint64_t need = (sh.n - sh.kp) * (sh.n - sh.ks) * s + 32 * sh.n * sh.n +
                            (meta_only ? sh.n * (sh.kp + sh.ks) * s : 0);
      CHECK(need == blob_scratch_bytes(uint32_t(sh.n), uint32_t(sh.kp), uint32_t(sh.ks), s, meta_only));
      if (held && (used > budget || need > budget - used || held_eligible >= max_blobs)) {
        want_first.push_back(i);
        used = 0;
        held = held_eligible = 0;
        tsum[0] = tsum[1] = tsum[2] = 0;
      }
      bool el = s >= 4 && st.batchable;
      uint64_t t[3] = {0, 0, 0};
      for (int g = 0; el && g < 3; ++g) {
        t[g] = (uint64_t(st.stage[g].n_lines) * uint64_t(span_of(s, st.stage[g].max_ls)) + 63) / 64;
        if (tsum[g] + t[g] > 0x7FFFFFFFu) el = false;
      }
      if (el)
        for (int g = 0; g < 3; ++g) tsum[g] += t[g];
      used += need;
      ++held;
      held_eligible += el;
    }
  }
  CHECK(plan.windows.size() == want_first.size() + 1);
  uint32_t next = 0, eligible_total = 0;
  std::set<uint32_t> seen;
  for (size_t wi = 0; wi < plan.windows.size(); ++wi) {
    const BlobWindow& w = plan.windows[wi];
    CHECK(w.first == next);
    CHECK(w.count >= 1);
    next += w.count;
    if (wi + 1 < plan.windows.size()) CHECK(next == want_first[wi]);
    uint32_t in_window = 0;
    for (uint32_t i = w.first; i < w.first + w.count; ++i) in_window += !status || status[i] == RS2_OK;
    CHECK(w.slots.size() == in_window);
    CHECK(in_window >= 1 || accepted == 0 || wi + 1 == plan.windows.size());
    CHECK(w.n_eligible <= w.slots.size() && w.n_eligible <= max_blobs);
    uint64_t scratch = 0, both = 0, pb = 0, sb = 0;
    std::vector<uint32_t> sizes;
    for (int g = 0; g < kBlobStages; ++g) {
      CHECK(w.tiles[g].size() == size_t(w.n_eligible) + 1);
      CHECK(w.tiles[g][0] == 0);
    }
    for (size_t q = 0; q < w.slots.size(); ++q) {
      const BlobSlot& sl = w.slots[q];
      CHECK(sl.blob >= w.first && sl.blob < w.first + w.count);
      CHECK(!status || status[sl.blob] == RS2_OK);
      CHECK(seen.insert(sl.blob).second);
      CHECK(sl.s == symbol_size(sh, call.len[sl.blob]));
      CHECK(sl.eligible == (q < w.n_eligible));
      // the caller's order inside each class
      if (q && q != w.n_eligible) CHECK(w.slots[q - 1].blob < sl.blob);
      const bool want = sl.s >= 4 && st.batchable;
      CHECK(sl.eligible == want);  // (no case here reaches the 2^31 tile bound)
      scratch += blob_scratch_bytes(uint32_t(sh.n), uint32_t(sh.kp), uint32_t(sh.ks), sl.s, meta_only);
      if (!sl.eligible) continue;
      size_t c = 0;
      while (c < sizes.size() && sizes[c] != sl.s) ++c;
      if (c == sizes.size()) sizes.push_back(sl.s);
      CHECK(sl.size_class == c);
      CHECK(sl.both_off == both);
      both += (sh.n - sh.kp) * (sh.n - sh.ks) * sl.s;
      for (int g = 0; g < kBlobStages; ++g) {
        const BlobStageCode& code = st.stage[g];
        CHECK(sl.pairs_span[g] == span_of(sl.s, code.max_ls));
        CHECK(sl.pairs_span[g] % 2 == 0 && sl.pairs_span[g] >= int32_t((sl.s + 3) / 4));
        const uint64_t tiles = (uint64_t(code.n_lines) * uint64_t(sl.pairs_span[g]) + 63) / 64;
        CHECK(tiles >= 1);
        CHECK(uint64_t(w.tiles[g][q + 1]) == uint64_t(w.tiles[g][q]) + tiles);
        // the job's offsets are the template's times s, and every store it can make lies inside
        // the blob's documented extents: primary n K_s s, secondary n K_p s, quadrant
        // (n - K_p)(n - K_s) s bytes
        const uint64_t ext[3] = {sh.n * sh.ks * sl.s, sh.n * sh.kp * sl.s,
                                 (sh.n - sh.kp) * (sh.n - sh.ks) * sl.s};
        const PlannedJob& t = code.tmpl;
        const int64_t last = int64_t(code.n_lines) - 1;
        for (int o2 = 0; o2 < t.job.n_out; ++o2)
          for (int p = 0; p < t.job.out[o2].trunc; ++p) {
            const int64_t o = t.offs[t.out_off(o2) + size_t(p)];
            if (o < 0) continue;
            const uint64_t end = uint64_t(o * int64_t(sl.s) + last * code.out_ls * int64_t(sl.s)) + sl.s;
            CHECK(end <= ext[g] && end <= uint64_t(code.out_extent) * sl.s);
          }
        if (g == kStageColsSys)
          for (size_t p = code.n_off; p < t.offs.size(); ++p) {
            if (t.offs[p] < 0) continue;
            const uint64_t end =
                uint64_t(t.offs[p] * int64_t(sl.s) + last * code.copy_ls * int64_t(sl.s)) + sl.s;
            CHECK(end <= sh.ks * sh.kp * sl.s && end <= ext[1]);
          }
      }
    }
    // metadata only: the slivers of every slot, back to back in the caller's order
    if (meta_only) {
      for (uint32_t i = w.first; i < w.first + w.count; ++i)
        for (const BlobSlot& sl : w.slots)
          if (sl.blob == i) {
            CHECK(sl.primary_off == pb && sl.secondary_off == sb);
            pb += sh.n * sh.ks * sl.s;
            sb += sh.n * sh.kp * sl.s;
          }
      CHECK(w.primary_bytes == pb && w.secondary_bytes == sb);
    } else {
      CHECK(w.primary_bytes == 0 && w.secondary_bytes == 0);
    }
    CHECK(w.sizes == sizes);
    CHECK(w.both_bytes == both);
    // a window of more than one blob stays inside the budget
    if (w.slots.size() > 1) CHECK(scratch <= budget);
    eligible_total += w.n_eligible;
  }
  CHECK(next == m);
  CHECK(seen.size() == accepted);
  if (eligible_out) *eligible_out = eligible_total;
  return plan.windows.size();
}

void run_cases(uint32_t n) {
  char label[160];
  std::snprintf(label, sizeof label, "n=%u", n);
  const Shape sh = shape(n);
  BlobStages st;
  CHECK(plan_blob_stages(n, st) == RS2_OK);
  CHECK(st.n == n && st.kp == sh.kp && st.ks == sh.ks);
  check_stages(label, sh, st);
  std::vector<uint32_t> sizes;
  if (n >= 1000)
    sizes.assign(kSizes1000, kSizes1000 + 4);
  else
    sizes.assign(kSizes, kSizes + 12);
  for (uint32_t s : sizes)
    std::printf("eligible n=%u s=%u in=%d/%d/%d out=%d/%d/%d C=%d mode=%d/%d/%d fused=%d: %d\n", n, s,
                st.stage[0].tmpl.job.n_in, st.stage[1].tmpl.job.n_in, st.stage[2].tmpl.job.n_in,
                st.stage[0].tmpl.job.n_out, st.stage[1].tmpl.job.n_out, st.stage[2].tmpl.job.n_out,
                st.stage[0].tmpl.C, st.stage[0].tmpl.mode, st.stage[1].tmpl.mode,
                st.stage[2].tmpl.mode, int(st.sys_fused), int(s >= 4 && st.batchable));
  const uint32_t smax = sizes.back();
  for (uint32_t per : {1u, 5u})
    for (int order = 0; order < 3; ++order)
      for (uint32_t hold : {1u, 2u, 0u})
        for (int meta = 0; meta < 2; ++meta) {
          const Call call = make_call(sh, sizes, per, order);
          const uint32_t m = uint32_t(call.len.size());
          const uint64_t one = blob_scratch_bytes(n, st.kp, st.ks, smax, meta != 0);
          // hold 0: every blob of the largest size fits (and so every blob of the call)
          const uint64_t budget = hold ? one * hold : one * m;
          std::snprintf(label, sizeof label, "n=%u per=%u order=%d hold=%u meta=%d", n, per, order,
                        hold, meta);
          BlobsMixedPlan plan;
          CHECK(plan_blobs_mixed(st, m, call.len.data(), call.off.data(),
                                 meta ? nullptr : call.poff.data(), meta ? nullptr : call.soff.data(),
                                 nullptr, meta != 0, budget, kWindowBlobs, nullptr, plan) == RS2_OK);
          uint32_t el = 0;
          const size_t windows =
              check_plan(label, sh, st, call, nullptr, meta != 0, budget, kWindowBlobs, plan, &el);
          std::printf("n=%u sizes=%zu per=%u order=%d hold=%u meta=%d blobs=%u windows=%zu eligible=%u\n",
                      n, sizes.size(), per, order, hold, meta, m, windows, el);
        }
  // the eligible-blob cap closes windows too
  {
    const Call call = make_call(sh, sizes, 5, 0);
    const uint32_t m = uint32_t(call.len.size());
    std::snprintf(label, sizeof label, "n=%u cap=3", n);
    BlobsMixedPlan plan;
    CHECK(plan_blobs_mixed(st, m, call.len.data(), call.off.data(), call.poff.data(),
                           call.soff.data(), nullptr, false, UINT64_MAX, 3, nullptr, plan) == RS2_OK);
    uint32_t el = 0;
    const size_t windows = check_plan(label, sh, st, call, nullptr, false, UINT64_MAX, 3, plan, &el);
    std::printf("cap n=%u blobs=%u cap=3 windows=%zu eligible=%u\n", n, m, windows, el);
  }
}

void run_refusals() {
  const char* label = "refusals";
  const Shape sh = shape(10);
  BlobStages st;
  CHECK(plan_blob_stages(10, st) == RS2_OK);
  const uint64_t too_large = sh.kp * sh.ks * 0xFFFEull + 1;
  // blob:               0    1          2    3    4    5
  std::vector<uint64_t> len = {100, too_large, 300, 400, 500, 28 * 4};
  std::vector<uint64_t> off = {0, 200, 401, 800, 1300, 2000};   // blob 2: odd offset
  std::vector<uint64_t> poff = {0, 0, 0, 1001, 4000, 6000};     // blob 3: odd primary offset
  std::vector<uint64_t> soff = {0, 0, 0, 2000, 5001, 7000};     // blob 4: odd secondary offset
  const int want[6] = {RS2_OK, RS2_E_DATA_TOO_LARGE, RS2_E_INVALID_ARGUMENT, RS2_E_INVALID_ARGUMENT,
                       RS2_E_INVALID_ARGUMENT, RS2_OK};
  int status[6] = {7, 7, 7, 7, 7, 7};
  BlobsMixedPlan plan;
  CHECK(plan_blobs_mixed(st, 6, len.data(), off.data(), poff.data(), soff.data(), nullptr, false,
                         UINT64_MAX, kWindowBlobs, status, plan) == RS2_OK);
  for (int i = 0; i < 6; ++i) CHECK(status[i] == want[i]);
  Call call{len, off, poff, soff};
  check_plan(label, sh, st, call, status, false, UINT64_MAX, kWindowBlobs, plan, nullptr);
  CHECK(plan.accepted == 2 && plan.windows.size() == 1 && plan.windows[0].slots.size() == 2);
  // status_out null: the first failing blob's code, nothing planned to run
  CHECK(plan_blobs_mixed(st, 6, len.data(), off.data(), poff.data(), soff.data(), nullptr, false,
                         UINT64_MAX, kWindowBlobs, nullptr, plan) == RS2_E_DATA_TOO_LARGE);
  CHECK(plan_blobs_mixed(st, 4, len.data() + 2, off.data() + 2, poff.data() + 2, soff.data() + 2,
                         nullptr, false, UINT64_MAX, kWindowBlobs, nullptr,
                         plan) == RS2_E_INVALID_ARGUMENT);
  // metadata only: the sliver offsets are ignored (blobs 3 and 4 pass)
  CHECK(plan_blobs_mixed(st, 6, len.data(), off.data(), nullptr, nullptr, nullptr, true,
                         UINT64_MAX, kWindowBlobs, status, plan) == RS2_OK);
  CHECK(status[3] == RS2_OK && status[4] == RS2_OK && status[2] == RS2_E_INVALID_ARGUMENT &&
        status[1] == RS2_E_DATA_TOO_LARGE && plan.accepted == 4);
  // host form: a null blob of non-zero length; a null blob of length 0 is a blob
  {
    const uint8_t byte = 0;
    const uint8_t* blobs[3] = {&byte, nullptr, nullptr};
    const uint64_t hl[3] = {1, 5, 0};
    int hs[3] = {7, 7, 7};
    CHECK(plan_blobs_mixed(st, 3, hl, nullptr, nullptr, nullptr, blobs, false, UINT64_MAX,
                           kWindowBlobs, hs, plan) == RS2_OK);
    CHECK(hs[0] == RS2_OK && hs[1] == RS2_E_INVALID_ARGUMENT && hs[2] == RS2_OK);
    CHECK(plan_blobs_mixed(st, 3, hl, nullptr, nullptr, nullptr, blobs, false, UINT64_MAX,
                           kWindowBlobs, nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  }
  // an n_shards without a recovery code: every blob is refused with the plan's code
  {
    BlobStages tiny;
    CHECK(plan_blob_stages(3, tiny) == RS2_OK && !tiny.planned && !tiny.batchable);
    int ts[1] = {7};
    const uint64_t tl[1] = {10}, to[1] = {0};
    CHECK(plan_blobs_mixed(tiny, 1, tl, to, to, to, nullptr, false, UINT64_MAX, kWindowBlobs, ts,
                           plan) == RS2_OK);
    CHECK(ts[0] == RS2_E_INCOMPATIBLE_PARAMETERS && plan.accepted == 0);
  }
  // whole-call refusals
  BlobStages none;
  CHECK(plan_blob_stages(0, none) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_blobs_mixed(st, 65536, len.data(), off.data(), poff.data(), soff.data(), nullptr,
                         false, UINT64_MAX, kWindowBlobs, nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_blobs_mixed(st, 1, nullptr, off.data(), poff.data(), soff.data(), nullptr, false,
                         UINT64_MAX, kWindowBlobs, nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_blobs_mixed(st, 1, len.data(), nullptr, nullptr, nullptr, nullptr, false, UINT64_MAX,
                         kWindowBlobs, nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_blobs_mixed(st, 1, len.data(), off.data(), nullptr, soff.data(), nullptr, false,
                         UINT64_MAX, kWindowBlobs, nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_blobs_mixed(st, 1, len.data(), off.data(), poff.data(), soff.data(), nullptr, false,
                         UINT64_MAX, 0, nullptr, plan) == RS2_E_INVALID_ARGUMENT);
  CHECK(plan_blobs_mixed(st, 0, nullptr, nullptr, nullptr, nullptr, nullptr, false, UINT64_MAX,
                         kWindowBlobs, nullptr, plan) == RS2_OK);
  CHECK(plan.windows.empty() && plan.accepted == 0);
  std::printf("refusals ok\n");
}

}  // namespace

int main() {
  for (uint32_t n : {10u, 13u, 100u, 1000u, 4500u}) run_cases(n);
  run_refusals();
  return 0;
}
