// The planner's span rule on the CPU (walrus_amd/csrc/rs2_planner.cpp: finish_plan,
// sliver_pairs_span), built from the planner sources alone with the host compiler by
// tests/test_planner_span.py.  It reads one call description per line from the file named on its
// command line -- the calls of tests/test_gpu_far_1_codec1d.py and the (axis, symbol size) groups
// of tests/test_gpu_far_2_slivers.py, written out by the test -- plans each the way the entry
// points do and prints the pairs_span the kernels would be launched with:
//
//   enc K R s src_sym_stride src_line_stride dst_sym_stride dst_line_stride
//       plan_encode + finish_plan (rs2_codec_encode_device_async)
//   dec K R s src_line_stride out_sym_stride out_line_stride out_limit m q0 off0 q1 off1 ...
//       plan_decode (+ copy_covered) + finish_plan (rs2_codec_decode_device_async / run_decode);
//       with every source symbol present no codec job is planned: "copy"
//   grp n axis s
//       plan_sliver_axis + plan_sliver_groups of one sliver
//
// Output: "<line number> span=<pairs_span> pairs=<n_pairs> max_ls=<largest line stride>" (or
// "<line number> copy").  A refused plan exits non-zero.
#include "../../walrus_amd/csrc/rs2_planner.h"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

namespace {

using namespace rs2;

[[noreturn]] void breach(const char* what, size_t line) {
  std::fprintf(stderr, "planner_span_check: line %zu: %s\n", line, what);
  std::exit(1);
}
#define CHECK(cond)                  \
  do {                               \
    if (!(cond)) breach(#cond, at);  \
  } while (0)

int64_t max_line_stride(const PlannedJob& pj) {
  int64_t m = std::max<int64_t>(pj.copy_ls, 0);
  for (int b = 0; b < pj.job.n_in; ++b) m = std::max(m, std::abs(pj.job.in[b].line_stride));
  for (int o = 0; o < pj.job.n_out; ++o) m = std::max(m, std::abs(pj.job.out[o].line_stride));
  return m;
}

void report(size_t at, const PlannedJob& pj) {
  std::printf("%zu span=%" PRId64 " pairs=%d max_ls=%" PRId64 "\n", at, int64_t(pj.job.pairs_span),
              int(pj.job.n_pairs), max_line_stride(pj));
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: planner_span_check CASES\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  if (!in) {
    std::fprintf(stderr, "planner_span_check: cannot read %s\n", argv[1]);
    return 2;
  }
  // nothing is dereferenced by the planner: the bases only have to be distinct and aligned
  static uint8_t src_mem[16], dst_mem[16];
  std::string text;
  size_t at = 0;
  while (std::getline(in, text)) {
    ++at;
    std::istringstream ls(text);
    std::string op;
    ls >> op;
    if (op == "enc") {
      uint32_t K, R;
      int s;
      int64_t src_ss, src_ls, dst_ss, dst_ls;
      CHECK(bool(ls >> K >> R >> s >> src_ss >> src_ls >> dst_ss >> dst_ls));
      PlannedJob pj;
      CHECK(plan_encode(K, R, s, src_mem, src_ls, [&](uint32_t i) { return int64_t(i) * src_ss; },
                        dst_mem, dst_ls, [&](uint32_t j) { return int64_t(j) * dst_ss; }, INT64_MAX,
                        pj) == RS2_OK);
      finish_plan(pj);
      report(at, pj);
    } else if (op == "dec") {
      uint32_t K, R, m;
      int s;
      int64_t src_ls, out_ss, out_ls;
      uint64_t limit;
      CHECK(bool(ls >> K >> R >> s >> src_ls >> out_ss >> out_ls >> limit >> m));
      DecodeSpec sp;
      sp.K = K;
      sp.R = R;
      sp.symbol_size = s;
      sp.present.assign(K + R, -1);
      uint32_t got = 0, originals = 0;
      for (uint32_t i = 0; i < m; ++i) {
        uint32_t q;
        int64_t off;
        CHECK(bool(ls >> q >> off));
        if (q >= K + R || sp.present[q] >= 0 || got == K) continue;
        sp.present[q] = off;
        ++got;
        originals += q < K;
      }
      CHECK(got == K);
      if (originals == K) {
        std::printf("%zu copy\n", at);
        continue;
      }
      sp.src_base = src_mem;
      sp.src_ls = src_ls;
      sp.dst_base = dst_mem;
      sp.dst_ls = out_ls;
      sp.dst_limit = int64_t(std::min<uint64_t>(limit, uint64_t(INT64_MAX)));
      sp.dst.resize(K);
      for (uint32_t i = 0; i < K; ++i) sp.dst[i] = int64_t(i) * out_ss;
      sp.copy_present = originals > 0 && s >= 4;
      PlannedJob pj;
      CHECK(plan_decode(sp, pj) == RS2_OK);
      if (sp.copy_present) (void)copy_covered(pj);
      finish_plan(pj);
      report(at, pj);
    } else if (op == "grp") {
      uint32_t n, s;
      int axis;
      CHECK(bool(ls >> n >> axis >> s));
      SliverAxisCode codes[2];
      CHECK(plan_sliver_axis(n, 0, codes[0]) == RS2_OK && plan_sliver_axis(n, 1, codes[1]) == RS2_OK);
      const uint8_t ax = uint8_t(axis);
      const uint16_t sz = uint16_t(s);
      const uint64_t off = 0;
      SliverGroupsPlan plan;
      CHECK(plan_sliver_groups(codes, 1, &ax, &sz, &off, nullptr, nullptr, ~uint64_t(0), 256, nullptr,
                               plan) == RS2_OK);
      CHECK(plan.windows.size() == 1 && plan.windows[0].groups.size() == 1);
      const SliverGroup& g = plan.windows[0].groups[0];
      CHECK(g.eligible);
      const int64_t k = g.k, r = int64_t(n) - g.k;
      std::printf("%zu span=%d pairs=%u max_ls=%" PRId64 "\n", at, int(g.pairs_span), (s + 3) / 4,
                  std::max(k, r) * int64_t(s));
    } else {
      CHECK(op.empty());
    }
  }
  return 0;
}
