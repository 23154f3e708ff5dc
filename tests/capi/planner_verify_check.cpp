// CPU driver of the verified-decode-batch half of the planner (walrus_amd/csrc/rs2_planner.h:
// verify_rows, verify_windows), built from the planner sources alone with the host compiler by
// tests/test_verify_plan.py, which writes the cases to stdin and compares every answer with its
// own restatement of the rules.  One line in, one line out:
//   rows K_p K_s s axis blob_len pulled idx[0] .. idx[pulled-1]   ->  "rows" then row:valid ...
//   windows budget max_blobs count need[0] .. need[count-1]       ->  "windows" then the ends
// A malformed line exits non-zero.
#include "../../walrus_amd/csrc/rs2_planner.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main() {
  using namespace rs2;
  std::string line;
  size_t n_lines = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "rows") {
      uint32_t kp = 0, ks = 0, s = 0, pulled = 0;
      int axis = 0;
      uint64_t blob_len = 0;
      in >> kp >> ks >> s >> axis >> blob_len >> pulled;
      std::vector<uint16_t> idx(pulled);
      for (uint32_t i = 0; i < pulled; ++i) {
        uint32_t v = 0;
        in >> v;
        idx[i] = uint16_t(v);
      }
      if (!in) return 2;
      std::vector<VerifyRow> rows(3, VerifyRow{7, 7});  // stale content must go
      verify_rows(kp, ks, s, axis, idx.data(), pulled, blob_len, rows);
      std::printf("rows");
      for (const VerifyRow& r : rows) std::printf(" %u:%u", r.row, r.valid);
      std::printf("\n");
    } else if (what == "windows") {
      uint64_t budget = 0;
      size_t max_blobs = 0, count = 0;
      in >> budget >> max_blobs >> count;
      std::vector<uint64_t> need(count);
      for (size_t i = 0; i < count; ++i) in >> need[i];
      if (!in) return 2;
      std::vector<uint32_t> ends(2, 9u);
      verify_windows(need, budget, max_blobs, ends);
      std::printf("windows");
      for (uint32_t e : ends) std::printf(" %u", e);
      std::printf("\n");
    } else {
      return 2;
    }
    ++n_lines;
  }
  std::fprintf(stderr, "planner_verify_check: %zu lines\n", n_lines);
  return 0;
}
