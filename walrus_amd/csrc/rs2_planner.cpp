// The codec job planner (rs2_planner.h): GF(2^16) tables, encode / decode job plans.  No device
// runtime here: everything below is host arithmetic on plain structs.
//
// Reference semantics: reed-solomon-simd 3.1.0 (Cargo.lock:8813): GF tables, skew, rates --
// restated in oracle/rs2_oracle.py, mirrored here.
#include "rs2_planner.h"

#include <atomic>
#include <cstdlib>
#include <iterator>
#include <map>
#include <mutex>
#include <tuple>

namespace rs2 {

namespace {
thread_local std::string g_last_error = "ok";
}

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

const char* last_error() { return g_last_error.c_str(); }

int env_int(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}

// ---------------------------------------------------------------------------------------------
// GF(2^16) tables (reed-solomon-simd engine/tables.rs restated; see oracle/rs2_oracle.py)
// ---------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kPoly = 0x1002D;
constexpr uint16_t kCantor[16] = {0x0001, 0xACCA, 0x3C0E, 0x163E, 0xC582, 0xED2E, 0x914C, 0x4012,
                                  0x6C98, 0x10D8, 0x6A72, 0xB900, 0xFDB8, 0xFB34, 0xFF38, 0x991E};
}  // namespace

Gf::Gf() : exp(kOrder), log(kOrder), skew(kModulus) {
  std::vector<uint32_t> e(kOrder), l(kOrder);
  uint32_t state = 1;
  for (uint32_t i = 0; i < kModulus; ++i) {
    e[state] = i;
    state <<= 1;
    if (state >= kOrder) state ^= kPoly;
  }
  e[0] = kModulus;
  l[0] = 0;
  for (int i = 0; i < 16; ++i) {
    const uint32_t width = 1u << i;
    for (uint32_t j = 0; j < width; ++j) l[j + width] = l[j] ^ kCantor[i];
  }
  for (uint32_t i = 0; i < kOrder; ++i) l[i] = e[l[i]];
  for (uint32_t i = 0; i < kOrder; ++i) e[l[i]] = i;
  e[kModulus] = e[0];
  for (uint32_t i = 0; i < kOrder; ++i) {
    exp[i] = uint16_t(e[i]);
    log[i] = uint16_t(l[i]);
  }
  // skew LUT
  std::vector<uint32_t> sk(kModulus, 0);
  uint32_t temp[15];
  for (int i = 1; i < 16; ++i) temp[i - 1] = 1u << i;
  for (int m = 0; m < 15; ++m) {
    const uint32_t step = 1u << (m + 1);
    sk[(1u << m) - 1] = 0;
    for (int i = m; i < 15; ++i) {
      const uint32_t s = 1u << (i + 1);
      for (uint32_t j = (1u << m) - 1; j < s; j += step) sk[j + s] = sk[j] ^ temp[i];
    }
    temp[m] = kModulus - log[mul(temp[m], log[temp[m] ^ 1])];
    for (int i = m + 1; i < 15; ++i) temp[i] = mul(temp[i], add_mod(log[temp[i] ^ 1], temp[m]));
  }
  for (uint32_t i = 0; i < kModulus; ++i) skew[i] = log[sk[i]];
}

const Gf& gf() {
  static const Gf g;
  return g;
}

void nib_table(uint32_t log_m, bool fft_zero, uint16_t* out) {
  const Gf& g = gf();
  const bool zero = fft_zero && log_m == kModulus;
  for (uint32_t e = 0; e < uint32_t(kTabU16); ++e) {
    const uint32_t x = e < 64 ? e : (e < 96 ? (e - 64) << 6 : (e - 96) << 11);
    out[e] = zero ? 0 : uint16_t(g.mul(x, log_m));
  }
}

std::vector<uint16_t> sd_stream(int C, int sd, int ppw) {
  const Gf& g = gf();
  const int NW = C >= ppw ? C / ppw : 1, PPW = C / NW;
  std::vector<uint16_t> out;
  out.reserve(size_t(std::max(C - 1, 0)) * kTabU16);
  uint16_t t[kTabU16];
  for (int w = 0; w < NW; ++w)
    for (int d = 1; d < PPW; d *= 2)
      for (int gi = 0; gi < PPW / (2 * d); ++gi) {
        const int r = w * PPW + 2 * d * gi;
        nib_table(g.skew[r + d + sd - 1], true, t);
        out.insert(out.end(), t, t + kTabU16);
      }
  for (int d = PPW; d < C; d *= 2)
    for (int gi = 0; gi < C / (2 * d); ++gi) {
      const int r = 2 * d * gi;
      nib_table(g.skew[r + d + sd - 1], true, t);
      out.insert(out.end(), t, t + kTabU16);
    }
  return out;
}

int group0_zero(int C, int sd, int ppw) {
  const Gf& g = gf();
  const int NW = C >= ppw ? C / ppw : 1, PPW = C / NW;
  if (NW == 1) return 0;
  for (int d = PPW; d < C; d *= 2)
    if (g.skew[d + sd - 1] != kModulus) return 0;
  return 1;
}

uint32_t next_pow2(uint32_t x) {
  uint32_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// reed-solomon-simd DefaultRate: high rate iff pow2(recovery) <= pow2(original)
bool use_high_rate(uint32_t k, uint32_t r) { return next_pow2(r) <= next_pow2(k); }

bool rate_supported(uint32_t k, uint32_t r) {
  if (k == 0 || r == 0 || k >= kOrder || r >= kOrder) return false;
  return std::min(next_pow2(k), next_pow2(r)) + std::max(k, r) <= kOrder;
}

namespace {
std::atomic<uint32_t> g_block_max{0};
}
uint32_t block_max() {
  uint32_t v = g_block_max.load(std::memory_order_relaxed);
  if (v) return v;
  uint32_t x = uint32_t(env_int("RS2_BLOCK_MAX", kMaxC));
  if (x < 1 || x > uint32_t(kMaxC) || (x & (x - 1))) x = uint32_t(kMaxC);
  g_block_max.store(x, std::memory_order_relaxed);
  return x;
}

int max_blocks(int C) { return C == kMaxC ? kMaxBlocksBig : kMaxBlocks; }

void set_block_max(uint32_t max_block) { g_block_max.store(max_block, std::memory_order_relaxed); }

void coef_xor(Coef& y, const Coef& x) {
  for (size_t i = 0; i < y.size(); ++i) y[i] ^= x[i];
}
namespace {
void coef_mul_xor(Coef& y, const Coef& x, uint32_t log_c) {
  const Gf& g = gf();
  for (size_t i = 0; i < y.size(); ++i) y[i] ^= g.mul(x[i], log_c);
}
}  // namespace
// IFFT layers d = C .. span/2 of a size-`span` transform with skew offset sd
void sym_ifft_top(std::vector<Coef>& V, uint32_t C, uint32_t span, uint32_t sd) {
  const Gf& g = gf();
  for (uint32_t d = C; d < span; d *= 2)
    for (uint32_t r = 0; r < span; r += 2 * d) {
      const uint32_t c = g.skew[r + d + sd - 1];
      for (uint32_t j = 0; j < d / C; ++j) {
        const uint32_t x = r / C + j, y = x + d / C;
        coef_xor(V[y], V[x]);
        if (c != kModulus) coef_mul_xor(V[x], V[y], c);
      }
    }
}
// FFT layers d = span/2 .. C of a size-`span` transform with skew offset sd
void sym_fft_top(std::vector<Coef>& V, uint32_t C, uint32_t span, uint32_t sd) {
  const Gf& g = gf();
  for (uint32_t d = span / 2; d >= C && d > 0; d /= 2) {
    for (uint32_t r = 0; r < span; r += 2 * d) {
      const uint32_t c = g.skew[r + d + sd - 1];
      for (uint32_t j = 0; j < d / C; ++j) {
        const uint32_t x = r / C + j, y = x + d / C;
        if (c != kModulus) coef_mul_xor(V[x], V[y], c);
        coef_xor(V[y], V[x]);
      }
    }
    if (d == C) break;
  }
}

// Mixing kinds and tables of output block oi from its coefficient vectors (M1 may be empty).
void set_mixing(PlannedJob& pj, int oi, const Coef* m1, const Coef& m2) {
  const Gf& g = gf();
  CodecJobBig& j = pj.job;
  const size_t ms = size_t(pj.mix_stride);
  if (pj.mix.empty()) pj.mix.assign(ms * ms * 2 * kTabU16, 0);
  for (int bi = 0; bi < j.n_in; ++bi) {
    const uint32_t c1 = m1 ? (*m1)[bi] : 0u, c2 = m2[bi];
    j.m1_kind[oi][bi] = uint8_t(c1 == 0 ? 0 : (c1 == 1 ? 1 : 2));
    j.m2_kind[oi][bi] = uint8_t(c2 == 0 ? 0 : (c2 == 1 ? 1 : 2));
    uint16_t* t = pj.mix.data() + (size_t(oi) * ms + bi) * 2 * kTabU16;
    if (c1 > 1) {
      nib_table(g.log[c1], false, t);
      pj.has_mix = true;
    }
    if (c2 > 1) {
      nib_table(g.log[c2], false, t + kTabU16);
      pj.has_mix = true;
    }
  }
}

bool copy_covered(PlannedJob& pj) {
  if (pj.copy_offs.empty()) return false;
  if (pj.mode == kModeRows) {  // the mixed-encode kernel has no copy-out (register budget)
    pj.copy_offs.clear();
    return false;
  }
  const CodecJobBig& j = pj.job;
  for (int b = 0; b < j.n_in; ++b) {
    bool any_copy = false;
    for (int p = 0; p < pj.C; ++p) any_copy |= pj.copy_offs[size_t(b) * pj.C + p] >= 0;
    if (!any_copy || j.shared_in) continue;
    bool loaded = false;
    for (int o = 0; o < j.n_out; ++o)
      loaded |= j.m2_kind[o][b] != 0 || (pj.mode == kModeDecode && j.m1_kind[o][b] != 0);
    if (!loaded) {
      pj.copy_offs.clear();
      return false;
    }
  }
  return true;
}

size_t finish_plan(PlannedJob& pj) {
  CodecJobBig& j = pj.job;
  // flattened lane space: pairs rounded up to even (lane pairs share a 64-byte chunk); lines may
  // then share a workgroup, whose per-lane line step must fit the kernel's 32-bit offsets
  int64_t max_ls = std::max<int64_t>(pj.copy_ls, 0);
  for (int b = 0; b < j.n_in; ++b) max_ls = std::max(max_ls, std::abs(j.in[b].line_stride));
  for (int o = 0; o < j.n_out; ++o) max_ls = std::max(max_ls, std::abs(j.out[o].line_stride));
  j.pairs_span = (j.n_pairs + 1) & ~1;
  if (64 * max_ls + 65536 >= (int64_t(1) << 31)) j.pairs_span = (j.n_pairs + 63) & ~63;
  const size_t n_off = pj.offs.size();
  if (!pj.copy_offs.empty()) pj.offs.insert(pj.offs.end(), pj.copy_offs.begin(), pj.copy_offs.end());
  return n_off;
}

// ---------------------------------------------------------------------------------------------
// decode planning: erasure locator logs (FWHT), per-block IFFTs, block mixing matrices
// ---------------------------------------------------------------------------------------------
// XOR-convolution of the erasure indicator with LOG over the decoder's subspace of size W:
//   L[p] = sum_{e erased} LOG[p ^ e]  (mod 65535),  via FWHT (W^-1 = 2^(16 - log W)).
// Arithmetic mod 65535 on 16-bit values as reed-solomon-simd does it (65535 aliases 0): the
// FWHT butterflies are one add and one fold each, no division.
namespace {
inline uint32_t add_mod16(uint32_t a, uint32_t b) {
  const uint32_t t = a + b;
  return (t + (t >> 16)) & 0xFFFFu;
}
inline uint32_t sub_mod16(uint32_t a, uint32_t b) {
  const uint32_t d = a - b;
  return (d + (d >> 16)) & 0xFFFFu;
}
void fwht16(uint32_t* a, uint32_t W) {
  for (uint32_t h = 1; h < W; h <<= 1)
    for (uint32_t i = 0; i < W; i += 2 * h)
      for (uint32_t j = i; j < i + h; ++j) {
        const uint32_t x = a[j], y = a[j + h];
        a[j] = add_mod16(x, y);
        a[j + h] = sub_mod16(x, y);
      }
}
// FWHT of LOG over the first W entries: the same for every erasure pattern of a size, so it is
// computed once per W (reed-solomon-simd keeps the 65536-point one, LOG_WALSH, as a table)
const std::vector<uint32_t>& log_walsh(uint32_t W) {
  static std::mutex mu;
  static std::map<uint32_t, std::vector<uint32_t>> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(W);
  if (it != cache.end()) return it->second;
  const Gf& g = gf();
  std::vector<uint32_t> lg(W);
  for (uint32_t i = 0; i < W; ++i) lg[i] = g.log[i] % kModulus;  // LOG[0] = 65535 == 0
  fwht16(lg.data(), W);
  return cache.emplace(W, std::move(lg)).first->second;
}
// Erasure locator logs, the decoder's eval_poly restricted to its W-point subspace:
//   L[p] = sum_{e erased} LOG[p ^ e]  (mod 65535)  = FWHT^-1(FWHT(erased) * FWHT(LOG)),
// with FWHT^-1 = FWHT / W and 1/W = 2^(16 - log W) mod 65535 (2^16 == 1): a 16-bit rotate.
std::vector<uint32_t> erasure_logs(const std::vector<uint8_t>& erased, uint32_t W) {
  const std::vector<uint32_t>& lw = log_walsh(W);
  std::vector<uint32_t> a(W);
  for (uint32_t i = 0; i < W; ++i) a[i] = erased[i] ? 1u : 0u;
  fwht16(a.data(), W);
  for (uint32_t i = 0; i < W; ++i) {
    const uint32_t x = a[i] == 0xFFFFu ? 0u : a[i], y = lw[i] == 0xFFFFu ? 0u : lw[i];
    a[i] = x * y % kModulus;  // < 65535^2 < 2^32
  }
  fwht16(a.data(), W);
  uint32_t logW = 0;
  while ((1u << logW) < W) ++logW;
  const uint32_t k = (16 - logW) & 15;
  for (uint32_t i = 0; i < W; ++i) {
    uint32_t x = a[i] == 0xFFFFu ? 0u : a[i];
    x = ((x << k) | (x >> (16 - k))) & 0xFFFFu;  // x * 2^k mod 65535 (k = 0: x)
    a[i] = x == 0xFFFFu ? 0u : x;
  }
  return a;
}

// Block-level mixing: out block o = FFT_o( sum_b M1[o][b] Dw(X_b) + M2[o][b] X_b ).
void build_mixing_matrices(int m, uint32_t cs, uint32_t W, std::vector<std::vector<uint32_t>>& M1,
                           std::vector<std::vector<uint32_t>>& M2) {
  const Gf& g = gf();
  std::vector<std::vector<uint32_t>> Va(m, std::vector<uint32_t>(m, 0)), Vb = Va;
  for (int i = 0; i < m; ++i) Va[i][i] = 1;
  auto xor_into = [&](std::vector<uint32_t>& a, const std::vector<uint32_t>& b) {
    for (int i = 0; i < m; ++i) a[i] ^= b[i];
  };
  auto mul_into = [&](std::vector<uint32_t>& a, const std::vector<uint32_t>& b, uint32_t c) {
    for (int i = 0; i < m; ++i) a[i] ^= g.mul(b[i], c);
  };
  for (uint32_t d = cs; d < W; d *= 2)
    for (uint32_t r = 0; r < W; r += 2 * d) {
      const uint32_t c = g.skew[r + d - 1];
      for (uint32_t j = 0; j < d / cs; ++j) {
        const int x = int(r / cs + j), y = int(x + d / cs);
        xor_into(Va[y], Va[x]);
        xor_into(Vb[y], Vb[x]);
        if (c != kModulus) {
          mul_into(Va[x], Va[y], c);
          mul_into(Vb[x], Vb[y], c);
        }
      }
    }
  // formal derivative: in-block part (Dw) moves alpha to beta; cross-block bits add blocks
  std::vector<std::vector<uint32_t>> nVa(m, std::vector<uint32_t>(m, 0));
  for (int i = 0; i < m; ++i)
    for (int t = 0; (1 << t) < m; ++t)
      if (!((i >> t) & 1) && (i | (1 << t)) < m) xor_into(nVa[i], Va[i | (1 << t)]);
  Vb = Va;
  Va = nVa;
  for (uint32_t d = W / 2; d >= cs && d > 0; d /= 2) {
    for (uint32_t r = 0; r < W; r += 2 * d) {
      const uint32_t c = g.skew[r + d - 1];
      for (uint32_t j = 0; j < d / cs; ++j) {
        const int x = int(r / cs + j), y = int(x + d / cs);
        if (c != kModulus) {
          mul_into(Va[x], Va[y], c);
          mul_into(Vb[x], Vb[y], c);
        }
        xor_into(Va[y], Va[x]);
        xor_into(Vb[y], Vb[x]);
      }
    }
    if (d == cs) break;
  }
  M1 = Vb;
  M2 = Va;
}
// The matrices depend on the transform's shape only, not on the erasure pattern: built once per
// (m, cs, W) like log_walsh (a batch plans one decode per blob, on several threads).
struct MixingMatrices {
  std::vector<std::vector<uint32_t>> M1, M2;
};
const MixingMatrices& mixing_matrices(int m, uint32_t cs, uint32_t W) {
  static std::mutex mu;
  static std::map<std::tuple<int, uint32_t, uint32_t>, MixingMatrices> cache;
  std::lock_guard<std::mutex> lk(mu);
  const auto key = std::make_tuple(m, cs, W);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  MixingMatrices mm;
  build_mixing_matrices(m, cs, W, mm.M1, mm.M2);
  return cache.emplace(key, std::move(mm)).first->second;
}
}  // namespace

int plan_decode(const DecodeSpec& sp, PlannedJob& pj) {
  const uint32_t K = sp.K, R = sp.R;
  if (!rate_supported(K, R)) return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "unsupported shard count");
  const bool high = use_high_rate(K, R);
  const uint32_t cs0 = high ? next_pow2(R) : next_pow2(K);
  const uint32_t end = high ? cs0 + K : cs0 + R;
  const uint32_t W = next_pow2(end);
  // blocks of C positions over the whole W-point transform (the chunk size cs0 only fixes
  // where originals and recovery shards sit)
  const uint32_t cs = std::min(cs0, block_max());
  const int m = int(W / cs);
  pj.in_sd.clear();
  pj.out_sd.clear();
  pj.in_first.clear();
  pj.copy_offs.clear();
  pj.mix.clear();
  pj.has_mix = false;
  pj.mode = kModeDecode;
  auto opos = [&](uint32_t i) { return high ? cs0 + i : i; };
  auto rpos = [&](uint32_t j) { return high ? j : cs0 + j; };
  std::vector<uint8_t> erased(W, 0);
  std::vector<int64_t> src_at(W, -1);
  for (uint32_t i = 0; i < K; ++i) {
    if (sp.present[i] >= 0) src_at[opos(i)] = sp.present[i];
    else erased[opos(i)] = 1;
  }
  for (uint32_t j = 0; j < R; ++j) {
    if (sp.present[K + j] >= 0) src_at[rpos(j)] = sp.present[K + j];
    else erased[rpos(j)] = 1;
  }
  if (high)
    for (uint32_t p = R; p < cs0; ++p) erased[p] = 1;
  else
    for (uint32_t p = end; p < W; ++p) erased[p] = 1;
  const std::vector<uint32_t> L = erasure_logs(erased, W);
  const MixingMatrices& mm = mixing_matrices(m, cs, W);
  const std::vector<std::vector<uint32_t>>&M1 = mm.M1, &M2 = mm.M2;

  CodecJobBig& j = pj.job;
  j = CodecJobBig{};
  j.symbol_size = sp.symbol_size;
  j.n_pairs = (sp.symbol_size + 3) / 4;
  j.shared_in = 0;
  pj.C = int(cs);
  // input blocks with at least one present position
  std::vector<int> in_blocks, out_blocks;
  for (int b = 0; b < m; ++b) {
    bool any = false;
    for (uint32_t p = 0; p < cs; ++p) any |= src_at[b * cs + p] >= 0;
    if (any) in_blocks.push_back(b);
  }
  for (int b = 0; b < m; ++b) {
    bool any = false;
    for (uint32_t i = 0; i < K; ++i)
      any |= sp.present[i] < 0 && opos(i) / cs == uint32_t(b);
    if (any) out_blocks.push_back(b);
  }
  if (in_blocks.size() > size_t(max_blocks(int(cs))) || out_blocks.size() > size_t(max_blocks(int(cs))))
    return fail(RS2_E_UNSUPPORTED, "too many decode blocks");
  pj.mix_stride = std::max(in_blocks.size(), out_blocks.size()) > size_t(kMaxBlocks) ? kMaxBlocksBig
                                                                                     : kMaxBlocks;
  // Block pair (rs2_codec.hip load_ifft, CodecJob::pair_p): with one output block, an input
  // block Q mixed with M1 = 0 (coefficient 1 once folded below) and another block P whose
  // active waves (ceil(count / ppw)) fit the workgroup together run their loads and in-wave
  // IFFT layers in one pass.  Q moves to the end of the input list (the kernel's convention).
  const int ppw = std::min<int>(int(cs), kPpwTarget), nw = int(cs) / ppw;
  auto block_waves = [&](int b) {
    int count = 0;
    for (uint32_t p = 0; p < cs; ++p)
      if (src_at[b * cs + p] >= 0) count = int(p) + 1;
    return (count + ppw - 1) / ppw;
  };
  int pair_p = -1, pair_nw = 0;
  static const bool no_pair = env_int("RS2_PAIR", 1) == 0;  // A/B knob: 0 = never pair
  if (!no_pair && nw > 1 && out_blocks.size() == 1) {
    const int o = out_blocks[0];
    for (size_t qi = 0; qi < in_blocks.size() && pair_p < 0; ++qi) {
      const int q = in_blocks[qi];
      if (M1[o][q] != 0 || M2[o][q] == 0) continue;
      for (size_t pi = 0; pi < in_blocks.size(); ++pi) {
        const int p = in_blocks[pi];
        if (p == q || (M1[o][p] == 0 && M2[o][p] == 0)) continue;
        if (block_waves(p) + block_waves(q) > nw) continue;
        in_blocks.erase(in_blocks.begin() + qi);
        in_blocks.push_back(q);
        pair_p = int(std::find(in_blocks.begin(), in_blocks.end(), p) - in_blocks.begin());
        pair_nw = block_waves(p);
        break;
      }
    }
  }
  std::fill(std::begin(j.pair_p), std::end(j.pair_p), int8_t(-1));
  std::fill(std::begin(j.pair_q), std::end(j.pair_q), int8_t(-1));
  std::fill(std::begin(j.pair_nw), std::end(j.pair_nw), int8_t(0));
  if (pair_p >= 0) {
    j.pair_p[0] = int8_t(pair_p);
    j.pair_q[0] = int8_t(in_blocks.size() - 1);
    j.pair_nw[0] = int8_t(pair_nw);
  }
  j.n_in = int(in_blocks.size());
  j.n_out = int(out_blocks.size());
  pj.n_z = j.n_out;
  pj.offs.assign(size_t(j.n_in + j.n_out) * cs, -1);
  pj.pre_logs.assign(size_t(j.n_out) * j.n_in * cs, 0);
  pj.post_logs.assign(size_t(j.n_out) * cs, 0);
  pj.has_pre = pj.has_post = true;
  for (int bi = 0; bi < j.n_in; ++bi) {
    const int b = in_blocks[bi];
    InBlock& ib = j.in[bi];
    ib.base = sp.src_base;
    ib.line_stride = sp.src_ls;
    int count = 0;
    for (uint32_t p = 0; p < cs; ++p) {
      const uint32_t gp = b * cs + p;
      if (src_at[gp] >= 0) {
        pj.offs[pj.in_off(bi) + p] = src_at[gp];
        count = int(p) + 1;
      }
    }
    ib.count = count;
    pj.in_sd.push_back(int(b * cs));
    pj.in_first.push_back(uint32_t(b * cs));
  }
  if (sp.copy_present) {
    pj.copy_base = sp.dst_base;
    pj.copy_ls = sp.dst_ls;
    pj.copy_limit = sp.dst_limit;
    pj.copy_offs.assign(size_t(j.n_in) * cs, -1);
    for (int bi = 0; bi < j.n_in; ++bi)
      for (uint32_t i = 0; i < K; ++i)
        if (sp.present[i] >= 0 && opos(i) / cs == uint32_t(in_blocks[bi]))
          pj.copy_offs[size_t(bi) * cs + opos(i) % cs] = sp.dst[i];
  }
  for (int oi = 0; oi < j.n_out; ++oi) {
    const int o = out_blocks[oi];
    OutBlock& ob = j.out[oi];
    ob.base = sp.dst_base;
    ob.line_stride = sp.dst_ls;
    ob.limit = sp.dst_limit;
    int trunc = 0;
    for (uint32_t i = 0; i < K; ++i) {
      if (sp.present[i] >= 0) continue;
      const uint32_t gp = opos(i);
      if (gp / cs != uint32_t(o)) continue;
      const uint32_t p = gp % cs;
      pj.offs[pj.out_off(oi) + p] = sp.dst[i];
      pj.post_logs[size_t(oi) * cs + p] = uint16_t(kModulus - L[gp]);  // 65535 == times one
      trunc = std::max(trunc, int(p) + 1);
    }
    ob.trunc = trunc;
    pj.out_sd.push_back(int(o * cs));
    // Fold one mixing coefficient of every input block into its pre-multiplier (the decoder
    // scales each loaded symbol by exp(L[p]) anyway).  With f = M1 (or M2 when M1 is zero) and
    // X'_b = IFFT_b(f * exp(L) * in_b) = f * X_b (IFFT and Dw are GF-linear):
    //   M1 Dw(X_b) + M2 X_b = Dw(X'_b) + (M2 / M1) X'_b
    // so the block costs at most one table multiply per position instead of three.  Each output
    // block folds its own coefficients, hence per-output pre tables (CodecJob::pre_z_stride).
    const Gf& g = gf();
    Coef c1(j.n_in), c2(j.n_in);
    for (int bi = 0; bi < j.n_in; ++bi) {
      const int b = in_blocks[bi];
      c1[bi] = M1[o][b];
      c2[bi] = M2[o][b];
      const uint32_t f = c1[bi] ? c1[bi] : c2[bi];
      if (f == 0) continue;  // this output does not use the block
      const uint32_t lf = g.log[f];
      if (c1[bi]) {
        c2[bi] = c2[bi] ? g.mul(c2[bi], kModulus - lf) : 0u;
        c1[bi] = 1;
      } else {
        c2[bi] = 1;
      }
      uint16_t* pl = pj.pre_logs.data() + (size_t(oi) * j.n_in + bi) * cs;
      for (uint32_t p = 0; p < cs; ++p)
        if (src_at[b * cs + p] >= 0) pl[p] = uint16_t(Gf::add_mod(L[b * cs + p], lf));
    }
    set_mixing(pj, oi, &c1, c2);
  }
  return RS2_OK;
}

bool batch_eligible(const PlannedJob& pj, bool fused) {
  const CodecJobBig& j = pj.job;
  if (pj.mode != kModeDecode) return false;
  if (j.n_in < 1 || j.n_out < 1 || j.n_in > kBatchBlocks || j.n_out > kBatchBlocks) return false;
  if (j.symbol_size < 4) return false;
  // (plan_decode sets copy_base only under copy_present; copy_covered empties copy_offs when the
  // fused copy-out is not covered)
  const bool nothing_to_copy = pj.copy_base == nullptr && pj.copy_offs.empty();
  return nothing_to_copy || (fused && !pj.copy_offs.empty());
}

void pack_batch_job(const PlannedJob& pj, CodecJobBatch& out, std::vector<uint16_t>& mix) {
  const CodecJobBig& b = pj.job;
  constexpr int MB = kBatchBlocks;
  static_cast<CodecScalars&>(out) = static_cast<const CodecScalars&>(b);
  std::copy(b.in, b.in + MB, out.in);
  std::copy(b.out, b.out + MB, out.out);
  for (int o = 0; o < MB; ++o) {
    std::copy(b.m1_kind[o], b.m1_kind[o] + MB, out.m1_kind[o]);
    std::copy(b.m2_kind[o], b.m2_kind[o] + MB, out.m2_kind[o]);
  }
  std::copy(b.pair_p, b.pair_p + MB, out.pair_p);
  std::copy(b.pair_q, b.pair_q + MB, out.pair_q);
  std::copy(b.pair_nw, b.pair_nw + MB, out.pair_nw);
  mix.clear();
  if (!pj.has_mix) return;
  const size_t ms = size_t(pj.mix_stride), row = size_t(2) * kTabU16;
  mix.assign(size_t(b.n_out) * MB * row, 0);
  for (int o = 0; o < b.n_out; ++o)
    for (int i = 0; i < b.n_in; ++i)
      std::copy(pj.mix.begin() + (size_t(o) * ms + i) * row,
                pj.mix.begin() + (size_t(o) * ms + i + 1) * row,
                mix.begin() + (size_t(o) * MB + i) * row);
}

void cut_batch_chunks(const std::vector<ChunkJob>& jobs, size_t table_budget, ChunkCut& cut) {
  cut = ChunkCut{};
  size_t start = 0, tab_bytes = 0;  // the open chunk: members[start ..), its table bytes
  for (uint32_t i = 0; i < jobs.size(); ++i) {
    const ChunkJob& j = jobs[i];
    if (!j.eligible) continue;
    const size_t need = j.n_logs * kTabU16 * 2;
    if (cut.members.size() > start) {
      const ChunkJob& first = jobs[cut.members[start]];
      if (j.C != first.C || j.pairs_span != first.pairs_span) {
        cut.demoted.push_back(i);
        continue;
      }
      if (tab_bytes + need > table_budget) {
        cut.ends.push_back(uint32_t(cut.members.size()));
        start = cut.members.size();
        tab_bytes = 0;
      }
    }
    cut.members.push_back(i);
    tab_bytes += need;
  }
  if (cut.members.size() > start) cut.ends.push_back(uint32_t(cut.members.size()));
}

int select_recovery_symbols(uint32_t k, uint32_t n, uint32_t count, const uint16_t* idx,
                            std::vector<std::pair<uint16_t, uint32_t>>& chosen) {
  chosen.clear();
  if (count < k) return fail(RS2_E_DECODING_UNSUCCESSFUL, "fewer recovery symbols than the sliver has");
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t i = 0; i < count && chosen.size() < k; ++i) {
    const uint16_t q = idx[i];
    if (q >= n || seen[q]) continue;  // invalid indices are ignored by the crate
    seen[q] = 1;
    chosen.emplace_back(q, i);
  }
  if (chosen.size() < k) {
    chosen.clear();
    return fail(RS2_E_NOT_ENOUGH_SHARDS, "not enough shards");
  }
  return RS2_OK;
}

void sliver_recover_spec(uint32_t k, uint32_t n, int symbol_size,
                         const std::vector<std::pair<uint16_t, uint32_t>>& chosen,
                         const uint8_t* src, uint8_t* dst, bool may_fuse, DecodeSpec& sp) {
  const int64_t s = symbol_size;
  sp.K = k;
  sp.R = n - k;
  sp.symbol_size = symbol_size;
  sp.present.assign(n, -1);
  uint32_t originals = 0;
  for (const auto& c : chosen) {
    sp.present[c.first] = int64_t(c.second) * s;
    originals += c.first < k;
  }
  sp.src_base = src;
  sp.src_ls = 0;
  sp.dst_base = dst;
  sp.dst_ls = 0;
  sp.dst.resize(k);
  for (uint32_t i = 0; i < k; ++i) sp.dst[i] = int64_t(i) * s;
  sp.dst_limit = int64_t(k) * s;
  sp.copy_present = originals > 0 && symbol_size >= 4 && may_fuse;
}

void verify_rows(uint32_t kp, uint32_t ks, uint32_t s, int axis, const uint16_t* pulled_idx,
                 uint32_t pulled, uint64_t blob_len, std::vector<VerifyRow>& rows) {
  rows.clear();
  std::vector<uint8_t> verified(kp, 0);
  if (axis == RS2_AXIS_PRIMARY)
    for (uint32_t i = 0; i < pulled; ++i)
      if (pulled_idx[i] < kp) verified[pulled_idx[i]] = 1;
  const uint64_t row = uint64_t(ks) * s;
  for (uint32_t i = 0; i < kp; ++i) {
    if (verified[i]) continue;
    const uint64_t at = uint64_t(i) * row;
    rows.push_back({i, uint32_t(blob_len > at ? std::min(row, blob_len - at) : 0)});
  }
}

void verify_windows(const std::vector<uint64_t>& need, uint64_t budget, size_t max_blobs,
                    std::vector<uint32_t>& ends) {
  ends.clear();
  uint64_t used = 0;
  size_t held = 0;
  for (size_t b = 0; b < need.size(); ++b) {
    // (need[b] > budget - used, not used + need[b] > budget: the sum may wrap)
    if (held && (held == max_blobs || used > budget || need[b] > budget - used)) {
      ends.push_back(uint32_t(b));
      used = 0;
      held = 0;
    }
    used += need[b];
    ++held;
  }
  if (held) ends.push_back(uint32_t(need.size()));
}

int merkle_level_bases(uint32_t n, uint32_t* level_base, uint64_t* n_nodes) {
  uint64_t cnt = n, base = 0;
  int l = 0;
  while (cnt > 1) {
    if (l < kSymbolLevels) level_base[l] = uint32_t(base);
    cnt += cnt & 1;
    base += cnt;
    cnt /= 2;
    ++l;
  }
  for (int j = l; j < kSymbolLevels; ++j) level_base[j] = uint32_t(base);
  if (n_nodes) *n_nodes = base + cnt;
  return l;
}

int plan_symbol_requests(uint32_t n, uint32_t k, uint32_t s, uint32_t n_slivers,
                         const uint32_t* target_counts, const uint16_t* targets, int trees,
                         bool have_nodes, uint64_t budget, SymbolRequestPlan& plan) {
  plan = SymbolRequestPlan{};
  if (trees != RS2_TREES_BUILD && trees != RS2_TREES_CACHED)
    return fail(RS2_E_INVALID_ARGUMENT, "trees must be RS2_TREES_BUILD or RS2_TREES_CACHED");
  const bool build = trees == RS2_TREES_BUILD;
  if (!build && !have_nodes)
    return fail(RS2_E_INVALID_ARGUMENT, "RS2_TREES_CACHED needs the trees in d_nodes");
  if (n_slivers > 65535) return fail(RS2_E_INVALID_ARGUMENT, "more than 65535 slivers in a call");
  if (n == 0 || n > 65535 || k == 0 || k > n)
    return fail(RS2_E_INVALID_ARGUMENT, "not a sliver's code");
  if (n_slivers && !target_counts) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  uint64_t total = 0;
  for (uint32_t i = 0; i < n_slivers; ++i) {
    total += target_counts[i];
    if (total > 0x7FFFFFFFu) return fail(RS2_E_INVALID_ARGUMENT, "too many requests in a call");
  }
  if (total && !targets) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  for (uint64_t j = 0; j < total; ++j)
    if (targets[j] >= n)  // slivers.rs check_index -> RecoverySymbolError::IndexTooLarge
      return fail(RS2_E_INVALID_ARGUMENT, "target index too large");
  plan.total = total;
  plan.path_len = merkle_level_bases(n, plan.level_base, &plan.n_nodes);
  plan.per_sliver = uint64_t(n - k) * s;
  if (build) plan.per_sliver += uint64_t(n) * 32 + (have_nodes ? 0 : plan.n_nodes * 32);
  const uint64_t fit = plan.per_sliver ? budget / plan.per_sliver : 65535;
  const uint32_t per_window = uint32_t(std::min<uint64_t>(std::max<uint64_t>(fit, 1), 65535));
  plan.table.resize(size_t(total));
  uint64_t req = 0;
  for (uint32_t first = 0; first < n_slivers; first += per_window) {
    SymbolWindow w;
    w.first_sliver = first;
    w.n_slivers = std::min(per_window, n_slivers - first);
    w.first_request = req;
    for (uint32_t slot = 0; slot < w.n_slivers; ++slot) {
      const uint32_t cnt = target_counts[first + slot];
      bool expand = build && (have_nodes || cnt > 0);
      for (uint32_t q = 0; q < cnt; ++q, ++req) {
        plan.table[size_t(req)] = slot << 16 | targets[req];
        expand |= targets[req] >= k;
      }
      if (!expand) continue;
      if (!w.runs.empty() && w.runs.back().first + w.runs.back().second == slot)
        ++w.runs.back().second;
      else
        w.runs.emplace_back(slot, 1u);
    }
    w.n_requests = uint32_t(req - w.first_request);
    w.needs_codec = !w.runs.empty() && n > k;
    plan.windows.push_back(std::move(w));
  }
  return RS2_OK;
}

int plan_sliver_axis(uint32_t n_shards, int axis, SliverAxisCode& code) {
  code = SliverAxisCode{};
  if (axis != RS2_AXIS_PRIMARY && axis != RS2_AXIS_SECONDARY)
    return fail(RS2_E_INVALID_ARGUMENT, "bad axis");
  if (n_shards == 0 || n_shards > 65535) return fail(RS2_E_INVALID_ARGUMENT, "n_shards must be non-zero");
  const uint32_t f = (n_shards - 1) / 3;
  code.n = n_shards;
  code.k = axis == RS2_AXIS_PRIMARY ? n_shards - f : n_shards - 2 * f;
  code.block_max = block_max();
  if (code.k >= n_shards || !rate_supported(code.k, n_shards - code.k)) return RS2_OK;
  auto unit = [](uint32_t i) { return int64_t(i); };
  if (plan_encode(code.k, n_shards - code.k, 2, nullptr, 0, unit, nullptr, 0, unit, INT64_MAX,
                  code.tmpl) != RS2_OK)
    return RS2_OK;
  code.planned = true;
  const CodecJobBig& j = code.tmpl.job;
  code.batchable = j.n_in >= 1 && j.n_out >= 1 && j.n_in <= kBatchBlocks &&
                   j.n_out <= kBatchBlocks && n_shards <= kGroupMaxLeaves;
  if (code.batchable) pack_batch_job(code.tmpl, code.job, code.mix);
  return RS2_OK;
}

int32_t sliver_pairs_span(int32_t n_pairs, int64_t max_ls) {
  if (64 * max_ls + 65536 >= (int64_t(1) << 31)) return (n_pairs + 63) & ~63;
  return (n_pairs + 1) & ~1;
}

namespace {
// Close a window of a mixed call: order its groups (eligible primary, eligible secondary, the
// rest), give the slivers their slots and the groups their tiles and buffer offsets.
// idx / grp: the window's accepted slivers in the caller's order and their group (as opened).
void close_sliver_window(const SliverAxisCode (&codes)[2], SliverWindow& w,
                         const std::vector<uint32_t>& idx, const std::vector<uint32_t>& grp) {
  std::vector<SliverGroup>& gs = w.groups;
  const uint32_t ng = uint32_t(gs.size());
  // tiles: eligibility may still fall to the 2^31 bound of an axis' launch
  uint64_t tiles_sum[2] = {0, 0};
  for (SliverGroup& g : gs) {
    if (!g.eligible) continue;
    const int64_t k = g.k, r = int64_t(codes[g.axis].n) - k;
    g.pairs_span = sliver_pairs_span(int32_t((g.s + 3) / 4), std::max(k, r) * int64_t(g.s));
    const uint64_t t = (uint64_t(g.count) * uint64_t(g.pairs_span) + 63) / 64;
    if (tiles_sum[g.axis] + t > 0x7FFFFFFFu) {
      g.eligible = false;
      continue;
    }
    tiles_sum[g.axis] += t;
  }
  auto cls = [](const SliverGroup& g) { return g.eligible ? int(g.axis) : 2; };
  std::vector<uint32_t> order(ng), place(ng);
  for (uint32_t i = 0; i < ng; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return cls(gs[a]) < cls(gs[b]); });
  std::vector<SliverGroup> sorted(ng);
  uint32_t slot = 0;
  w.tiles[0].assign(1, 0);
  w.tiles[1].assign(1, 0);
  w.axis_first[0] = w.axis_first[1] = w.axis_groups[0] = w.axis_groups[1] = 0;
  w.gather_bytes = w.repair_bytes = 0;
  w.n_eligible_slots = 0;
  for (uint32_t p = 0; p < ng; ++p) {
    SliverGroup g = gs[order[p]];
    place[order[p]] = p;
    g.first_slot = slot;
    slot += g.count;
    g.gather_off = w.gather_bytes;
    w.gather_bytes += uint64_t(g.count) * g.k * g.s;
    if (g.eligible) {
      const uint32_t a = g.axis;
      if (w.axis_groups[a]++ == 0) w.axis_first[a] = p;
      g.first_tile = w.tiles[a].back();
      w.tiles[a].push_back(g.first_tile +
                           uint32_t((uint64_t(g.count) * uint64_t(g.pairs_span) + 63) / 64));
      g.repair_off = w.repair_bytes;
      w.repair_bytes += uint64_t(g.count) * (codes[a].n - g.k) * g.s;
      w.n_eligible_slots = slot;
    }
    sorted[p] = g;
  }
  gs = std::move(sorted);
  w.n_slots = slot;
  w.perm.assign(slot, 0);
  std::vector<uint32_t> next(ng);
  for (uint32_t p = 0; p < ng; ++p) next[p] = gs[p].first_slot;
  for (size_t i = 0; i < idx.size(); ++i) w.perm[next[place[grp[i]]]++] = idx[i];
}

// The windows of a mixed call over the slivers with ok[i] set (the caller validated them): the
// rule of plan_sliver_groups, and a window also closes before the sliver that would make it hold
// more than max_slivers accepted slivers.  `extra`: scratch a sliver holds beyond
// sliver_scratch_bytes (the mixed recovery symbols' slot-ordered trees).
void window_slivers(const SliverAxisCode (&codes)[2], uint32_t n_slivers, const uint8_t* axis,
                    const uint16_t* symbol_size, const std::vector<uint8_t>& ok, uint64_t budget,
                    uint32_t max_groups, uint32_t max_slivers, SliverGroupsPlan& plan,
                    uint64_t extra = 0) {
  const uint32_t n = codes[0].n;
  SliverWindow w;
  std::vector<uint32_t> idx, grp;
  std::map<uint32_t, uint32_t> open;  // axis << 16 | s -> group of the open window
  uint64_t used = 0;
  auto close = [&](uint32_t end) {
    w.count = end - w.first;
    close_sliver_window(codes, w, idx, grp);
    plan.windows.push_back(std::move(w));
    w = SliverWindow{};
    w.first = end;
    idx.clear();
    grp.clear();
    open.clear();
    used = 0;
  };
  for (uint32_t i = 0; i < n_slivers; ++i) {
    if (!ok[i]) continue;  // a refused sliver holds nothing: it stays in the open window
    const uint32_t s = symbol_size[i], key = uint32_t(axis[i]) << 16 | s;
    const uint64_t need = sliver_scratch_bytes(n, s) + extra;
    auto it = open.find(key);
    // (need > budget - used, not used + need > budget: the sum may wrap)
    if (i > w.first && !idx.empty() &&
        (used > budget || need > budget - used || idx.size() >= max_slivers ||
         (it == open.end() && open.size() == max_groups))) {
      close(i);
      it = open.end();
    }
    if (it == open.end()) {
      SliverGroup g;
      g.k = codes[axis[i]].k;
      g.s = s;
      g.axis = axis[i];
      g.eligible = s >= 4 && codes[axis[i]].batchable;
      it = open.emplace(key, uint32_t(w.groups.size())).first;
      w.groups.push_back(g);
    }
    ++w.groups[it->second].count;
    idx.push_back(i);
    grp.push_back(it->second);
    used += need;
  }
  close(n_slivers);
}
}  // namespace

int plan_sliver_groups(const SliverAxisCode (&codes)[2], uint32_t n_slivers, const uint8_t* axis,
                       const uint16_t* symbol_size, const uint64_t* sliver_off,
                       const uint8_t* const* slivers, const uint64_t* sliver_len, uint64_t budget,
                       uint32_t max_groups, int* status_out, SliverGroupsPlan& plan) {
  plan = SliverGroupsPlan{};
  if (n_slivers > 65535) return fail(RS2_E_INVALID_ARGUMENT, "more than 65535 slivers in a call");
  if (max_groups == 0 || codes[0].n == 0 || codes[0].n != codes[1].n)
    return fail(RS2_E_INVALID_ARGUMENT, "not a sliver's code");
  if (n_slivers == 0) return RS2_OK;
  if (!axis || !symbol_size || (!sliver_off && !(slivers && sliver_len)))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  auto check = [&](uint32_t i) -> int {
    if (axis[i] != RS2_AXIS_PRIMARY && axis[i] != RS2_AXIS_SECONDARY)
      return fail(RS2_E_INVALID_ARGUMENT, "bad axis");
    const uint32_t s = symbol_size[i];
    if (s == 0 || s % 2)
      return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "symbol_size must be a multiple of the required alignment");
    if (sliver_off && sliver_off[i] % 2)
      return fail(RS2_E_INVALID_ARGUMENT, "sliver_off[i] must be a multiple of 2 bytes");
    if (!sliver_off && (!slivers[i] || sliver_len[i] != uint64_t(codes[axis[i]].k) * s))
      return fail(RS2_E_INCORRECT_DATA_LENGTH, "sliver length does not match its axis and symbol size");
    return RS2_OK;
  };
  std::vector<uint8_t> ok(n_slivers, 0);
  for (uint32_t i = 0; i < n_slivers; ++i) {
    const int rc = check(i);
    if (status_out) status_out[i] = rc;
    else if (rc != RS2_OK) return rc;
    ok[i] = rc == RS2_OK;
    plan.accepted += ok[i];
  }
  window_slivers(codes, n_slivers, axis, symbol_size, ok, budget, max_groups, UINT32_MAX, plan);
  return RS2_OK;
}

void cut_range_chunks(const std::vector<ChunkJob>& jobs, int64_t lines, size_t table_budget,
                      std::vector<RangeChunk>& chunks, std::vector<uint32_t>& demoted) {
  chunks.clear();
  demoted.clear();
  constexpr uint64_t kGrid = 0x7FFFFFFFu;
  std::vector<int> classes;  // C values in the order of first appearance
  for (const ChunkJob& j : jobs)
    if (j.eligible && std::find(classes.begin(), classes.end(), j.C) == classes.end())
      classes.push_back(j.C);
  for (int C : classes) {
    RangeChunk ch;
    size_t tab_bytes = 0;
    auto flush = [&] {
      if (!ch.members.empty()) chunks.push_back(std::move(ch));
      ch = RangeChunk{};
      tab_bytes = 0;
    };
    for (uint32_t i = 0; i < jobs.size(); ++i) {
      const ChunkJob& j = jobs[i];
      if (!j.eligible || j.C != C) continue;
      const uint64_t t = (uint64_t(lines) * uint64_t(j.pairs_span) + 63) / 64;
      if (t < 1 || t > kGrid) {
        demoted.push_back(i);
        continue;
      }
      const size_t need = j.n_logs * kTabU16 * 2;
      if (!ch.members.empty() && (tab_bytes + need > table_budget || ch.tiles.back() + t > kGrid))
        flush();
      if (ch.members.empty()) {
        ch.C = C;
        ch.tiles.assign(1, 0);
      }
      ch.members.push_back(i);
      ch.tiles.push_back(uint32_t(ch.tiles.back() + t));
      tab_bytes += need;
    }
    flush();
  }
  std::sort(demoted.begin(), demoted.end());
}

int plan_recover_mixed(const SliverAxisCode (&codes)[2], uint32_t n_slivers, const uint8_t* axis,
                       const uint16_t* symbol_size, const uint32_t* counts,
                       const uint16_t* symbol_idx, const uint64_t* symbols_off,
                       const uint64_t* sliver_off, uint64_t budget, uint32_t max_groups,
                       uint32_t max_slivers, int* status_out, std::vector<MixedRecoverItem>& items,
                       SliverGroupsPlan& plan) {
  plan = SliverGroupsPlan{};
  items.clear();
  if (n_slivers > 65535) return fail(RS2_E_INVALID_ARGUMENT, "more than 65535 slivers in a call");
  if (max_groups == 0 || max_slivers == 0 || codes[0].n == 0 || codes[0].n != codes[1].n)
    return fail(RS2_E_INVALID_ARGUMENT, "not a sliver's code");
  const uint32_t n = codes[0].n;
  if (codes[0].k >= n || codes[1].k >= n)
    return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "no repair symbols");
  if (n_slivers == 0) return RS2_OK;
  if (!axis || !symbol_size || !counts) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  uint64_t total = 0;
  for (uint32_t i = 0; i < n_slivers; ++i) total += counts[i];
  if (total && !symbol_idx) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  items.reserve(n_slivers);
  std::vector<uint8_t> ok(n_slivers, 0);
  uint64_t first = 0;
  for (uint32_t i = 0; i < n_slivers; first += counts[i], ++i) {
    MixedRecoverItem it;
    it.slot = i;
    it.first = first;
    auto check = [&]() -> int {
      if (axis[i] != RS2_AXIS_PRIMARY && axis[i] != RS2_AXIS_SECONDARY)
        return fail(RS2_E_INVALID_ARGUMENT, "bad axis");
      const uint32_t s = symbol_size[i];
      if (s == 0 || s % 2)
        return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "symbol_size must be a multiple of the required alignment");
      if (symbols_off && symbols_off[i] % 2)
        return fail(RS2_E_INVALID_ARGUMENT, "symbols_off[i] must be a multiple of 2 bytes");
      if (sliver_off && sliver_off[i] % 2)
        return fail(RS2_E_INVALID_ARGUMENT, "sliver_off[i] must be a multiple of 2 bytes");
      return select_recovery_symbols(codes[axis[i]].k, n, counts[i], symbol_idx + first, it.chosen);
    };
    const int rc = check();
    if (status_out) status_out[i] = rc;
    else if (rc != RS2_OK) return rc;
    if (rc != RS2_OK) continue;
    ok[i] = 1;
    ++plan.accepted;
    items.push_back(std::move(it));
  }
  window_slivers(codes, n_slivers, axis, symbol_size, ok, budget, max_groups, max_slivers, plan);
  return RS2_OK;
}

int plan_symbols_mixed(const SliverAxisCode (&codes)[2], uint32_t n_slivers, const uint8_t* axis,
                       const uint16_t* symbol_size, const uint64_t* sliver_off,
                       const uint64_t* symbols_off, const uint8_t* const* slivers,
                       const uint64_t* sliver_len, const uint32_t* target_counts,
                       const uint16_t* targets, int trees, bool have_nodes, uint64_t budget,
                       uint32_t max_groups, int* status_out, SymbolsMixedPlan& plan) {
  plan = SymbolsMixedPlan{};
  if (trees != RS2_TREES_BUILD && trees != RS2_TREES_CACHED)
    return fail(RS2_E_INVALID_ARGUMENT, "trees must be RS2_TREES_BUILD or RS2_TREES_CACHED");
  const bool build = trees == RS2_TREES_BUILD;
  if (!build && !have_nodes)
    return fail(RS2_E_INVALID_ARGUMENT, "RS2_TREES_CACHED needs the trees in d_nodes");
  if (n_slivers > 65535) return fail(RS2_E_INVALID_ARGUMENT, "more than 65535 slivers in a call");
  if (max_groups == 0 || codes[0].n == 0 || codes[0].n != codes[1].n)
    return fail(RS2_E_INVALID_ARGUMENT, "not a sliver's code");
  const uint32_t n = codes[0].n;
  plan.path_len = merkle_level_bases(n, plan.level_base, &plan.n_nodes);
  if (n_slivers == 0) return RS2_OK;
  if (!axis || !symbol_size || !target_counts || (slivers != nullptr) != (sliver_len != nullptr))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  uint64_t total = 0;
  for (uint32_t i = 0; i < n_slivers; ++i) {
    total += target_counts[i];
    if (total > 0x7FFFFFFFu) return fail(RS2_E_INVALID_ARGUMENT, "too many requests in a call");
  }
  if (total && !targets) return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  plan.total = total;
  std::vector<uint8_t> ok(n_slivers, 0);
  std::vector<uint32_t> first_req(n_slivers + 1, 0);
  for (uint32_t i = 0; i < n_slivers; ++i) {
    first_req[i + 1] = first_req[i] + target_counts[i];
    auto check = [&]() -> int {
      if (axis[i] != RS2_AXIS_PRIMARY && axis[i] != RS2_AXIS_SECONDARY)
        return fail(RS2_E_INVALID_ARGUMENT, "bad axis");
      const uint32_t s = symbol_size[i];
      if (s == 0 || s % 2)
        return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "symbol_size must be a multiple of the required alignment");
      if (sliver_off && sliver_off[i] % 2)
        return fail(RS2_E_INVALID_ARGUMENT, "sliver_off[i] must be a multiple of 2 bytes");
      if (symbols_off && symbols_off[i] % 2)
        return fail(RS2_E_INVALID_ARGUMENT, "symbols_off[i] must be a multiple of 2 bytes");
      for (uint32_t j = first_req[i]; j < first_req[i + 1]; ++j)
        if (targets[j] >= n)  // slivers.rs check_index -> RecoverySymbolError::IndexTooLarge
          return fail(RS2_E_INVALID_ARGUMENT, "target index too large");
      if (slivers && (!slivers[i] || sliver_len[i] != uint64_t(codes[axis[i]].k) * s))
        return fail(RS2_E_INCORRECT_DATA_LENGTH, "sliver length does not match its axis and symbol size");
      return RS2_OK;
    };
    const int rc = check();
    if (status_out) status_out[i] = rc;
    else if (rc != RS2_OK) return rc;
    ok[i] = rc == RS2_OK;
    plan.accepted += ok[i];
  }
  // the windows: over every accepted sliver, whether or not it is expanded
  SliverGroupsPlan cut;
  window_slivers(codes, n_slivers, axis, symbol_size, ok, budget, max_groups, UINT32_MAX, cut,
                 build ? plan.n_nodes * 32 : 0);
  plan.table.assign(size_t(total), kRequestSkipped);
  std::vector<uint8_t> expand;
  for (const SliverWindow& cw : cut.windows) {
    SymbolsMixedWindow w;
    w.first = cw.first;
    w.count = cw.count;
    w.first_request = first_req[cw.first];
    w.n_requests = first_req[cw.first + cw.count] - first_req[cw.first];
    // the slivers to expand, laid out as a window of their own
    expand.assign(cw.count, 0);
    for (uint32_t q = 0; q < cw.count; ++q) {
      const uint32_t i = cw.first + q;
      if (!ok[i]) continue;
      bool e = build && (have_nodes || target_counts[i] > 0);
      const uint32_t k = codes[axis[i]].k;
      for (uint32_t j = first_req[i]; j < first_req[i + 1] && !e; ++j) e = targets[j] >= k;
      expand[q] = e;
    }
    SliverGroupsPlan ex;
    window_slivers(codes, cw.count, axis + cw.first, symbol_size + cw.first, expand, UINT64_MAX,
                   UINT32_MAX, UINT32_MAX, ex);
    w.ex = std::move(ex.windows.front());
    for (uint32_t& i : w.ex.perm) i += cw.first;
    w.ex.first = cw.first;
    w.perm = w.ex.perm;
    for (uint32_t q = 0; q < cw.count; ++q)
      if (ok[cw.first + q] && !expand[q]) w.perm.push_back(cw.first + q);
    w.n_slots = uint32_t(w.perm.size());
    w.slot_request.resize(w.n_slots);
    w.slot_requests.resize(w.n_slots);
    for (uint32_t slot = 0; slot < w.n_slots; ++slot) {
      const uint32_t i = w.perm[slot];
      w.slot_request[slot] = first_req[i];
      w.slot_requests[slot] = target_counts[i];
      w.served += target_counts[i];
      w.with_requests += target_counts[i] > 0;
      for (uint32_t j = first_req[i]; j < first_req[i + 1]; ++j)
        plan.table[j] = slot << 16 | targets[j];
    }
    plan.windows.push_back(std::move(w));
  }
  return RS2_OK;
}

// ---------------------------------------------------------------------------------------------
// mixed blob encode
// ---------------------------------------------------------------------------------------------
int plan_blob_stages(uint32_t n_shards, BlobStages& st) {
  st = BlobStages{};
  if (n_shards == 0 || n_shards > 65535) return fail(RS2_E_INVALID_ARGUMENT, "n_shards must be non-zero");
  const int64_t n = n_shards, f = (n - 1) / 3, kp = n - 2 * f, ks = n - f;
  st.n = n_shards;
  st.kp = uint32_t(kp);
  st.ks = uint32_t(ks);
  st.block_max = block_max();
  if (kp >= n || ks >= n) return RS2_OK;
  BlobStageCode& cs = st.stage[kStageColsSys];
  BlobStageCode& rw = st.stage[kStageRows];
  BlobStageCode& cr = st.stage[kStageColsRep];
  // unit symbol offsets: every offset and stride below is in symbols (the job's times s)
  if (plan_encode(uint32_t(kp), uint32_t(n - kp), 2, nullptr, 1,
                  [&](uint32_t r) { return int64_t(r) * ks; }, nullptr, 1,
                  [&](uint32_t j) { return (kp + int64_t(j)) * ks; }, INT64_MAX, cs.tmpl) != RS2_OK)
    return RS2_OK;
  set_copy(cs.tmpl, nullptr, kp, INT64_MAX, [&](uint32_t r) { return int64_t(r); });
  st.sys_fused = copy_covered(cs.tmpl);
  cs.n_lines = uint32_t(ks);
  cs.in_ls = cs.out_ls = 1;
  cs.copy_ls = kp;
  cs.out_extent = n * ks;
  cs.copy_extent = ks * kp;
  if (plan_encode(uint32_t(ks), uint32_t(n - ks), 2, nullptr, ks,
                  [&](uint32_t c) { return int64_t(c); }, nullptr, 1,
                  [&](uint32_t j) { return (ks + int64_t(j)) * kp; }, INT64_MAX, rw.tmpl) != RS2_OK)
    return RS2_OK;
  rw.n_lines = uint32_t(kp);
  rw.in_ls = ks;
  rw.out_ls = 1;
  rw.out_extent = n * kp;
  if (plan_encode(uint32_t(kp), uint32_t(n - kp), 2, nullptr, kp,
                  [&](uint32_t r) { return int64_t(r); }, nullptr, 1,
                  [&](uint32_t j) { return int64_t(j) * (n - ks); }, INT64_MAX, cr.tmpl) != RS2_OK)
    return RS2_OK;
  cr.n_lines = uint32_t(n - ks);
  cr.in_ls = kp;
  cr.out_ls = 1;
  cr.out_extent = (n - kp) * (n - ks);
  st.planned = true;
  st.batchable = n_shards <= kGroupMaxLeaves;
  for (BlobStageCode& c : st.stage) {
    const CodecJobBig& j = c.tmpl.job;
    st.batchable = st.batchable && j.n_in >= 1 && j.n_out >= 1 && j.n_in <= kBatchBlocks &&
                   j.n_out <= kBatchBlocks;
    c.max_ls = std::max(std::max(c.in_ls, c.out_ls), c.copy_ls);
    c.n_off = c.tmpl.offs.size();
    if (!c.tmpl.copy_offs.empty())
      c.tmpl.offs.insert(c.tmpl.offs.end(), c.tmpl.copy_offs.begin(), c.tmpl.copy_offs.end());
  }
  if (st.batchable)
    for (BlobStageCode& c : st.stage) pack_batch_job(c.tmpl, c.job, c.mix);
  return RS2_OK;
}

int plan_blobs_mixed(const BlobStages& st, uint32_t n_blobs, const uint64_t* blob_lens,
                     const uint64_t* blob_off, const uint64_t* primary_off,
                     const uint64_t* secondary_off, const uint8_t* const* blobs, bool meta_only,
                     uint64_t budget, uint32_t max_blobs, int* status_out, BlobsMixedPlan& plan) {
  plan = BlobsMixedPlan{};
  if (n_blobs > 65535) return fail(RS2_E_INVALID_ARGUMENT, "more than 65535 blobs in a call");
  if (max_blobs == 0 || st.n == 0) return fail(RS2_E_INVALID_ARGUMENT, "not a blob's code");
  if (n_blobs == 0) return RS2_OK;
  if (!blob_lens || (!blob_off && !blobs) ||
      (blob_off && !meta_only && (!primary_off || !secondary_off)))
    return fail(RS2_E_INVALID_ARGUMENT, "null argument");
  const uint64_t n_sym = uint64_t(st.kp) * st.ks;
  std::vector<uint32_t> sym(n_blobs, 0);
  auto check = [&](uint32_t b) -> int {
    uint64_t sz = (std::max<uint64_t>(blob_lens[b], 1) + n_sym - 1) / n_sym;
    sz = (sz + 1) / 2 * 2;
    if (sz > 0xFFFF) return fail(RS2_E_DATA_TOO_LARGE, "blob too large for the symbol size");
    if (st.kp >= st.n || st.ks >= st.n)
      return fail(RS2_E_INCOMPATIBLE_PARAMETERS, "n_shards too small for a recovery code");
    sym[b] = uint32_t(sz);
    if (blob_off) {
      if (blob_off[b] % 2) return fail(RS2_E_INVALID_ARGUMENT, "blob_off[b] must be a multiple of 2 bytes");
      if (!meta_only && (primary_off[b] % 2 || secondary_off[b] % 2))
        return fail(RS2_E_INVALID_ARGUMENT, "sliver offsets must be multiples of 2 bytes");
    } else if (!blobs[b] && blob_lens[b]) {
      return fail(RS2_E_INVALID_ARGUMENT, "null blob of non-zero length");
    }
    return RS2_OK;
  };
  std::vector<uint8_t> ok(n_blobs, 0);
  for (uint32_t b = 0; b < n_blobs; ++b) {
    const int rc = check(b);
    if (status_out) status_out[b] = rc;
    else if (rc != RS2_OK) return rc;
    ok[b] = rc == RS2_OK;
    plan.accepted += ok[b];
  }
  BlobWindow w;
  std::vector<BlobSlot> late;  // the open window's ineligible slots
  std::map<uint32_t, uint32_t> open;  // s -> size class of the open window
  uint64_t used = 0, tiles_sum[kBlobStages] = {0, 0, 0};
  auto close = [&](uint32_t end) {
    w.count = end - w.first;
    w.n_eligible = uint32_t(w.slots.size());
    w.slots.insert(w.slots.end(), late.begin(), late.end());
    plan.windows.push_back(std::move(w));
    w = BlobWindow{};
    w.first = end;
    for (int g = 0; g < kBlobStages; ++g) w.tiles[g].assign(1, 0);
    late.clear();
    open.clear();
    used = 0;
    for (uint64_t& t : tiles_sum) t = 0;
  };
  for (int g = 0; g < kBlobStages; ++g) w.tiles[g].assign(1, 0);
  for (uint32_t b = 0; b < n_blobs; ++b) {
    if (!ok[b]) continue;  // a refused blob holds nothing: it stays in the open window
    const uint32_t s = sym[b];
    const uint64_t need = blob_scratch_bytes(st.n, st.kp, st.ks, s, meta_only);
    const bool held = !w.slots.empty() || !late.empty();
    // (need > budget - used, not used + need > budget: the sum may wrap)
    if (held && (used > budget || need > budget - used || w.slots.size() >= max_blobs)) {
      close(b);
    }
    BlobSlot sl;
    sl.blob = b;
    sl.s = s;
    sl.eligible = s >= 4 && st.batchable;
    uint64_t t[kBlobStages] = {0, 0, 0};
    if (sl.eligible)
      for (int g = 0; g < kBlobStages; ++g) {
        const BlobStageCode& c = st.stage[g];
        sl.pairs_span[g] = sliver_pairs_span(int32_t((s + 3) / 4), c.max_ls * int64_t(s));
        t[g] = (uint64_t(c.n_lines) * uint64_t(sl.pairs_span[g]) + 63) / 64;
        if (tiles_sum[g] + t[g] > 0x7FFFFFFFu) sl.eligible = false;
      }
    if (meta_only) {
      sl.primary_off = w.primary_bytes;
      sl.secondary_off = w.secondary_bytes;
      w.primary_bytes += uint64_t(st.n) * st.ks * s;
      w.secondary_bytes += uint64_t(st.n) * st.kp * s;
    }
    if (sl.eligible) {
      auto it = open.find(s);
      if (it == open.end()) {
        it = open.emplace(s, uint32_t(w.sizes.size())).first;
        w.sizes.push_back(s);
      }
      sl.size_class = it->second;
      sl.both_off = w.both_bytes;
      w.both_bytes += uint64_t(st.n - st.kp) * (st.n - st.ks) * s;
      for (int g = 0; g < kBlobStages; ++g) {
        tiles_sum[g] += t[g];
        w.tiles[g].push_back(uint32_t(tiles_sum[g]));
      }
      w.slots.push_back(sl);
    } else {
      late.push_back(sl);
    }
    used += need;
  }
  close(n_blobs);
  return RS2_OK;
}

}  // namespace rs2
