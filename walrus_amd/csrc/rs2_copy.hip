// Data-movement kernels of the MI355X Red Stuff engine (gfx950): nothing here hashes.
//
// symbol_copy_kernel     strided symbol copies (transposed systematic slivers, decode copies).
// segment_copy_*_kernel  segment copies of the partitioned encode's exchange packing.
// quilt_layout_kernel    quilt V1 column fill.
// batch_blob_copy_kernel the blobs of a batch into their systematic primary slivers.
// build_mul_tables       per-position GF multiplier nibble tables for the decoder.
// row_gather_kernel      the Default check's unverified rows, gathered back to back.
// check_rows_gather_kernel  the same for a verified decode batch: a source and valid length per row.
// host_upload_kernel     small host -> device uploads from pinned slots, upload_signal_kernel.
// tail_rows_kernel       the encode's zero-padded tail rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "rs2_device.h"
#include "rs2_kernels.h"

namespace rs2 {

template <int N, int I = 0, typename F>
__device__ __forceinline__ void sfor(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    sfor<N, I + 1>(f);
  }
}

// ------------------------------------------------------------------------------------------
// symbol copies (transposed systematic slivers, present originals of a decode)
//   dst + a*dsa + b*dsb  <-  src + a*ssa + b*ssb   (s bytes, u16 granularity), a = blockIdx.y
//   bytes at dst offset >= dst_limit are not written
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    symbol_copy_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ src_a,
                       int64_t ssb, uint8_t* __restrict__ dst, const int64_t* __restrict__ dst_a,
                       int64_t dsb, int count_b, int s, int64_t dst_limit) {
  const int a = blockIdx.y;
  const int64_t so = src_a[a], dof = dst_a[a];
  const int hw = s >> 1;
  const int64_t total = int64_t(count_b) * hw;
  for (int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x; idx < total;
       idx += int64_t(gridDim.x) * 256) {
    const int b = int(idx / hw), k = int(idx % hw);
    const int64_t d = dof + b * dsb + 2 * k;
    const uint16_t v = *reinterpret_cast<const uint16_t*>(src + so + b * ssb + 2 * k);
    if (d + 2 <= dst_limit) {
      *reinterpret_cast<uint16_t*>(dst + d) = v;
    } else if (d < dst_limit) {
      dst[d] = uint8_t(v);
    }
  }
}

// Segment copies (the partitioned encode's exchange packing, partition.py): segment (a, b) is
// `len` bytes from src + src_a[a] + b*ssb to dst + dst_a[a] + b*dsb.  Lanes take consecutive
// U-byte units of consecutive segments, so a wave moves 64 units of one or more contiguous
// segments per instruction; the launcher picks the widest U that divides every offset, stride,
// length and base (U = 16 for the 4 GiB C4 blob's s = 19,280).  Unit -> (segment, a, b) uses
// multiply-high division by host-made constants (flat index < 2^31 per launch).
struct FastDiv {
  uint32_t m, l, d;
};
__device__ __forceinline__ uint32_t fast_div(uint32_t x, FastDiv f) {
  return uint32_t((uint64_t(__umulhi(x, f.m)) + x) >> f.l);
}
template <int U>
struct UnitT;
template <> struct UnitT<1> { using T = uint8_t; };
template <> struct UnitT<2> { using T = uint16_t; };
template <> struct UnitT<4> { using T = uint32_t; };
template <> struct UnitT<8> { using T = uint2; };
template <> struct UnitT<16> { using T = uint4; };

// long segments (>= 256 units): one workgroup per 1024-unit chunk of one segment, so the
// segment's offsets are workgroup-uniform (scalar loads) and every lane moves 4 units
template <int U>
__global__ void __launch_bounds__(256)
    segment_copy_wide_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                             const int64_t* __restrict__ src_a, const int64_t* __restrict__ dst_a,
                             int64_t ssb, int64_t dsb, FastDiv chunks, FastDiv per_a, uint32_t ups) {
  using T = typename UnitT<U>::T;
  const uint32_t seg = fast_div(blockIdx.x, chunks), c = blockIdx.x - seg * chunks.d;
  const uint32_t a = fast_div(seg, per_a), b = seg - a * per_a.d;
  const uint8_t* sp = src + src_a[a] + int64_t(b) * ssb;
  uint8_t* dp = dst + dst_a[a] + int64_t(b) * dsb;
  const uint32_t u0 = c * 1024u + threadIdx.x;
  T v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (u0 + 256u * k < ups) v[k] = *reinterpret_cast<const T*>(sp + int64_t(u0 + 256u * k) * U);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (u0 + 256u * k < ups) *reinterpret_cast<T*>(dp + int64_t(u0 + 256u * k) * U) = v[k];
}

template <int U>
__global__ void __launch_bounds__(256)
    segment_copy_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                        const int64_t* __restrict__ src_a, const int64_t* __restrict__ dst_a,
                        int64_t ssb, int64_t dsb, FastDiv per_seg, FastDiv per_a, uint32_t total) {
  using T = typename UnitT<U>::T;
  for (uint32_t f = blockIdx.x * 256u + threadIdx.x; f < total; f += gridDim.x * 256u) {
    const uint32_t seg = fast_div(f, per_seg), u = f - seg * per_seg.d;
    const uint32_t a = fast_div(seg, per_a), b = seg - a * per_a.d;
    const T v = *reinterpret_cast<const T*>(src + src_a[a] + int64_t(b) * ssb + int64_t(u) * U);
    *reinterpret_cast<T*>(dst + dst_a[a] + int64_t(b) * dsb + int64_t(u) * U) = v;
  }
}

// Quilt V1 column fill (quilt_encoding.rs:1447-1528): quilt symbol (r, c) <- payload bytes
// [r*s, r*s + s) of column c's run (zero past the column's length).  One thread per aligned
// 16-byte piece of the quilt (a plain vector store); its 8 u16 elements are gathered from the
// column runs (symbols are only 2-byte aligned, and an even s never splits an element).
__global__ void __launch_bounds__(256)
    quilt_layout_kernel(const uint8_t* __restrict__ payload, const int64_t* __restrict__ col_off,
                        const uint32_t* __restrict__ col_len, int n_cols, int s, int64_t total,
                        uint8_t* __restrict__ quilt) {
  const int64_t row_bytes = int64_t(n_cols) * s;
  const int64_t pieces = (total + 15) >> 4;
  for (int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x; t < pieces;
       t += int64_t(gridDim.x) * 256) {
    const int64_t g = t << 4;
    int64_t r = g / row_bytes;
    const int64_t x = g - r * row_bytes;
    int c = int(x / s);
    int k = int(x - int64_t(c) * s);
    uint32_t w[4];
    sfor<8>([&](auto ee) {
      constexpr int e = decltype(ee)::value;
      uint32_t v = 0;
      if (g + 2 * e < total) {
        const int64_t at = r * s + k;  // byte of column c's run
        const int64_t len = col_len[c];
        const uint8_t* src = payload + col_off[c] + at;
        if (at + 2 <= len) {
          v = *reinterpret_cast<const uint16_t*>(src);
        } else if (at < len) {
          v = src[0];
        }
      }
      if constexpr ((e & 1) == 0) {
        w[e >> 1] = v;
      } else {
        w[e >> 1] |= v << 16;
      }
      k += 2;
      if (k == s) {
        k = 0;
        if (++c == n_cols) {
          c = 0;
          ++r;
        }
      }
    });
    if (g + 16 <= total) {
      *reinterpret_cast<uint4*>(quilt + g) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      for (int e = 0; 2 * e < int(total - g); ++e)
        *reinterpret_cast<uint16_t*>(quilt + g + 2 * e) = uint16_t(w[e >> 1] >> (16 * (e & 1)));
    }
  }
}

// Blob batches: the message of blob y (its blob_lens[y] bytes at src + y*src_stride, zero-filled
// to msg bytes) -> dst + y*dst_stride, the blob's systematic primary slivers.  One thread per
// 16-byte piece; aligned whole pieces move as one vector load / store.
__global__ void __launch_bounds__(256)
    batch_blob_copy_kernel(const uint8_t* __restrict__ src, int64_t src_stride,
                           const uint64_t* __restrict__ blob_lens, int64_t msg,
                           uint8_t* __restrict__ dst, int64_t dst_stride) {
  const int64_t y = blockIdx.y;
  const int64_t len = int64_t(blob_lens[y]);
  const uint8_t* sp0 = src + y * src_stride;
  uint8_t* dp0 = dst + y * dst_stride;
  for (int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x; t * 16 < msg;
       t += int64_t(gridDim.x) * 256) {
    const int64_t g = t * 16;
    const uint8_t* sp = sp0 + g;
    uint8_t* dp = dp0 + g;
    const bool aligned = ((reinterpret_cast<uintptr_t>(sp) | reinterpret_cast<uintptr_t>(dp)) & 15) == 0;
    if (aligned && g + 16 <= len && g + 16 <= msg) {
      *reinterpret_cast<uint4*>(dp) = *reinterpret_cast<const uint4*>(sp);
    } else if (aligned && g >= len && g + 16 <= msg) {
      *reinterpret_cast<uint4*>(dp) = make_uint4(0u, 0u, 0u, 0u);
    } else {
      for (int e = 0; e < 16 && g + e < msg; ++e) dp[e] = g + e < len ? sp[e] : uint8_t(0);
    }
  }
}

// Per-position multiplier tables (rs2_planner.cpp nib_table layout): out[i][e] = x(e) * exp(logs[i])
// with x(e) = e (e < 64), (e - 64) << 6 (e < 96), (e - 96) << 11  (log 65535 == 0).
__global__ void __launch_bounds__(256)
    build_mul_tables_kernel(const uint16_t* __restrict__ exp_t, const uint16_t* __restrict__ log_t,
                            const uint16_t* __restrict__ logs, int count,
                            uint16_t* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= count * kTabU16) return;
  const int i = idx / kTabU16, e = idx % kTabU16;
  const uint32_t x = e < 64 ? uint32_t(e) : (e < 96 ? uint32_t(e - 64) << 6 : uint32_t(e - 96) << 11);
  uint16_t r = 0;
  if (x) {
    const uint32_t sum = uint32_t(log_t[x]) + logs[i];
    r = exp_t[(sum + (sum >> 16)) & 0xFFFFu];
  }
  out[idx] = r;
}

// Row gather (the device Default check's unverified rows, rs2_engine.cpp default_check): row a
// of `row_bytes` bytes from src + src_off[a] to dst + a * row_bytes.  Rows are only 2-byte
// aligned (K_s * s bytes), so each thread writes one 4-byte-aligned destination dword from two
// aligned source dwords and an alignbyte; the dwords at a row's two ends are written bytewise.
// grid (ceil(dwords per row / 256), rows).
__global__ void __launch_bounds__(256) row_gather_kernel(const uint8_t* __restrict__ src,
                                                         const int64_t* __restrict__ src_off,
                                                         uint8_t* __restrict__ dst,
                                                         int64_t row_bytes) {
  const int64_t a = blockIdx.y;
  const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst) + uintptr_t(a * row_bytes);
  const uintptr_t d1 = d0 + uintptr_t(row_bytes);
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src) + uintptr_t(src_off[a]);
  const uintptr_t D = (d0 & ~uintptr_t(3)) + 4 * (uintptr_t(blockIdx.x) * 256 + threadIdx.x);
  if (D >= d1) return;
  if (D >= d0 && D + 4 <= d1) {
    const uintptr_t S = s0 + (D - d0);
    const uintptr_t Sa = S & ~uintptr_t(3);
    const uint32_t sh = uint32_t(S & 3);
    const uint32_t lo = *reinterpret_cast<const uint32_t*>(Sa);
    // the second dword only when the bytes span it (never read past the source row's end)
    const uint32_t hi = sh ? *reinterpret_cast<const uint32_t*>(Sa + 4) : 0u;
    *reinterpret_cast<uint32_t*>(D) = __builtin_amdgcn_alignbyte(hi, lo, sh);
    return;
  }
  for (uintptr_t x = D; x < D + 4; ++x)
    if (x >= d0 && x < d1)
      *reinterpret_cast<uint8_t*>(x) = *reinterpret_cast<const uint8_t*>(s0 + (x - d0));
}

// Row gather of a verified decode batch (rs2_decode_and_verify_batch_*): row_gather_kernel with a
// source address and a valid length per row.  Row a of the launch (row0 + a of the table) is
// row_bytes bytes at dst + (row0 + a) * row_bytes: bytes [0, valid) from the row's source, zeros
// from there on.  Nothing at or past src + valid is read -- it may be another blob's slot or the
// end of the caller's buffer.  Sources and destinations are 2-byte aligned and row_bytes is even,
// so a lane moves 16 bytes of one row as one, four or eight aligned words, by the alignment the
// two ends share; the piece that holds the valid end goes element by element, its odd last byte
// alone.  The row index is folded into grid.x (`chunks` workgroups of 4 KiB per row): a window
// holds more rows than grid.y may count.
__global__ void __launch_bounds__(256)
    check_rows_gather_kernel(const CheckRow* __restrict__ rows, int64_t row0, uint32_t chunks,
                             int64_t row_bytes, uint8_t* __restrict__ dst) {
  const int64_t a = row0 + blockIdx.x / chunks;
  const int64_t g = (int64_t(blockIdx.x % chunks) * 256 + threadIdx.x) * 16;
  if (g >= row_bytes) return;
  const CheckRow row = rows[a];
  const int64_t valid = row.valid;
  const int n = int(row_bytes - g < 16 ? row_bytes - g : 16);  // even
  const uint8_t* sp = row.src + g;
  uint8_t* dp = dst + a * row_bytes + g;
  const uintptr_t dal = reinterpret_cast<uintptr_t>(dp);
  if (n == 16 && g + 16 <= valid) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(sp) | dal;
    if ((al & 15) == 0) {
      *reinterpret_cast<uint4*>(dp) = *reinterpret_cast<const uint4*>(sp);
    } else if ((al & 3) == 0) {
      uint32_t v[4];
      sfor<4>([&](auto j) { v[decltype(j)::value] = reinterpret_cast<const uint32_t*>(sp)[decltype(j)::value]; });
      sfor<4>([&](auto j) { reinterpret_cast<uint32_t*>(dp)[decltype(j)::value] = v[decltype(j)::value]; });
    } else {
      uint16_t v[8];
      sfor<8>([&](auto j) { v[decltype(j)::value] = reinterpret_cast<const uint16_t*>(sp)[decltype(j)::value]; });
      sfor<8>([&](auto j) { reinterpret_cast<uint16_t*>(dp)[decltype(j)::value] = v[decltype(j)::value]; });
    }
    return;
  }
  if (n == 16 && g >= valid && (dal & 15) == 0) {
    *reinterpret_cast<uint4*>(dp) = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  for (int e = 0; e < n; e += 2) {
    uint16_t v = 0;
    if (g + e + 2 <= valid)
      v = *reinterpret_cast<const uint16_t*>(sp + e);
    else if (g + e < valid)
      v = sp[e];  // the blob's odd last byte; the element's high byte is padding
    *reinterpret_cast<uint16_t*>(dp + e) = v;
  }
}

// Sliver gather of a mixed verification window (rs2_sliver_checker_*): slot a's `len` bytes from
// its own place in the caller's memory to dst + dst_off, so that a group's slivers sit back to
// back at one stride for the codec and the leaf hash.  The slivers' lengths differ with their
// symbol size, so a workgroup (one 4 KiB chunk of one sliver) finds its slot by a search of the
// slots' first chunks; nothing at or past src + len is read.  Both ends are 2-byte aligned and len
// is even: a lane moves 16 bytes as one, four or eight aligned words, by the alignment the two
// ends share, and the sliver's last piece element by element.
__global__ void __launch_bounds__(256)
    sliver_gather_kernel(const SliverSlot* __restrict__ slots, int n_slots,
                         uint8_t* __restrict__ dst) {
  const uint32_t chunk = blockIdx.x;
  int lo = 0, hi = n_slots - 1;  // the last slot whose chunk0 <= chunk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (slots[mid].chunk0 <= chunk)
      lo = mid;
    else
      hi = mid - 1;
  }
  const SliverSlot sl = slots[lo];
  const int64_t g = (int64_t(chunk - sl.chunk0) * 256 + threadIdx.x) * 16;
  const int64_t len = sl.len;
  if (g >= len) return;
  const int n = int(len - g < 16 ? len - g : 16);  // even
  const uint8_t* sp = sl.src + g;
  uint8_t* dp = dst + sl.dst_off + g;
  if (n == 16) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(sp) | reinterpret_cast<uintptr_t>(dp);
    if ((al & 15) == 0) {
      *reinterpret_cast<uint4*>(dp) = *reinterpret_cast<const uint4*>(sp);
    } else if ((al & 3) == 0) {
      uint32_t v[4];
      sfor<4>([&](auto j) { v[decltype(j)::value] = reinterpret_cast<const uint32_t*>(sp)[decltype(j)::value]; });
      sfor<4>([&](auto j) { reinterpret_cast<uint32_t*>(dp)[decltype(j)::value] = v[decltype(j)::value]; });
    } else {
      uint16_t v[8];
      sfor<8>([&](auto j) { v[decltype(j)::value] = reinterpret_cast<const uint16_t*>(sp)[decltype(j)::value]; });
      sfor<8>([&](auto j) { reinterpret_cast<uint16_t*>(dp)[decltype(j)::value] = v[decltype(j)::value]; });
    }
    return;
  }
  for (int e = 0; e < n; e += 2)
    *reinterpret_cast<uint16_t*>(dp + e) = *reinterpret_cast<const uint16_t*>(sp + e);
}

// Message staging of a mixed blob encode window (rs2_blob_encoder_*): blob a's `len` bytes from
// its own place in the caller's memory to its systematic primary slivers, zeros from there up to
// its message length `msg` (K_p K_s s, even).  The lengths differ, so a workgroup (one 4 KiB chunk
// of one message) finds its blob by a search of the blobs' first chunks, as sliver_gather_kernel.
// Nothing at or past src + len is read -- it may be the next blob or the end of the caller's
// buffer.  Both ends are 2-byte aligned: a lane moves 16 bytes as one, four or eight aligned
// words, by the alignment the two ends share; the piece that holds the blob's end goes element by
// element, its odd last byte alone (check_rows_gather_kernel's rule).
// A blob whose systematic-column code has no fused copy-out (a mixing code: n_shards = 13, or
// above 1534 at the default block limit) names its secondary buffer: the lane then also writes
// its elements transposed -- symbol (r, c) of the message to secondary sliver c, row r -- two
// bytes at a time, which the codec's own loads do for every other blob.
__global__ void __launch_bounds__(256)
    blob_stage_kernel(const BlobStage* __restrict__ blobs, int n_blobs, int kp, int ks) {
  const uint32_t chunk = blockIdx.x;
  int lo = 0, hi = n_blobs - 1;  // the last blob whose chunk0 <= chunk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (blobs[mid].chunk0 <= chunk)
      lo = mid;
    else
      hi = mid - 1;
  }
  const BlobStage bl = blobs[lo];
  const int64_t g = (int64_t(chunk - bl.chunk0) * 256 + threadIdx.x) * 16;
  const int64_t msg = int64_t(bl.msg), valid = int64_t(bl.len);
  if (g >= msg) return;
  const int n = int(msg - g < 16 ? msg - g : 16);  // even
  const uint8_t* sp = bl.src + g;
  uint8_t* dp = bl.dst + g;
  const uintptr_t dal = reinterpret_cast<uintptr_t>(dp);
  // the message's 2-byte element at g + e: the blob's bytes, then padding
  auto element = [&](int e) -> uint16_t {
    if (g + e + 2 <= valid) return *reinterpret_cast<const uint16_t*>(sp + e);
    if (g + e < valid) return sp[e];  // the blob's odd last byte; the high byte is padding
    return 0;
  };
  if (bl.sec) {
    const int64_t s = bl.s;  // even, so an element never straddles two symbols
    for (int e = 0; e < n; e += 2) {
      const int64_t x = g + e, sym = x / s, r = sym / ks, c = sym - r * ks;
      *reinterpret_cast<uint16_t*>(bl.sec + (c * kp + r) * s + (x - sym * s)) = element(e);
    }
  }
  if (n == 16 && g + 16 <= valid) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(sp) | dal;
    if ((al & 15) == 0) {
      *reinterpret_cast<uint4*>(dp) = *reinterpret_cast<const uint4*>(sp);
    } else if ((al & 3) == 0) {
      uint32_t v[4];
      sfor<4>([&](auto j) { v[decltype(j)::value] = reinterpret_cast<const uint32_t*>(sp)[decltype(j)::value]; });
      sfor<4>([&](auto j) { reinterpret_cast<uint32_t*>(dp)[decltype(j)::value] = v[decltype(j)::value]; });
    } else {
      uint16_t v[8];
      sfor<8>([&](auto j) { v[decltype(j)::value] = reinterpret_cast<const uint16_t*>(sp)[decltype(j)::value]; });
      sfor<8>([&](auto j) { reinterpret_cast<uint16_t*>(dp)[decltype(j)::value] = v[decltype(j)::value]; });
    }
    return;
  }
  if (n == 16 && g >= valid && (dal & 15) == 0) {
    *reinterpret_cast<uint4*>(dp) = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  for (int e = 0; e < n; e += 2) *reinterpret_cast<uint16_t*>(dp + e) = element(e);
}

// Metadata of a mixed blob encode window to the caller's arrays: the window's pair hashes
// (64 n bytes per slot) and ids (32 bytes per slot) lie in slot order; slot y's go to blob
// dst_index[y] of hashes_out / ids_out.  All four bases are 16-byte aligned; a lane moves 16 bytes.
__global__ void __launch_bounds__(256)
    blob_meta_scatter_kernel(const uint8_t* __restrict__ hashes, const uint8_t* __restrict__ ids,
                             const uint32_t* __restrict__ dst_index, int64_t hash_bytes,
                             uint8_t* __restrict__ hashes_out, uint8_t* __restrict__ ids_out) {
  const int64_t slot = blockIdx.y, to = dst_index[blockIdx.y];
  const int64_t g = (int64_t(blockIdx.x) * 256 + threadIdx.x) * 16;
  if (g < hash_bytes) {
    *reinterpret_cast<uint4*>(hashes_out + to * hash_bytes + g) =
        *reinterpret_cast<const uint4*>(hashes + slot * hash_bytes + g);
  } else if (g < hash_bytes + 32) {
    const int64_t o = g - hash_bytes;
    *reinterpret_cast<uint4*>(ids_out + to * 32 + o) =
        *reinterpret_cast<const uint4*>(ids + slot * 32 + o);
  }
}

// Small host -> device uploads (rs2_engine.cpp UploadSlots): the kernel reads the pinned,
// device-mapped host slot over PCIe and writes the device buffer, in stream order like any
// launch -- no DMA-engine copy, whose cross-engine dependency on the stream's earlier kernels
// made the issuing thread wait for them (6-28 ms stalls, gpurun_out/r05c traces).  16 bytes
// per lane when both ends are 16-byte aligned, else bytes.
// Completion is reported to the host without an event: a copy with a completion word runs as
// ONE workgroup (a lane per 16 bytes, striding; the slot uploads are a few KiB, <= 512 KiB),
// whose lane 0, once every lane's loads of the slot have returned (the barrier), stores `gen`
// into the slot's word of a coherent, mapped host array; the host reuses the slot once it reads
// that generation.  So a slot's reuse depends on nothing but this kernel having read it -- not on
// the lifetime of the stream it ran on (a plan, verifier or caller stream torn down since).  The
// store is relaxed: the host reads nothing else the GPU wrote, so no release (whose L2
// write-back on gfx950 every other kernel on the XCD would pay for) is needed.
// done == nullptr: no report, a 16-byte chunk per lane over as many workgroups as it takes.
__global__ void __launch_bounds__(256) host_upload_kernel(const uint8_t* __restrict__ src,
                                                          uint8_t* __restrict__ dst, int64_t n,
                                                          uint64_t* done, uint64_t gen) {
  const bool aligned =
      ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
  auto chunk = [&](int64_t i) {
    if (i + 16 <= n && aligned) {
      *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(src + i);
    } else {
      for (int b = 0; b < 16 && i + b < n; ++b) dst[i + b] = src[i + b];
    }
  };
  if (done) {
    for (int64_t i = int64_t(threadIdx.x) * 16; i < n; i += 256 * 16) chunk(i);
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(done, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  const int64_t i = (int64_t(blockIdx.x) * 256 + threadIdx.x) * 16;
  if (i < n) chunk(i);
}

// The job ring's completion report (UploadSlots::launch_with_job): queued behind the consumer
// kernel that reads the job, one lane stores the generation (stream order: the consumer is done;
// relaxed, as host_upload_kernel's).
__global__ void __launch_bounds__(64) upload_signal_kernel(uint64_t* done, uint64_t gen) {
  if (threadIdx.x == 0) __hip_atomic_store(done, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The encode's padded tail rows (rs2_engine.cpp encode_device): dst[i] = i < have ? src[i] : 0
// for i < total, 4 bytes per thread (byte loads: src is only 2-byte aligned), one launch in place
// of a D2D copy plus a memset (which the runtime splits into three fill kernels on unaligned
// ranges) on the encode's critical path.
__global__ void __launch_bounds__(256) tail_rows_kernel(const uint8_t* __restrict__ src, int64_t have,
                                                        uint8_t* __restrict__ dst, int64_t total) {
  const int64_t i = (int64_t(blockIdx.x) * 256 + threadIdx.x) * 4;
  if (i >= total) return;
  if (i + 4 <= have) {
    const uint32_t v = uint32_t(src[i]) | (uint32_t(src[i + 1]) << 8) |
                       (uint32_t(src[i + 2]) << 16) | (uint32_t(src[i + 3]) << 24);
    if (i + 4 <= total && ((reinterpret_cast<uintptr_t>(dst) + uintptr_t(i)) & 3u) == 0) {
      *reinterpret_cast<uint32_t*>(dst + i) = v;
      return;
    }
  }
  for (int b = 0; b < 4 && i + b < total; ++b) dst[i + b] = i + b < have ? src[i + b] : uint8_t(0);
}

}  // namespace rs2

// ------------------------------------------------------------------------------------------
// launchers (declared in rs2_kernels.h, called from rs2_engine.cpp)
// ------------------------------------------------------------------------------------------
extern "C" {

hipError_t rs2k_launch_symbol_copy(const uint8_t* src, const int64_t* d_src_a, int64_t ssb,
                                   uint8_t* dst, const int64_t* d_dst_a, int64_t dsb, int count_a,
                                   int count_b, int s, int64_t dst_limit, hipStream_t stream) {
  if (count_a <= 0 || count_b <= 0) return hipSuccess;
  const int64_t total = int64_t(count_b) * (s >> 1);
  unsigned bx = unsigned((total + 255) / 256);
  if (bx > 64) bx = 64;
  hipLaunchKernelGGL(rs2::symbol_copy_kernel, dim3(bx, count_a), dim3(256), 0, stream, src,
                     d_src_a, ssb, dst, d_dst_a, dsb, count_b, s, dst_limit);
  return hipGetLastError();
}

static rs2::FastDiv make_fast_div(uint32_t d) {
  uint32_t l = 0;
  while ((uint64_t(1) << l) < d) ++l;
  const uint32_t m = uint32_t(((uint64_t(1) << 32) * ((uint64_t(1) << l) - d)) / d + 1);
  return rs2::FastDiv{m, l, d};
}

hipError_t rs2k_launch_segment_copy(const uint8_t* src, uint8_t* dst, uint32_t count_a,
                                    const int64_t* d_src_a, const int64_t* d_dst_a, uint32_t count_b,
                                    int64_t ssb, int64_t dsb, uint32_t len, int unit,
                                    hipStream_t stream) {
  if (count_a == 0 || count_b == 0 || len == 0) return hipSuccess;
  const uint32_t ups = len / uint32_t(unit);
  if (ups >= 256) {
    const uint32_t chunks = (ups + 1023) / 1024;
    const uint64_t blocks = uint64_t(count_a) * count_b * chunks;
    if (blocks >= (uint64_t(1) << 31)) return hipErrorInvalidValue;
    const rs2::FastDiv fc = make_fast_div(chunks), fa = make_fast_div(count_b);
#define RS2_SEGW(UU)                                                                           \
  hipLaunchKernelGGL(rs2::segment_copy_wide_kernel<UU>, dim3(unsigned(blocks)), dim3(256), 0,  \
                     stream, src, dst, d_src_a, d_dst_a, ssb, dsb, fc, fa, ups)
    switch (unit) {
      case 16: RS2_SEGW(16); break;
      case 8: RS2_SEGW(8); break;
      case 4: RS2_SEGW(4); break;
      case 2: RS2_SEGW(2); break;
      default: RS2_SEGW(1); break;
    }
#undef RS2_SEGW
    return hipGetLastError();
  }
  const uint64_t per_a = uint64_t(count_b) * ups;
  // a-ranges of at most 2^31 units per launch
  const uint32_t a_step = uint32_t(std::max<uint64_t>(1, (uint64_t(1) << 31) / per_a));
  for (uint32_t a0 = 0; a0 < count_a; a0 += a_step) {
    const uint32_t na = std::min(a_step, count_a - a0);
    const uint64_t total = uint64_t(na) * per_a;
    if (total >= (uint64_t(1) << 32)) return hipErrorInvalidValue;  // one segment row > 2^32 units
    const unsigned grid = unsigned(std::min<uint64_t>((total + 255) / 256, 256 * 64));
    const rs2::FastDiv fs = make_fast_div(ups), fa = make_fast_div(count_b);
#define RS2_SEG(UU)                                                                          \
  hipLaunchKernelGGL(rs2::segment_copy_kernel<UU>, dim3(grid), dim3(256), 0, stream, src, dst, \
                     d_src_a + a0, d_dst_a + a0, ssb, dsb, fs, fa, uint32_t(total))
    switch (unit) {
      case 16: RS2_SEG(16); break;
      case 8: RS2_SEG(8); break;
      case 4: RS2_SEG(4); break;
      case 2: RS2_SEG(2); break;
      default: RS2_SEG(1); break;
    }
#undef RS2_SEG
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t rs2k_launch_quilt_layout(int n_rows, int n_cols, int s, const uint8_t* payload,
                                    const int64_t* col_off, const uint32_t* col_len,
                                    uint8_t* quilt, hipStream_t stream) {
  if (n_rows <= 0 || n_cols <= 0 || s <= 0) return hipSuccess;
  if (reinterpret_cast<uintptr_t>(quilt) & 15) return hipErrorInvalidValue;
  const int64_t total = int64_t(n_rows) * n_cols * s;
  int64_t blocks = (((total + 15) >> 4) + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(rs2::quilt_layout_kernel, dim3(unsigned(blocks)), dim3(256), 0, stream,
                     payload, col_off, col_len, n_cols, s, total, quilt);
  return hipGetLastError();
}

hipError_t rs2k_launch_batch_blob_copy(const uint8_t* src, int64_t src_stride,
                                       const uint64_t* d_blob_lens, int64_t msg, uint8_t* dst,
                                       int64_t dst_stride, int n_blobs, hipStream_t stream) {
  if (n_blobs <= 0 || msg <= 0) return hipSuccess;
  if (n_blobs > 65535) return hipErrorInvalidValue;
  const int64_t pieces = (msg + 15) / 16;
  const unsigned bx = unsigned(std::min<int64_t>((pieces + 255) / 256, 4096));
  hipLaunchKernelGGL(rs2::batch_blob_copy_kernel, dim3(bx, unsigned(n_blobs)), dim3(256), 0, stream,
                     src, src_stride, d_blob_lens, msg, dst, dst_stride);
  return hipGetLastError();
}

hipError_t rs2k_launch_build_mul_tables(const uint16_t* d_exp, const uint16_t* d_log,
                                        const uint16_t* d_logs, int count, uint16_t* d_out,
                                        hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  const unsigned blocks = unsigned((count * rs2::kTabU16 + 255) / 256);
  hipLaunchKernelGGL(rs2::build_mul_tables_kernel, dim3(blocks), dim3(256), 0, stream, d_exp,
                     d_log, d_logs, count, d_out);
  return hipGetLastError();
}

hipError_t rs2k_launch_row_gather(const uint8_t* src, const int64_t* d_src_off, uint8_t* dst,
                                  int64_t row_bytes, int rows, hipStream_t stream) {
  if (rows <= 0 || row_bytes <= 0) return hipSuccess;
  const int64_t words = row_bytes / 4 + 2;  // the aligned span of a row
  const int64_t bx = (words + 255) / 256;
  if (bx >= (int64_t(1) << 31) || rows > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rs2::row_gather_kernel, dim3(unsigned(bx), unsigned(rows)), dim3(256), 0,
                     stream, src, d_src_off, dst, row_bytes);
  return hipGetLastError();
}

hipError_t rs2k_launch_check_rows_gather(const rs2::CheckRow* d_rows, int64_t n_rows,
                                         int64_t row_bytes, uint8_t* dst, hipStream_t stream) {
  if (n_rows <= 0 || row_bytes <= 0) return hipSuccess;
  const int64_t chunks = (row_bytes + 4095) / 4096;
  if (chunks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
  // as many rows per launch as grid.x can count
  const int64_t per_launch = ((int64_t(1) << 31) - 1) / chunks;
  for (int64_t row0 = 0; row0 < n_rows; row0 += per_launch) {
    const int64_t cnt = std::min(per_launch, n_rows - row0);
    hipLaunchKernelGGL(rs2::check_rows_gather_kernel, dim3(unsigned(cnt * chunks)), dim3(256), 0,
                       stream, d_rows, row0, uint32_t(chunks), row_bytes, dst);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t rs2k_launch_sliver_gather(const rs2::SliverSlot* d_slots, int n_slots, int64_t n_chunks,
                                     uint8_t* d_dst, hipStream_t stream) {
  if (n_slots <= 0 || n_chunks <= 0) return hipSuccess;
  if (n_chunks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rs2::sliver_gather_kernel, dim3(unsigned(n_chunks)), dim3(256), 0, stream,
                     d_slots, n_slots, d_dst);
  return hipGetLastError();
}

hipError_t rs2k_launch_blob_stage(const rs2::BlobStage* d_blobs, int n_blobs, int64_t n_chunks,
                                  int kp, int ks, hipStream_t stream) {
  if (n_blobs <= 0 || n_chunks <= 0) return hipSuccess;
  if (n_chunks >= (int64_t(1) << 31) || kp < 1 || ks < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rs2::blob_stage_kernel, dim3(unsigned(n_chunks)), dim3(256), 0, stream,
                     d_blobs, n_blobs, kp, ks);
  return hipGetLastError();
}

hipError_t rs2k_launch_blob_meta_scatter(const uint8_t* d_hashes, const uint8_t* d_ids,
                                         const uint32_t* d_dst_index, int n_slots, int n,
                                         uint8_t* d_hashes_out, uint8_t* d_ids_out,
                                         hipStream_t stream) {
  if (n_slots <= 0) return hipSuccess;
  if (n_slots > 65535 || n < 1) return hipErrorInvalidValue;
  const int64_t hash_bytes = int64_t(n) * 64;
  hipLaunchKernelGGL(rs2::blob_meta_scatter_kernel,
                     dim3(unsigned((hash_bytes + 32 + 4095) / 4096), unsigned(n_slots)), dim3(256),
                     0, stream, d_hashes, d_ids, d_dst_index, hash_bytes, d_hashes_out, d_ids_out);
  return hipGetLastError();
}

hipError_t rs2k_launch_host_upload(const void* src, void* dst, int64_t n, uint64_t* done,
                                   uint64_t gen, hipStream_t stream) {
  if (n <= 0 && !done) return hipSuccess;
  // with a completion word: one workgroup (see host_upload_kernel)
  const int64_t blocks = done ? 1 : (n + 4095) / 4096;
  if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rs2::host_upload_kernel, dim3(unsigned(blocks)), dim3(256), 0, stream,
                     static_cast<const uint8_t*>(src), static_cast<uint8_t*>(dst), n, done, gen);
  return hipGetLastError();
}

hipError_t rs2k_launch_upload_signal(uint64_t* done, uint64_t gen, hipStream_t stream) {
  hipLaunchKernelGGL(rs2::upload_signal_kernel, dim3(1), dim3(64), 0, stream, done, gen);
  return hipGetLastError();
}

hipError_t rs2k_launch_tail_rows(const uint8_t* src, int64_t have, uint8_t* dst, int64_t total,
                                 hipStream_t stream) {
  if (total <= 0) return hipSuccess;
  const int64_t blocks = (total + 1023) / 1024;
  if (blocks >= (int64_t(1) << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rs2::tail_rows_kernel, dim3(unsigned(blocks)), dim3(256), 0, stream, src,
                     have, dst, total);
  return hipGetLastError();
}

}  // extern "C"
