// Launchers of the HIP kernels, declared once.  The files that define them (rs2_codec.hip per
// block size, rs2_hash.hip, rs2_copy.hip) and the host file that calls them (rs2_engine.cpp) include this
// header, so a prototype that drifts on one side is a compile error ("conflicting types"), not
// a link that succeeds and corrupts the kernel's arguments at run time.  Default arguments are
// given here only; the definitions repeat none.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rs2_device.h"

extern "C" {
#define RS2_DECL(CC)                                                                      \
  hipError_t rs2k_launch_codec_##CC(const rs2::CodecJob* job, int n_tiles, int n_lines, \
                                    int n_z, int mode, hipStream_t stream);
RS2_DECL(1)
RS2_DECL(2)
RS2_DECL(4)
RS2_DECL(8)
RS2_DECL(16)
RS2_DECL(32)
RS2_DECL(64)
RS2_DECL(128)
RS2_DECL(256)
RS2_DECL(512)
#undef RS2_DECL
// the decode batch (one CodecJobBatch per blob in device memory, rs2_decode_batch_kernel)
#define RS2_DECL_BATCH(CC)                                                                   \
  hipError_t rs2k_launch_decode_batch_##CC(const rs2::CodecJobBatch* d_jobs, int n_blobs,  \
                                           int tiles_per_blob, int n_z, hipStream_t stream);
RS2_DECL_BATCH(1)
RS2_DECL_BATCH(2)
RS2_DECL_BATCH(4)
RS2_DECL_BATCH(8)
RS2_DECL_BATCH(16)
RS2_DECL_BATCH(32)
RS2_DECL_BATCH(64)
RS2_DECL_BATCH(128)
RS2_DECL_BATCH(256)
RS2_DECL_BATCH(512)
#undef RS2_DECL_BATCH
// encode groups of a mixed sliver verification (rs2_encode_groups_kernel): a tile range per job
#define RS2_DECL_GROUPS(CC)                                                                    \
  hipError_t rs2k_launch_encode_groups_##CC(const rs2::CodecJobBatch* d_jobs,                 \
                                            const uint32_t* d_tile_first, int n_jobs,         \
                                            int n_tiles, int n_z, int mode, hipStream_t stream);
RS2_DECL_GROUPS(1)
RS2_DECL_GROUPS(2)
RS2_DECL_GROUPS(4)
RS2_DECL_GROUPS(8)
RS2_DECL_GROUPS(16)
RS2_DECL_GROUPS(32)
RS2_DECL_GROUPS(64)
RS2_DECL_GROUPS(128)
RS2_DECL_GROUPS(256)
RS2_DECL_GROUPS(512)
#undef RS2_DECL_GROUPS
// decode ranges of a mixed sliver recovery (rs2_decode_ranges_kernel): a tile range per job
#define RS2_DECL_RANGES(CC)                                                                    \
  hipError_t rs2k_launch_decode_ranges_##CC(const rs2::CodecJobBatch* d_jobs,                 \
                                            const uint32_t* d_tile_first, int n_jobs,         \
                                            int n_tiles, int n_z, hipStream_t stream);
RS2_DECL_RANGES(1)
RS2_DECL_RANGES(2)
RS2_DECL_RANGES(4)
RS2_DECL_RANGES(8)
RS2_DECL_RANGES(16)
RS2_DECL_RANGES(32)
RS2_DECL_RANGES(64)
RS2_DECL_RANGES(128)
RS2_DECL_RANGES(256)
RS2_DECL_RANGES(512)
#undef RS2_DECL_RANGES
// leaf digests of the received symbols of a mixed proof check (leaf_hash_runs_kernel): d_runs
// holds n_slivers SymbolRun; max_count: the largest symbol count of a sliver (grid.x)
hipError_t rs2k_launch_leaf_hash_runs(const rs2::SymbolRun* d_runs, int n_slivers,
                                      uint32_t max_count, uint8_t* d_digests, hipStream_t stream);
// mixed sliver verification, one window: the slots' slivers gathered (d_slots: n_slots + 1
// SliverSlot, the last one's chunk0 the launch's chunks), the eligible slots' leaves (d_groups:
// n_groups + 1 SliverLeafGroup, leaf (slot, c) at d_leaves + (slot * n + c) * 32), and the roots
// and verdicts of the window's `count` caller entries (d_slot_of[i]: slot or kSliverSkipped;
// d_roots / d_expected / d_verdict at the window's first entry, each may be null)
hipError_t rs2k_launch_sliver_gather(const rs2::SliverSlot* d_slots, int n_slots, int64_t n_chunks,
                                     uint8_t* d_dst, hipStream_t stream);
hipError_t rs2k_launch_leaf_hash_groups(const rs2::SliverLeafGroup* d_groups, int n_groups,
                                        int n_slots, int n, uint8_t* d_leaves, hipStream_t stream);
hipError_t rs2k_launch_sliver_finish(const uint8_t* d_slot_roots, const uint32_t* d_slot_of,
                                     int count, const uint8_t* d_expected, uint8_t* d_roots,
                                     int32_t* d_verdict, hipStream_t stream);
// mixed blob encode, one window: the eligible blobs' messages staged into their systematic primary
// slivers (d_blobs: n_blobs + 1 BlobStage, the last one's chunk0 the launch's chunks), their
// leaves (d_blobs: n_blobs + 1 BlobLeaves, the last one's first_tile the launch's tiles; n_tiles
// that count), and their pair hashes and ids from slot order to the caller's blobs
// (d_dst_index[slot]: the blob)
hipError_t rs2k_launch_blob_stage(const rs2::BlobStage* d_blobs, int n_blobs, int64_t n_chunks,
                                  int kp, int ks, hipStream_t stream);
hipError_t rs2k_launch_leaf_hash_blobs(const rs2::BlobLeaves* d_blobs, int n_blobs, int64_t n_tiles,
                                       int n, int kp, int ks, hipStream_t stream);
hipError_t rs2k_launch_blob_meta_scatter(const uint8_t* d_hashes, const uint8_t* d_ids,
                                         const uint32_t* d_dst_index, int n_slots, int n,
                                         uint8_t* d_hashes_out, uint8_t* d_ids_out,
                                         hipStream_t stream);
hipError_t rs2k_launch_leaf_hash(rs2::SymbolMap map, int mode, int64_t count, int n_blobs,
                                 uint8_t* d_out, hipStream_t stream);
hipError_t rs2k_launch_merkle_trees(const uint8_t* d_leaves, int n, int n_row_trees,
                                    int n_col_trees, int64_t row_base, int64_t row_stride,
                                    int64_t col_base, int64_t col_stride, uint8_t* d_out,
                                    int64_t out_stride, hipStream_t stream,
                                    uint8_t* d_nodes = nullptr, int64_t nodes_stride = 0,
                                    int n_blobs = 1, int64_t leaves_blob_stride = 0,
                                    int64_t out_blob_stride = 0, uint8_t* d_scratch = nullptr);
hipError_t rs2k_launch_batch_blob_copy(const uint8_t* src, int64_t src_stride,
                                       const uint64_t* d_blob_lens, int64_t msg, uint8_t* dst,
                                       int64_t dst_stride, int n_blobs, hipStream_t stream);
hipError_t rs2k_launch_proof_gather(const uint8_t* d_sys, const uint8_t* d_rep, int n, int k,
                                    int s, const uint8_t* d_nodes, int64_t nodes_stride,
                                    const uint16_t* d_targets, int count, int path_len,
                                    uint8_t* d_sym, uint8_t* d_proof, hipStream_t stream);
// one window of a bulk recovery-symbol call: d_sys / d_rep / d_nodes at the window's first sliver,
// d_requests its `count` entries (slot << 16 | target), d_sym / d_proof at its first request
hipError_t rs2k_launch_symbol_requests(const uint8_t* d_sys, const uint8_t* d_rep, int n, int k,
                                       int s, const uint8_t* d_nodes, int64_t nodes_stride,
                                       const uint32_t* d_requests, int64_t count, int path_len,
                                       rs2::SymbolLevels levels, uint8_t* d_sym, uint8_t* d_proof,
                                       hipStream_t stream);
// one window of a mixed recovery-symbol call: d_slots its n_slots SymbolSlot, d_requests `count`
// entries (slot << 16 | target, or kRequestSkipped), the first of them request r0 of the call;
// d_proof at the call's first request.  The scatter moves the window's trees from slot order
// (d_src) to d_dst + d_dst_index[slot] * n_nodes * 32.
hipError_t rs2k_launch_symbol_requests_slots(const rs2::SymbolSlot* d_slots, int n_slots,
                                             const uint32_t* d_requests, int64_t count, int64_t r0,
                                             int path_len, rs2::SymbolLevels levels,
                                             uint8_t* d_proof, hipStream_t stream);
hipError_t rs2k_launch_tree_nodes_scatter(const uint8_t* d_src, const uint32_t* d_dst_index,
                                          int n_slots, int64_t n_nodes, uint8_t* d_dst,
                                          hipStream_t stream);
hipError_t rs2k_launch_proof_roots(const uint8_t* d_leaf_digests, const uint32_t* d_leaf_index,
                                   const uint8_t* d_paths, int path_len, int count,
                                   uint8_t* d_roots, hipStream_t stream);
// d_per_sliver: n_slivers x {first symbol, target index} (uint32 pairs); max_count: the largest
// symbol count of a sliver (grid.x); total: symbols of the call
hipError_t rs2k_launch_recovery_proof_check(const uint8_t* d_leaf_digests,
                                            const uint32_t* d_per_sliver, int n_slivers,
                                            uint32_t max_count, uint32_t total,
                                            const uint8_t* d_paths, int path_len,
                                            const uint8_t* d_expected, uint8_t* d_ok,
                                            hipStream_t stream);
hipError_t rs2k_launch_sliver_verdict(const uint8_t* d_roots, const uint8_t* d_expected,
                                      const uint8_t* d_skipped, int count, int32_t* d_verdict,
                                      hipStream_t stream);
hipError_t rs2k_launch_merkle_root(const uint8_t* d_pair_hashes, int n, uint64_t blob_len,
                                   uint8_t* d_blob_id, hipStream_t stream, int n_blobs = 1,
                                   const uint64_t* d_blob_lens = nullptr);
hipError_t rs2k_launch_merkle_level(const uint8_t* d_in, int64_t cnt, uint8_t* d_out,
                                    hipStream_t stream);
hipError_t rs2k_launch_symbol_copy(const uint8_t* src, const int64_t* d_src_a, int64_t ssb,
                                   uint8_t* dst, const int64_t* d_dst_a, int64_t dsb, int count_a,
                                   int count_b, int s, int64_t dst_limit, hipStream_t stream);
hipError_t rs2k_launch_segment_copy(const uint8_t* src, uint8_t* dst, uint32_t count_a,
                                    const int64_t* d_src_a, const int64_t* d_dst_a, uint32_t count_b,
                                    int64_t ssb, int64_t dsb, uint32_t len, int unit,
                                    hipStream_t stream);
hipError_t rs2k_launch_quilt_layout(int n_rows, int n_cols, int s, const uint8_t* payload,
                                    const int64_t* col_off, const uint32_t* col_len,
                                    uint8_t* quilt, hipStream_t stream);
hipError_t rs2k_launch_host_upload(const void* src, void* dst, int64_t n, uint64_t* done,
                                   uint64_t gen, hipStream_t stream);
hipError_t rs2k_launch_upload_signal(uint64_t* done, uint64_t gen, hipStream_t stream);
hipError_t rs2k_launch_codec_big_512(const rs2::CodecJobBig* d_job, int n_tiles, int n_lines,
                                     int n_z, int mode, hipStream_t stream);
hipError_t rs2k_launch_tail_rows(const uint8_t* src, int64_t have, uint8_t* dst, int64_t total,
                                 hipStream_t stream);
hipError_t rs2k_launch_row_gather(const uint8_t* src, const int64_t* d_src_off, uint8_t* dst,
                                  int64_t row_bytes, int rows, hipStream_t stream);
// verified decode batches: the window's rows gathered back to back (d_rows: n_rows CheckRow),
// and the verdicts of its n_slots slots (d_roots: a root per row, or with `strict` an id per slot)
hipError_t rs2k_launch_check_rows_gather(const rs2::CheckRow* d_rows, int64_t n_rows,
                                         int64_t row_bytes, uint8_t* dst, hipStream_t stream);
hipError_t rs2k_launch_blob_verdict(const rs2::CheckSlot* d_slots, int n_slots,
                                    const rs2::CheckRow* d_rows, const uint8_t* d_roots,
                                    const uint8_t* d_expected, int64_t expected_stride, int strict,
                                    int32_t* d_verdict, hipStream_t stream);
hipError_t rs2k_launch_build_mul_tables(const uint16_t* d_exp, const uint16_t* d_log,
                                        const uint16_t* d_logs, int count, uint16_t* d_out,
                                        hipStream_t stream);
}
