// Decode launches of the tap entry points (include/dstd_gcn_taps.h): the
// adjacency scratch of a block, in either of its two formats, to the dense
// fp32 layouts a caller receives.  dstd_capi.hip issues one launch per
// tapped adjacency, right after the launch that wrote the scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dstd {

// Split-f16 planes (dstd_hilo.h): rows of [2 planes][NA][SL] halves, row =
// (sample, graph, frame) spatial / (sample, joint) temporal, plane row q
// holding, in slot order, 2^-sa Adj[p = slot_idx(slot)][q].
//   out[row][p][q] = (hi + lo) * 2^sa          (fp32; pad slots dropped)
// sa is the range shift of the planes, from the HLS_BOUND field of the conv_rm
// scale slot(s) exactly as the writer (k_adj_hl) and the GC kernels take it.
struct TapDecodeHLArgs {
  const uint16_t* planes;
  float* out;          // [rows][NA][NA]
  long rows;
  int NA, SL;
  int seq;             // slot order: 0 interleaved (SlotMap<V, true>, spatial), 1 sequential (SlotMap<T, false>)
  const float* scale[2];  // HLJ_RM scale slots; [1] null for one graph, else both graphs share max(bound)
};
// fp32 rows (exact arithmetic, generic shapes): rows of ld floats, the first
// n valid, compacted to dst[rows][n].
struct TapCompactArgs {
  const float* src;
  float* dst;
  long rows;
  int n, ld;           // ld a multiple of 4 (adj_ld_spatial / adj_ld_temporal)
};

hipError_t launch_tap_decode_hl(const TapDecodeHLArgs& a, hipStream_t s);
hipError_t launch_tap_compact(const TapCompactArgs& a, hipStream_t s);

}  // namespace dstd
