// The window kernels of a rollout's forward, shared by dstd_predict.hip (eval
// forward) and dstd_rollout.hip (train forward): include/dstd_gcn_predict.h
// states what they compute.
//
// Destination-driven, as dstd_data.hip: a wave owns row (b, s) of a window and
// its lanes walk the row's consecutive floats, so every load and store is a
// contiguous run.  Plain dword accesses: rows are V * 3 = 66 / 69 / 75 floats,
// only 4-byte aligned, and a B = 256 window is 2.4 MB -- the launch is
// latency-bound.  64-bit element offsets, no LDS, no atomics; the row
// arithmetic is wave-uniform.
//
// Everything here has internal linkage: each translation unit that includes
// this header compiles its own copy of the two kernels.
#pragma once
#include "dstd_common.h"

namespace {

constexpr int kMaxBlocks = 1 << 16;  // grid cap; the rows beyond are reached by the grid-stride loop

// window 0: x0[b][s] = obs[b][min(s, Tin - 1)]
__global__ __launch_bounds__(DSTD_THREADS) void k_window_obs(const float* obs, float* x0, int B, int T, int Tin,
                                                             int R) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long rows = (long long)B * T;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / T;
    const int s = (int)(r - b * T);
    const float* src = obs + (b * Tin + (s < Tin ? s : Tin - 1)) * R;
    float* dst = x0 + r * R;
    for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
  }
}

// Between window k and k + 1, row (b, s) of the window:
//   out[b][f0 + s - Tin] = y[b][s]                       for s >= Tin while f0 + s - Tin < H   (f0 = k * Tout)
//   xn[b][s]             = seq[b][T - Tin + min(s, Tin - 1)], seq = x below Tin, y from Tin on
// xn == nullptr (after the last forward): the slice of out alone.
__global__ __launch_bounds__(DSTD_THREADS) void k_window_roll(const float* x, const float* y, float* out, float* xn,
                                                              int B, int T, int Tin, int R, int H, int f0) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long rows = (long long)B * T;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / T;
    const int s = (int)(r - b * T);
    const int f = f0 + s - Tin;
    if (s >= Tin && f < H) {
      const float* src = y + r * R;
      float* dst = out + (b * H + f) * R;
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
    }
    if (xn) {
      const int t = T - Tin + (s < Tin ? s : Tin - 1);  // Tout <= t <= T - 1
      const float* src = (t < Tin ? x : y) + (b * T + t) * R;
      float* dst = xn + r * R;
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
    }
  }
}

inline int row_grid(int B, int T) {
  const long long blocks = ((long long)B * T + DSTD_WAVES - 1) / DSTD_WAVES;
  return (int)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

inline size_t rup256(size_t n) { return (n + 255) & ~size_t(255); }
inline size_t window_bytes(int B, int T, int V) { return rup256((size_t)B * T * V * 3 * sizeof(float)); }

}  // namespace
