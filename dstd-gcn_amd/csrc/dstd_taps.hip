// Decode kernels of the tap entry points (include/dstd_gcn_taps.h, dstd_taps.h):
// a block's adjacency scratch -> the dense fp32 adjacency a caller receives.
// Not on the forward's hot path: they run only in a tap call, one launch per
// tapped adjacency, and are bound by the fp32 they store.
#include "dstd_taps.h"

#include "dstd_common.h"
#include "dstd_hilo.h"

namespace dstd {

namespace {

constexpr int kTapThreads = 256;

// 2^sa of planes whose HLJ_RM bound is bnd (dstd_hilo.h "range scaling": the
// writer stores 2^-sa Adj with sa = hl_range_shift(frexp exponent of the bound))
__device__ __forceinline__ float plane_upscale(float bnd) {
  const int sa = hl_range_shift((int)(__float_as_uint(bnd) >> 23) - 126);
  return __uint_as_float((uint32_t)(127 + sa) << 23);
}

// stored slot of contraction index p (the inverse of SlotMap::slot_idx; every
// K-step before the last holds all four lane groups, so goff(s) = 4 s)
__device__ __forceinline__ int slot_of(int p, int seq) {
  if (!seq) return p;  // interleaved: idx = 32 s + 8 kg + e
  const int s = p >> 5, r = p & 31;  // sequential: idx = 32 s + 16 (e >> 2) + 4 kg + (e & 3)
  return 8 * (4 * s + ((r & 15) >> 2)) + 4 * (r >> 4) + (r & 3);
}

// One workgroup per plane row.  The hi and lo planes arrive as 16-byte loads
// (8 slots of one column q each), (hi + lo) * 2^sa goes to an LDS tile
// [q][SL + 1] (odd stride: the transposed read below is conflict-free), and
// the tile leaves as out[p][q] with q on consecutive lanes.
__global__ __launch_bounds__(kTapThreads) void k_tap_decode_hl(TapDecodeHLArgs a) {
  extern __shared__ float tile[];
  const int tid = threadIdx.x;
  const int NA = a.NA, SL = a.SL, LS = SL + 1, ncol = NA * SL;
  const size_t row = blockIdx.x;
  const uint4* hi = reinterpret_cast<const uint4*>(a.planes + row * 2 * (size_t)ncol);
  const uint4* lo = hi + ncol / 8;
  float bnd = a.scale[0][HLS_BOUND];
  if (a.scale[1]) bnd = fmaxf(bnd, a.scale[1][HLS_BOUND]);
  const float up = plane_upscale(bnd);
  for (int i = tid; i < ncol / 8; i += kTapThreads) {
    const f16x8 h = __builtin_bit_cast(f16x8, hi[i]), l = __builtin_bit_cast(f16x8, lo[i]);
    const int c = 8 * i, q = c / SL, s0 = c - q * SL;
#pragma unroll
    for (int e = 0; e < 8; ++e) tile[q * LS + s0 + e] = ((float)h[e] + (float)l[e]) * up;
  }
  __syncthreads();
  float* o = a.out + row * (size_t)NA * NA;
  for (int i = tid; i < NA * NA; i += kTapThreads) {
    const int p = i / NA, q = i - p * NA;
    o[i] = tile[q * LS + min(slot_of(p, a.seq), SL - 1)];
  }
}

// One workgroup per 1024-float chunk of a row: a 16-byte load per lane into
// LDS, then four stores with consecutive lanes on consecutive floats.
__global__ __launch_bounds__(kTapThreads) void k_tap_compact(TapCompactArgs a, int chunks) {
  __shared__ float buf[4 * kTapThreads];
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x / chunks;
  const int c0 = (int)(blockIdx.x % chunks) * 4 * kTapThreads;
  if (c0 + 4 * tid < a.ld)
    *reinterpret_cast<float4*>(buf + 4 * tid) = *reinterpret_cast<const float4*>(a.src + row * a.ld + c0 + 4 * tid);
  __syncthreads();
  float* o = a.dst + row * a.n;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = k * kTapThreads + tid;
    if (c0 + c < a.n) o[c0 + c] = buf[c];
  }
}

}  // namespace

hipError_t launch_tap_decode_hl(const TapDecodeHLArgs& a, hipStream_t s) {
  if (!a.planes || !a.out || !a.scale[0] || a.rows <= 0 || a.rows > 0x7fffffffL || a.NA <= 0 || a.SL <= 0 ||
      a.SL % 8 != 0)
    return hipErrorInvalidValue;
  // every index has a stored slot
  const int last = a.seq ? 8 * (4 * ((a.NA - 1) >> 5) + ((((a.NA - 1) & 31) & 15) >> 2)) : a.NA - 1;
  const size_t lds = (size_t)a.NA * (a.SL + 1) * sizeof(float);
  if (last >= a.SL || lds > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tap_decode_hl, dim3((unsigned)a.rows), dim3(kTapThreads), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_tap_compact(const TapCompactArgs& a, hipStream_t s) {
  if (!a.src || !a.dst || a.rows <= 0 || a.n <= 0 || a.ld < a.n || a.ld % 4 != 0) return hipErrorInvalidValue;
  const int chunks = cdiv(a.ld, 4 * kTapThreads);
  if (a.rows * (long)chunks > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tap_compact, dim3((unsigned)(a.rows * chunks)), dim3(kTapThreads), 0, s, a, chunks);
  return hipGetLastError();
}

}  // namespace dstd
