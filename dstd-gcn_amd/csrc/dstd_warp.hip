// Warping gather (include/ext/dstd_gcn_warp.h): the batch of
// dstd_batch_gather_aug (dstd_augment.hip) with every window resampled in time
// at a per-sample playback rate, in the same single launch.
//
// The shape of k_batch_gather_aug: a wave owns destination row (b, s) of all
// four outputs and its lanes walk consecutive floats of that row; the row comes
// from a readfirstlane of the wave number, so the index, start, room, rate,
// frame-map and xf loads are wave-uniform.  No LDS, no atomics, 64-bit element
// offsets.
//
// A destination row has up to three source positions: window frame s (all_seqs,
// targets), frame_in[s] (inputs) and frame_inv[s] (inputs_inv).  Each is a pair
// (i, a): source row i of the window and the weight of row i + 1.  The pair is
// the same in every lane; gfx950 has no scalar float arithmetic, so p = rate * f
// and its comparisons run on the vector unit and the pair goes back to scalar
// registers through readfirstlane.  `a == 0` is then a scalar branch: a
// position that falls on a stored frame copies it and does not touch row i + 1.
//
// Rounding: the header fixes x_i + a * (x_{i+1} - x_i) with the difference, the
// product and the sum each rounded to fp32 on its own, after the mirror and
// before the transform.  As in dstd_augment.hip, contraction is off for the
// whole file (#pragma clang fp contract(off) below), for the reason given there.
// The mirror's negation comes before the blend and not after it: the two orders
// differ in the sign of a zero sum.
//
// The kernel is instantiated per (warp, transform, noise).  Without a rate the
// positions are (s, 0), (frame_in[s], 0) and (frame_inv[s], 0) with no
// arithmetic, and the instance is k_batch_gather_aug's loop.
#include "../../include/dstd_gcn.h"
#include "../../include/ext/dstd_gcn_warp.h"
#include "dstd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxBlocks = 1 << 16;  // grid cap; the rows beyond are reached by the grid-stride loop
constexpr int kMaxRoom = 1 << 20;    // the header's cap of R: (float)R and (int)p are exact below it

// the splitmix64 finaliser, as k_batch_gather_aug (dstd_augment.hip) uses it
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

// amp * (2u - 1), u the 24-bit uniform of element `key` under the pre-multiplied seed
__device__ __forceinline__ float jitter(unsigned long long seed_mul, unsigned long long key, float amp) {
  const unsigned long long h = mix64(seed_mul + key);
  const float u = (float)(unsigned)(h >> 40) * (1.f / 16777216.f);  // [0, 1), 24 bits: exact
  return amp * (2.f * u - 1.f);                           // 2u - 1 exact, one rounding
}

// a sample's row-major 3x4 [A | t]
struct Affine {
  float a00, a01, a02, t0, a10, a11, a12, t1, a20, a21, a22, t2;
};

// where a window frame lies in the stored rows: row i of the window, blended
// with row i + 1 by a (0: row i alone)
struct Pos {
  int i;
  float a;
};

// The header's position of window frame f at playback rate `rate` with R rows
// of room; wave-uniform in, scalar registers out.
__device__ __forceinline__ Pos warp_pos(float rate, int f, int R) {
  const float p = rate * (float)f;  // one rounding
  int i = 0;
  float a = 0.f;
  if (p > 0.f) {  // false for 0, negatives and NaN
    if (p >= (float)R) {
      i = R;
    } else {
      i = (int)p;          // truncation; 0 <= i < R
      a = p - (float)i;    // exact
    }
  }
  return Pos{__builtin_amdgcn_readfirstlane(i),
             __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a)))};
}

// Column c of the row at `row` (`neg`: negated, the mirror's coordinate 0),
// blended with the row `pitch` floats further on when the position lies between
// two stored rows.
template <bool WARP>
__device__ __forceinline__ float blend(const float* row, long long pitch, int c, bool neg, float a) {
  float v = row[c];
  if (neg) v = -v;
  if (WARP && a != 0.f) {  // wave-uniform
    float v1 = row[pitch + c];
    if (neg) v1 = -v1;
    const float d = v1 - v;
    const float t = a * d;
    v = v + t;  // three roundings (contraction is off)
  }
  return v;
}

// Column c of the window frame at position (row, a) as a (possibly mirrored,
// possibly warped, possibly transformed) window shows it; false where a table
// entry points outside the row.
template <bool WARP, bool XF>
__device__ __forceinline__ bool load_col(const dstd_seq_store& q, const float* row, float a, int c, bool mir,
                                         const Affine& m, float* out) {
  if (c < 0 || c >= q.D) return false;
  const int j = c / 3, cc = c - 3 * j;
  int sj = j;
  if (mir) {
    sj = q.mirror_src[j];
    if (sj < 0 || 3 * sj + 2 >= q.D) return false;
  }
  if (!XF) {
    *out = blend<WARP>(row, q.D, 3 * sj + cc, mir && cc == 0, a);
    return true;
  }
  const float x = blend<WARP>(row, q.D, 3 * sj, mir, a);
  const float y = blend<WARP>(row, q.D, 3 * sj + 1, false, a);
  const float z = blend<WARP>(row, q.D, 3 * sj + 2, false, a);
  // all three components, then the lane's own (dstd_augment.hip load_col: the
  // twelve coefficients stay in scalar registers this way)
  const float q0 = ((m.a00 * x + m.a01 * y) + m.a02 * z) + m.t0;
  const float q1 = ((m.a10 * x + m.a11 * y) + m.a12 * z) + m.t1;
  const float q2 = ((m.a20 * x + m.a21 * y) + m.a22 * z) + m.t2;
  *out = cc == 0 ? q0 : cc == 1 ? q1 : q2;
  return true;
}

template <bool WARP, bool XF, bool NOISE>
__global__ __launch_bounds__(DSTD_THREADS) void k_batch_gather_warp(dstd_seq_store q, const int* room,
                                                                    const long long* index, int B, const float* rate,
                                                                    const float* xf, float amp,
                                                                    unsigned long long seed_mul, float* inputs,
                                                                    float* inputs_inv, float* targets,
                                                                    float* all_seqs) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long rows = (long long)B * q.T;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + wave; r < rows; r += stride) {
    const long long b = r / q.T;
    const int s = (int)(r - b * q.T);
    const long long w0 = index[b];  // the index value: what the noise is keyed by
    long long w = w0;
    bool mir = false;
    if (w >= q.N && q.mirror_src) {
      w -= q.N;
      mir = true;
    }
    if (w < 0 || w >= q.N) continue;
    const long long st = q.starts[w];
    if (st < 0 || st > q.F - q.T) continue;
    // rows st .. st + R may be read: R >= T - 1, and st + R <= F - 1
    const int rw = room ? room[w] : q.T - 1;
    if (rw < q.T - 1) continue;
    long long lim = q.F - 1 - st;
    if (rw < lim) lim = rw;
    const int R = (int)(lim < kMaxRoom ? lim : kMaxRoom);
    Affine m = {};
    if (XF) {
      const float* x = xf + b * 12;
      m = Affine{x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9], x[10], x[11]};
    }
    float speed = 1.f;
    if (WARP) speed = rate[b];
    const Pos ps = WARP ? warp_pos(speed, s, R) : Pos{s, 0.f};
    if (all_seqs) {
      const float* src = q.frames + (st + ps.i) * q.D;
      float* dst = all_seqs + r * q.D;
      for (int d = lane; d < q.D; d += DSTD_WAVE) {
        float v;
        if (load_col<WARP, XF>(q, src, ps.a, d, mir, m, &v)) dst[d] = v;
      }
    }
    if (!inputs && !inputs_inv && !targets) continue;
    // the window frames of this destination row in the two input tensors
    const int fi = inputs ? q.frame_in[s] : -1;
    const int fv = inputs_inv ? q.frame_inv[s] : -1;
    const bool ok_i = fi >= 0 && fi < q.T, ok_v = fv >= 0 && fv < q.T;
    const Pos pi = WARP ? warp_pos(speed, ok_i ? fi : 0, R) : Pos{ok_i ? fi : 0, 0.f};
    const Pos pv = WARP ? warp_pos(speed, ok_v ? fv : 0, R) : Pos{ok_v ? fv : 0, 0.f};
    const long long o = r * q.Du;
    // noise keys of element k: ((w0 * T + f) * Du + k), f the WINDOW frame
    const unsigned long long key_i = ((unsigned long long)w0 * q.T + (ok_i ? fi : 0)) * q.Du;
    const unsigned long long key_v = ((unsigned long long)w0 * q.T + (ok_v ? fv : 0)) * q.Du;
    if (q.used) {  // never with XF or a mirror: refused on the host
      const float* ut = q.used + (st + ps.i) * q.Du;
      const float* ui = q.used + (st + pi.i) * q.Du;
      const float* uv = q.used + (st + pv.i) * q.Du;
      for (int k = lane; k < q.Du; k += DSTD_WAVE) {
        if (targets) targets[o + k] = blend<WARP>(ut, q.Du, k, false, ps.a);
        if (ok_i) {
          const float v = blend<WARP>(ui, q.Du, k, false, pi.a);
          inputs[o + k] = NOISE ? v + jitter(seed_mul, key_i + k, amp) : v;
        }
        if (ok_v) {
          const float v = blend<WARP>(uv, q.Du, k, false, pv.a);
          inputs_inv[o + k] = NOISE ? v + jitter(seed_mul, key_v + k, amp) : v;
        }
      }
    } else {
      const float* rt = q.frames + (st + ps.i) * q.D;
      const float* ri = q.frames + (st + pi.i) * q.D;
      const float* rv = q.frames + (st + pv.i) * q.D;
      for (int k = lane; k < q.Du; k += DSTD_WAVE) {
        const int c = q.dim_used[k];
        float v;
        if (targets && load_col<WARP, XF>(q, rt, ps.a, c, mir, m, &v)) targets[o + k] = v;
        if (ok_i && load_col<WARP, XF>(q, ri, pi.a, c, mir, m, &v))
          inputs[o + k] = NOISE ? v + jitter(seed_mul, key_i + k, amp) : v;
        if (ok_v && load_col<WARP, XF>(q, rv, pv.a, c, mir, m, &v))
          inputs_inv[o + k] = NOISE ? v + jitter(seed_mul, key_v + k, amp) : v;
      }
    }
  }
}

template <bool WARP, bool XF>
auto* pick_noise(bool noise) {
  return noise ? k_batch_gather_warp<WARP, XF, true> : k_batch_gather_warp<WARP, XF, false>;
}

template <bool WARP>
auto* pick_xf(bool xf, bool noise) {
  return xf ? pick_noise<WARP, true>(noise) : pick_noise<WARP, false>(noise);
}

}  // namespace

extern "C" {

int dstd_batch_gather_warp(const dstd_seq_store* s, const int* room, const long long* index, int B,
                           const float* rate, const float* xf, float noise_amp, unsigned long long seed,
                           float* inputs, float* inputs_inv, float* targets, float* all_seqs, void* stream) {
  if (!s || !index || B <= 0) return DSTD_EINVAL;
  if (!s->frames || !s->starts || !s->dim_used || !s->frame_in || !s->frame_inv) return DSTD_EINVAL;
  if (s->T < 1 || s->F < 1 || s->N < 1 || s->D % 3 != 0 || s->Du < 1 || s->Du > s->D) return DSTD_EINVAL;
  if (!inputs && !inputs_inv && !targets && !all_seqs) return DSTD_EINVAL;
  if (s->used && s->mirror_src) return DSTD_EINVAL;
  if (xf && s->used) return DSTD_EINVAL;
  if (!(noise_amp >= 0.f) || noise_amp > 3.402823466e+38f) return DSTD_EINVAL;  // negative, NaN, infinite
  StreamDeviceGuard dev_guard_(stream, s->frames);
  const long long rows = (long long)B * s->T;
  const long long blocks = (rows + DSTD_WAVES - 1) / DSTD_WAVES;
  const int grid = (int)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
  const bool noise = noise_amp > 0.f;
  const unsigned long long seed_mul = seed * 0x9e3779b97f4a7c15ULL;
  auto* k = rate ? pick_xf<true>(xf != nullptr, noise) : pick_xf<false>(xf != nullptr, noise);
  k<<<grid, DSTD_THREADS, 0, (hipStream_t)stream>>>(*s, room, index, B, rate, xf, noise_amp, seed_mul, inputs,
                                                    inputs_inv, targets, all_seqs);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? DSTD_OK : (int)err;
}

}  // extern "C"
