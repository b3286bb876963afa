// Augmenting gather (include/ext/dstd_gcn_augment.h): the batch of
// dstd_batch_gather (dstd_data.hip) with a per-sample affine transform of every
// joint and a counter-based jitter of the observed frames, in the same single
// launch.
//
// The shape of k_batch_gather: a wave owns destination row (b, s) of all four
// outputs and its lanes walk consecutive floats of that row.  The index, start,
// frame-map and xf loads are wave-uniform (the row comes from a readfirstlane
// of the wave number, so they are scalar loads where the compiler can prove
// them unclobbered).  No LDS, no atomics, 64-bit element offsets.
//
// A transformed column needs all three coordinates of its joint, so a lane
// reads three source floats where the plain gather reads one; the three lanes
// of a joint read the same 12 bytes, which one cache line serves.  The 12
// floats of the sample's [A | t] are loaded once per row; a lane computes all
// three components of its joint and keeps its own.
//
// Rounding: the header fixes q[c] = ((A0*x + A1*y) + A2*z) + t and
// inputs = clean + amp * (2u - 1) with every product and sum rounded to fp32 on
// its own.  HIP contracts a * b + c into an fma by default, and without
// OCML_BASIC_ROUNDED_OPERATIONS __fmul_rn / __fadd_rn are plain * and + that
// contract alike, so this file turns contraction off for all of its code
// (#pragma clang fp contract(off) below).  The only float multiply-adds left in
// the disassembly are the compiler's own expansion of the 64-bit division
// r / T; none touches a value.  2u - 1 is exact whether contracted or not.
//
// The kernel is instantiated per (transform, noise): without either it is
// k_batch_gather's copy loop -- no arithmetic touches a value, -0.0 stays -0.0
// -- and at amplitude 0 no "+ 0" is executed either.
#include "../../include/dstd_gcn.h"
#include "../../include/ext/dstd_gcn_augment.h"
#include "dstd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxBlocks = 1 << 16;  // grid cap; the rows beyond are reached by the grid-stride loop

// the splitmix64 finaliser, as k_dropout (dstd_train.hip) uses it
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

// Column c of frame row `row` as a (possibly mirrored, possibly transformed)
// window shows it; false where a table entry points outside the row.
template <bool XF>
__device__ __forceinline__ bool load_col(const dstd_seq_store& q, const float* row, int c, bool mir,
                                         const Affine& m, float* out) {
  if (c < 0 || c >= q.D) return false;
  const int j = c / 3, cc = c - 3 * j;
  int sj = j;
  if (mir) {
    sj = q.mirror_src[j];
    if (sj < 0 || 3 * sj + 2 >= q.D) return false;
  }
  if (!XF) {
    const float v = row[3 * sj + cc];
    *out = (mir && cc == 0) ? -v : v;
    return true;
  }
  float x = row[3 * sj];
  const float y = row[3 * sj + 1], z = row[3 * sj + 2];
  if (mir) x = -x;
  // all three components, then the lane's own: selecting among the RESULTS keeps
  // the twelve coefficients in scalar registers (selecting among the
  // coefficients becomes a dynamically indexed vector, which costs scratch)
  const float q0 = ((m.a00 * x + m.a01 * y) + m.a02 * z) + m.t0;
  const float q1 = ((m.a10 * x + m.a11 * y) + m.a12 * z) + m.t1;
  const float q2 = ((m.a20 * x + m.a21 * y) + m.a22 * z) + m.t2;
  *out = cc == 0 ? q0 : cc == 1 ? q1 : q2;  // three products, three sums, each rounded (contraction is off)
  return true;
}

template <bool XF, bool NOISE>
__global__ __launch_bounds__(DSTD_THREADS) void k_batch_gather_aug(dstd_seq_store q, const long long* index, int B,
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
    Affine m = {};
    if (XF) {
      const float* x = xf + b * 12;
      m = Affine{x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[9], x[10], x[11]};
    }
    const float* src = q.frames + (st + s) * q.D;
    if (all_seqs) {
      float* dst = all_seqs + r * q.D;
      for (int d = lane; d < q.D; d += DSTD_WAVE) {
        float v;
        if (load_col<XF>(q, src, d, mir, m, &v)) dst[d] = v;
      }
    }
    if (!inputs && !inputs_inv && !targets) continue;
    // the source frames of this destination row in the two input tensors
    const int fi = inputs ? q.frame_in[s] : -1;
    const int fv = inputs_inv ? q.frame_inv[s] : -1;
    const bool ok_i = fi >= 0 && fi < q.T, ok_v = fv >= 0 && fv < q.T;
    const long long o = r * q.Du;
    // noise keys of element k: ((w0 * T + f) * Du + k), f the SOURCE frame
    const unsigned long long key_i = ((unsigned long long)w0 * q.T + (ok_i ? fi : 0)) * q.Du;
    const unsigned long long key_v = ((unsigned long long)w0 * q.T + (ok_v ? fv : 0)) * q.Du;
    if (q.used) {  // never with XF: refused on the host
      const float* ut = q.used + (st + s) * q.Du;
      const float* ui = q.used + (st + (ok_i ? fi : 0)) * q.Du;
      const float* uv = q.used + (st + (ok_v ? fv : 0)) * q.Du;
      for (int k = lane; k < q.Du; k += DSTD_WAVE) {
        if (targets) targets[o + k] = ut[k];
        if (ok_i) inputs[o + k] = NOISE ? ui[k] + jitter(seed_mul, key_i + k, amp) : ui[k];
        if (ok_v) inputs_inv[o + k] = NOISE ? uv[k] + jitter(seed_mul, key_v + k, amp) : uv[k];
      }
    } else {
      const float* ri = q.frames + (st + (ok_i ? fi : 0)) * q.D;
      const float* rv = q.frames + (st + (ok_v ? fv : 0)) * q.D;
      for (int k = lane; k < q.Du; k += DSTD_WAVE) {
        const int c = q.dim_used[k];
        float v;
        if (targets && load_col<XF>(q, src, c, mir, m, &v)) targets[o + k] = v;
        if (ok_i && load_col<XF>(q, ri, c, mir, m, &v))
          inputs[o + k] = NOISE ? v + jitter(seed_mul, key_i + k, amp) : v;
        if (ok_v && load_col<XF>(q, rv, c, mir, m, &v))
          inputs_inv[o + k] = NOISE ? v + jitter(seed_mul, key_v + k, amp) : v;
      }
    }
  }
}

}  // namespace

extern "C" {

int dstd_batch_gather_aug(const dstd_seq_store* s, const long long* index, int B, const float* xf, float noise_amp,
                          unsigned long long seed, float* inputs, float* inputs_inv, float* targets, float* all_seqs,
                          void* stream) {
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
  auto* k = xf ? (noise ? k_batch_gather_aug<true, true> : k_batch_gather_aug<true, false>)
               : (noise ? k_batch_gather_aug<false, true> : k_batch_gather_aug<false, false>);
  k<<<grid, DSTD_THREADS, 0, (hipStream_t)stream>>>(*s, index, B, xf, noise_amp, seed_mul, inputs, inputs_inv,
                                                    targets, all_seqs);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? DSTD_OK : (int)err;
}

}  // extern "C"
