// Weighted, multi-term training loss (include/dstd_gcn_loss.h): jl2 / tl2 / cl1 /
// cl2 of the reference's engine/utils/loss.py for the batch and its time
// reversal in one forward (partials + final) and one backward launch.
//
// A work item is one joint of one sample over a chunk of kChunk frames,
// walked in time with the previous frame's difference kept in registers: the
// item loads each of its elements once; tl2 adds one halo frame per chunk in
// the forward (two in the backward), and the backward stays a gather -- frame
// s collects from the differences s-1 and s, no two threads write one element.
// Reductions are per-thread sums in item order, a wave64 butterfly, a fixed
// order over the waves and over the kBlocks partials: no float atomics.
#include "../../include/dstd_gcn.h"
#include "../../include/dstd_gcn_loss.h"
#include "dstd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBlocks = 128;  // workgroups per problem, both kernels
constexpr int kChunk = 8;     // frames per work item
constexpr int kSums = 3;      // partial sums per problem: jl2, tl2, cl1 (= cl2)
constexpr unsigned kAllTerms = DSTD_LOSS_JL2 | DSTD_LOSS_TL2 | DSTD_LOSS_CL1 | DSTD_LOSS_CL2;

struct LossArgs {
  dstd_loss_problem p[2];
  float* dp[2];
};

struct Vec3 {
  float x, y, z;
};

__device__ __forceinline__ float block_sum(float v, float* red) {
  // wave64 butterfly, then one value per wave through LDS
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < kThreads / 64; ++i) t += red[i];
  return t;
}

// mean_j w_j in a fixed order (1 without weights); the same code in the
// forward's final stage and in the backward, so both use the same bits
__device__ __forceinline__ float mean_weight(const float* w, int V, float* red) {
  if (!w) return 1.f;
  float s = 0.f;
  for (int v = threadIdx.x; v < V; v += kThreads) s += w[v];
  return block_sum(s, red) / (float)V;
}

// pred - targ of joint v of sample b at pred frame s
__device__ __forceinline__ Vec3 diff_at(const dstd_loss_problem& q, int b, int s, int v) {
  const size_t ip = (((size_t)b * q.T + s) * q.V + v) * 3;
  const size_t it = (((size_t)b * q.targ_T + (q.targ_t0 + q.targ_step * s)) * q.V + v) * 3;
  return Vec3{q.pred[ip] - q.targ[it], q.pred[ip + 1] - q.targ[it + 1], q.pred[ip + 2] - q.targ[it + 2]};
}

__device__ __forceinline__ float norm3(const Vec3& a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }

__device__ __forceinline__ Vec3 sub3(const Vec3& a, const Vec3& b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }

// a / ||a||, 0 at the kink (torch.norm backward)
__device__ __forceinline__ Vec3 unit3(const Vec3& a) {
  const float n = norm3(a);
  const float f = n > 0.f ? 1.f / n : 0.f;
  return Vec3{f * a.x, f * a.y, f * a.z};
}

__device__ __forceinline__ float sign1(float a) { return a > 0.f ? 1.f : (a < 0.f ? -1.f : 0.f); }

// partials[(problem * kSums + k) * kBlocks + block]
__global__ __launch_bounds__(kThreads) void k_losses_partial(LossArgs a, unsigned terms, const float* w,
                                                             float* partials) {
  __shared__ float red[kThreads / 64];
  const dstd_loss_problem& q = a.p[blockIdx.y];
  const bool tl2 = terms & DSTD_LOSS_TL2;
  const int nch = cdiv(q.T, kChunk);
  const size_t items = (size_t)q.B * nch * q.V;
  float aj = 0.f, at = 0.f, ac = 0.f;
  for (size_t e = blockIdx.x * (size_t)kThreads + threadIdx.x; e < items; e += (size_t)kBlocks * kThreads) {
    const int v = (int)(e % q.V);
    const int c = (int)(e / q.V % nch);
    const int b = (int)(e / q.V / nch);
    const float wj = w ? w[v] : 1.f;
    const int s0 = c * kChunk, s1 = min(q.T, s0 + kChunk);
    Vec3 d = diff_at(q, b, s0, v);
    for (int s = s0; s < s1; ++s) {
      aj += wj * norm3(d);
      ac += wj * (fabsf(d.x) + fabsf(d.y) + fabsf(d.z));
      // the next frame: the chunk's own, or the halo tl2 needs across chunks
      if (s + 1 < s1 || (tl2 && s + 1 < q.T)) {
        const Vec3 n = diff_at(q, b, s + 1, v);
        if (tl2) at += wj * norm3(sub3(n, d));
        d = n;
      }
    }
  }
  const float sums[kSums] = {aj, at, ac};
  for (int k = 0; k < kSums; ++k) {
    const float t = block_sum(sums[k], red);
    if (threadIdx.x == 0) partials[((size_t)blockIdx.y * kSums + k) * kBlocks + blockIdx.x] = t;
  }
}

// one workgroup per problem
__global__ __launch_bounds__(kThreads) void k_losses_final(LossArgs a, unsigned terms, const float* w,
                                                           const float* partials, float* values) {
  __shared__ float red[kThreads / 64];
  const dstd_loss_problem& q = a.p[blockIdx.x];
  float t[kSums];
  for (int k = 0; k < kSums; ++k) {
    float s = 0.f;
    for (int e = threadIdx.x; e < kBlocks; e += kThreads) s += partials[((size_t)blockIdx.x * kSums + k) * kBlocks + e];
    t[k] = block_sum(s, red);
  }
  const float wbar = mean_weight(w, q.V, red);
  if (threadIdx.x == 0) {
    const float n = (float)((size_t)q.B * q.T * q.V);
    const float nt = (float)((size_t)q.B * (q.T - 1) * q.V);
    const float cl = t[2] / (3.f * n);
    float* out = values + (size_t)blockIdx.x * DSTD_LOSS_NTERMS;
    out[0] = (terms & DSTD_LOSS_JL2) ? wbar * t[0] / n : 0.f;
    out[1] = (terms & DSTD_LOSS_TL2) ? wbar * t[1] / nt : 0.f;
    out[2] = (terms & DSTD_LOSS_CL1) ? cl : 0.f;
    out[3] = (terms & DSTD_LOSS_CL2) ? cl : 0.f;
  }
}

__global__ __launch_bounds__(kThreads) void k_losses_bwd(LossArgs a, unsigned terms, const float* w,
                                                         const float* coef, float scale) {
  __shared__ float red[kThreads / 64];
  const dstd_loss_problem& q = a.p[blockIdx.y];
  float* dp = a.dp[blockIdx.y];
  const float* cf = coef + (size_t)blockIdx.y * DSTD_LOSS_NTERMS;
  const bool tl2 = terms & DSTD_LOSS_TL2;
  const float wbar = mean_weight(w, q.V, red);
  const float n = (float)((size_t)q.B * q.T * q.V);
  const float nt = (float)((size_t)q.B * (q.T - 1) * q.V);
  const float cj = (terms & DSTD_LOSS_JL2) ? cf[0] * scale * wbar / n : 0.f;
  const float ct = tl2 ? cf[1] * scale * wbar / nt : 0.f;
  const float cc = (((terms & DSTD_LOSS_CL1) ? cf[2] : 0.f) + ((terms & DSTD_LOSS_CL2) ? cf[3] : 0.f)) * scale / (3.f * n);
  const int nch = cdiv(q.T, kChunk);
  const size_t items = (size_t)q.B * nch * q.V;
  for (size_t e = blockIdx.x * (size_t)kThreads + threadIdx.x; e < items; e += (size_t)kBlocks * kThreads) {
    const int v = (int)(e % q.V);
    const int c = (int)(e / q.V % nch);
    const int b = (int)(e / q.V / nch);
    const float wj = w ? w[v] : 1.f;
    const float cjw = cj * wj, ctw = ct * wj, ccw = cc * wj;
    const int s0 = c * kChunk, s1 = min(q.T, s0 + kChunk);
    Vec3 d = diff_at(q, b, s0, v);
    // unit vector of the difference s-1 -> s (none before frame 0)
    Vec3 up = Vec3{0.f, 0.f, 0.f};
    if (tl2 && s0 > 0) up = unit3(sub3(d, diff_at(q, b, s0 - 1, v)));
    for (int s = s0; s < s1; ++s) {
      const Vec3 uj = unit3(d);
      Vec3 g = Vec3{cjw * uj.x + ccw * sign1(d.x), cjw * uj.y + ccw * sign1(d.y), cjw * uj.z + ccw * sign1(d.z)};
      Vec3 nx = d;
      Vec3 un = Vec3{0.f, 0.f, 0.f};  // difference s -> s+1 (none after the last frame)
      if (s + 1 < s1 || (tl2 && s + 1 < q.T)) {
        nx = diff_at(q, b, s + 1, v);
        if (tl2) un = unit3(sub3(nx, d));
      }
      if (tl2) {
        g.x += ctw * (up.x - un.x);
        g.y += ctw * (up.y - un.y);
        g.z += ctw * (up.z - un.z);
        up = un;
      }
      const size_t o = (((size_t)b * q.T + s) * q.V + v) * 3;
      dp[o] = g.x;
      dp[o + 1] = g.y;
      dp[o + 2] = g.z;
      d = nx;
    }
  }
}

// argument checks shared by the two entry points; no GPU call
bool problems_ok(const dstd_loss_problem* p, int n, unsigned terms) {
  if (!p || (n != 1 && n != 2) || terms == 0 || (terms & ~kAllTerms)) return false;
  for (int i = 0; i < n; ++i) {
    const dstd_loss_problem& q = p[i];
    if (!q.pred || !q.targ || q.B <= 0 || q.T <= 0 || q.V <= 0 || q.targ_T <= 0) return false;
    if (q.targ_step != 1 && q.targ_step != -1) return false;
    const long long last = (long long)q.targ_t0 + (long long)q.targ_step * (q.T - 1);
    if (q.targ_t0 < 0 || q.targ_t0 >= q.targ_T || last < 0 || last >= q.targ_T) return false;
    if ((terms & DSTD_LOSS_TL2) && q.T < 2) return false;  // the reference: mean of an empty tensor
    if (q.V != p[0].V) return false;
  }
  return true;
}

LossArgs pack(const dstd_loss_problem* p, int n, float* const* dpreds) {
  LossArgs a{};
  for (int i = 0; i < n; ++i) {
    a.p[i] = p[i];
    a.dp[i] = dpreds ? dpreds[i] : nullptr;
  }
  return a;
}

}  // namespace

extern "C" {

size_t dstd_losses_workspace_bytes(void) { return (size_t)2 * kSums * kBlocks * sizeof(float) + 256; }

int dstd_losses_fwd(const dstd_loss_problem* problems, int n_problems, unsigned terms, const float* joint_w,
                    float* values, void* workspace, size_t workspace_bytes, void* stream) {
  if (!problems_ok(problems, n_problems, terms) || !values || !workspace) return DSTD_EINVAL;
  if (workspace_bytes < dstd_losses_workspace_bytes()) return DSTD_EINVAL;
  StreamDeviceGuard dev_guard_(stream, problems[0].pred);
  const LossArgs a = pack(problems, n_problems, nullptr);
  hipStream_t s = (hipStream_t)stream;
  float* partials = (float*)workspace;
  k_losses_partial<<<dim3(kBlocks, n_problems), kThreads, 0, s>>>(a, terms, joint_w, partials);
  k_losses_final<<<n_problems, kThreads, 0, s>>>(a, terms, joint_w, partials, values);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? DSTD_OK : (int)err;
}

int dstd_losses_bwd(const dstd_loss_problem* problems, int n_problems, unsigned terms, const float* joint_w,
                    const float* coef, float scale, float* const* dpreds, void* stream) {
  if (!problems_ok(problems, n_problems, terms) || !coef || !dpreds) return DSTD_EINVAL;
  for (int i = 0; i < n_problems; ++i)
    if (!dpreds[i]) return DSTD_EINVAL;
  StreamDeviceGuard dev_guard_(stream, problems[0].pred);
  const LossArgs a = pack(problems, n_problems, dpreds);
  k_losses_bwd<<<dim3(kBlocks, n_problems), kThreads, 0, (hipStream_t)stream>>>(a, terms, joint_w, coef, scale);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? DSTD_OK : (int)err;
}

}  // extern "C"
