// Grouped evaluation (include/ext/dstd_gcn_eval.h): the per-frame test metric
// of a batch drawn from a device-resident set, accumulated per group by one
// launch that reads the targets from the resident frames.
//
// One workgroup per (eval frame, group).  The element loop and the reduction
// are k_frame_mpjpe's (dstd_train.hip): elements e = b * J + j strided over the
// workgroup, fmaf of the three squared differences, sqrtf, a per-thread sum,
// the wave64 butterfly and one value per wave through LDS, then thread 0 adds
// s / J.  A row of another group, or a skipped one, adds nothing to its
// thread's sum, so with one group and every row valid the sums are that
// kernel's bit for bit on the all_seqs dstd_batch_gather would have written.
// A (group, frame) pair belongs to one workgroup: no float atomics.  The
// index, group and start loads are per element but hit one cache line per
// row; at B = 256, J = 32 a workgroup walks 32 elements per thread.
#include "../../include/dstd_gcn.h"
#include "../../include/ext/dstd_gcn_eval.h"
#include "dstd_common.h"

namespace {

constexpr int kRedThreads = 256;

template <typename F>
__device__ __forceinline__ F block_sum(F v, F* red) {
  // wave64 butterfly, then one value per wave through LDS
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  F t = 0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
  return t;
}

// the frame row of batch row b at window frame f, if b is a row of group g
// whose window lies in the store; *mir: the window is a mirrored one
__device__ __forceinline__ const float* row_of(const dstd_seq_store& q, const long long* index, const int* group,
                                               int b, int f, int g, bool* mir) {
  long long w = index[b];
  const long long n_index = q.mirror_src ? 2 * q.N : q.N;
  if (w < 0 || w >= n_index) return nullptr;
  if ((group ? group[w] : 0) != g) return nullptr;
  *mir = w >= q.N;
  if (*mir) w -= q.N;
  const long long st = q.starts[w];
  if (st < 0 || st > q.F - q.T) return nullptr;
  return q.frames + (st + f) * q.D;
}

// coordinate c of joint j of a row, as a (possibly mirrored) window shows it;
// false where the mirror table points outside the row
__device__ __forceinline__ bool load_joint(const dstd_seq_store& q, const float* row, int j, int c, bool mir,
                                           float* out) {
  if (!mir) {
    *out = row[3 * j + c];
    return true;
  }
  const int sj = q.mirror_src[j];
  if (sj < 0 || 3 * sj + 2 >= q.D) return false;
  const float v = row[3 * sj + c];
  *out = c == 0 ? -v : v;
  return true;
}

__global__ __launch_bounds__(kRedThreads) void k_store_group_mpjpe(dstd_seq_store q, const long long* index, int B,
                                                                   const float* outs, int t_out0,
                                                                   const int* used_pos, int n_used,
                                                                   const int* joint_src, const int* frames,
                                                                   const int* group, float* sums, int* counts) {
  __shared__ float red[kRedThreads / 64];
  __shared__ int redi[kRedThreads / 64];
  const int k = blockIdx.x, g = blockIdx.y, f = frames[k], J = q.D / 3, K = gridDim.x;
  const bool frame_ok = f >= 0 && f < q.T;
  if (k == 0) {  // the rows of this group, whatever the frame tables hold
    int n = 0;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
      bool mir;
      n += row_of(q, index, group, b, 0, g, &mir) != nullptr;
    }
    n = block_sum(n, redi);
    if (threadIdx.x == 0) counts[g] += n;
  }
  if (!frame_ok) return;  // uniform per workgroup
  float s = 0.f;
  int bad = 0;
  for (int e = threadIdx.x; e < B * J; e += blockDim.x) {
    const int n = e / J, j = e - n * J;
    bool mir;
    const float* tg = row_of(q, index, group, n, f, g, &mir);
    if (!tg) continue;
    const int src = joint_src[j];
    if (src < 0 || src >= J) {
      bad = 1;
      continue;
    }
    float acc = 0.f;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int d = 3 * src + c;
      const int u = used_pos[d];
      float tv, pv;
      ok = ok && u < n_used && load_joint(q, tg, j, c, mir, &tv);
      if (!ok) break;
      if (u >= 0 && f >= t_out0)
        pv = outs[((size_t)n * (q.T - t_out0) + (f - t_out0)) * n_used + u];
      else
        ok = load_joint(q, tg, src, c, mir, &pv);
      if (!ok) break;
      const float df = tv - pv;
      acc = fmaf(df, df, acc);
    }
    if (!ok) {
      bad = 1;
      continue;
    }
    s += sqrtf(acc);
  }
  s = block_sum(s, red);
  // a table entry out of range: the pair is left as it was
  if (__syncthreads_or(bad)) return;
  if (threadIdx.x == 0) sums[(size_t)g * K + k] += s / J;
}

}  // namespace

extern "C" {

int dstd_store_group_mpjpe(const dstd_seq_store* s, const long long* index, int B, const float* outputs, int t_out0,
                           const int* used_pos, int n_used, const int* joint_src, const int* frames, int n_frames,
                           const int* group, int n_groups, float* sums, int* counts, void* stream) {
  if (!s || !index || !outputs || !used_pos || !joint_src || !frames || !sums || !counts) return DSTD_EINVAL;
  if (!s->frames || !s->starts) return DSTD_EINVAL;
  if (B <= 0 || n_frames <= 0 || n_groups <= 0 || n_used <= 0) return DSTD_EINVAL;
  if (s->T < 1 || s->F < 1 || s->N < 1 || s->D % 3 != 0 || s->D < 3) return DSTD_EINVAL;
  if (t_out0 < 0 || t_out0 >= s->T) return DSTD_EINVAL;
  if (n_groups > DSTD_EVAL_MAX_GROUPS) return DSTD_ELIMIT;
  if ((long long)B * (s->D / 3) > 0x7fffffffLL) return DSTD_ELIMIT;  // the element loop counts in int
  StreamDeviceGuard dev_guard_(stream, s->frames);
  k_store_group_mpjpe<<<dim3(n_frames, n_groups), kRedThreads, 0, (hipStream_t)stream>>>(
      *s, index, B, outputs, t_out0, used_pos, n_used, joint_src, frames, group, sums, counts);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? DSTD_OK : (int)err;
}

}  // extern "C"
