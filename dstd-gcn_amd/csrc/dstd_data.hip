// Device-resident dataset (include/dstd_gcn_data.h): one launch assembles the
// reference loader's 4-tuple (inputs, inputs_inv, targets, all_seqs) of a batch
// from frames kept in device memory, through an index vector.
//
// Destination-driven: a wave owns destination row (b, s) of all four outputs
// and its lanes walk consecutive floats of that row, so every store is a
// contiguous run and every load is one too, except where dim_used skips
// columns or a mirrored window exchanges joints (runs of 3 floats).  Plain
// dword accesses: rows are 66 / 69 / 75 / 96 / 114 floats, only 4- or 8-byte
// aligned, and a B = 32 batch is 1.3 MB -- the launch is latency-bound, not
// bandwidth-bound.  No LDS, no atomics; the index, start and frame-map loads
// are wave-uniform.
#include "../../include/dstd_gcn.h"
#include "../../include/dstd_gcn_data.h"
#include "dstd_common.h"

namespace {

constexpr int kMaxBlocks = 1 << 16;  // grid cap; the rows beyond are reached by the grid-stride loop

// column c of frame row f, as a (possibly mirrored) window shows it; false
// where a table entry points outside the row
__device__ __forceinline__ bool load_col(const dstd_seq_store& q, const float* row, int c, bool mir, float* out) {
  if (c < 0 || c >= q.D) return false;
  if (!mir) {
    *out = row[c];
    return true;
  }
  const int j = c / 3, cc = c - 3 * j;
  const int sj = q.mirror_src[j];
  if (sj < 0 || 3 * sj + 2 >= q.D) return false;
  const float v = row[3 * sj + cc];
  *out = cc == 0 ? -v : v;
  return true;
}

__global__ __launch_bounds__(DSTD_THREADS) void k_batch_gather(dstd_seq_store q, const long long* index, int B,
                                                               float* inputs, float* inputs_inv, float* targets,
                                                               float* all_seqs) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long rows = (long long)B * q.T;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / q.T;
    const int s = (int)(r - b * q.T);
    long long w = index[b];
    bool mir = false;
    if (w >= q.N && q.mirror_src) {
      w -= q.N;
      mir = true;
    }
    if (w < 0 || w >= q.N) continue;
    const long long st = q.starts[w];
    if (st < 0 || st > q.F - q.T) continue;
    const float* src = q.frames + (st + s) * q.D;
    if (all_seqs) {
      float* dst = all_seqs + r * q.D;
      for (int d = lane; d < q.D; d += DSTD_WAVE) {
        float v;
        if (load_col(q, src, d, mir, &v)) dst[d] = v;
      }
    }
    if (!inputs && !inputs_inv && !targets) continue;
    // the source frames of this destination row in the two input tensors
    const int fi = inputs ? q.frame_in[s] : -1;
    const int fv = inputs_inv ? q.frame_inv[s] : -1;
    const bool ok_i = fi >= 0 && fi < q.T, ok_v = fv >= 0 && fv < q.T;
    const long long o = r * q.Du;
    if (q.used) {
      const float* ut = q.used + (st + s) * q.Du;
      const float* ui = q.used + (st + (ok_i ? fi : 0)) * q.Du;
      const float* uv = q.used + (st + (ok_v ? fv : 0)) * q.Du;
      for (int k = lane; k < q.Du; k += DSTD_WAVE) {
        if (targets) targets[o + k] = ut[k];
        if (ok_i) inputs[o + k] = ui[k];
        if (ok_v) inputs_inv[o + k] = uv[k];
      }
    } else {
      const float* ri = q.frames + (st + (ok_i ? fi : 0)) * q.D;
      const float* rv = q.frames + (st + (ok_v ? fv : 0)) * q.D;
      for (int k = lane; k < q.Du; k += DSTD_WAVE) {
        const int c = q.dim_used[k];
        float v;
        if (targets && load_col(q, src, c, mir, &v)) targets[o + k] = v;
        if (ok_i && load_col(q, ri, c, mir, &v)) inputs[o + k] = v;
        if (ok_v && load_col(q, rv, c, mir, &v)) inputs_inv[o + k] = v;
      }
    }
  }
}

}  // namespace

extern "C" {

int dstd_batch_gather(const dstd_seq_store* s, const long long* index, int B, float* inputs, float* inputs_inv,
                      float* targets, float* all_seqs, void* stream) {
  if (!s || !index || B <= 0) return DSTD_EINVAL;
  if (!s->frames || !s->starts || !s->dim_used || !s->frame_in || !s->frame_inv) return DSTD_EINVAL;
  if (s->T < 1 || s->F < 1 || s->N < 1 || s->D % 3 != 0 || s->Du < 1 || s->Du > s->D) return DSTD_EINVAL;
  if (!inputs && !inputs_inv && !targets && !all_seqs) return DSTD_EINVAL;
  if (s->used && s->mirror_src) return DSTD_EINVAL;
  StreamDeviceGuard dev_guard_(stream, s->frames);
  const long long rows = (long long)B * s->T;
  const long long blocks = (rows + DSTD_WAVES - 1) / DSTD_WAVES;
  const int grid = (int)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
  k_batch_gather<<<grid, DSTD_THREADS, 0, (hipStream_t)stream>>>(*s, index, B, inputs, inputs_inv, targets, all_seqs);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? DSTD_OK : (int)err;
}

}  // extern "C"
