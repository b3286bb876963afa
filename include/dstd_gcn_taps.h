/*
 * dstd_gcn_taps.h -- the sample-wise graphs and the block activations of an
 * eval forward, returned next to its output.
 *
 * With the reference (pure PyTorch) these are what a forward hook on conv_rm,
 * on a DSTDGCB or on an encoder sees.  Here a forward is one C call, so the
 * tap entry points below run the same forward and copy out, per DSTDGCB,
 *
 *   adj_s  the two constrained dynamic spatial adjacencies
 *          alpha_sm * conv_rm(tanh(P - Q)) + A_s * W_s + R_s   (model/dstdgcn.py:83-87, 146-149)
 *   adj_t  the dynamic temporal adjacency
 *          alpha_tm * conv_rm(tanh(P - Q)) + A_t + R_t         (:88-93, 158-160)
 *   x      the block's input
 *   h      prelu(bn(sum of the spatial GCs) + residual), the temporal GC's input (:151-154)
 *
 * Conventions are those of dstd_gcn.h: caller-owned dense contiguous fp32
 * device buffers, no allocation, no state, every launch enqueued on `stream`,
 * the same return codes.  Under the default (split-f16) arithmetic at the
 * shapes that have split kernels an adjacency is decoded from the hi/lo f16
 * planes the GC kernels contract -- (hi + lo) * 2^sa in fp32 -- so it holds the
 * numbers the forward actually used; everywhere else it is the fp32 adjacency
 * the exact kernels read.
 *
 * Schedule: a tap call runs the unit-parallel launch sequence at any batch
 * size (each adjacency and each graph convolution in a launch of its own), so
 * that the adjacencies exist in memory between launches.  The output y equals
 * the default forward's.
 */
#ifndef DSTD_GCN_TAPS_H
#define DSTD_GCN_TAPS_H

#include "dstd_gcn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What to copy out of one DSTDGCB.  Any member may be NULL: not wanted, not
 * written. */
typedef struct dstd_block_taps {
  float* adj_s; /* [B][2][T][V][V]  adj_s[n][i][t][v][w]: the matrix conv_s[i] contracts,
                   out[.., t, w] = sum_v xf[.., t, v] * adj_s[n][i][t][v][w] */
  float* adj_t; /* [B][V][T][T]     adj_t[n][v][t][u]: out[.., u, v] = sum_t xf[.., t, v] * adj_t[n][v][t][u] */
  float* x;     /* [B][cin][T][V]   the block's input, NCTV */
  float* h;     /* [B][cout][T][V]  the temporal GC's input, NCTV */
} dstd_block_taps;

/* The tap calls need no more scratch than the plain forwards. */
size_t dstd_block_taps_workspace_bytes(int B, int cin, int cout, int T, int V);
size_t dstd_model_taps_workspace_bytes(int B, int T, int V, int num_feature, int num_layers);

/* y = DSTDGCB(x) in eval mode with the block's taps.  flags: DSTD_FWD_EXACT_FP32
 * or 0; any other bit is DSTD_EINVAL.  Bad arguments and shapes outside the
 * envelope are refused before any GPU work, nothing is written. */
int dstd_block_fwd_taps(const dstd_block_params* p, const float* x, int B, int T, int V, float* y,
                        const dstd_block_taps* taps, void* workspace, size_t workspace_bytes, void* stream,
                        unsigned flags);

/* y = DSTDGCN(x) in eval mode with the taps of every block.  taps: num_layers
 * + 2 entries in forward order (conv_st_in, encoders 0.., conv_st_out); the x
 * of entry 0 is cat(x, x - x[:, -1]) in NCTV ([B][6][T][V]).  flags as above. */
int dstd_model_fwd_taps(const dstd_model_params* p, const float* x, int B, float* y, const dstd_block_taps* taps,
                        void* workspace, size_t workspace_bytes, void* stream, unsigned flags);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_TAPS_H */
