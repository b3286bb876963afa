/*
 * dstd_gcn.h -- C ABI of the MI355X-native DSTDGC hot path.
 *
 * The reference (Jaakk0F/DSTD-GCN) is pure PyTorch: its "FFI" for this path is
 * the nn.Module API in /root/reference/model/dstdgcn.py.  Each entry point
 * below replaces one forward of that API; the Python host layer
 * (dstd-gcn_amd/model/dstdgcn.py) binds them with ctypes exactly as
 * INTEGRATION.md shows.
 *
 *   dstd_dstdgc_fwd   <- DSTDGC.forward      model/dstdgcn.py:80-94
 *   dstd_block_fwd    <- DSTDGCB.forward     model/dstdgcn.py:141-163
 *   dstd_model_fwd    <- DSTDGCN.forward     model/dstdgcn.py:293-317 (eval)
 *
 * Conventions
 *   - All tensors are device pointers to contiguous fp32.  Activations at the
 *     op / block boundary are NCTV ([B][C][T][V], the reference layout); the
 *     model boundary is [B][T][V][3] in and out (model/dstdgcn.py:295, 314).
 *   - Weights are passed per call, in the reference's shapes: conv weights
 *     [O][I] (the trailing 1x1 of Conv2d is dropped), BN vectors [C*V].
 *   - Scalars that are nn.Parameters (alpha_sm, alpha_tm, PReLU slopes) are
 *     device pointers to one float so a call never synchronises.
 *   - Scratch comes from a caller-owned workspace of at least
 *     dstd_*_workspace_bytes(...) bytes; the library allocates nothing and
 *     keeps no state, so calls may be captured into a HIP graph.  A call
 *     reads no byte of the workspace that it has not written itself and
 *     writes none past the size it asked for; a refused call writes nothing
 *     (tests/test_gpu_guards.py).
 *   - The workspace base (and a train forward's `saved` base) must be aligned
 *     to 256 bytes.  The regions carved from it start at offsets rounded up to
 *     256 bytes from the base, and kernels address them with 16-byte vector
 *     loads and stores (the split-f16 weight images are read as uint4), so a
 *     base of lesser alignment misaligns every region.  This is a requirement
 *     on the caller; the entry points do not check it.
 *   - Every call is enqueued on `stream` (hipStream_t passed as void*).
 *   - Return 0 on success, a positive hipError_t from a failed launch, or a
 *     negative DSTD_E* code for bad arguments.  dstd_error_string() names it.
 *   - Limits: T <= 128, V <= 32, channels <= 64, red_channels == 2 (any other
 *     red_channels: dstd_dstdgc_train_fwd_r in dstd_gcn_train.h).
 */
#ifndef DSTD_GCN_H
#define DSTD_GCN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSTD_OK 0
#define DSTD_EINVAL -1      /* bad shape / null pointer */
#define DSTD_EWORKSPACE -2  /* workspace too small */
#define DSTD_ELIMIT -3      /* shape outside the supported envelope */
#define DSTD_ECOLLECTIVE -5 /* a caller-supplied collective returned non-zero (dstd_bn_sync, dstd_gcn_train.h) */

#define DSTD_MODE_SPATIAL 0
#define DSTD_MODE_TEMPORAL 1
#define DSTD_MAX_LAYERS 16

/* One DSTDGC (model/dstdgcn.py:53-94).  Shapes: wf [cout][cin], bf [cout],
 * wm1/wm2 [2][cin], bm1/bm2 [2], wrm [ref][2*ref], brm [ref]
 * (ref = T for spatial, V for temporal). */
typedef struct dstd_gc_weights {
  const float* wf;
  const float* bf;
  const float* wm1;
  const float* bm1;
  const float* wm2;
  const float* bm2;
  const float* wrm;
  const float* brm;
} dstd_gc_weights;

/* BatchNorm wrapper (model/dstdgcn.py:35-50): nn.BatchNorm1d(C*V), eval mode.
 * All four vectors are [C*V] with channel index c*V + v. */
typedef struct dstd_bn {
  const float* weight;
  const float* bias;
  const float* running_mean;
  const float* running_var;
  float eps;
} dstd_bn;

/* DSTDGCB (model/dstdgcn.py:97-163).  A_s may alias R_s (it does in the
 * reference, :107-109); the runtime adjacency is A_s*W_s + R_s per graph. */
typedef struct dstd_block_params {
  int cin, cout;
  const float* A_s;      /* [2][V][V] */
  const float* W_s;      /* [2][V][V] */
  const float* R_s;      /* [2][V][V] */
  const float* A_t;      /* [1][T][T] */
  const float* R_t;      /* [1][T][T] */
  const float* alpha_sm; /* [1] */
  const float* alpha_tm; /* [1] */
  dstd_gc_weights conv_s[2];
  dstd_gc_weights conv_t;
  dstd_bn bn;
  const float* prelu;    /* [1] */
  const float* res_w;    /* [cout][cin] or NULL when cin == cout */
  const float* res_b;    /* [cout] */
  dstd_bn res_bn;
} dstd_block_params;

/* DSTDGCN (model/dstdgcn.py:252-317). */
typedef struct dstd_model_params {
  int T, V, num_layers, num_feature, in_channels;
  dstd_block_params st_in;                  /* conv_st_in.stgcn.0.0 */
  dstd_bn bn_in;                            /* bn_in.bn */
  const float* prelu;                       /* prelu.weight */
  dstd_block_params enc[DSTD_MAX_LAYERS];   /* encoders.<i>.0.stgcn.0.0 */
  dstd_bn enc_bn[DSTD_MAX_LAYERS];          /* encoders.<i>.1.bn */
  const float* enc_prelu[DSTD_MAX_LAYERS];  /* encoders.<i>.2.weight */
  dstd_block_params st_out;                 /* conv_st_out.stgcn.0.0 */
} dstd_model_params;

const char* dstd_version(void);
/* sha256 (first 16 hex digits) of the sources this library was built from
 * (dstd-gcn_amd/Makefile HASHED): ties a shipped binary to its tree. */
const char* dstd_source_hash(void);
const char* dstd_error_string(int code);

size_t dstd_dstdgc_workspace_bytes(int mode, int B, int cin, int cout, int T, int V);
size_t dstd_block_workspace_bytes(int B, int cin, int cout, int T, int V);
size_t dstd_model_workspace_bytes(int B, int T, int V, int num_feature, int num_layers);

/* y = DSTDGC(x, A, alpha); x [B][cin][T][V] -> y [B][cout][T][V].
 * A: [V][V] (spatial) or [T][T] (temporal), already combined by the caller
 * (DSTDGCB passes A_s*W_s+R_s or A_t+R_t). */
int dstd_dstdgc_fwd(int mode, const float* x, int B, int cin, int cout, int T, int V,
                    const dstd_gc_weights* w, const float* A, const float* alpha, float* y,
                    void* workspace, size_t workspace_bytes, void* stream);

/* y = DSTDGCB(x) in eval mode; x [B][cin][T][V] -> y [B][cout][T][V]. */
int dstd_block_fwd(const dstd_block_params* p, const float* x, int B, int T, int V, float* y,
                   void* workspace, size_t workspace_bytes, void* stream);
/* dstd_block_fwd with flags (DSTD_FWD_EXACT_FP32, DSTD_FWD_FUSED_TEMPORAL). */
int dstd_block_fwd_ex(const dstd_block_params* p, const float* x, int B, int T, int V, float* y,
                      void* workspace, size_t workspace_bytes, void* stream, unsigned flags);

/* y = DSTDGCN(x) in eval mode; x, y [B][T][V][in_channels/2]. */
int dstd_model_fwd(const dstd_model_params* p, const float* x, int B, float* y, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- measurement hooks (bench.py) ---------------------------------------
 * Kernel families of one forward, in launch order per DSTDGCB:
 *   ADJ_S (tanh GEMM, both graphs), SPATIAL (spatial GC + mid epilogue),
 *   ADJ_T (tanh GEMM), TEMPORAL (temporal GC + tail epilogue); BLOCK: the
 *   whole DSTDGCB in one launch (spatial + temporal GC, DSTD_FWD_SEPARATE_BLOCK). */
#define DSTD_KIND_FOLD 0
#define DSTD_KIND_PREP 1
#define DSTD_KIND_ADJ_S 2
#define DSTD_KIND_SPATIAL 3
#define DSTD_KIND_ADJ_T 4
#define DSTD_KIND_TEMPORAL 5
#define DSTD_KIND_BLOCK 6
#define DSTD_KIND_COUNT 7

/* Every launch whose family bit is set in kind_mask is bracketed by a
 * (start, stop) pair of hipEvents taken from events[2*i], events[2*i+1];
 * kinds[i] and block[i] record the family and the DSTDGCB index (-1 outside
 * blocks).  The call appends at `count` (pairs) and stops recording when
 * `capacity` pairs are used.  Events come from dstd_events_create. */
typedef struct dstd_profile {
  unsigned kind_mask;
  int capacity;
  int count;
  void** events;
  int* kinds;
  int* block;
  int only_block; /* >= 0: bracket only launches of that DSTDGCB (two events per
                     forward keep the timed region close to an unprofiled one) */
} dstd_profile;

int dstd_model_fwd_profiled(const dstd_model_params* p, const float* x, int B, float* y, void* workspace,
                            size_t workspace_bytes, void* stream, dstd_profile* prof);

/* dstd_model_fwd with flags (and an optional profile, as _profiled).
 * DSTD_FWD_REUSE_CONSTANTS: the workspace still holds the folded constants
 * and split-f16 weight images of a previous forward of the SAME parameters
 * (same pointers, unmodified values), batch size and workspace, so the two
 * parameter-preparation launches are skipped.  The caller vouches for it
 * (the Python layer checks torch's per-tensor version counters). */
#define DSTD_FWD_REUSE_CONSTANTS 1u
/* Arithmetic of the graph convolutions, per call (no process-wide state).
 * Default (flag clear): split-f16 MFMA -- each fp32 operand as an f16 hi/lo
 * pair under a power-of-two range scale, three v_mfma_f32_16x16x32_f16 per
 * product, fp32 accumulation -- where the shape has kernels: (T, V) in
 * {(35,22), (35,25), (40,23), (75,22)}, Cin/Cout 64 (6 -> 64 and 64 -> 3 at
 * the model's ends); everything else exact fp32.  DSTD_FWD_EXACT_FP32: the
 * exact-fp32 MFMA kernels (v_mfma_f32_16x16x4_f32) everywhere.  Both stay
 * within the reference parity bars over the whole fp32 range
 * (tests/test_gpu_parity.py).  No counterpart in the reference (pure fp32
 * ATen, model/dstdgcn.py:80-94). */
#define DSTD_FWD_EXACT_FP32 2u
/* Launch schedule, for A/B and the bit-identity test (same results either
 * way): every block's spatial adjacency planes in a launch of their own
 * (k_adj_hl<0>) instead of built by the previous block's fused temporal
 * launch after its units (phase 3, the default) -- and block 0's, built from
 * the model input, in its own launch instead of inside block 0's
 * k_block_fused launch. */
#define DSTD_FWD_SEPARATE_ADJ 4u
/* Launch schedule: the temporal graph convolutions with their adjacency
 * built in LDS (k_temporal_fused, one workgroup per sample) at any batch
 * size where the shape has the kernel.  Default: only when B >= the device's
 * compute units -- below that the unit-parallel pair (k_adj_hl + k_temporal_hl)
 * is faster.  Same results either way; for testing and A/B.  Also accepted by
 * dstd_block_fwd_ex. */
#define DSTD_FWD_FUSED_TEMPORAL 8u
/* Launch schedule: the spatial and the temporal graph convolution of a block
 * in two launches (k_spatial_hl, then k_temporal_fused) instead of one
 * (k_block_fused: one workgroup per sample runs the sample's spatial GC, then
 * its fused temporal GC; the default wherever the fused temporal kernel runs
 * and the block is one of the model's three kinds).  Same results bit for
 * bit; for testing and A/B.  Also accepted by dstd_block_fwd_ex. */
#define DSTD_FWD_SEPARATE_BLOCK 16u
/* One launch per encoder block.  By default a run of consecutive encoder
 * blocks that would each be one whole-block launch runs as a single launch
 * (one workgroup per sample loops over the blocks of the run; up to 8 blocks
 * per launch): conv_st_in, the encoder run, conv_st_out are 3 launches instead
 * of num_layers + 2.  Same results bit for bit; for testing and A/B.
 * DSTD_FWD_SEPARATE_BLOCK and DSTD_FWD_SEPARATE_ADJ imply it.  A call that
 * carries a profile (prof with capacity > 0) always runs one launch per
 * block: the event brackets and their block indices are per block.  Accepted
 * (and without effect) by dstd_block_fwd_ex. */
#define DSTD_FWD_SEPARATE_ENCODERS 32u
/* conv_st_in and conv_st_out in launches of their own around the encoder
 * run (3 launches per forward).  By default the whole forward -- conv_st_in,
 * 1 to 5 encoder blocks, conv_st_out -- is one launch where every block would
 * be a whole-block launch (one workgroup per sample runs the sample's blocks
 * in turn); num_layers 0 or above 5 keeps the 3-launch schedule.  Same
 * results bit for bit; for testing and A/B.  DSTD_FWD_SEPARATE_ENCODERS,
 * DSTD_FWD_SEPARATE_BLOCK and DSTD_FWD_SEPARATE_ADJ imply it, and so does a
 * call that carries a profile.  dstd_model_fwd_ex only. */
#define DSTD_FWD_SEPARATE_ENDS 64u
int dstd_model_fwd_ex(const dstd_model_params* p, const float* x, int B, float* y, void* workspace,
                      size_t workspace_bytes, void* stream, unsigned flags, dstd_profile* prof);

/* The launch schedule ("Launch schedule").  first_block and
 * num_blocks: the DSTDGCBs a launch covers (conv_st_in 0, the encoders
 * 1..num_layers, conv_st_out num_layers + 1); PREP: -1, 0. */
#define DSTD_LAUNCH_PREP 0           /* x6 = cat(x, x - x[:, -1]) and block 0's spatial P/Q */
#define DSTD_LAUNCH_ADJ_S 1          /* a block's spatial adjacencies */
#define DSTD_LAUNCH_SPATIAL 2        /* its spatial GC */
#define DSTD_LAUNCH_ADJ_T 3          /* its temporal adjacency */
#define DSTD_LAUNCH_TEMPORAL 4       /* its temporal GC on that adjacency */
#define DSTD_LAUNCH_TEMPORAL_FUSED 5 /* its temporal GC with the adjacency built in LDS */
#define DSTD_LAUNCH_BLOCK 6          /* the whole block */
#define DSTD_LAUNCH_ENC_RUN 7        /* num_blocks consecutive encoder blocks */
#define DSTD_LAUNCH_MODEL 8          /* the whole forward */
typedef struct { int kind, first_block, num_blocks; } dstd_launch;
/* the launches dstd_model_fwd_ex would enqueue after the parameter preparation;
 * profiled: the call carries a profile with capacity > 0; taps (dstd_model_fwd_taps,
 * dstd_gcn_taps.h): bit 0 tapped, bit 1 block 0's input is tapped;
 * cus <= 0: the current device's. Returns the count (may exceed capacity), or DSTD_E*. */
int dstd_model_fwd_schedule(int B, int T, int V, int num_feature, int num_layers, unsigned flags,
                            int profiled, int taps, int cus, dstd_launch* out, int capacity);
int dstd_events_create(int n, void** events);
int dstd_events_destroy(int n, void** events);
int dstd_event_elapsed_ms(void* start, void* stop, float* ms);


#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_H */
