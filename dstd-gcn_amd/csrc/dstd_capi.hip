// C ABI (include/dstd_gcn.h): argument checking, workspace carving and the
// launch sequence of one DSTDGC / DSTDGCB / DSTDGCN forward.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include <vector>

#include "../../include/dstd_gcn.h"
#include "../../include/dstd_gcn_taps.h"
#include "dstd_common.h"
#include "dstd_hilo.h"
#include "dstd_host.h"
#include "dstd_kernels.h"
#include "dstd_plan.h"
#include "dstd_taps.h"

using namespace dstd;

namespace {

bool shape_ok(int B, int T, int V) { return B > 0 && T > 1 && V > 0; }
bool limits_ok(int T, int V, int cin, int cout) {
  return T <= kMaxT && V <= kMaxV && cin >= 1 && cin <= kMaxC && cout >= 1 && cout <= kMaxC;
}
// the model's integer arguments (dstd_model_fwd_ex and dstd_model_fwd_schedule alike)
int model_shape_code(int B, int T, int V, int C, int layers) {
  if (!shape_ok(B, T, V) || layers < 0 || layers > DSTD_MAX_LAYERS) return DSTD_EINVAL;
  return limits_ok(T, V, 6, C) ? DSTD_OK : DSTD_ELIMIT;
}
constexpr unsigned kModelFwdFlags = DSTD_FWD_REUSE_CONSTANTS | DSTD_FWD_EXACT_FP32 | DSTD_FWD_SEPARATE_ADJ |
                                    DSTD_FWD_FUSED_TEMPORAL | DSTD_FWD_SEPARATE_BLOCK | DSTD_FWD_SEPARATE_ENCODERS |
                                    DSTD_FWD_SEPARATE_ENDS;
// Optional per-launch event brackets (dstd_model_fwd_profiled).
struct Prof {
  dstd_profile* p = nullptr;
  int block = -1;
  int open = -1;
  void begin(int kind, hipStream_t s) {
    open = -1;
    if (!p || !(p->kind_mask & (1u << kind)) || p->count >= p->capacity) return;
    if (p->only_block >= 0 && p->only_block != block) return;
    open = p->count++;
    p->kinds[open] = kind;
    if (p->block) p->block[open] = block;
    (void)hipEventRecord((hipEvent_t)p->events[2 * open], s);
  }
  void end(hipStream_t s) {
    if (open >= 0) (void)hipEventRecord((hipEvent_t)p->events[2 * open + 1], s);
    open = -1;
  }
};

// Folded per-block constants (filled by k_fold).
struct BlockFold {
  float* bn_s;
  float* bn_h;
  float* rbn_s;
  float* rbn_h;
  float* astat_s;  // [2][V][V]
  float* astat_t;  // [T][T]
  // split-f16 weight images (k_hl_prep, dstd_hilo.h) of the 64 -> 64 GC kernels
  uint4* hl_ws[3];  // conv_s[g].conv_f, [2]: residual conv (cin != cout)
  uint4* hl_pqs;    // conv_t.conv_m1/m2 (P/Q written by the spatial kernel)
  uint4* hl_wt;     // conv_t.conv_f
  uint4* hl_pqt;    // next block's conv_s[*].conv_m1/m2 (P/Q written by the temporal kernel)
  uint4* hl_rms[2]; // conv_s[g].conv_rm (spatial adjacency)
  uint4* hl_rmt;    // conv_t.conv_rm (temporal adjacency)
  float* hl_scale;  // 9 scale slots (kHLSlot floats each, dstd_hilo.h): ws0, ws1, pqs, wt, pqt, rms0, rms1, rmt, ws2
  float* hl_rbias;  // [2T + V]: fused conv_rm biases (HLJob::bias_out) of rms0, rms1, rmt
};

struct BlockScratch {
  float* adj_s;  // [B][2][T][V][V]
  float* adj_t;  // [B][V][T][T]
  float* pq_s;   // [B][8][T][V]
  float* pq_t;   // [B][4][T][V]
};

void carve_fold(Carver& cv, BlockFold& f, int T, int V, int cout, bool res) {
  f.bn_s = cv.take((size_t)cout * V);
  f.bn_h = cv.take((size_t)cout * V);
  f.rbn_s = res ? cv.take((size_t)cout * V) : nullptr;
  f.rbn_h = res ? cv.take((size_t)cout * V) : nullptr;
  f.astat_s = cv.take((size_t)2 * V * V);
  f.astat_t = cv.take((size_t)T * T);
  auto img = [&](int n) { return reinterpret_cast<uint4*>(cv.take((size_t)4 * n)); };
  f.hl_ws[0] = img(kHLConvImg);
  f.hl_ws[1] = img(kHLConvImg);
  f.hl_ws[2] = img(kHLConvImg);
  f.hl_pqs = img(kHLPQImg);
  f.hl_wt = img(kHLConvImg);
  f.hl_pqt = img(kHLPQImg);
  f.hl_rms[0] = img(hl_rm_img(T, 2 * T));
  f.hl_rms[1] = img(hl_rm_img(T, 2 * T));
  f.hl_rmt = img(hl_rm_img(V, 2 * V));
  f.hl_scale = cv.take(9 * kHLSlot);
  f.hl_rbias = cv.take((size_t)2 * T + V);
}

// adjacency scratch: the larger of the fp32 rows and the split-f16 planes
size_t adj_s_floats(int B, int T, int V) {
  const size_t row = std::max((size_t)adj_ld_spatial(V), (size_t)V * hl_sl_spatial(V));
  return (size_t)B * 2 * T * row;
}
size_t adj_t_floats(int B, int T, int V) {
  const size_t row = std::max((size_t)adj_ld_temporal(T), (size_t)T * hl_sl_temporal(T));
  return (size_t)B * V * row;
}

void carve_scratch(Carver& cv, BlockScratch& s, int B, int T, int V) {
  s.adj_s = cv.take(adj_s_floats(B, T, V));
  s.adj_t = cv.take(adj_t_floats(B, T, V));
  s.pq_s = cv.take((size_t)B * 8 * T * V);
  s.pq_t = cv.take((size_t)B * 4 * T * V);
}

using FoldList = std::vector<FoldJob>;

void add_bn_job(FoldList& fa, const dstd_bn& bn, int C, int V, float* s, float* h) {
  fa.emplace_back();
  FoldJob& j = fa.back();
  j.kind = FOLD_BN;
  j.n = C * V;
  j.C = C;
  j.V = V;
  j.p0 = bn.weight;
  j.p1 = bn.bias;
  j.p2 = bn.running_mean;
  j.p3 = bn.running_var;
  j.eps = bn.eps;
  j.o0 = s;
  j.o1 = h;
}

void add_block_jobs(FoldList& fa, const dstd_block_params* p, const BlockFold& f, int T, int V) {
  add_bn_job(fa, p->bn, p->cout, V, f.bn_s, f.bn_h);
  if (p->cin != p->cout) add_bn_job(fa, p->res_bn, p->cout, V, f.rbn_s, f.rbn_h);
  fa.emplace_back();
  FoldJob& a = fa.back();
  a.kind = FOLD_AWR;  // A_s*W_s + R_s for both graphs (model/dstdgcn.py:146-149)
  a.n = 2 * V * V;
  a.p0 = p->A_s;
  a.p1 = p->W_s;
  a.p2 = p->R_s;
  a.o0 = f.astat_s;
  fa.emplace_back();
  FoldJob& t = fa.back();
  t.kind = FOLD_AR;  // A_t + R_t (:158-160)
  t.n = T * T;
  t.p0 = p->A_t;
  t.p1 = p->R_t;
  t.o0 = f.astat_t;
}

hipError_t run_fold(const FoldList& jobs, hipStream_t s) {
  for (size_t i = 0; i < jobs.size(); i += kMaxFoldJobs) {
    FoldArgs fa{};
    for (size_t j = i; j < jobs.size() && j < i + kMaxFoldJobs; ++j) fa.jobs[fa.njobs++] = jobs[j];
    hipError_t e = launch_fold(fa, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

using HLList = std::vector<HLJob>;

hipError_t run_hl_prep(const HLList& jobs, hipStream_t s) {
  for (size_t i = 0; i < jobs.size(); i += kMaxHLJobs) {
    HLPrepArgs ha{};
    for (size_t j = i; j < jobs.size() && j < i + kMaxHLJobs; ++j) ha.jobs[ha.njobs++] = jobs[j];
    hipError_t e = launch_hl_prep(ha, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

void add_hl_conv(HLList& l, const float* w, const float* b, int rows, int cols, uint4* img, float* sc) {
  HLJob j{};
  j.kind = HLJ_CONV;
  j.w[0] = w;
  j.bias = b;
  j.nblk = 1;
  j.rows = rows;
  j.cols = cols;
  j.img = img;
  j.inv_scale = sc;
  l.push_back(j);
}
void add_hl_rm(HLList& l, const float* w, const float* b, int rows, int cols, uint4* img, float* sc, float* bout,
               const float* alpha, const float* astat, int nastat) {
  HLJob j{};
  j.kind = HLJ_RM;
  j.w[0] = w;
  j.alpha = alpha;
  j.astat = astat;
  j.nastat = nastat;
  j.bias = b;
  j.bias_out = bout;
  j.nblk = 1;
  j.rows = rows;
  j.cols = cols;
  j.img = img;
  j.inv_scale = sc;
  l.push_back(j);
}
void add_hl_pq(HLList& l, const float* const* w, int nblk, int cols, uint4* img, float* sc) {
  HLJob j{};
  j.kind = HLJ_PQ;
  for (int i = 0; i < nblk; ++i) j.w[i] = w[i];
  j.nblk = nblk;
  j.cols = cols;
  j.img = img;
  j.inv_scale = sc;
  l.push_back(j);
}

// What the temporal kernel does after the block (see TemporalEpi).
struct BlockTail {
  int epi;
  const float* xres;
  const float* bn_s;
  const float* bn_h;
  const float* prelu;
  const dstd_block_params* next;  // next block: its spatial P/Q are produced here
  // its folded constants: its spatial adjacency planes are built here too
  // where the plan says so (BlockPlan::next_adj, k_temporal_fused phase 3)
  const BlockFold* next_f = nullptr;
};

// One DSTDGCB of a forward: parameters, folded constants, NTVC buffers
// (x -> spatial GC -> h -> temporal GC + tail -> y).
struct BlockRun {
  const dstd_block_params* p;
  const BlockFold* f;
  const float* x;
  float* h;
  float* y;
  BlockTail tail;
};

// conv_m1 / conv_m2 of a block's two spatial DSTDGCs: the four two-row weight
// blocks and biases behind its spatial P/Q (channels P_0, Q_0, P_1, Q_1 pairs)
struct SpatialPQ {
  const float* w[4];
  const float* b[4];
};
SpatialPQ spatial_pq_params(const dstd_block_params* p) {
  const dstd_gc_weights &g0 = p->conv_s[0], &g1 = p->conv_s[1];
  return SpatialPQ{{g0.wm1, g0.wm2, g1.wm1, g1.wm2}, {g0.bm1, g0.bm2, g1.bm1, g1.bm2}};
}

// The generic (fp32 rows) adjacency geometry of a mode, one graph per sample:
// nrow, K, NA, ncol, ldo, out_sN.
void adj_geometry(AdjArgs& a, int mode, int T, int V) {
  const bool sp = mode == DSTD_MODE_SPATIAL;
  a.mode = mode;
  a.T = T;
  a.V = V;
  a.nrow = sp ? T : V;
  a.K = 2 * a.nrow;
  a.NA = sp ? V : T;
  a.ncol = a.NA * a.NA;
  a.ldo = sp ? adj_ld_spatial(V) : adj_ld_temporal(T);
  a.out_sN = (long)a.nrow * a.ldo;
}

// scale slot i of a block's weight images (BlockFold::hl_scale)
float* hls(const BlockFold& f, int i) { return f.hl_scale + kHLSlot * i; }

// Weight images of the block's split-f16 launches.
void add_block_hl_jobs(HLList& l, const dstd_block_params* p, const BlockFold& f, const BlockTail& tail,
                       const BlockPlan& hl, int T, int V) {
  if (hl.s) {
    add_hl_rm(l, p->conv_s[0].wrm, p->conv_s[0].brm, T, 2 * T, f.hl_rms[0], hls(f, 5), f.hl_rbias, p->alpha_sm,
              f.astat_s, V * V);
    add_hl_rm(l, p->conv_s[1].wrm, p->conv_s[1].brm, T, 2 * T, f.hl_rms[1], hls(f, 6), f.hl_rbias + T, p->alpha_sm,
              f.astat_s + V * V, V * V);
    add_hl_conv(l, p->conv_s[0].wf, p->conv_s[0].bf, p->cout, p->cin, f.hl_ws[0], hls(f, 0));
    add_hl_conv(l, p->conv_s[1].wf, p->conv_s[1].bf, p->cout, p->cin, f.hl_ws[1], hls(f, 1));
    if (p->cin != p->cout) add_hl_conv(l, p->res_w, p->res_b, p->cout, p->cin, f.hl_ws[2], hls(f, 8));
    const float* w[2] = {p->conv_t.wm1, p->conv_t.wm2};
    add_hl_pq(l, w, 2, p->cout, f.hl_pqs, hls(f, 2));
  }
  if (hl.t) {
    add_hl_rm(l, p->conv_t.wrm, p->conv_t.brm, V, 2 * V, f.hl_rmt, hls(f, 7), f.hl_rbias + 2 * T, p->alpha_tm,
              f.astat_t, T * T);
    add_hl_conv(l, p->conv_t.wf, p->conv_t.bf, p->cout, p->cout, f.hl_wt, hls(f, 3));
    if (tail.next) add_hl_pq(l, spatial_pq_params(tail.next).w, 4, 64, f.hl_pqt, hls(f, 4));
  }
}

// The arguments of every launch a DSTDGCB can take part in, on NTVC
// activations, built once per block whatever the plan does with it (its own
// launches, a run of k_enc_chain, k_model_chain): aa / ta the adjacency
// launches and sa / tt the GC launches of the generic fp32 kernels; where hl
// says so the split-f16 forms instead: ah / aht, the GC kernels ha / ht and
// the next block's spatial adjacency sn (hl.next_adj).
// xmodel (conv_st_in of the model, split spatial only): the model input
// [B][T][V][3]; the kernels build x6 and block-0's spatial P/Q from it, x is
// not read.
struct BlockArgs {
  bool from_model;
  AdjArgs aa, ta;
  SpatialArgs sa;
  TemporalArgs tt;
  AdjHLArgs ah, aht, sn;
  SpatialHLArgs ha;
  TemporalHLArgs ht;
};
void build_block_args(BlockArgs& A, const BlockRun& r, const BlockScratch& sc, int B, int T, int V, const BlockPlan& hl,
                      const float* xmodel) {
  A = BlockArgs{};
  const dstd_block_params* p = r.p;
  const BlockFold& f = *r.f;
  const BlockTail& tail = r.tail;
  const float* x = r.x;
  float *h = r.h, *y = r.y;
  const bool res = p->cin != p->cout;
  const bool from_model = A.from_model = xmodel && hl.s && p->cin == 6;
  AdjArgs &aa = A.aa, &ta = A.ta;
  SpatialArgs& sa = A.sa;
  TemporalArgs& tt = A.tt;
  AdjHLArgs &ah = A.ah, &aht = A.aht, &sn = A.sn;
  SpatialHLArgs& ha = A.ha;
  TemporalHLArgs& ht = A.ht;
  // (1) spatial adjacency for both graphs
  aa.pq = sc.pq_s;
  aa.pql = pq_layout_vt(8, T, V);
  for (int g = 0; g < 2; ++g) {
    aa.p_ch[g] = 4 * g;
    aa.q_ch[g] = 4 * g + 2;
    aa.W[g] = p->conv_s[g].wrm;
    aa.bias[g] = p->conv_s[g].brm;
    aa.astat[g] = f.astat_s + g * V * V;
  }
  adj_geometry(aa, DSTD_MODE_SPATIAL, T, V);
  aa.B = B;
  aa.ngroups = 2;
  aa.alpha = p->alpha_sm;
  aa.out = sc.adj_s;
  if (hl.s) {  // split-f16 planes [B][2][T][2][V][SL]
    aa.hl = 1;
    aa.ncol = V * hl_sl_spatial(V);
    aa.ldo = 2 * aa.ncol;
    aa.out_sN = (long)T * aa.ncol;
  }
  aa.out_sG = aa.out_sN;  // [B][2 graphs]
  aa.out_sN = 2 * aa.out_sG;
  if (hl.s) {
    ah.pq = aa.pq;
    ah.pql = aa.pql;
    ah.B = B;
    ah.ngroups = 2;
    for (int g = 0; g < 2; ++g) {
      ah.p_ch[g] = aa.p_ch[g];
      ah.wimg[g] = f.hl_rms[g];
      ah.wscale[g] = hls(f, 5 + g);
      ah.bias[g] = f.hl_rbias + g * T;
      ah.astat[g] = aa.astat[g];
    }
    ah.alpha = aa.alpha;
    ah.out = reinterpret_cast<uint16_t*>(aa.out);
    ah.out_sN = 2 * aa.out_sN;  // halves
    ah.out_sG = 2 * aa.out_sG;
    if (from_model) {
      ah.xin = xmodel;
      const SpatialPQ m = spatial_pq_params(p);
      for (int i = 0; i < 4; ++i) {
        ah.mw[i / 2][i % 2] = m.w[i];
        ah.mb[i / 2][i % 2] = m.b[i];
      }
    }
  }

  // (2) spatial GC + bn + residual + prelu, P_t/Q_t of h
  if (hl.s) {
    ha.x = from_model ? xmodel : x;
    ha.xmodel = from_model ? 1 : 0;
    ha.B = B;
    ha.T = T;
    ha.V = V;
    ha.Cin = p->cin;
    ha.Cout = p->cout;
    ha.adj = reinterpret_cast<const uint16_t*>(sc.adj_s);
    for (int g = 0; g < 2; ++g) {
      ha.wimg[g] = f.hl_ws[g];
      ha.wscale[g] = hls(f, g);
      ha.adjb[g] = hls(f, 5 + g);
      ha.bf[g] = p->conv_s[g].bf;
    }
    if (res) {
      ha.wimg[2] = f.hl_ws[2];
      ha.wscale[2] = hls(f, 8);
      ha.bf[2] = p->res_b;
      ha.rbn_s = f.rbn_s;
      ha.rbn_h = f.rbn_h;
    }
    ha.bn_s = f.bn_s;
    ha.bn_h = f.bn_h;
    ha.prelu = p->prelu;
    ha.y = h;
    ha.pqimg = f.hl_pqs;
    ha.pqscale = hls(f, 2);
    ha.pqb[0] = p->conv_t.bm1;
    ha.pqb[1] = p->conv_t.bm2;
    ha.pq = sc.pq_t;
  } else {
    sa.x = x;
    sa.B = B;
    sa.T = T;
    sa.V = V;
    sa.Cin = p->cin;
    sa.Cout = p->cout;
    sa.NI = 2;
    sa.G = res ? 3 : 2;
    sa.adj = sc.adj_s;
    sa.adj_ld = adj_ld_spatial(V);
    for (int g = 0; g < 2; ++g) {
      sa.wf[g] = p->conv_s[g].wf;
      sa.bf[g] = p->conv_s[g].bf;
    }
    sa.wf[2] = res ? p->res_w : nullptr;
    sa.bf[2] = res ? p->res_b : nullptr;
    sa.epi = 1;
    sa.bn_s = f.bn_s;
    sa.bn_h = f.bn_h;
    sa.rbn_s = f.rbn_s;
    sa.rbn_h = f.rbn_h;
    sa.prelu = p->prelu;
    sa.y = h;
    sa.pqw[0] = p->conv_t.wm1;
    sa.pqw[1] = p->conv_t.wm2;
    sa.pqb[0] = p->conv_t.bm1;
    sa.pqb[1] = p->conv_t.bm2;
    sa.npqw = 2;
    sa.pq = sc.pq_t;
    sa.pql = pq_layout_tv(4, T, V);
    sa.Tt = 0;
  }

  // (3) temporal adjacency
  ta.pq = sc.pq_t;
  ta.pql = pq_layout_tv(4, T, V);
  ta.p_ch[0] = 0;
  ta.q_ch[0] = 2;
  ta.W[0] = p->conv_t.wrm;
  ta.bias[0] = p->conv_t.brm;
  ta.astat[0] = f.astat_t;
  adj_geometry(ta, DSTD_MODE_TEMPORAL, T, V);
  ta.B = B;
  ta.ngroups = 1;
  ta.alpha = p->alpha_tm;
  ta.out = sc.adj_t;
  ta.out_sG = 0;
  if (hl.t) {  // split-f16 planes [B][V][2][T][SL]
    ta.hl = 1;
    ta.ncol = T * hl_sl_temporal(T);
    ta.ldo = 2 * ta.ncol;
    ta.out_sN = (long)V * ta.ncol;
  }
  if (hl.t) {
    aht.pq = ta.pq;
    aht.pql = ta.pql;
    aht.B = B;
    aht.ngroups = 1;
    aht.p_ch[0] = ta.p_ch[0];
    aht.wimg[0] = f.hl_rmt;
    aht.wscale[0] = hls(f, 7);
    aht.bias[0] = f.hl_rbias + 2 * T;
    aht.astat[0] = ta.astat[0];
    aht.alpha = ta.alpha;
    aht.out = reinterpret_cast<uint16_t*>(ta.out);
    aht.out_sN = 2 * ta.out_sN;
    aht.out_sG = 0;
  }

  // (4) temporal GC + tail epilogue (+ next block's spatial P/Q)
  if (hl.t) {
    ht.h = h;
    ht.B = B;
    ht.T = T;
    ht.V = V;
    ht.C = p->cout;
    ht.adj = reinterpret_cast<const uint16_t*>(sc.adj_t);
    ht.wimg = f.hl_wt;
    ht.wscale = hls(f, 3);
    ht.adjb = hls(f, 7);
    ht.bf = p->conv_t.bf;
    ht.epi = tail.epi;
    ht.xres = tail.xres;
    ht.bn_s = tail.bn_s;
    ht.bn_h = tail.bn_h;
    ht.prelu = tail.prelu;
    ht.y = y;
    if (tail.next) {
      const SpatialPQ m = spatial_pq_params(tail.next);
      ht.pqimg = f.hl_pqt;
      ht.pqscale = hls(f, 4);
      for (int i = 0; i < 4; ++i) ht.pqb[i] = m.b[i];
      ht.pq = sc.pq_s;
    }
    // the next block's spatial adjacency (its launch_adj_hl mode 0 arguments)
    if (hl.next_adj) {
      const dstd_block_params* q = tail.next;
      const BlockFold& nf = *tail.next_f;
      const int ncol = V * hl_sl_spatial(V);
      sn.pq = sc.pq_s;
      sn.pql = pq_layout_vt(8, T, V);
      sn.B = B;
      sn.ngroups = 2;
      for (int g = 0; g < 2; ++g) {
        sn.p_ch[g] = 4 * g;
        sn.wimg[g] = nf.hl_rms[g];
        sn.wscale[g] = hls(nf, 5 + g);
        sn.bias[g] = nf.hl_rbias + g * T;
        sn.astat[g] = nf.astat_s + g * V * V;
      }
      sn.alpha = q->alpha_sm;
      sn.out = reinterpret_cast<uint16_t*>(sc.adj_s);
      sn.out_sG = 2L * T * ncol;  // halves
      sn.out_sN = 2 * sn.out_sG;
    }
  } else {
    tt.h = h;
    tt.B = B;
    tt.T = T;
    tt.V = V;
    tt.Cin = p->cout;
    tt.Cout = p->cout;
    tt.adj = sc.adj_t;
    tt.adj_ld = adj_ld_temporal(T);
    tt.wf = p->conv_t.wf;
    tt.bf = p->conv_t.bf;
    tt.epi = tail.epi;
    tt.xres = tail.xres;
    tt.bn_s = tail.bn_s;
    tt.bn_h = tail.bn_h;
    tt.prelu = tail.prelu;
    tt.y = y;
    if (tail.next) {
      const SpatialPQ m = spatial_pq_params(tail.next);
      for (int i = 0; i < 4; ++i) {
        tt.pqw[i] = m.w[i];
        tt.pqb[i] = m.b[i];
      }
      tt.npqw = 4;
      tt.pq = sc.pq_s;
      tt.pql = pq_layout_vt(8, T, V);
    }
    tt.Vt = 0;
  }
}

hipError_t to_layout(const float* src, float* dst, int B, int C, int TV, int to_ntvc, hipStream_t s);

// A tapped adjacency (include/dstd_gcn_taps.h) out of the block's scratch,
// which holds it from the adjacency launch until the next one: split-f16
// planes decoded ((hi + lo) * 2^sa), fp32 rows compacted.  rows: (sample,
// graph, frame) spatial, (sample, joint) temporal; NA = V / T.
hipError_t tap_adjacency(const float* scratch, float* out, bool split, long rows, int NA, int SL, int ld, int seq,
                         const float* scale0, const float* scale1, hipStream_t s) {
  if (split) {
    TapDecodeHLArgs d{reinterpret_cast<const uint16_t*>(scratch), out, rows, NA, SL, seq, {scale0, scale1}};
    return launch_tap_decode_hl(d, s);
  }
  TapCompactArgs c{scratch, out, rows, NA * NA, ld};
  return launch_tap_compact(c, s);
}

// One of a DSTDGCB's own launches (plan_block_launches) with its profile
// bracket and the tap copies that follow it.  pq_s must already hold P/Q of
// the block's input for its two spatial DSTDGCs; the block's weight images
// (add_block_hl_jobs) must be prepared when hl says so.
// tap (the tap entry points only; needs the unit-parallel schedule, plan_block
// unit): what to copy out between the launches; r.x must hold the block's
// input even where the kernels do not read it (xmodel).
hipError_t run_block_launch(int kind, const BlockRun& r, const BlockArgs& A, const BlockPlan& hl, const BlockScratch& sc,
                            int B, int T, int V, hipStream_t s, Prof& pf, const dstd_block_taps* tap) {
  const BlockFold& f = *r.f;
  const AdjHLArgs* sn = hl.next_adj ? &A.sn : nullptr;
  if (tap && (hl.s_pre || hl.adj0 || hl.bf || hl.tf)) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  switch (kind) {
    case DSTD_LAUNCH_ADJ_S:  // spatial adjacency for both graphs (a tapped block's first launch)
      if (tap && tap->x) e = to_layout(r.x, tap->x, B, r.p->cin, T * V, 0, s);
      if (e != hipSuccess) return e;
      pf.begin(DSTD_KIND_ADJ_S, s);
      e = hl.s ? launch_adj_hl(A.ah, 0, T, V, s) : launch_adj(A.aa, s);
      pf.end(s);
      if (e == hipSuccess && tap && tap->adj_s)
        e = tap_adjacency(sc.adj_s, tap->adj_s, hl.s, (long)B * 2 * T, V, hl_sl_spatial(V), adj_ld_spatial(V), 0,
                          hls(f, 5), hls(f, 6), s);
      return e;
    case DSTD_LAUNCH_SPATIAL:  // spatial GC + bn + residual + prelu, P_t/Q_t of h
      pf.begin(DSTD_KIND_SPATIAL, s);
      e = hl.s ? launch_spatial_hl(A.ha, s) : launch_spatial(A.sa, s);
      pf.end(s);
      if (e == hipSuccess && tap && tap->h) e = to_layout(r.h, tap->h, B, r.p->cout, T * V, 0, s);
      return e;
    case DSTD_LAUNCH_ADJ_T:  // temporal adjacency
      pf.begin(DSTD_KIND_ADJ_T, s);
      e = hl.t ? launch_adj_hl(A.aht, 1, T, V, s) : launch_adj(A.ta, s);
      pf.end(s);
      if (e == hipSuccess && tap && tap->adj_t)
        e = tap_adjacency(sc.adj_t, tap->adj_t, hl.t, (long)B * V, T, hl_sl_temporal(T), adj_ld_temporal(T), 1,
                          hls(f, 7), nullptr, s);
      return e;
    case DSTD_LAUNCH_TEMPORAL:  // temporal GC + tail epilogue (+ next block's spatial P/Q)
      pf.begin(DSTD_KIND_TEMPORAL, s);
      e = hl.t ? launch_temporal_hl(A.ht, s) : launch_temporal(A.tt, s);
      pf.end(s);
      return e;
    case DSTD_LAUNCH_TEMPORAL_FUSED:  // the same with its adjacency built in LDS (+ the next block's planes)
      pf.begin(DSTD_KIND_TEMPORAL, s);
      e = launch_temporal_fused(A.ht, A.aht, sn, s);
      pf.end(s);
      return e;
    case DSTD_LAUNCH_BLOCK:  // spatial + fused temporal GC (+ block 0's own planes)
      pf.begin(DSTD_KIND_BLOCK, s);
      e = launch_block_fused(A.ha, A.ht, A.aht, sn, s, hl.adj0 && A.from_model ? &A.ah : nullptr);
      pf.end(s);
      return e;
    default: return hipErrorInvalidValue;
  }
}

// a block's k_block_fused arguments, validated (block_fused_args), as the
// BLOCK launch and the two chain launches take them
hipError_t fused_args(const BlockArgs& A, const BlockPlan& hl, BlockFusedArgs* out) {
  return block_fused_args(A.ha, A.ht, A.aht, hl.next_adj ? &A.sn : nullptr, out,
                          hl.adj0 && A.from_model ? &A.ah : nullptr);
}

// P/Q of a block's input for its two spatial DSTDGCs.  x6 (the model's PREP
// launch): x is the model input [B][T][V][3] and x6 = cat(x, x - x[:, -1]) is
// written too (:298-305).
hipError_t spatial_pq(const dstd_block_params* p, const float* x_ntvc, int B, int T, int V, float* pq_s, hipStream_t s,
                      float* x6 = nullptr) {
  const SpatialPQ m = spatial_pq_params(p);
  PQArgs pa{};
  pa.x = x_ntvc;
  pa.B = B;
  pa.T = T;
  pa.V = V;
  pa.Cin = p->cin;
  pa.make_x6 = x6 ? 1 : 0;
  pa.x6 = x6;
  for (int i = 0; i < 4; ++i) {
    pa.w[i] = m.w[i];
    pa.b[i] = m.b[i];
  }
  pa.nw = 4;
  pa.pq = pq_s;
  pa.pql = pq_layout_vt(8, T, V);
  return launch_pq(pa, s);
}

// ---- layouts ---------------------------------------------------------------
struct OpLayout {
  float* xin;
  float* yout;
  float* pq;
  float* adj;
};
void carve_op(Carver& cv, OpLayout& L, int mode, int B, int cin, int cout, int T, int V) {
  L.xin = cv.take((size_t)B * T * V * cin);
  L.yout = cv.take((size_t)B * T * V * cout);
  L.pq = cv.take((size_t)B * 4 * T * V);
  L.adj = cv.take(mode == DSTD_MODE_SPATIAL ? (size_t)B * T * adj_ld_spatial(V) : (size_t)B * V * adj_ld_temporal(T));
}

struct BlockLayout {
  float* xin;
  float* h;
  float* yout;
  BlockFold f;
  BlockScratch sc;
};
void carve_block(Carver& cv, BlockLayout& L, int B, int cin, int cout, int T, int V) {
  L.xin = cv.take((size_t)B * T * V * cin);
  L.h = cv.take((size_t)B * T * V * cout);
  L.yout = cv.take((size_t)B * T * V * cout);
  carve_fold(cv, L.f, T, V, cout, cin != cout);
  carve_scratch(cv, L.sc, B, T, V);
}

struct ModelLayout {
  float* act[3];
  BlockFold f_in, f_out, f_enc[DSTD_MAX_LAYERS];
  float* bnin_s;
  float* bnin_h;
  float* ebn_s[DSTD_MAX_LAYERS];
  float* ebn_h[DSTD_MAX_LAYERS];
  BlockScratch sc;
};
void carve_model(Carver& cv, ModelLayout& L, int B, int T, int V, int C, int layers, int cin_model,
                 int cout_model) {
  for (int i = 0; i < 3; ++i) L.act[i] = cv.take((size_t)B * T * V * C);
  carve_fold(cv, L.f_in, T, V, C, cin_model != C);
  carve_fold(cv, L.f_out, T, V, cout_model, C != cout_model);
  for (int i = 0; i < layers; ++i) {
    carve_fold(cv, L.f_enc[i], T, V, C, false);
    L.ebn_s[i] = cv.take((size_t)C * V);
    L.ebn_h[i] = cv.take((size_t)C * V);
  }
  L.bnin_s = cv.take((size_t)C * V);
  L.bnin_h = cv.take((size_t)C * V);
  carve_scratch(cv, L.sc, B, T, V);
}

// The forward's blocks run[0 .. num_layers + 2): conv_st_in -> bn_in -> prelu
// (dropout is identity in eval); encoders x = prelu_e(bn_e(DSTDGCB(x) + x));
// conv_st_out + output residual written straight into y [B][T][V][3].
// Buffers rotate over act[0..2].
void model_block_runs(BlockRun* run, const dstd_model_params* p, const ModelLayout& L, const float* x, float* y,
                      bool one_launch) {
  const int L_ = p->num_layers, NB = L_ + 2;
  float *cur = L.act[0], *h = L.act[1], *out = L.act[2];
  run[0] = BlockRun{&p->st_in, &L.f_in, cur, h, out, BlockTail{TEPI_IN, nullptr, L.bnin_s, L.bnin_h, p->prelu, nullptr}};
  for (int i = 0; i < L_; ++i) {
    float* t = cur;  // x: the previous block's y, h: its x, y: its h
    cur = out;
    out = h;
    h = t;
    run[1 + i] = BlockRun{&p->enc[i], &L.f_enc[i], cur, h, out,
                          BlockTail{TEPI_ENC, cur, L.ebn_s[i], L.ebn_h[i], p->enc_prelu[i], nullptr}};
  }
  // conv_st_out's h is [B][T][V][3]: in an act buffer, sample n's rows lie
  // inside the 64-channel slice of sample 3n / 64, which that sample's
  // workgroup may still be reading or writing as an encoder block's
  // activation -- between launches every encoder block was over before
  // conv_st_out began.  In the one-launch schedule it goes to the temporal
  // adjacency scratch, which no launch of that schedule touches (every
  // temporal adjacency is built in LDS) and which holds B V T T floats or more.
  run[NB - 1] = BlockRun{&p->st_out, &L.f_out, out, one_launch ? L.sc.adj_t : h, y,
                         BlockTail{TEPI_OUT, x, nullptr, nullptr, nullptr, nullptr}};
  for (int b = 0; b + 1 < NB; ++b) {
    run[b].tail.next = run[b + 1].p;
    run[b].tail.next_f = run[b + 1].f;
  }
}

hipError_t to_layout(const float* src, float* dst, int B, int C, int TV, int to_ntvc, hipStream_t s) {
  TransposeArgs t{src, dst, B, C, TV, to_ntvc};
  return launch_transpose(t, s);
}

// the block and the model forward behind the plain and the tap entry points
int block_fwd(const dstd_block_params* p, const float* x, int B, int T, int V, float* y, void* workspace,
              size_t workspace_bytes, void* stream, unsigned flags, const dstd_block_taps* taps);
int model_fwd(const dstd_model_params* p, const float* x, int B, float* y, void* workspace, size_t workspace_bytes,
              void* stream, unsigned flags, dstd_profile* prof, const dstd_block_taps* taps);

}  // namespace

extern "C" {

const char* dstd_version(void) { return "dstd-gcn-mi355x 0.2 (gfx950; forward: split-f16 MFMA 16x16x32, fp32 storage / accumulate; training: fp32 MFMA 16x16x4)"; }

const char* dstd_error_string(int code) {
  switch (code) {
    case DSTD_OK: return "ok";
    case DSTD_EINVAL: return "invalid argument (null pointer or bad shape)";
    case DSTD_EWORKSPACE: return "workspace too small";
    case DSTD_ELIMIT: return "shape outside the supported envelope (T<=128, V<=32, C<=64)";
    case DSTD_ECOLLECTIVE: return "the dstd_bn_sync collective returned an error (SyncBN)";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
  }
}

size_t dstd_dstdgc_workspace_bytes(int mode, int B, int cin, int cout, int T, int V) {
  Carver cv{nullptr};
  OpLayout L;
  carve_op(cv, L, mode, B, cin, cout, T, V);
  return cv.off + 256;
}

size_t dstd_block_workspace_bytes(int B, int cin, int cout, int T, int V) {
  Carver cv{nullptr};
  BlockLayout L;
  carve_block(cv, L, B, cin, cout, T, V);
  return cv.off + 256;
}

size_t dstd_model_workspace_bytes(int B, int T, int V, int num_feature, int num_layers) {
  Carver cv{nullptr};
  ModelLayout L;
  carve_model(cv, L, B, T, V, num_feature, num_layers, 6, 3);
  return cv.off + 256;
}

int dstd_dstdgc_fwd(int mode, const float* x, int B, int cin, int cout, int T, int V, const dstd_gc_weights* w,
                    const float* A, const float* alpha, float* y, void* workspace, size_t workspace_bytes,
                    void* stream) {
  StreamDeviceGuard dev_guard_(stream, x);
  if (!x || !y || !A || !alpha || !gc_ok(w) || !workspace || !shape_ok(B, T, V)) return DSTD_EINVAL;
  if (mode != DSTD_MODE_SPATIAL && mode != DSTD_MODE_TEMPORAL) return DSTD_EINVAL;
  if (!limits_ok(T, V, cin, cout)) return DSTD_ELIMIT;
  if (workspace_bytes < dstd_dstdgc_workspace_bytes(mode, B, cin, cout, T, V)) return DSTD_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  Carver cv{(char*)workspace};
  OpLayout L;
  carve_op(cv, L, mode, B, cin, cout, T, V);
  const int TV = T * V;
  DSTD_TRY(to_layout(x, L.xin, B, cin, TV, 1, s));
  PQArgs pa{};
  pa.x = L.xin;
  pa.B = B;
  pa.T = T;
  pa.V = V;
  pa.Cin = cin;
  pa.w[0] = w->wm1;
  pa.w[1] = w->wm2;
  pa.b[0] = w->bm1;
  pa.b[1] = w->bm2;
  pa.nw = 2;
  pa.pq = L.pq;
  pa.pql = pq_layout_tv(4, T, V);
  DSTD_TRY(launch_pq(pa, s));
  AdjArgs aa{};
  aa.pq = L.pq;
  aa.pql = pa.pql;
  aa.p_ch[0] = 0;
  aa.q_ch[0] = 2;
  aa.W[0] = w->wrm;
  aa.bias[0] = w->brm;
  aa.astat[0] = A;  // the caller's combined adjacency is row independent
  adj_geometry(aa, mode, T, V);
  aa.B = B;
  aa.ngroups = 1;
  aa.alpha = alpha;
  aa.out = L.adj;
  aa.out_sG = 0;
  DSTD_TRY(launch_adj(aa, s));
  if (mode == DSTD_MODE_SPATIAL) {
    SpatialArgs sa{};
    sa.x = L.xin;
    sa.B = B;
    sa.T = T;
    sa.V = V;
    sa.Cin = cin;
    sa.Cout = cout;
    sa.NI = 1;
    sa.G = 1;
    sa.adj = L.adj;
    sa.adj_ld = adj_ld_spatial(V);
    sa.wf[0] = w->wf;
    sa.bf[0] = w->bf;
    sa.epi = 0;
    sa.y = L.yout;
    DSTD_TRY(launch_spatial(sa, s));
  } else {
    TemporalArgs ta{};
    ta.h = L.xin;
    ta.B = B;
    ta.T = T;
    ta.V = V;
    ta.Cin = cin;
    ta.Cout = cout;
    ta.adj = L.adj;
    ta.adj_ld = adj_ld_temporal(T);
    ta.wf = w->wf;
    ta.bf = w->bf;
    ta.epi = TEPI_RAW;
    ta.y = L.yout;
    DSTD_TRY(launch_temporal(ta, s));
  }
  DSTD_TRY(to_layout(L.yout, y, B, cout, TV, 0, s));
  return DSTD_OK;
}

int dstd_block_fwd(const dstd_block_params* p, const float* x, int B, int T, int V, float* y, void* workspace,
                   size_t workspace_bytes, void* stream) {
  return dstd_block_fwd_ex(p, x, B, T, V, y, workspace, workspace_bytes, stream, 0u);
}

int dstd_block_fwd_ex(const dstd_block_params* p, const float* x, int B, int T, int V, float* y, void* workspace,
                      size_t workspace_bytes, void* stream, unsigned flags) {
  if (flags & ~(DSTD_FWD_EXACT_FP32 | DSTD_FWD_FUSED_TEMPORAL | DSTD_FWD_SEPARATE_BLOCK | DSTD_FWD_SEPARATE_ENCODERS))
    return DSTD_EINVAL;
  return block_fwd(p, x, B, T, V, y, workspace, workspace_bytes, stream, flags, nullptr);
}

size_t dstd_block_taps_workspace_bytes(int B, int cin, int cout, int T, int V) {
  return dstd_block_workspace_bytes(B, cin, cout, T, V);
}

int dstd_block_fwd_taps(const dstd_block_params* p, const float* x, int B, int T, int V, float* y,
                        const dstd_block_taps* taps, void* workspace, size_t workspace_bytes, void* stream,
                        unsigned flags) {
  if ((flags & ~DSTD_FWD_EXACT_FP32) || !taps) return DSTD_EINVAL;
  return block_fwd(p, x, B, T, V, y, workspace, workspace_bytes, stream, flags, taps);
}

}  // extern "C"

namespace {

// dstd_block_fwd_ex; taps (dstd_block_fwd_taps): the unit-parallel schedule
// with the block's taps copied out between its launches
int block_fwd(const dstd_block_params* p, const float* x, int B, int T, int V, float* y, void* workspace,
              size_t workspace_bytes, void* stream, unsigned flags, const dstd_block_taps* taps) {
  StreamDeviceGuard dev_guard_(stream, x);
  if (!x || !y || !workspace || !block_ptrs_ok(p) || !shape_ok(B, T, V)) return DSTD_EINVAL;
  if (!limits_ok(T, V, p->cin, p->cout)) return DSTD_ELIMIT;
  if (workspace_bytes < dstd_block_workspace_bytes(B, p->cin, p->cout, T, V)) return DSTD_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  Carver cv{(char*)workspace};
  BlockLayout L;
  carve_block(cv, L, B, p->cin, p->cout, T, V);
  Plan pl;
  plan_single_block(pl, p->cin, p->cout, B, T, V, hl_device_cus(), flags, taps != nullptr);
  const BlockRun r{p, &L.f, L.xin, L.h, L.yout, BlockTail{TEPI_RAW, nullptr, nullptr, nullptr, nullptr, nullptr}};
  FoldList fa;
  add_block_jobs(fa, p, L.f, T, V);
  DSTD_TRY(run_fold(fa, s));
  DSTD_TRY(to_layout(x, L.xin, B, p->cin, T * V, 1, s));
  DSTD_TRY(spatial_pq(p, L.xin, B, T, V, L.sc.pq_s, s));
  HLList hj;
  add_block_hl_jobs(hj, p, L.f, r.tail, pl.blk[0], T, V);
  DSTD_TRY(run_hl_prep(hj, s));
  BlockArgs A;
  build_block_args(A, r, L.sc, B, T, V, pl.blk[0], nullptr);
  Prof pf;
  for (int i = 0; i < pl.n; ++i)
    DSTD_TRY(run_block_launch(pl.launch[i].kind, r, A, pl.blk[0], L.sc, B, T, V, s, pf, taps));
  DSTD_TRY(to_layout(L.yout, y, B, p->cout, T * V, 0, s));
  return DSTD_OK;
}


}  // namespace

extern "C" {

int dstd_model_fwd(const dstd_model_params* p, const float* x, int B, float* y, void* workspace,
                   size_t workspace_bytes, void* stream) {
  return dstd_model_fwd_ex(p, x, B, y, workspace, workspace_bytes, stream, 0u, nullptr);
}

int dstd_model_fwd_profiled(const dstd_model_params* p, const float* x, int B, float* y, void* workspace,
                            size_t workspace_bytes, void* stream, dstd_profile* prof) {
  return dstd_model_fwd_ex(p, x, B, y, workspace, workspace_bytes, stream, 0u, prof);
}

int dstd_model_fwd_ex(const dstd_model_params* p, const float* x, int B, float* y, void* workspace,
                      size_t workspace_bytes, void* stream, unsigned flags, dstd_profile* prof) {
  if (flags & ~kModelFwdFlags) return DSTD_EINVAL;
  return model_fwd(p, x, B, y, workspace, workspace_bytes, stream, flags, prof, nullptr);
}

int dstd_model_fwd_schedule(int B, int T, int V, int num_feature, int num_layers, unsigned flags, int profiled,
                            int taps, int cus, dstd_launch* out, int capacity) {
  // taps: dstd_model_fwd_taps, which takes DSTD_FWD_EXACT_FP32 only and no profile
  if ((flags & ~((taps & 1) ? DSTD_FWD_EXACT_FP32 : kModelFwdFlags)) || (taps & ~3) || taps == 2 ||
      ((taps & 1) && profiled) || capacity < 0 || (capacity > 0 && !out))
    return DSTD_EINVAL;
  if (const int e = model_shape_code(B, T, V, num_feature, num_layers)) return e;
  Plan pl;
  plan_model(pl, B, T, V, num_feature, num_layers, cus > 0 ? cus : hl_device_cus(), flags, profiled != 0, taps);
  for (int i = 0; i < pl.n && i < capacity; ++i) out[i] = pl.launch[i];
  return pl.n;
}

size_t dstd_model_taps_workspace_bytes(int B, int T, int V, int num_feature, int num_layers) {
  return dstd_model_workspace_bytes(B, T, V, num_feature, num_layers);
}

int dstd_model_fwd_taps(const dstd_model_params* p, const float* x, int B, float* y, const dstd_block_taps* taps,
                        void* workspace, size_t workspace_bytes, void* stream, unsigned flags) {
  if ((flags & ~DSTD_FWD_EXACT_FP32) || !taps) return DSTD_EINVAL;
  return model_fwd(p, x, B, y, workspace, workspace_bytes, stream, flags, nullptr, taps);
}

}  // extern "C"

namespace {

// dstd_model_fwd_ex; taps (dstd_model_fwd_taps, num_layers + 2 entries): the
// unit-parallel schedule, one launch per adjacency and per GC, with every
// block's taps copied out between its launches
int model_fwd(const dstd_model_params* p, const float* x, int B, float* y, void* workspace, size_t workspace_bytes,
              void* stream, unsigned flags, dstd_profile* prof, const dstd_block_taps* taps) {
  // (1) arguments
  StreamDeviceGuard dev_guard_(stream, x);
  if (!p || !x || !y || !workspace) return DSTD_EINVAL;
  if (prof && (prof->capacity < 0 || (prof->capacity > 0 && (!prof->events || !prof->kinds)))) return DSTD_EINVAL;
  const int T = p->T, V = p->V, C = p->num_feature, L_ = p->num_layers, NB = L_ + 2;
  if (p->in_channels != 6) return DSTD_EINVAL;
  if (const int e = model_shape_code(B, T, V, C, L_)) return e;
  if (!block_ptrs_ok(&p->st_in) || !block_ptrs_ok(&p->st_out) || !bn_ok(p->bn_in) || !p->prelu) return DSTD_EINVAL;
  if (p->st_in.cin != 6 || p->st_in.cout != C || p->st_out.cin != C || p->st_out.cout != 3) return DSTD_EINVAL;
  for (int i = 0; i < L_; ++i) {
    if (!block_ptrs_ok(&p->enc[i]) || !bn_ok(p->enc_bn[i]) || !p->enc_prelu[i]) return DSTD_EINVAL;
    if (p->enc[i].cin != C || p->enc[i].cout != C) return DSTD_EINVAL;
  }
  if (workspace_bytes < dstd_model_workspace_bytes(B, T, V, C, L_)) return DSTD_EWORKSPACE;

  // (2) workspace
  hipStream_t s = (hipStream_t)stream;
  Carver cv{(char*)workspace};
  ModelLayout L;
  carve_model(cv, L, B, T, V, C, L_, 6, 3);

  // (3) plan
  Plan pl;
  plan_model(pl, B, T, V, C, L_, hl_device_cus(), flags, prof && prof->capacity > 0,
             taps ? 1 | (taps[0].x ? 2 : 0) : 0);
  const dstd_launch* first = pl.launch + (pl.prep ? 1 : 0);  // (PREP: step 4)
  const bool one_launch = first->kind == DSTD_LAUNCH_MODEL;

  BlockRun run[kPlanMaxBlocks];
  model_block_runs(run, p, L, x, y, one_launch);


  // (4) constants (DSTD_FWD_REUSE_CONSTANTS: still in the workspace) and PREP
  Prof pf;
  pf.p = prof;
  const bool reuse = (flags & DSTD_FWD_REUSE_CONSTANTS) != 0;
  if (!reuse) {
    FoldList fa;
    add_block_jobs(fa, &p->st_in, L.f_in, T, V);
    add_block_jobs(fa, &p->st_out, L.f_out, T, V);
    add_bn_job(fa, p->bn_in, C, V, L.bnin_s, L.bnin_h);
    for (int i = 0; i < L_; ++i) {
      add_block_jobs(fa, &p->enc[i], L.f_enc[i], T, V);
      add_bn_job(fa, p->enc_bn[i], C, V, L.ebn_s[i], L.ebn_h[i]);
    }
    pf.begin(DSTD_KIND_FOLD, s);
    DSTD_TRY(run_fold(fa, s));
    pf.end(s);
  }
  if (pl.prep) {
    pf.begin(DSTD_KIND_PREP, s);
    DSTD_TRY(spatial_pq(&p->st_in, x, B, T, V, L.sc.pq_s, s, L.act[0]));
    pf.end(s);
  }
  if (!reuse) {
    HLList hj;
    for (int b = 0; b < NB; ++b) add_block_hl_jobs(hj, run[b].p, *run[b].f, run[b].tail, pl.blk[b], T, V);
    pf.begin(DSTD_KIND_FOLD, s);
    DSTD_TRY(run_hl_prep(hj, s));
    pf.end(s);
  }

  // (5) the plan's launches
  BlockArgs A[kPlanMaxBlocks];
  for (int b = 0; b < NB; ++b) build_block_args(A[b], run[b], L.sc, B, T, V, pl.blk[b], b == 0 ? x : nullptr);
  for (const dstd_launch* l = first; l < pl.launch + pl.n; ++l) {
    const int b0 = l->first_block, b1 = b0 + l->num_blocks;
    BlockFusedArgs ba;
    if (taps && l->num_blocks != 1) return hipErrorInvalidValue;
    switch (l->kind) {
      case DSTD_LAUNCH_MODEL: {
        ModelChain c{};  // the encoder blocks set the shared geometry: they go first
        for (int i = 0; i < NB; ++i) {
          const int b = i < L_ ? 1 + i : i == L_ ? 0 : NB - 1;
          DSTD_TRY(fused_args(A[b], pl.blk[b], &ba));
          DSTD_TRY(model_chain_append(&c, ba));
        }
        DSTD_TRY(launch_model_chain(c, s));
        break;
      }
      case DSTD_LAUNCH_ENC_RUN: {
        EncChainArgs c{};
        for (int b = b0; b < b1; ++b) {
          DSTD_TRY(fused_args(A[b], pl.blk[b], &ba));
          DSTD_TRY(enc_chain_append(&c, ba));
        }
        DSTD_TRY(launch_enc_chain(c, s));
        break;
      }
      default:
        pf.block = b0;
        DSTD_TRY(run_block_launch(l->kind, run[b0], A[b0], pl.blk[b0], L.sc, B, T, V, s, pf, taps ? &taps[b0] : nullptr));
    }
  }
  return DSTD_OK;
}


}  // namespace

extern "C" {


int dstd_events_create(int n, void** events) {
  if (n < 0 || (n > 0 && !events)) return DSTD_EINVAL;
  for (int i = 0; i < n; ++i) {
    hipEvent_t e;
    DSTD_TRY(hipEventCreate(&e));
    events[i] = (void*)e;
  }
  return DSTD_OK;
}

int dstd_events_destroy(int n, void** events) {
  if (n < 0 || (n > 0 && !events)) return DSTD_EINVAL;
  for (int i = 0; i < n; ++i)
    if (events[i]) DSTD_TRY(hipEventDestroy((hipEvent_t)events[i]));
  return DSTD_OK;
}

int dstd_event_elapsed_ms(void* start, void* stop, float* ms) {
  if (!start || !stop || !ms) return DSTD_EINVAL;
  return (int)hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop);
}

}  // extern "C"

// ---- host-side probe of the chain appends (tests/test_chain_host.py) -------
// Not part of the C ABI.  Builds the blocks of a num_feature = 64 model forward
// at B = 256 as model_fwd does (carve_model, plan_model on 256 compute units,
// model_block_runs, build_block_args, fused_args) over made-up addresses that
// nothing dereferences, XORs xor_word into the 32-bit word at byte_offset of
// block's BlockFusedArgs (block 0 conv_st_in, 1.. the encoders, layers + 1
// conv_st_out) and runs the appends of the plan's whole-forward launch
// (whole_model) or of its run of encoder blocks, launching nothing.  Returns
// 0: every block accepted and the launch's arguments rebuild (*_chain_block) to
// exactly the blocks appended; 1: an append refused; 2: accepted, but a rebuild
// differs; DSTD_EINVAL: no such chain, block or word.
namespace {

struct FakeAddresses {
  uintptr_t next;
  const float* operator()() { return reinterpret_cast<const float*>(next += 4096); }
};
void fake_block_params(dstd_block_params& p, int cin, int cout, FakeAddresses& fake) {
  p.cin = cin;
  p.cout = cout;
  for (const float** q : {&p.A_s, &p.W_s, &p.R_s, &p.A_t, &p.R_t, &p.alpha_sm, &p.alpha_tm, &p.prelu, &p.res_w, &p.res_b})
    *q = fake();
  for (dstd_gc_weights* w : {&p.conv_s[0], &p.conv_s[1], &p.conv_t})
    for (const float** q : {&w->wf, &w->bf, &w->wm1, &w->bm1, &w->wm2, &w->bm2, &w->wrm, &w->brm}) *q = fake();
}

}  // namespace

extern "C" int dstd_debug_chain_probe(int T, int V, int layers, int whole_model, int block, int byte_offset,
                                      unsigned xor_word) {
  constexpr int B = 256, C = 64, cus = 256;
  const int NB = layers + 2;
  if (layers < 1 || model_shape_code(B, T, V, C, layers) != DSTD_OK || block < 0 || block >= NB || byte_offset < 0 ||
      byte_offset % 4 || byte_offset + 4 > (int)sizeof(BlockFusedArgs))
    return DSTD_EINVAL;
  FakeAddresses fake{uintptr_t(1) << 32};
  dstd_model_params p{};
  p.T = T;
  p.V = V;
  p.in_channels = 6;
  p.num_feature = C;
  p.num_layers = layers;
  fake_block_params(p.st_in, 6, C, fake);
  fake_block_params(p.st_out, C, 3, fake);
  p.prelu = fake();
  for (int i = 0; i < layers; ++i) {
    fake_block_params(p.enc[i], C, C, fake);
    p.enc_prelu[i] = fake();
  }
  const float* x = fake();
  float* y = const_cast<float*>(fake());
  Carver cv{reinterpret_cast<char*>(uintptr_t(1) << 40)};
  ModelLayout L;
  carve_model(cv, L, B, T, V, C, layers, 6, 3);
  Plan pl;
  plan_model(pl, B, T, V, C, layers, cus, whole_model ? 0u : DSTD_FWD_SEPARATE_ENDS, false, 0);
  const dstd_launch* l = pl.launch;
  const int kind = whole_model ? DSTD_LAUNCH_MODEL : DSTD_LAUNCH_ENC_RUN;
  while (l < pl.launch + pl.n && l->kind != kind) ++l;
  if (l == pl.launch + pl.n || block < l->first_block || block >= l->first_block + l->num_blocks) return DSTD_EINVAL;
  BlockRun run[kPlanMaxBlocks];
  model_block_runs(run, &p, L, x, y, whole_model != 0);
  BlockFusedArgs ba[kPlanMaxBlocks];
  for (int b = l->first_block; b < l->first_block + l->num_blocks; ++b) {
    BlockArgs A;
    build_block_args(A, run[b], L.sc, B, T, V, pl.blk[b], b == 0 ? x : nullptr);
    if (fused_args(A, pl.blk[b], &ba[b]) != hipSuccess) return DSTD_EINVAL;
  }
  unsigned word;
  memcpy(&word, (const char*)&ba[block] + byte_offset, 4);
  word ^= xor_word;
  memcpy((char*)&ba[block] + byte_offset, &word, 4);
  bool same = true;
  if (whole_model) {
    ModelChain c{};
    for (int i = 0; i < NB; ++i)  // as model_fwd: the encoder blocks first
      if (model_chain_append(&c, ba[i < layers ? 1 + i : i == layers ? 0 : NB - 1]) != hipSuccess) return 1;
    if (!model_chain_complete(c)) return 1;
    for (int b = 0; b < NB; ++b) {
      const BlockFusedArgs r = model_chain_block(c.a, b == 0 ? CHAIN_IN : b == NB - 1 ? CHAIN_OUT : CHAIN_ENC, b - 1);
      same = same && !memcmp(&r, &ba[b], sizeof(r));
    }
  } else {
    EncChainArgs c{};
    for (int b = l->first_block; b < l->first_block + l->num_blocks; ++b)
      if (enc_chain_append(&c, ba[b]) != hipSuccess) return 1;
    for (int i = 0; i < c.nblk; ++i) {
      const BlockFusedArgs r = enc_chain_block(c, i);
      same = same && !memcmp(&r, &ba[l->first_block + i], sizeof(r));
    }
  }
  return same ? 0 : 2;
}
