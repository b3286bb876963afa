// The launch schedule of the eval forward ("Launch schedule").
//
// Host only, integers in, integers out: which kernels a dstd_model_fwd_ex /
// dstd_block_fwd_ex call runs, in which order, is decided here and nowhere
// else.  dstd_capi.hip builds each block's arguments once, walks the list and
// launches; a validator that rejects what the plan chose is an error of the
// call, never a reason to run another schedule.  dstd_model_fwd_schedule
// (include/dstd_gcn.h) returns the same list without touching a GPU.
//
// Not in the list: the two parameter-preparation launches (run_fold,
// run_hl_prep: DSTD_FWD_REUSE_CONSTANTS skips them, nothing else moves them)
// and the tap copies (dstd_gcn_taps.h), which follow the launch whose result
// they copy.  PREP is the list's first entry; the executor enqueues it between
// the two parameter-preparation launches.
#pragma once
#include "../../include/dstd_gcn.h"
#include "dstd_hilo.h"
#include "dstd_kernels.h"

namespace dstd {

// How one DSTDGCB runs.  s / t: its spatial / temporal GC (and their
// adjacencies) on the split-f16 kernels (dstd_hilo.hip), else generic fp32.
struct BlockPlan {
  bool s, t;
  bool tf;        // the temporal GC with its adjacency built in LDS (k_temporal_fused, no k_adj_hl<1>)
  bool bf;        // spatial + fused temporal GC in one launch (k_block_fused)
  bool s_pre;     // the spatial adjacency planes were built by the previous block's temporal launch
  bool adj0;      // (conv_st_in with bf) its spatial planes from the model input in that launch
  bool next_adj;  // builds the next block's spatial adjacency planes (phase 3): that block has s_pre
};

constexpr int kPlanMaxBlocks = DSTD_MAX_LAYERS + 2;
struct Plan {
  unsigned flags;  // effective: with every implied flag set
  int nb;          // blocks: conv_st_in, num_layers encoders, conv_st_out
  BlockPlan blk[kPlanMaxBlocks];
  bool prep;       // the PREP launch (launch_pq with make_x6) runs
  int n;
  dstd_launch launch[1 + 4 * kPlanMaxBlocks];
  void add(int kind, int first, int count) { launch[n++] = dstd_launch{kind, first, count}; }
};

// Every implication between flags that include/dstd_gcn.h documents.
//   taps                          -> SEPARATE_ADJ | SEPARATE_BLOCK | SEPARATE_ENCODERS
//                                    (and the unit-parallel schedule, plan_block's unit)
//   SEPARATE_ADJ, SEPARATE_BLOCK,
//   a profile                     -> SEPARATE_ENCODERS (no encoder run)
//   SEPARATE_ENCODERS             -> SEPARATE_ENDS (no whole-forward launch)
inline unsigned plan_effective_flags(unsigned flags, bool profiled, bool tapped) {
  if (tapped) flags |= DSTD_FWD_SEPARATE_ADJ | DSTD_FWD_SEPARATE_BLOCK | DSTD_FWD_SEPARATE_ENCODERS;
  if (profiled || (flags & (DSTD_FWD_SEPARATE_ADJ | DSTD_FWD_SEPARATE_BLOCK))) flags |= DSTD_FWD_SEPARATE_ENCODERS;
  if (flags & DSTD_FWD_SEPARATE_ENCODERS) flags |= DSTD_FWD_SEPARATE_ENDS;
  return flags;
}

// One block on its own terms (s_pre, adj0 and next_adj depend on its
// neighbours: plan_model).  epi: the temporal kernel's tail (TemporalEpi);
// next_cin: the next block's input channels, 0 without one (the tail then
// produces no spatial P/Q).  Split-f16 GC kernels where the shape has them,
// unless the call asks for exact fp32.
// unit: the unit-parallel schedule at any batch size (the tap entry points:
// every adjacency in a launch of its own, so that it exists in the scratch).
inline BlockPlan plan_block(int cin, int cout, int epi, int next_cin, int B, int T, int V, int cus, unsigned flags,
                            bool unit) {
  BlockPlan r{};
  if (flags & DSTD_FWD_EXACT_FP32) return r;
  r.s = spatial_hl_supported(T, V) &&
        ((cin == 64 && cout == 64) || (cin == 6 && cout == 64) || (cin == 64 && cout == 3));
  r.t = temporal_hl_supported(T, V) &&
        ((cout == 64 && (epi == TEPI_ENC || epi == TEPI_IN || epi == TEPI_RAW) && (!next_cin || next_cin == 64)) ||
         (cout == 3 && (epi == TEPI_OUT || epi == TEPI_RAW) && !next_cin));
  // one workgroup per sample: below one sample per CU the fused kernel leaves
  // CUs idle and the unit-parallel pair (k_adj_hl<1> + k_temporal_hl) wins
  // (B = 16..128: 25-30% faster forward; B = 256: 8% slower, profiles/r03m_small_batch_ab.txt)
  r.tf = r.t && !unit && temporal_fused_supported(T, V) &&
         ((B >= cus && temporal_fused_default(T, V)) || (flags & DSTD_FWD_FUSED_TEMPORAL));
  // the whole block as one launch wherever both GCs run split and the
  // temporal one fused (one workgroup per sample either way)
  r.bf = r.s && r.tf && !(flags & DSTD_FWD_SEPARATE_BLOCK) && block_fused_supported(T, V, cin, cout, epi);
  return r;
}

// The launches of block b on its own, in order.  from_model: the block reads
// the model input itself (conv_st_in of a model forward on the split kernels).
inline void plan_block_launches(Plan& pl, int b, bool from_model) {
  const BlockPlan& k = pl.blk[b];
  if (!k.s_pre && !(k.adj0 && from_model)) pl.add(DSTD_LAUNCH_ADJ_S, b, 1);
  if (!k.bf) pl.add(DSTD_LAUNCH_SPATIAL, b, 1);
  if (!k.tf) pl.add(DSTD_LAUNCH_ADJ_T, b, 1);
  pl.add(k.bf ? DSTD_LAUNCH_BLOCK : k.tf ? DSTD_LAUNCH_TEMPORAL_FUSED : DSTD_LAUNCH_TEMPORAL, b, 1);
}

// dstd_block_fwd_ex / dstd_block_fwd_taps: one block, raw tail, no next block
inline void plan_single_block(Plan& pl, int cin, int cout, int B, int T, int V, int cus, unsigned flags, bool tapped) {
  pl = Plan{};
  pl.flags = plan_effective_flags(flags, false, tapped);
  pl.nb = 1;
  pl.blk[0] = plan_block(cin, cout, TEPI_RAW, 0, B, T, V, cus, pl.flags, tapped);
  plan_block_launches(pl, 0, false);
}

// dstd_model_fwd_ex / dstd_model_fwd_taps.  C: num_feature, L: num_layers;
// cus: the device's compute units; profiled: the call carries a profile with
// capacity > 0; taps: bit 0 tapped, bit 1 block 0's input is tapped.
inline void plan_model(Plan& pl, int B, int T, int V, int C, int L, int cus, unsigned flags, bool profiled, int taps) {
  pl = Plan{};
  const bool tapped = (taps & 1) != 0;
  const unsigned fl = pl.flags = plan_effective_flags(flags, profiled, tapped);
  const int nb = pl.nb = L + 2;
  BlockPlan* k = pl.blk;
  for (int b = 0; b < nb; ++b) {
    const bool first = b == 0, last = b == nb - 1;
    k[b] = plan_block(first ? 6 : C, last ? 3 : C, first ? TEPI_IN : last ? TEPI_OUT : TEPI_ENC, last ? 0 : C, B, T, V,
                      cus, fl, tapped);
  }
  // a block's spatial adjacency from the previous block's fused temporal
  // launch (phase 3), which writes the P/Q it is built from
  for (int b = 1; b < nb && !(fl & DSTD_FWD_SEPARATE_ADJ); ++b)
    if (k[b].s && k[b - 1].tf && C == 64 && temporal_fused_phase3(T, V)) k[b].s_pre = k[b - 1].next_adj = true;
  // block 0's spatial planes (from the model input) inside its block launch
  // rather than a k_adj_hl<0> launch of their own
  k[0].adj0 = k[0].bf && !(fl & DSTD_FWD_SEPARATE_ADJ) && block_fused_adj0_supported(T, V);
  // the split kernels build x6 and block 0's spatial P/Q from x themselves (a
  // tap of block 0's input still needs x6 in memory)
  pl.prep = !k[0].s || (taps & 2);
  if (pl.prep) pl.add(DSTD_LAUNCH_PREP, -1, 0);

  // an encoder block that can share a launch with its neighbours: it would
  // run k_block_fused on planes from the previous launch and build the next's
  const bool runs = !(fl & DSTD_FWD_SEPARATE_ENCODERS) && enc_chain_supported(T, V);
  auto chained = [&](int b) { return runs && b >= 1 && b <= L && k[b].bf && k[b].s_pre && k[b].next_adj; };
  // The whole forward as one launch (k_model_chain): conv_st_in with its own
  // planes (adj0), 1..kModelChainMaxEnc encoder blocks that would form one run,
  // conv_st_out on planes from the last encoder block's phase 3.
  bool model = runs && !(fl & DSTD_FWD_SEPARATE_ENDS) && !tapped && L >= 1 && L <= kModelChainMaxEnc &&
               model_chain_supported(T, V) && k[0].bf && k[0].adj0 && k[0].next_adj && k[nb - 1].bf && k[nb - 1].s_pre;
  for (int b = 1; model && b <= L; ++b) model = chained(b);
  if (model) {
    pl.add(DSTD_LAUNCH_MODEL, 0, nb);
    return;
  }
  // A run of consecutive encoder blocks as one launch (k_enc_chain), at most
  // kEncChainMax of them; a stretch of one keeps its own launch.
  for (int b = 0; b < nb;) {
    int e = b;
    while (e < nb && e - b < kEncChainMax && chained(e)) ++e;
    if (e - b >= 2) {
      pl.add(DSTD_LAUNCH_ENC_RUN, b, e - b);
      b = e;
    } else {
      plan_block_launches(pl, b, b == 0 && k[0].s);
      ++b;
    }
  }
}

}  // namespace dstd
