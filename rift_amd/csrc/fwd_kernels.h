// Which kernel every stage of a forward runs: decided ONCE, before the first allocation, from the path switches, the per-call flags and
// the batch shape below.  The stages of forward_impl (engine.hip) read nothing else for a path: no switch of Ctx::Switches, no shape
// condition of their own, no pointer an earlier stage may have left.  Host-only and free of HIP, like fwd_plan.h, so that
// tests/test_host_api.py can compile it with the system compiler and check it over its inputs.
//
// KernelIn has no `dry` member and no pointer: the sizing pass and the launch pass of rift_forward get the SAME plan, so they walk the
// same allocations (rift_forward checks that they did).  Everything in it is a function of rift_forward's sizing key and of the switches
// fixed when the context is made.
//
// The layer-wise paths (fwd_layerwise.h) are the reference forward: what RIFT_F_FP32 runs and what the RIFT_*_UNFUSED switches select
// stage by stage.
#pragma once

struct KernelIn {
  // the path switches of Ctx::Switches (RIFT_*_UNFUSED, RIFT_FO_W, RIFT_PE_W, RIFT_NAT_COMPACT, RIFT_PE_LIVE, RIFT_PE_PACK, RIFT_RANK_IN_PREP,
  // RIFT_ENC112, RIFT_DEC_DEFER, RIFT_DEC_SPLIT, RIFT_DEC_LAYERS, RIFT_DEC_TS)
  bool nat_fused, dec_fused, enc_fused, pe_fused, fo_fused, fpn_fused, ego_fused, heads_fused, pi_fused;
  bool fo_w, pe_w, nat_compact, pe_live, pe_pack, rank_in_prep, enc112;
  int dec_defer_max; bool dec_split; int dec_layers; bool dec_ts;
  // per call: RIFT_F_FP32 / _TRAIN / (_TRAIN and not _NO_DROP) / _NEED_TRAJ, RiftOutputs::trajectory given, RIFT_F_DEFER_HEAD, rift_prof_enable
  bool fp32, train, drop, need_traj, want_traj, defer_head, prof_on;
  bool forked;                 // StreamPlan::forked of the launch pass (fwd_plan.h)
  int bs, A, Mp, S, R;         // the batch shape; token slots N = A + Mp + S
  int enc_nw;                  // build constant: the waves of enc_fused_kernel (ENC_NW); only the eight-wave build emits the decoder's operands
  // RIFT_NAT_GROUP (0: off) and RIFT_NO_SKIP (1: nothing a DropPath drop would skip is skipped): the history encoder's DropPath grouping
  bool nat_group = true, no_skip = false;
};

enum PePath { PE_LAYERWISE = 0, PE_PAIR_MID, PE_PAIR_W };            // one encoder after the other; the pair with pe_mid_kernel / pe_w_kernel as pass B
enum FoPath { FO_LAYERWISE = 0, FO_EACH, FO_THREE, FO_THREE_W };     // GEMMs; fourier_fused_kernel per embedding; the three in one launch by it / by fo_w_kernel
enum EncPath { ENC_LAYERWISE = 0, ENC_FUSED96, ENC_FUSED112, ENC_W };
enum DecImage { IMG_NONE = 0, IMG_TILE, IMG_DENSE };                 // the decoder's K | V^T operand image: none, key tiles (dec_w.h), dense per head (dec_kv.h)
enum DecPath { DEC_LAYERWISE = 0, DEC_FUSED, DEC_FUSED_DENSE };      // DEC_FUSED gathers from IMG_TILE, DEC_FUSED_DENSE (rounds of eight key tiles) from IMG_DENSE
struct LayerRange { int l0, l1; };

struct KernelPlan {
  // agent history
  bool hist_wave;              // the three NAT levels as the wave-private kernels, one launch each; else layer-wise
  bool fpn_fused;              // fpn_tail_kernel, and with it the levels' Oc rows as 16-bit operand words
  bool nat_compact;            // the history chain on the compacted valid sequences
  bool rank_in_prep;           // ... ranked by the first blocks of prep_kernel instead of nat_rank_kernel
  bool nat_group;              // levels 1 and 2 take their sequences grouped by DropPath pattern and skip what a whole tile / round drops (nat_l0w.h: nat_group_body)
  bool ego_fused;
  // map chain
  PePath pe;
  bool pe_stats_persistent;    // pass A as pe_stats1p_kernel: one statistics partial per workgroup
  bool pe_pack, pe_live;       // pass B on packed reference-line rounds / on the live rounds of pass A's counts
  FoPath fourier;
  bool q0_early;               // the decoder queries behind the three-in-one embedding on the forked map chain, ahead of the join
  // scene encoder and what it hands the decoder
  EncPath enc;
  DecImage enc_image;          // what the encoder's tail emits
  bool enc_kpm_x0p;            // ... and with it the compacted rows' key padding and cat_x_proj's ego-token half
  bool dec_kv_frag;            // dec_kv_frag_kernel makes the dense image from the encoder's output
  // planning decoder
  DecPath dec;
  int dec_n_now; LayerRange dec_now[2];      // the launches of the forward itself (layer-wise: one range, the layers that run)
  bool dec_defer;              // the decoder, or its second half, goes with the deferred head (rift_forward_head_back)
  bool dec_split;              // ... its second half: layers [0, 2) run now and hand their dropout streams on
  LayerRange dec_later;
  // heads
  bool pi_fused, heads_fused;
  bool head_traj;              // the trajectory heads run on the policy head's q_final
};

// wave-private history levels: also what lets the stream plan fork (PlanIn::nat_fused)
inline bool plan_hist_wave(const KernelIn& in) { return in.nat_fused && !in.fp32; }

inline KernelPlan plan_kernels(const KernelIn& in) {
  KernelPlan p;
  const int N = in.A + in.Mp + in.S, R = in.R, bs = in.bs;
  const bool bf = !in.fp32;      // the 16-bit operand mode: every fused kernel is one of it
  // ---- agent history.  Compaction needs the whole fused chain: the wave-private levels write compacted rows and only fpn_tail_kernel
  // scatters them back; the layer-wise / fp32 path keeps all sequences
  p.hist_wave = plan_hist_wave(in);
  p.fpn_fused = p.hist_wave && in.fpn_fused;
  p.nat_compact = p.fpn_fused && in.nat_compact;
  p.rank_in_prep = p.nat_compact && in.rank_in_prep && in.A <= 256;
  // a train-mode forward with drops on the compacted wave-private chain (the lists are made from the class counts); else the levels get no
  // list: rank order and every half-block computed
  p.nat_group = p.nat_compact && in.drop && in.nat_group && !in.no_skip;
  p.ego_fused = bf && in.ego_fused;
  // ---- PointsEncoders
  p.pe = !(bf && in.pe_fused) ? PE_LAYERWISE : (in.pe_w ? PE_PAIR_W : PE_PAIR_MID);
  p.pe_stats_persistent = p.pe == PE_PAIR_W && in.train;
  p.pe_pack = p.pe == PE_PAIR_W && in.pe_pack;
  p.pe_live = p.pe_stats_persistent && in.pe_live;
  // ---- Fourier embeddings: token positions, speed limits and reference-line positions depend on inputs only, so with both PointsEncoders
  // done side by side they are ONE launch (static objects bring a fourth embedding: each on its own then)
  const bool three = bf && in.fo_fused && p.pe != PE_LAYERWISE && in.S == 0;
  p.fourier = !(bf && in.fo_fused) ? FO_LAYERWISE : (!three ? FO_EACH : (in.fo_w ? FO_THREE_W : FO_THREE));
  p.q0_early = in.forked && three;
  // ---- scene encoder.  97 .. 112 token slots (what train_cbv collates: 49 + 60 = 109): the fused kernel on its 112-row layout when the
  // decoder's eight-key-tile variant consumes its image; RIFT_ENC112=0 keeps those shapes on enc_w_kernel
  const bool tail = in.dec_fused && R <= 8 && in.enc_nw == 8;      // the fused encoder's tail can emit the decoder's operands
  const bool wide = N > 96 && N <= 112 && in.enc112 && tail;
  p.enc = !(bf && in.enc_fused) ? ENC_LAYERWISE : (N <= 96 ? ENC_FUSED96 : (wide ? ENC_FUSED112 : (N <= 192 ? ENC_W : ENC_LAYERWISE)));
  p.enc_image = IMG_NONE;
  if (p.enc == ENC_FUSED96 && tail) p.enc_image = IMG_TILE;
  if (p.enc == ENC_FUSED112) p.enc_image = IMG_DENSE;
  if (p.enc == ENC_W && in.dec_fused && R <= 16) p.enc_image = IMG_DENSE;
  p.enc_kpm_x0p = p.enc_image != IMG_NONE && p.enc != ENC_W;
  // ---- planning decoder: the kernel's tile variant at R <= 8 lines and N <= 96 slots, from the encoder's image only; its dense variant up
  // to 16 lines and 192 slots, from whoever makes the dense image
  const bool dense_shape = (R > 8 || N > 96) && R <= 16 && N <= 192;
  p.dec_kv_frag = bf && in.dec_fused && dense_shape && p.enc_image == IMG_NONE;
  p.dec = !(bf && in.dec_fused) ? DEC_LAYERWISE : (dense_shape ? DEC_FUSED_DENSE : (p.enc_image == IMG_TILE ? DEC_FUSED : DEC_LAYERWISE));
  // Deferral.  Which batches: measured per size (profiles/r04_batch_sweep.txt; ms per step with / without): 32 0.18 / 0.23, 64 0.21 / 0.24, 80 0.253 / 0.264,
  // 88 0.259 / 0.254, 96 0.315 / 0.300, 104 0.325 / 0.321, 112 0.338 / 0.359, 128 0.368 / 0.381, 160 0.433 / 0.440, 192 0.503 / 0.520, 256 0.656 / 0.65 -- a win
  // except between 84 and 108 scenes and at a chip-filling batch.  With the trajectory heads on, the tail behind the decoder is longer and
  // the caller's queue carries the prediction head too: measured worth it up to twice the batch -- 128 scenes 0.419 -> 0.391 ms, 256 scenes
  // 0.707 -> 0.713.  RIFT_DEC_DEFER=<n> replaces the table by bs <= n (0: never).  Not while profiling per kernel or with the decoder's
  // timestamp tap on.
  const bool size_ok = in.dec_defer_max >= 0 ? bs <= in.dec_defer_max : (in.need_traj ? bs <= 128 : (bs <= 84 || (bs >= 108 && bs <= 192)));
  p.dec_defer = p.dec != DEC_LAYERWISE && in.defer_head && size_ok && !in.prof_on && !in.dec_ts;
  // ... and split: layers 0 - 1 here, behind the encoder, layers 2 - 3 in front of the deferred head -- token assembly + encoder + half a decoder
  // on the caller's queue against half a decoder + tail on the update stream (9 + 88 + 55 against 55 + 80 us at 32 scenes) instead of 97 against
  // 190.  The dropout streams of the second launch carry on from the states the first one leaves (rng_io): the draws are a single launch's.
  // Measured (ms per step, split / one launch): 64 scenes 0.217 / 0.229, 32 scenes 0.20 - 0.21 / 0.20 - 0.21 (the host issues a 32-scene step in 0.15 - 0.2 ms: it
  // bounds that one now); with the trajectory heads on the caller's queue carries the prediction head as well and the split LOSES (0.30 / 0.26 at 64): off there.
  p.dec_split = p.dec_defer && in.dec_split && !in.need_traj;
  // RIFT_DEC_LAYERS (diagnostic) 0 / 2: the non-deferred decoder stops after that many layers; 22: an eval forward's layers as two launches of
  // the kernel; anything else: all four, one launch
  const LayerRange none = {0, 0}, all = {0, 4}, lo = {0, 2}, hi = {2, 4};
  p.dec_n_now = 1; p.dec_now[0] = all; p.dec_now[1] = none; p.dec_later = none;
  if (p.dec_defer) {
    p.dec_n_now = p.dec_split ? 1 : 0; p.dec_now[0] = p.dec_split ? lo : none; p.dec_later = p.dec_split ? hi : all;
  } else if (in.dec_layers == 22 && p.dec != DEC_LAYERWISE && !in.drop) {
    p.dec_n_now = 2; p.dec_now[0] = lo; p.dec_now[1] = hi;
  } else if (in.dec_layers == 2) {
    p.dec_now[0] = lo;
  } else if (in.dec_layers == 0) {
    p.dec_n_now = 0; p.dec_now[0] = none;
  }
  // ---- heads
  p.pi_fused = bf && in.pi_fused;
  p.heads_fused = bf && in.heads_fused;
  p.head_traj = in.need_traj && in.want_traj;
  return p;
}
