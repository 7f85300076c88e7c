// The entries of include/rift_hip.h that do not depend on the MFMA operand format: the objective and its backward, AdamW and clipping,
// the PPO critic, the advantage scans, the candidate rollout, the group-advantage tick, the control tick and collate -- and the entries of
// the five extension headers (rift_drivable.h, rift_advantage.h, rift_select.h, rift_footprint.h, rift_offroad.h), defined here with C linkage under their declarations.  They
// use no MFMA and no operand conversion and touch the format-free half of a context only (ctx_core.h), so they are compiled ONCE per
// library and serve contexts of both engine builds; the exported trampolines (abi.cpp) call the rift_* ones directly.
// Every entry follows one protocol (launch.h): the message cleared, its refusals on the host (refuse: "<entry called>: <why>"), call_open,
// its work, call_close; every kernel goes through launch(), so the profiler's record and the two launch diagnostics see all of them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "launch.h"
#include "../../include/rift_drivable.h"
#include "../../include/rift_advantage.h"
#include "../../include/rift_select.h"
#include "../../include/rift_footprint.h"
#include "../../include/rift_offroad.h"
#include "lanes.h"
#include "loss.h"
#include "critic.h"
#include "adv.h"
#include "adv_params.h"
#include "rollout.h"
#include "drivable_map.h"
#include "tick_multi.h"
#include "control.h"
#include "select_params.h"
#include "collision_params.h"
#include "offroad_params.h"
#include "eval_params.h"
#include "objective_params.h"

// devmem.h's hooks: every device allocation and release of the library
__attribute__((visibility("hidden"))) int rift_dev_alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
__attribute__((visibility("hidden"))) void rift_dev_free(void* p) { (void)hipFree(p); }

namespace rift {

int shared_set_attributes() {
  const int big = 160 * 1024;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, big);
  if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&lds_poison_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, big);
  return (int)e;
}

namespace abi {

// The logits of a row are held MAXPL per lane of one wave: f(integral_constant<MAXPL>) with the smallest of 2, 4, 16 that holds G of them
// (loss_kernel, control_tick_kernel)
template <class F>
static void with_logits_per_lane(int G, F&& f) {
  if (G <= 64 * 2) f(std::integral_constant<int, 2>());
  else if (G <= 64 * 4) f(std::integral_constant<int, 4>());
  else f(std::integral_constant<int, 16>());
}

// A scratch buffer that launches still in flight may read grows behind a device-wide wait (ro_raw, tick_scratch, ga_scratch)
template <class T>
static int grow_behind_wait(RiftCtx* c, DevBuf<T>& buf, size_t need, size_t grow_to) {
  if (need > buf.cap() && buf.get()) HIPCHK(c, hipDeviceSynchronize());
  DEVCHK(c, buf.reserve(need, grow_to));
  return RIFT_OK;
}

// scratch of pi_backward_kernel: dz per row and one 16897-float partial per workgroup of RIFT_PI_BWD_ROWS rows (grow-only)
static int pi_backward_scratch(RiftCtx* c, int rows, int nwg) {
  DEVCHK(c, c->l_dz.reserve((size_t)rows));
  DEVCHK(c, c->l_partial.reserve((size_t)nwg * RIFT_PI_NPARAM));
  return RIFT_OK;
}

// pi_head's backward from l_dz, summed over the workgroups into out->flat_grad_sum.  bs > 0: the objective's sums of bs scenes (l_S, l_cnt)
// go to `stats` and out->exchange; bs == 0: no objective, zero scenes, the two sums land in `stats` (the sink)
static void pi_backward_sums(RiftCtx* c, int rows, int nwg, const RiftLossOut* out, int bs, double* stats) {
  launch(c, "pi_backward_kernel", pi_backward_kernel, dim3(nwg), dim3(256), 0, (const float*)c->last_qfinal, (const float*)c->last_hpi,
         (const float*)c->l_dz.get(), rows, c->pi.ln_g, c->pi.ln_b, c->pi.w3, 1e-5f, c->l_partial.get());
  launch(c, "loss_reduce_kernel", loss_reduce_kernel, dim3(cdiv(RIFT_PI_NPARAM, 256)), dim3(256), 0, (const float*)c->l_partial.get(), nwg,
         out->flat_grad_sum, bs ? (const double*)c->l_S.get() : nullptr, bs ? (const double*)c->l_cnt.get() : nullptr, bs, stats,
         bs ? out->exchange : nullptr);
}

// rift_loss_backward (ob == nullptr: the kernel with the reference's literals) and rift_loss_backward_ex (ob: its accepted settings)
static int loss_backward_impl(RiftCtx* c, const char* who, int kind, const RiftLossIn* in, const RiftObjectiveParams* ob, const RiftLossOut* out,
                              double* terms, void* stream) {
  if (!c->loaded) { c->err = std::string(who) + " before rift_forward" + NOT_LOADED; return RIFT_ERR_STATE; }
  if (!c->last_qfinal) { c->err = std::string(who) + " before rift_forward"; return RIFT_ERR_STATE; }
  const int bs = c->last_bs, R = c->last_R, M = 12, G = R * M, rows = bs * G, nwg = cdiv(rows, RIFT_PI_BWD_ROWS);
  if (G > 64 * 16) { c->err = "group too large"; return RIFT_ERR_ARG; }
  LossP p; memset(&p, 0, sizeof(p));
  p.kind = kind; p.bs = bs; p.G = G; p.M = M; p.prob = c->last_prob; p.r_kpm = c->last_rkpm;
  p.old_logits = in->old_group_logits; p.ref_logits = in->ref_group_logits; p.adv64 = in->group_advantage;
  p.valid = in->group_valid_mask; p.action_mode = (const long long*)in->action_mode;
  p.scal_a = kind == RIFT_LOSS_PPO ? in->advantage : in->returns; p.old_log_prob = in->old_log_prob;
  p.clip_eps = in->clip_epsilon; p.lambda_entropy = in->lambda_entropy; p.argmax_rm = (long long*)out->argmax_rm;
  if ((kind == RIFT_LOSS_RIFT || kind == RIFT_LOSS_GRPO) && (!p.old_logits || !p.adv64 || !p.valid)) { c->err = "missing loss inputs"; return RIFT_ERR_ARG; }
  if (kind == RIFT_LOSS_GRPO && !ob && !p.ref_logits) { c->err = "missing ref logits"; return RIFT_ERR_ARG; }
  if (kind == RIFT_LOSS_PPO && (!p.action_mode || !p.scal_a || !p.old_log_prob)) { c->err = "missing ppo inputs"; return RIFT_ERR_ARG; }
  if (kind == RIFT_LOSS_REINFORCE && !p.scal_a) { c->err = "missing returns"; return RIFT_ERR_ARG; }
  if (kind == RIFT_LOSS_SFT && !p.action_mode) { c->err = "missing teacher mode (action_mode)"; return RIFT_ERR_ARG; }
  TRY(call_open(c, stream));
  DEVCHK(c, c->l_S.reserve((size_t)bs)); DEVCHK(c, c->l_cnt.reserve((size_t)bs));
  TRY(pi_backward_scratch(c, rows, nwg));
  if (ob && terms) DEVCHK(c, c->l_T.reserve((size_t)bs * LOSS_NTERM));
  p.S = c->l_S.get(); p.cnt = c->l_cnt.get(); p.dlogit = c->l_dz.get();
  const dim3 lgrid(cdiv(bs, 4)), lblock(256);
  if (ob) {
    p.clip_lo = (float)ob->clip_low; p.clip_hi = (float)ob->clip_high; p.kl_gw = (float)ob->kl_beta; p.ent_gw = (float)ob->entropy_coef;
    p.dual_clip = ob->dual_clip; p.kl_beta = ob->kl_beta; p.ent_coef = ob->entropy_coef; p.T = terms ? c->l_T.get() : nullptr;
    with_logits_per_lane(G, [&](auto m) { launch(c, "loss_kernel", loss_kernel<decltype(m)::value, true>, lgrid, lblock, 0, p); });
    if (terms) launch(c, "loss_terms_kernel", loss_terms_kernel, dim3(1), dim3(64), 0, (const double*)c->l_T.get(), (const double*)c->l_cnt.get(), bs, terms);
  }
  else with_logits_per_lane(G, [&](auto m) { launch(c, "loss_kernel", loss_kernel<decltype(m)::value>, lgrid, lblock, 0, p); });
  pi_backward_sums(c, rows, nwg, out, bs, out->stats);
  return call_close(c);
}

int rift_loss_backward(RiftCtx* c, int kind, const RiftLossIn* in, const RiftLossOut* out, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!in || !out || !out->stats || !out->flat_grad_sum) return refuse(c, "rift_loss_backward", "in, out, out->stats or out->flat_grad_sum == NULL");
  return loss_backward_impl(c, "rift_loss_backward", kind, in, nullptr, out, nullptr, stream);
}

int rift_loss_backward_ex(RiftCtx* c, int kind, const RiftLossIn* in, const RiftObjectiveParams* params, const RiftLossOut* out, double* terms,
                          void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!in || !out || !out->stats || !out->flat_grad_sum) return refuse(c, "rift_loss_backward_ex", "in, out, out->stats or out->flat_grad_sum == NULL");
  if (const char* why = rift_objective_params_refusal(kind, params, in->ref_group_logits != nullptr)) return refuse(c, "rift_loss_backward_ex", why);
  return loss_backward_impl(c, "rift_loss_backward_ex", kind, in, params, out, terms, stream);
}

int rift_head_backward(RiftCtx* c, const float* dlogits, int bs, int R, const RiftLossOut* out, int accumulate, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!dlogits || !out || !out->flat_grad_sum) return refuse(c, "rift_head_backward", "dlogits, out or out->flat_grad_sum == NULL");
  if (!c->loaded) { c->err = "rift_head_backward before rift_forward" + NOT_LOADED; return RIFT_ERR_STATE; }
  if (!c->last_qfinal) { c->err = "rift_head_backward before rift_forward"; return RIFT_ERR_STATE; }
  if (bs != c->last_bs || R != c->last_R)
    return refuse(c, "rift_head_backward", "dlogits of (" + std::to_string(bs) + ", " + std::to_string(R) + ", 12) against a forward of (" +
                                               std::to_string(c->last_bs) + ", " + std::to_string(c->last_R) + ", 12)");
  TRY(call_open(c, stream));
  const int M = 12, rows = bs * R * M, nwg = cdiv(rows, RIFT_PI_BWD_ROWS);
  TRY(pi_backward_scratch(c, rows, nwg));
  DEVCHK(c, c->l_sink.reserve(2));
  launch(c, "head_dz_kernel", head_dz_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, dlogits, (const uint8_t*)c->last_rkpm, rows, M, c->l_dz.get());
  pi_backward_sums(c, rows, nwg, out, 0, c->l_sink.get());
  if (out->grad_w1 || out->grad_b1 || out->grad_ln_w || out->grad_ln_b || out->grad_w2 || out->grad_b2)
    launch(c, "head_scatter_kernel", head_scatter_kernel, dim3(cdiv(RIFT_PI_NPARAM, 256)), dim3(256), 0, (const float*)out->flat_grad_sum,
           out->grad_w1, out->grad_b1, out->grad_ln_w, out->grad_ln_b, out->grad_w2, out->grad_b2, accumulate);
  return call_close(c);
}

int rift_loss_finalize(RiftCtx* c, const RiftLossOut* out, int accumulate, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!out || !out->stats || !out->flat_grad_sum) return refuse(c, "rift_loss_finalize", "out, out->stats or out->flat_grad_sum == NULL");
  TRY(call_open(c, stream));
  launch(c, "loss_finalize_kernel", loss_finalize_kernel, dim3(cdiv(RIFT_PI_NPARAM, 256)), dim3(256), 0, (const float*)out->flat_grad_sum,
         (const double*)out->stats, out->grad_w1, out->grad_b1, out->grad_ln_w, out->grad_ln_b, out->grad_w2, out->grad_b2,
         out->loss, accumulate, (const double*)out->exchange, out->stats);
  return call_close(c);
}

int rift_other_vehicle_rollout(RiftCtx* c, const double* actions, const double* speed, const double* location, const double* yaw_deg,
                               const double* extent, int N, int T, int near_lane_change, double bbox_inflation_ratio, double* vertices,
                               void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (N < 0 || T <= 0) return refuse(c, "rift_other_vehicle_rollout", "N < 0 or T <= 0");
  if (N == 0) return RIFT_OK;
  if (!actions || !speed || !location || !yaw_deg || !extent || !vertices) return refuse(c, "rift_other_vehicle_rollout", "null pointer");
  TRY(call_open(c, stream));
  launch(c, "other_vehicle_rollout_kernel", other_vehicle_rollout_kernel, dim3(cdiv(N, 64)), dim3(64), 0, actions, speed, location, yaw_deg, extent,
         N, T, near_lane_change, bbox_inflation_ratio, vertices);
  return call_close(c);
}

// rift_collision_matrix (sel == nullptr) and riftfp_collision_matrix (include/rift_footprint.h; sel: its accepted params): `who` is the
// entry's name in the message.  The envelope test without first_actor is collision_matrix_kernel's, whichever entry asks for it.
static int collision_matrix(RiftCtx* c, const char* who, const float* center_vertices, int G, int Tc, const double* other_vertices, int N, int Ts,
                            const RiftCollisionParams* sel, uint8_t* collision, int32_t* first_actor, void* stream) {
  if (G <= 0 || Ts <= 0 || Tc < Ts || N < 0 || !center_vertices || !collision || (N > 0 && !other_vertices)) return refuse(c, who, "G <= 0, Ts <= 0, Tc < Ts, N < 0 or a null pointer");
  TRY(call_open(c, stream));
  const int mode = sel ? sel->mode : RIFTFP_ENVELOPE;
  if (mode == RIFTFP_ENVELOPE && !first_actor)
    launch(c, "collision_matrix_kernel", collision_matrix_kernel, dim3(cdiv((long long)G * Ts, 256)), dim3(256), 0, center_vertices, G, Tc,
           other_vertices, N, Ts, collision);
  else
    launch(c, "footprint_collision_kernel", footprint_collision_kernel, dim3(cdiv((long long)G * Ts, 256)), dim3(256), 0, center_vertices, G, Tc,
           other_vertices, N, Ts, mode, collision, first_actor);
  return call_close(c);
}

int rift_collision_matrix(RiftCtx* c, const float* center_vertices, int G, int Tc, const double* other_vertices, int N, int Ts,
                          uint8_t* collision, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  return collision_matrix(c, "rift_collision_matrix", center_vertices, G, Tc, other_vertices, N, Ts, nullptr, collision, nullptr, stream);
}

int rift_off_road_matrix(RiftCtx* c, const float* rollout_center, int n_points, const uint8_t* off_road_mask, int H, int W,
                         double origin_x, double origin_y, double heading, double res_x, double res_y, double off_x, double off_y,
                         uint8_t* off_road, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (n_points <= 0 || H <= 0 || W <= 0 || !rollout_center || !off_road_mask || !off_road || res_x == 0.0 || res_y == 0.0) return refuse(c, "rift_off_road_matrix", "n_points, H or W <= 0, a null pointer or a resolution of 0");
  TRY(call_open(c, stream));
  launch(c, "off_road_kernel", off_road_kernel, dim3(cdiv(n_points, 256)), dim3(256), 0, rollout_center, n_points, off_road_mask,
         H, W, origin_x, origin_y, std::cos(heading), std::sin(heading), res_x, res_y, off_x, off_y, off_road);
  return call_close(c);
}

int rift_sft_teacher_mode(RiftCtx* c, const float* trajectory, const float* teacher_infos, int bs, int R, int M, int T, int frame_rate,
                          int64_t* mode_rm, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!trajectory || !teacher_infos || !mode_rm || bs <= 0 || R <= 0 || M <= 0 || T <= 0 || frame_rate <= 0) return refuse(c, "rift_sft_teacher_mode", "a null pointer, or bs, R, M, T or frame_rate <= 0");
  TRY(call_open(c, stream));
  launch(c, "sft_teacher_mode_kernel", sft_teacher_mode_kernel, dim3(bs), dim3(64), 0, trajectory, teacher_infos, bs, R * M, M, T, frame_rate,
         (long long*)mode_rm);
  return call_close(c);
}

int rift_loss_finalize_clip(RiftCtx* c, const RiftLossOut* out, int accumulate, float max_norm, float* total_norm, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!out || !out->stats || !out->flat_grad_sum || !(max_norm > 0.f)) return refuse(c, "rift_loss_finalize_clip", "out, out->stats or out->flat_grad_sum == NULL, or max_norm not above 0");
  if (!out->grad_w1 || !out->grad_b1 || !out->grad_ln_w || !out->grad_ln_b || !out->grad_w2 || !out->grad_b2)
    return refuse(c, "rift_loss_finalize_clip", "one of the six gradient tensors is NULL");
  TRY(call_open(c, stream));
  launch(c, "loss_finalize_clip_kernel", loss_finalize_clip_kernel, dim3(1), dim3(1024), 0, (const float*)out->flat_grad_sum,
         (const double*)out->stats, out->grad_w1, out->grad_b1, out->grad_ln_w, out->grad_ln_b, out->grad_w2, out->grad_b2,
         out->loss, accumulate, (const double*)out->exchange, out->stats, max_norm, total_norm);
  return call_close(c);
}

int rift_clip_grad_norm(RiftCtx* c, float* const* grads, const int64_t* numels, int n, float max_norm, float* total_norm, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!grads || !numels || n <= 0 || n > 16) return refuse(c, "rift_clip_grad_norm", "grads or numels == NULL, or n outside [1, 16]");
  TRY(call_open(c, stream));
  ClipList L; memset(&L, 0, sizeof(L));
  long long tot = 0;
  for (int i = 0; i < n; ++i) { L.g[i] = grads[i]; L.n[i] = numels[i]; tot += numels[i]; }
  L.count = n;
  const int nb = (int)std::min<long long>(64, (tot + 2047) / 2048);
  DEVCHK(c, c->clip_part.reserve(64));
  launch(c, "clip_norm_partial_kernel", clip_norm_partial_kernel, dim3(nb), dim3(256), 0, L, c->clip_part.get());
  launch(c, "clip_scale_kernel", clip_scale_kernel, dim3(nb), dim3(256), 0, L, (const double*)c->clip_part.get(), nb, max_norm, total_norm);
  return call_close(c);
}

// AdamW's scalars at step `step_new`, formed in double on the host and rounded once, as torch does; put() fills the fields that AdamList and
// TailAdam (loss.h) share, step_size and decay are a tensor's own from its lr and weight decay
struct AdamScalars {
  double bc1, bc2, beta2, omb1, omb2, eps;
  AdamScalars(double step_new, double beta1, double b2, double e)
      : bc1(1.0 - std::pow(beta1, step_new)), bc2(1.0 - std::pow(b2, step_new)), beta2(b2), omb1(1.0 - beta1), omb2(1.0 - b2), eps(e) {}
  float step_size(double lr) const { return (float)(lr / bc1); }
  static float decay(double lr, double weight_decay) { return (float)(1.0 - lr * weight_decay); }
  template <class List> void put(List& l) const { l.beta2 = (float)beta2; l.omb1 = (float)omb1; l.omb2 = (float)omb2; l.bc2_sqrt = (float)std::sqrt(bc2); l.eps = (float)eps; }
};

int rift_adamw_step(RiftCtx* c, int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    float* const* steps, const int64_t* numels, const double* lr, const double* weight_decay, double step_new,
                    double beta1, double beta2, double eps, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (n <= 0 || n > 16 || !params || !grads || !exp_avg || !exp_avg_sq || !steps || !numels || !lr || !weight_decay) return refuse(c, "rift_adamw_step", "n outside [1, 16], or a null pointer");
  if (!(step_new >= 1.0)) return refuse(c, "rift_adamw_step", "step_new below 1");
  AdamList L; memset(&L, 0, sizeof(L));
  const AdamScalars s(step_new, beta1, beta2, eps);
  long long tot = 0;
  for (int i = 0; i < n; ++i) {
    if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || !steps[i] || numels[i] <= 0) return refuse(c, "rift_adamw_step", "a tensor with a null pointer or no elements");
    L.p[i] = params[i]; L.g[i] = grads[i]; L.m[i] = exp_avg[i]; L.v[i] = exp_avg_sq[i]; L.step[i] = steps[i];
    L.n[i] = numels[i]; L.step_size[i] = s.step_size(lr[i]); L.decay[i] = s.decay(lr[i], weight_decay[i]); L.step_new[i] = (float)step_new;
    tot += numels[i];
  }
  L.count = n; L.beta1 = (float)beta1; s.put(L);
  TRY(call_open(c, stream));
  launch(c, "adamw_kernel", adamw_kernel, dim3((int)std::min<long long>(256, (tot + 255) / 256)), dim3(256), 0, L);
  return call_close(c);
}

int rift_update_tail(RiftCtx* c, const RiftLossOut* out, int accumulate, float max_norm, float* total_norm, int n, float* const* params,
                     const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, float* const* steps, const double* lr,
                     const double* weight_decay, double step_new, double beta1, double beta2, double eps, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!out || !out->stats || !out->flat_grad_sum || !(max_norm > 0.f) || n != 6) return refuse(c, "rift_update_tail", "out, out->stats or out->flat_grad_sum == NULL, max_norm not above 0, or n != 6");
  if (!params || !grads || !exp_avg || !exp_avg_sq || !steps || !lr || !weight_decay || !(step_new >= 1.0)) return refuse(c, "rift_update_tail", "a null pointer, or step_new below 1");
  float* const gseg[6] = {out->grad_w1, out->grad_b1, out->grad_ln_w, out->grad_ln_b, out->grad_w2, out->grad_b2};
  TailAdam A; memset(&A, 0, sizeof(A));
  const AdamScalars s(step_new, beta1, beta2, eps);
  for (int sgi = 0; sgi < 6; ++sgi) {
    int j = -1;
    for (int t = 0; t < 6; ++t) if (gseg[sgi] && grads[t] == gseg[sgi]) j = t;
    if (j < 0 || !params[j] || !exp_avg[j] || !exp_avg_sq[j] || !steps[j]) return refuse(c, "rift_update_tail", "the AdamW list does not hold the six pi_head gradient tensors");
    A.p[sgi] = params[j]; A.m[sgi] = exp_avg[j]; A.v[sgi] = exp_avg_sq[j]; A.step[sgi] = steps[j];
    A.step_size[sgi] = s.step_size(lr[j]); A.decay[sgi] = s.decay(lr[j], weight_decay[j]);
  }
  A.step_new = (float)step_new; s.put(A);
  TRY(call_open(c, stream));
  launch(c, "update_tail_kernel", update_tail_kernel, dim3(1), dim3(1024), 0, (const float*)out->flat_grad_sum, (const double*)out->stats,
         out->grad_w1, out->grad_b1, out->grad_ln_w, out->grad_ln_b, out->grad_w2, out->grad_b2, out->loss, accumulate,
         (const double*)out->exchange, out->stats, max_norm, total_norm, A);
  return call_close(c);
}

// ---- PPO critic ------------------------------------------------------------------------------------
static int critic_scratch(RiftCtx* c, int n) {
  const size_t need = (size_t)((n + 15) / 16 * 16) * (128 + 4 * 256 + 1 + 2 * 128 + 2);
  DEVCHK(c, c->cr_buf.reserve(need));
  DEVCHK(c, c->cr_part.reserve((size_t)((n + 15) / 16)));
  return RIFT_OK;
}

static CriticW critic_w(const RiftCritic* w) {
  CriticW q;
  q.w0 = w->w0; q.b0 = w->b0; q.w1 = w->w1; q.b1 = w->b1; q.w2 = w->w2; q.b2 = w->b2;
  q.savg = w->state_avg; q.sstd = w->state_std; q.vavg = w->value_avg; q.vstd = w->value_std;
  return q;
}

int rift_critic_forward(RiftCtx* c, const RiftCritic* w, const float* state, int n, float* value, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!w || !state || !value || n < 0) return refuse(c, "rift_critic_forward", "w, state or value == NULL, or n < 0");
  if (n == 0) return RIFT_OK;
  TRY(call_open(c, stream));
  CriticRowsP p; memset(&p, 0, sizeof(p));
  p.w = critic_w(w); p.state = state; p.n = n; p.value = value;
  launch(c, "critic_rows_kernel", critic_rows_kernel, dim3(cdiv(n, 16)), dim3(256), 0, p);
  return call_close(c);
}

// The critic's backward for n rows: forward recomputed by critic_rows_kernel, whose per-row output delta is the SmoothL1 derivative against
// `target` or the caller's `dvalue`; then flat = scale * sum_rows delta_row * d value_row / d theta -- one thread per parameter, rows summed in order
static int critic_backward_sums(RiftCtx* c, const RiftCritic* w, const float* state, const float* target, const float* dvalue, int n, float scale,
                                float* flat) {
  TRY(critic_scratch(c, n));
  const int np = (n + 15) / 16 * 16, nwg = cdiv(n, 16);
  CriticRowsP p; memset(&p, 0, sizeof(p));
  p.w = critic_w(w); p.state = state; p.target = target; p.dvalue = dvalue; p.n = n;
  p.sn = c->cr_buf.get(); p.h1 = p.sn + (size_t)np * 128; p.h2 = p.h1 + (size_t)np * 256; p.dh1 = p.h2 + (size_t)np * 256;
  p.dh2 = p.dh1 + (size_t)np * 256; p.dout = p.dh2 + (size_t)np * 256; p.sl1_part = c->cr_part.get();
  p.gsa = p.dout + np; p.gss = p.gsa + (size_t)np * 128; p.gva = p.gss + (size_t)np * 128; p.gvs = p.gva + np;
  launch(c, "critic_rows_kernel", critic_rows_kernel, dim3(nwg), dim3(256), 0, p);
  // one sum per segment of `flat`, in its order: the rows' deltas `d` (cd columns) against the layer's input `x` (cx columns: an outer sum,
  // one thread per weight), or alone (x == NULL: a column sum, one thread per column)
  const struct { const float* d; int cd; const float* x; int cx, block, off; } sums[] = {
      {p.dh1, 256, p.sn, 128, 256, 0},      {p.dh1, 256, nullptr, 0, 256, RIFT_CRITIC_OFF_B0},
      {p.dh2, 256, p.h1, 256, 256, RIFT_CRITIC_OFF_W1}, {p.dh2, 256, nullptr, 0, 256, RIFT_CRITIC_OFF_B1},
      {p.dout, 1, p.h2, 256, 256, RIFT_CRITIC_OFF_W2},  {p.dout, 1, nullptr, 0, 64, RIFT_CRITIC_OFF_B2},
      {p.gsa, 128, nullptr, 0, 128, RIFT_CRITIC_OFF_SAVG}, {p.gss, 128, nullptr, 0, 128, RIFT_CRITIC_OFF_SSTD},
      {p.gva, 1, nullptr, 0, 64, RIFT_CRITIC_OFF_VAVG},    {p.gvs, 1, nullptr, 0, 64, RIFT_CRITIC_OFF_VSTD}};
  for (const auto& s : sums)
    if (s.x) launch(c, "critic_outer_sum_kernel", critic_outer_sum_kernel, dim3(cdiv(s.cd * s.cx, s.block)), dim3(s.block), 0, s.d, s.cd, s.x, s.cx, n, scale, flat + s.off);
    else launch(c, "critic_col_sum_kernel", critic_col_sum_kernel, dim3(1), dim3(s.block), 0, s.d, s.cd, n, scale, flat + s.off);
  return RIFT_OK;
}

int rift_critic_loss_backward(RiftCtx* c, const RiftCritic* w, const float* state, const float* reward_sum, int n, double* stats,
                              float* flat, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!w || !state || !reward_sum || !stats || !flat || n <= 0) return refuse(c, "rift_critic_loss_backward", "a null pointer or n <= 0");
  TRY(call_open(c, stream));
  // flat = -sum_rows d SmoothL1 / d theta
  TRY(critic_backward_sums(c, w, state, reward_sum, nullptr, n, -1.f, flat));
  launch(c, "critic_stats_kernel", critic_stats_kernel, dim3(1), dim3(64), 0, (const double*)c->cr_part.get(), cdiv(n, 16), stats);
  return call_close(c);
}

int rift_critic_backward(RiftCtx* c, const RiftCritic* w, const float* state, const float* dvalue, int n, float* flat, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!w || !state || !dvalue || !flat || n <= 0) return refuse(c, "rift_critic_backward", "a null pointer or n <= 0");
  TRY(call_open(c, stream));
  TRY(critic_backward_sums(c, w, state, nullptr, dvalue, n, 1.f, flat));
  return call_close(c);
}

int rift_critic_finalize(RiftCtx* c, const float* flat, const double* stats, float* g_w0, float* g_b0, float* g_w1, float* g_b1,
                         float* g_w2, float* g_b2, float* g_savg, float* g_sstd, float* g_vavg, float* g_vstd, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!flat || !stats) return refuse(c, "rift_critic_finalize", "flat or stats == NULL");
  TRY(call_open(c, stream));
  launch(c, "critic_finalize_kernel", critic_finalize_kernel, dim3(cdiv(RIFT_CRITIC_NPARAM, 256)), dim3(256), 0, flat, stats, g_w0, g_b0,
         g_w1, g_b1, g_w2, g_b2, g_savg, g_sstd, g_vavg, g_vstd);
  return call_close(c);
}

// An empty buffer is a valid (no-op) input of the three scans below, as it is for the reference's loops.
int rift_gae(RiftCtx* c, const double* rewards, const float* undones, const float* values, const float* next_values,
             const float* unterminated, float gamma, float lambda_, int n, float* advantages, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (n < 0) return refuse(c, "rift_gae", "n < 0");
  if (n == 0) return RIFT_OK;
  TRY(call_open(c, stream));
  const GaeCoef k{rewards, undones, values, next_values, unterminated, gamma, lambda_};
  launch(c, "affine_scan_reverse_kernel", affine_scan_reverse_kernel<GaeCoef, float>, dim3(1), dim3(RIFT_SCAN_THREADS), 0, k, n, advantages);
  return call_close(c);
}

int rift_discounted_return(RiftCtx* c, const double* rewards, const float* dones, double gamma, int n, double* returns,
                           void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (n < 0) return refuse(c, "rift_discounted_return", "n < 0");
  if (n == 0) return RIFT_OK;
  TRY(call_open(c, stream));
  const ReturnCoef k{rewards, dones, gamma};
  launch(c, "affine_scan_reverse_kernel", affine_scan_reverse_kernel<ReturnCoef, double>, dim3(1), dim3(RIFT_SCAN_THREADS), 0, k, n, returns);
  return call_close(c);
}

int rift_normalize_advantage(RiftCtx* c, float* x, int n, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (n < 0) return refuse(c, "rift_normalize_advantage", "n < 0");
  if (n == 0) return RIFT_OK;
  TRY(call_open(c, stream));
  launch(c, "normalize_unbiased_kernel", normalize_unbiased_kernel, dim3(1), dim3(256), 0, x, n);
  return call_close(c);
}

int rift_group_advantage(RiftCtx* c, const double* returns, int n_groups, int G, double* advantage, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (n_groups <= 0 || G <= 0) return refuse(c, "rift_group_advantage", "n_groups <= 0 or G <= 0");
  TRY(call_open(c, stream));
  launch(c, "group_zscore_kernel", group_zscore_kernel, dim3(cdiv(n_groups, 4)), dim3(256), 0, returns, n_groups, G, advantage);
  return call_close(c);
}

// The reward half of RiftEvalParams as the kernels take it (adv.h)
static RewardP reward_of(const RiftEvalParams& e) {
  return RewardP{e.alpha_collision, e.alpha_boundary, e.alpha_comfort, e.alpha_l_align, e.alpha_vel_align, e.alpha_l_center, e.alpha_center_bias,
                 e.alpha_velocity, e.alpha_timestep, e.reward_model == RIFT_REWARD_SPARSE ? 1 : 0};
}

int rift_eval_params_default(RiftCtx* c, RiftEvalParams* out) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!out) return refuse(c, "rift_eval_params_default", "out == NULL");
  rift_eval_params_set_default(out);
  return RIFT_OK;
}

template <bool TERMS, class RP>
static void launch_rollout_return(RiftCtx* c, const float* delta_dis, const float* delta_angle, const float* speed, const float* acc,
                                  const float* ang_vel, const float* ang_acc, const uint8_t* collision, int collision_ld, const uint8_t* off_road,
                                  int off_road_ld, int G, int Ts, double gamma, const RP& rp, double* returns, double* terms) {
  launch(c, "rollout_return_kernel", rollout_return_kernel<TERMS, RP>, dim3(cdiv(G, 4)), dim3(256), 0, delta_dis, delta_angle, speed,
         acc, ang_vel, ang_acc, collision, collision_ld, off_road, off_road_ld, G, Ts, gamma, rp, returns, Ts, terms);
}

int rift_rollout_return(RiftCtx* c, const float* delta_dis, const float* delta_angle, const float* speed, const float* acc,
                        const float* ang_vel, const float* ang_acc, const uint8_t* collision, int collision_ld,
                        const uint8_t* off_road, int off_road_ld, int G, int Ts, double gamma, double* returns, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (G <= 0 || Ts <= 0) return refuse(c, "rift_rollout_return", "G <= 0 or Ts <= 0");
  TRY(call_open(c, stream));
  launch_rollout_return<false>(c, delta_dis, delta_angle, speed, acc, ang_vel, ang_acc, collision, collision_ld, off_road, off_road_ld, G, Ts, gamma,
                               RewardDefaults(), returns, nullptr);
  return call_close(c);
}

int rift_rollout_return_ex(RiftCtx* c, const float* delta_dis, const float* delta_angle, const float* speed, const float* acc,
                           const float* ang_vel, const float* ang_acc, const uint8_t* collision, int collision_ld,
                           const uint8_t* off_road, int off_road_ld, int G, int Ts, const RiftEvalParams* params, double* returns,
                           double* terms, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (const char* why = rift_eval_params_refusal(params)) return refuse(c, "rift_rollout_return_ex", why);
  if (G <= 0 || Ts <= 0 || !returns) return refuse(c, "rift_rollout_return_ex", "G <= 0, Ts <= 0 or returns == NULL");
  TRY(call_open(c, stream));
  const RewardP rp = reward_of(*params);
  const double g = params->gamma;
#define RIFT_RR(TERMS, RP) launch_rollout_return<TERMS>(c, delta_dis, delta_angle, speed, acc, ang_vel, ang_acc, collision, collision_ld, off_road, off_road_ld, G, Ts, g, RP, returns, terms)
  if (reward_is_default(rp)) { if (terms) RIFT_RR(true, RewardDefaults()); else RIFT_RR(false, RewardDefaults()); }      // the default weights: the old entry's instance
  else { if (terms) RIFT_RR(true, rp); else RIFT_RR(false, rp); }
#undef RIFT_RR
  return call_close(c);
}

int rift_ref_line_info(RiftCtx* c, const float* traj, int G, int Tfull, int Ts, int M, const float* ref_pos, const float* ref_ang,
                       const int32_t* ref_len, int Pmax, float* delta_dis, float* delta_angle, int32_t* closest_idx, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!traj || !ref_pos || !ref_ang || !ref_len || G <= 0 || Ts <= 0 || M <= 0) return refuse(c, "rift_ref_line_info", "a null pointer, or G <= 0, Ts <= 0 or M <= 0");
  TRY(call_open(c, stream));
  launch(c, "ref_line_info_kernel", ref_line_info_kernel, dim3(cdiv((long long)G * Ts, 128)), dim3(128), 0, traj, G, Tfull, Ts, M,
         ref_pos, ref_ang, (const int*)ref_len, Pmax, delta_dis, delta_angle, (int*)closest_idx);
  return call_close(c);
}

// the closed-loop candidate rollout (rollout.h): eight lanes per candidate, or one (RIFT_RO8=0)
static void launch_rollout(RiftCtx* c, const RolloutP& p) {
  if (c->ro8) launch(c, "rollout8_kernel", rollout8_kernel, dim3(cdiv(p.G, 8)), dim3(64), (size_t)RIFT_RO_LDS_BYTES, p);
  else launch(c, "rollout_kernel", rollout_kernel, dim3(cdiv(p.G, 64)), dim3(64), (size_t)RIFT_RO_LDS_BYTES, p);
}

int rift_rollout(RiftCtx* c, const RiftRolloutIO* io, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!io || !io->trajectories || !io->center_state || io->G <= 0 || io->Tfull < 40 || io->G_per_group <= 0) return refuse(c, "rift_rollout", "io, its trajectories or its center_state == NULL, or G <= 0, Tfull < 40 or G_per_group <= 0");
  RolloutP p; memset(&p, 0, sizeof(p));
  p.traj = io->trajectories; p.G = io->G; p.Tfull = io->Tfull; p.Gper = io->G_per_group; p.state = io->center_state;
  p.turn_buf = io->turn_buf; p.turn_ptr = (int*)io->turn_ptr; p.turn_len = (int*)io->turn_len;
  p.speed_buf = io->speed_buf; p.speed_ptr = (int*)io->speed_ptr; p.speed_len = (int*)io->speed_len;
  p.center = io->center; p.angle = io->angle; p.speed = io->speed; p.acc = io->acc; p.ang_vel = io->ang_vel; p.ang_acc = io->ang_acc;
  p.vertices = io->vertices; p.closest_index = (int*)io->closest_index; p.aim_idx = (int*)io->aim_idx;
  if (!p.center || !p.angle || !p.speed || !p.acc || !p.ang_vel || !p.ang_acc || !p.vertices || !p.closest_index || !p.aim_idx) return refuse(c, "rift_rollout", "an output pointer is NULL");
  TRY(call_open(c, stream));
  // the raw speed history between the two kernels
  TRY(grow_behind_wait(c, c->ro_raw, (size_t)io->G * RIFT_RO_LEN, std::max((size_t)io->G * 2, (size_t)256) * RIFT_RO_LEN));
  p.raw_speed = c->ro_raw.get();
  launch_rollout(c, p);
  launch(c, "rollout_kinematics_kernel", rollout_kinematics_kernel, dim3(cdiv(io->G * RIFT_RO_LEN, 256)), dim3(256), 0, p);
  return call_close(c);
}

// ---- the drivable-area map (include/rift_drivable.h; drivable_grid.h, drivable_map.h) ------------------------------
// the images are released only after the stream that last read them has been waited for
static int drivable_map_release(RiftCtx* c) {
  if (c->dmap.used) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipStreamSynchronize(c->dmap.used_on)); }
  c->dmap.img.reset(); c->dmap.grid = DrivableGrid(); c->dmap.loaded = false; c->dmap.used = false; c->dmap.used_on = nullptr;
  return RIFT_OK;
}

extern "C" int riftdm_load(RiftCtx* c, const double* vertices, const int32_t* poly_start, int n_polys, double cell, double margin, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  DrivableGrid g;
  if (const char* why = drivable_grid_build(vertices, poly_start, n_polys, cell, margin, &g)) return refuse(c, "riftdm_load", why);
  TRY(call_open(c, stream));
  TRY(drivable_map_release(c));
  DrivableImages& im = c->dmap.img;
  DEVCHK(c, im.reserve(g));
  auto up = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
  hipError_t e = up(im.vertices.get(), vertices, (size_t)g.n_vertices * 2 * sizeof(double));
  if (e == hipSuccess) e = up(im.aabb.get(), g.aabb.data(), g.aabb.size() * sizeof(double));
  if (e == hipSuccess) e = up(im.poly_start.get(), poly_start, n_polys ? ((size_t)n_polys + 1) * sizeof(int32_t) : 0);
  if (e == hipSuccess) e = up(im.cell_start.get(), g.cell_start.data(), g.cell_start.size() * sizeof(int32_t));
  if (e == hipSuccess) e = up(im.cell_poly.get(), g.cell_poly.data(), g.cell_poly.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // the host arrays are the caller's and this function's: done with them on return (once per town)
  if (e != hipSuccess) { im.reset(); return refuse(c, "riftdm_load", hipGetErrorString(e), RIFT_ERR_HIP); }
  g.aabb = {}; g.cell_start = {}; g.cell_poly = {};          // (the numbers stay: riftdm_info)
  c->dmap.grid = std::move(g); c->dmap.loaded = true;
  return RIFT_OK;
}

extern "C" int riftdm_clear(RiftCtx* c) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  return drivable_map_release(c);
}

extern "C" int riftdm_info(RiftCtx* c, RiftDrivableInfo* out) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!out) return refuse(c, "riftdm_info", "out == NULL");
  if (!c->dmap.loaded) return refuse(c, "riftdm_info", "no drivable-area map is loaded (riftdm_load)", RIFT_ERR_STATE);
  const DrivableGrid& g = c->dmap.grid;
  memset(out, 0, sizeof(*out));
  out->n_polys = g.n_polys; out->n_vertices = g.n_vertices; out->nx = g.nx; out->ny = g.ny; out->max_cell_list = g.max_list;
  out->cell = g.cell; out->margin = g.margin; out->x0 = g.x0; out->y0 = g.y0; out->device_bytes = (int64_t)c->dmap.img.bytes();
  return RIFT_OK;
}

// Every refusal of a call that reads the map, on the host and ahead of any launch; then the images as a kernel takes them, and the stream noted
static int drivable_map_use(RiftCtx* c, const char* who, double resolution, void* stream, DrivableMapDev* m) {
  if (!c->dmap.loaded) return refuse(c, who, "no drivable-area map is loaded (riftdm_load)", RIFT_ERR_STATE);
  const DrivableGrid& g = c->dmap.grid;
  if (const char* why = drivable_res_refusal(g.margin, (double)(float)resolution)) return refuse(c, who, why);
  const DrivableImages& im = c->dmap.img;
  m->vertices = im.vertices.get(); m->aabb = im.aabb.get(); m->poly_start = im.poly_start.get(); m->cell_start = im.cell_start.get(); m->cell_poly = im.cell_poly.get();
  m->x0 = g.x0; m->y0 = g.y0; m->cell = g.cell; m->margin = g.margin; m->nx = g.nx; m->ny = g.ny;
  c->dmap.used = true; c->dmap.used_on = (hipStream_t)stream;
  return RIFT_OK;
}

// the refusals that riftdm_off_road_matrix and riftdm_raster (`who`) share, then the map and the raster's pose as their kernels take them
static int drivable_call(RiftCtx* c, const char* who, int H, int W, double ox, double oy, double heading, const RiftEvalParams* params, void* stream,
                         DrivableMapDev* m, RasterPose* q) {
  if (const char* why = rift_eval_params_refusal(params)) return refuse(c, who, why);
  if (H <= 0 || W <= 0 || (long long)H * W > (1LL << 30)) return refuse(c, who, "H or W <= 0 (or H * W above 2^30)");
  if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(heading)) return refuse(c, who, "a pose that is not finite");
  TRY(drivable_map_use(c, who, params->resolution, stream, m));
  *q = RasterPose{ox, oy, std::cos(heading), std::sin(heading), (double)(float)params->resolution, (double)(float)(H / 2.0), (double)(float)(W / 2.0),
                  drivable_inv_res((double)(float)params->resolution)};
  return RIFT_OK;
}

extern "C" int riftdm_off_road_matrix(RiftCtx* c, const float* rollout_center, int n_points, int H, int W, double ox, double oy, double heading,
                                      const RiftEvalParams* params, uint8_t* off_road, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (n_points <= 0 || !rollout_center || !off_road) return refuse(c, "riftdm_off_road_matrix", "n_points <= 0 or a null pointer");
  DrivableMapDev m; RasterPose q;
  TRY(drivable_call(c, "riftdm_off_road_matrix", H, W, ox, oy, heading, params, stream, &m, &q));
  TRY(call_open(c, stream));
  launch(c, "off_road_map_kernel", off_road_map_kernel, dim3(cdiv(n_points, 256)), dim3(256), 0, rollout_center, n_points, m, q, H, W, off_road);
  return call_close(c);
}

extern "C" int riftdm_raster(RiftCtx* c, int H, int W, double ox, double oy, double heading, const RiftEvalParams* params, uint8_t* mask, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!mask) return refuse(c, "riftdm_raster", "mask == NULL");
  DrivableMapDev m; RasterPose q;
  TRY(drivable_call(c, "riftdm_raster", H, W, ox, oy, heading, params, stream, &m, &q));
  TRY(call_open(c, stream));
  launch(c, "drivable_raster_kernel", drivable_raster_kernel, dim3(cdiv((long long)H * W, 256)), dim3(256), 0, m, q, H, W, mask);
  return call_close(c);
}

// ---- one rollout tick's group advantages (rift_hip.h) ---------------------------------------------------------------
// Everything but the candidate rollouts is independent between the CBVs: one launch per stage serves a chunk of up to RIFT_TICK_CHUNK of
// them (tick_multi.h) -- reference-line deviations and neighbour forecasts first, then the rollouts CBV by CBV in list order (the shared PID
// state), then kinematics, flags, returns and z-scores: K + 7 launches instead of 9 K.  Three entries share it; TickCall is what they pass on.
// (own_offset: the pixel offset of a CBV comes from its own raster -- the _ex entries; else 200, 200 whatever the raster.  use_map: a CBV
// with a NULL mask and H, W > 0 takes its off-road flags from the drivable-area map -- riftdm_group_advantage_tick.  footprint: the
// collision flags come from the footprints themselves, stage 8 in place of stage 3 -- riftfp_group_advantage_tick in FOOTPRINT mode.
// offroad_footprint: the off-road flags come from the centre and the four corners, stage 9 in place of stage 4 / 7 --
// riftof_group_advantage_tick with the FOOTPRINT extent)
struct TickCall {
  const char* who; const float* trajectory; int Rb, Tfull; const RiftTickCBV* cbvs; int K;
  float* turn_buf; int32_t *turn_ptr, *turn_len; float* speed_buf; int32_t *speed_ptr, *speed_len;
  RiftEvalParams ev; bool own_offset, use_map; double *advantage, *returns, *terms;
  bool footprint = false, offroad_footprint = false;
};
constexpr int TICK_M = 12, TICK_TS = 40, TICK_TR = RIFT_RO_LEN;

// stage 1: the call's refusals; the largest group and neighbour count of the tick, and whether a CBV asks for the map
static int tick_check(RiftCtx* c, const TickCall& t, int* Gmax, int* Nmax, bool* any_map) {
  if (!t.trajectory || !t.cbvs || t.K <= 0 || t.Rb <= 0 || t.Tfull < 80 || !t.advantage || !t.turn_buf || !t.turn_ptr || !t.turn_len || !t.speed_buf || !t.speed_ptr || !t.speed_len) return refuse(c, t.who, "a null pointer, or K <= 0, Rb <= 0 or Tfull < 80");
  for (int k = 0; k < t.K; ++k) {
    const RiftTickCBV& v = t.cbvs[k];
    if (v.R <= 0 || v.R > t.Rb || v.batch_index < 0 || v.Pmax <= 0 || v.n_actors < 0 || !v.center_state || !v.ref_pos || !v.ref_angle || !v.ref_len ||
        (v.n_actors > 0 && !v.actors) || (v.off_road_mask && (v.H <= 0 || v.W <= 0))) return refuse(c, t.who, "bad entry");
    if (t.use_map && !v.off_road_mask) {           // (the map entry: NULL mask and H, W > 0 -- from the map; H == W == 0 -- no flags)
      if (v.H < 0 || v.W < 0 || (v.H == 0) != (v.W == 0)) return refuse(c, t.who, "H or W <= 0 where the map is asked for");
      *any_map = *any_map || v.H > 0;
    }
    *Gmax = std::max(*Gmax, v.R * TICK_M); *Nmax = std::max(*Nmax, v.n_actors);
  }
  return RIFT_OK;
}

// stage 2: a CBV's intermediates in tick_scratch -- byte offsets of 256-aligned pieces, one set (`per` bytes) per CBV of a chunk
struct TickLayout { size_t dd, da, ci, center, angle, speed, acc, av, aa, vert, cl, aim, raw, ov, col, offr, ret, per; };
static TickLayout tick_layout(int Gmax, int Nmax) {
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t G = (size_t)Gmax, Ts = TICK_TS, TR = TICK_TR;
  TickLayout l;
  l.dd = take(G * Ts * 4); l.da = take(G * Ts * 4); l.ci = take(G * Ts * 4);
  l.center = take(G * TR * 2 * 4); l.angle = take(G * TR * 4); l.speed = take(G * TR * 4); l.acc = take(G * TR * 4); l.av = take(G * TR * 4);
  l.aa = take(G * TR * 4); l.vert = take(G * TR * 8 * 4); l.cl = take(G * 79 * 4); l.aim = take(G * 79 * 4); l.raw = take(G * TR * 4);
  l.ov = take((size_t)std::max(Nmax, 1) * Ts * 8 * 8); l.col = take(G * Ts); l.offr = take(G * TR); l.ret = take(G * 8);
  l.per = off;
  return l;
}

// stage 3: the descriptors of the chunk that starts at CBV k0; its largest group and neighbour count, and whether one of its CBVs uses the map
struct TickChunk { TickArr a; int gmax, nmax; bool map; };
static void tick_fill(RiftCtx* c, const TickCall& t, const TickLayout& l, const DrivableMapDev& dmap, bool any_map, int k0, TickChunk* ch) {
  TickArr& a = ch->a; memset(ch, 0, sizeof(*ch));
  a.K = std::min(RIFT_TICK_CHUNK, t.K - k0); a.gamma = t.ev.gamma; a.near_lane_change = t.ev.near_lane_change ? 1 : 0; a.inflation = t.ev.bbox_inflation_ratio;
  a.res = (double)(float)t.ev.resolution;                       // resolution_hw is a float32 array in the reference (traj_evaluator.py:102)
  a.reward = reward_of(t.ev); a.reward_default = reward_is_default(a.reward) ? 1 : 0;
  a.map = dmap; a.map_inv_res = drivable_inv_res(a.res);
  for (int j = 0; j < a.K; ++j) {
    const RiftTickCBV& v = t.cbvs[k0 + j];
    ch->map = ch->map || (any_map && !v.off_road_mask && v.H > 0);
    char* S = c->tick_scratch.get() + l.per * (size_t)j;
    const size_t row = (size_t)(k0 + j) * t.Rb * TICK_M;      // the CBV's row of the caller's (K, Rb, 12) tensors
    TickK& d = a.d[j];
    d.traj = t.trajectory + (size_t)v.batch_index * t.Rb * TICK_M * t.Tfull * 6; d.G = v.R * TICK_M; d.Tfull = t.Tfull; d.Pmax = v.Pmax; d.N = v.n_actors; d.H = v.H; d.W = v.W;
    d.ref_pos = v.ref_pos; d.ref_ang = v.ref_angle; d.ref_len = (const int*)v.ref_len;
    d.dd = (float*)(S + l.dd); d.da = (float*)(S + l.da); d.ci = (int*)(S + l.ci);
    d.actors = v.actors; d.ov = (double*)(S + l.ov);
    RolloutP& p = d.ro;
    p.traj = d.traj; p.G = d.G; p.Tfull = t.Tfull; p.Gper = d.G; p.state = v.center_state;
    p.turn_buf = t.turn_buf; p.turn_ptr = (int*)t.turn_ptr; p.turn_len = (int*)t.turn_len; p.speed_buf = t.speed_buf; p.speed_ptr = (int*)t.speed_ptr; p.speed_len = (int*)t.speed_len;
    p.center = (float*)(S + l.center); p.angle = (float*)(S + l.angle); p.speed = (float*)(S + l.speed); p.acc = (float*)(S + l.acc);
    p.ang_vel = (float*)(S + l.av); p.ang_acc = (float*)(S + l.aa); p.vertices = (float*)(S + l.vert);
    p.closest_index = (int*)(S + l.cl); p.aim_idx = (int*)(S + l.aim); p.raw_speed = (float*)(S + l.raw);
    d.mask = v.off_road_mask; d.ox = v.pose[0]; d.oy = v.pose[1]; d.ch = std::cos(v.pose[2]); d.sh = std::sin(v.pose[2]);
    d.off_x = t.own_offset ? (double)(float)(v.H / 2.0) : 200.0; d.off_y = t.own_offset ? (double)(float)(v.W / 2.0) : 200.0;   // x gets H / 2: the reference's quirk (rift_hip.h)
    d.col = (uint8_t*)(S + l.col); d.offr = (uint8_t*)(S + l.offr);
    d.ret = t.returns ? t.returns + row : (double*)(S + l.ret);       // straight to the caller's tensor when asked for
    d.terms = t.terms ? t.terms + row * 8 : nullptr;
    d.adv = t.advantage + row;
    ch->gmax = std::max(ch->gmax, d.G); ch->nmax = std::max(ch->nmax, d.N);
  }
}

// stage 4: a chunk's launches.  tick_stage: one stage of tick_multi_kernel, `blocks` blocks of `block` threads for each CBV of the chunk
template <int STAGE>
static void tick_stage(RiftCtx* c, const TickArr& a, int blocks, int block) {
  static const char* const label[] = {"tick_multi_kernel_0", "tick_multi_kernel_1", "tick_multi_kernel_2", "tick_multi_kernel_3",
                                      "tick_multi_kernel_4", "tick_multi_kernel_5", "tick_multi_kernel_6", "tick_multi_kernel_7",
                                      "tick_multi_kernel_8", "tick_multi_kernel_9"};
  launch(c, label[STAGE], tick_multi_kernel<STAGE>, dim3(blocks, a.K), dim3(block), 0, a);
}
static void tick_launch(RiftCtx* c, const TickChunk& ch, bool footprint, bool offroad_footprint) {
  const TickArr& a = ch.a;
  tick_stage<0>(c, a, cdiv(ch.gmax * TICK_TS, 128), 128);
  if (ch.nmax > 0) tick_stage<1>(c, a, cdiv(ch.nmax, 64), 64);
  for (int j = 0; j < a.K; ++j) launch_rollout(c, a.d[j].ro);
  tick_stage<2>(c, a, cdiv(ch.gmax * TICK_TR, 256), 256);
  if (footprint) tick_stage<8>(c, a, cdiv(ch.gmax * TICK_TS, 256), 256);     // (in place of stage 3: the footprints themselves, include/rift_footprint.h)
  else tick_stage<3>(c, a, cdiv(ch.gmax * TICK_TS, 256), 256);
  if (offroad_footprint) tick_stage<9>(c, a, cdiv(ch.gmax * TICK_TR * 8, 256), 256);      // (in place of stage 4 / 7: 8 lanes per step, include/rift_offroad.h)
  else if (ch.map) tick_stage<7>(c, a, cdiv(ch.gmax * TICK_TR, 256), 256);      // (in place of stage 4: masks, the map and "no flags" in one launch)
  else tick_stage<4>(c, a, cdiv(ch.gmax * TICK_TR, 256), 256);
  tick_stage<5>(c, a, cdiv(ch.gmax, 4), 256);
  tick_stage<6>(c, a, 1, 256);
}

static int group_advantage_tick(RiftCtx* c, const TickCall& t, void* stream) {
  int Gmax = 0, Nmax = 0;
  bool any_map = false;
  TRY(tick_check(c, t, &Gmax, &Nmax, &any_map));
  DrivableMapDev dmap; memset(&dmap, 0, sizeof(dmap));
  if (any_map) TRY(drivable_map_use(c, t.who, t.ev.resolution, stream, &dmap));
  TRY(call_open(c, stream));
  const TickLayout l = tick_layout(Gmax, Nmax);
  const size_t need = l.per * (size_t)std::min(t.K, RIFT_TICK_CHUNK);
  TRY(grow_behind_wait(c, c->tick_scratch, need, need * 2));
  for (int k0 = 0; k0 < t.K; k0 += RIFT_TICK_CHUNK) {
    TickChunk ch;
    tick_fill(c, t, l, dmap, any_map, k0, &ch);
    tick_launch(c, ch, t.footprint, t.offroad_footprint);
    TRY(call_close(c));
  }
  return RIFT_OK;
}

int rift_group_advantage_tick(RiftCtx* c, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                              float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                              double gamma, double* advantage, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  TickCall t{"rift_group_advantage_tick", trajectory, Rb, Tfull, cbvs, K, turn_buf, turn_ptr, turn_len, speed_buf, speed_ptr, speed_len,
             RiftEvalParams(), false, false, advantage, nullptr, nullptr};
  rift_eval_params_set_default(&t.ev);
  t.ev.gamma = gamma;
  return group_advantage_tick(c, t, stream);
}

int rift_group_advantage_tick_ex(RiftCtx* c, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                 float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                 const RiftEvalParams* params, double* advantage, double* returns, double* terms, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (const char* why = rift_eval_params_refusal(params)) return refuse(c, "rift_group_advantage_tick_ex", why);
  return group_advantage_tick(c, TickCall{"rift_group_advantage_tick_ex", trajectory, Rb, Tfull, cbvs, K, turn_buf, turn_ptr, turn_len, speed_buf,
                                          speed_ptr, speed_len, *params, true, false, advantage, returns, terms}, stream);
}

extern "C" int riftdm_group_advantage_tick(RiftCtx* c, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                           float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                           const RiftEvalParams* params, double* advantage, double* returns, double* terms, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (const char* why = rift_eval_params_refusal(params)) return refuse(c, "riftdm_group_advantage_tick", why);
  return group_advantage_tick(c, TickCall{"riftdm_group_advantage_tick", trajectory, Rb, Tfull, cbvs, K, turn_buf, turn_ptr, turn_len, speed_buf,
                                          speed_ptr, speed_len, *params, true, true, advantage, returns, terms}, stream);
}

// ---- collision flags from the footprints themselves (include/rift_footprint.h; collision_params.h, footprint.h) ----------------------
extern "C" int riftfp_params_default(RiftCollisionParams* out) {
  if (!out) return RIFT_ERR_ARG;
  riftfp_params_set_default(out);
  return RIFT_OK;
}

extern "C" int riftfp_collision_matrix(RiftCtx* c, const float* center_vertices, int G, int Tc, const double* other_vertices, int N, int Ts,
                                       const RiftCollisionParams* params, uint8_t* collision, int32_t* first_actor, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (const char* why = riftfp_refusal(params)) return refuse(c, "riftfp_collision_matrix", why);
  return collision_matrix(c, "riftfp_collision_matrix", center_vertices, G, Tc, other_vertices, N, Ts, params, collision, first_actor, stream);
}

extern "C" int riftfp_group_advantage_tick(RiftCtx* c, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                           float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                           const RiftEvalParams* params, const RiftCollisionParams* collision, double* advantage, double* returns,
                                           double* terms, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (const char* why = riftfp_refusal(collision)) return refuse(c, "riftfp_group_advantage_tick", why);
  if (const char* why = rift_eval_params_refusal(params)) return refuse(c, "riftfp_group_advantage_tick", why);
  TickCall t{"riftfp_group_advantage_tick", trajectory, Rb, Tfull, cbvs, K, turn_buf, turn_ptr, turn_len, speed_buf,
             speed_ptr, speed_len, *params, true, true, advantage, returns, terms};
  t.footprint = collision->mode == RIFTFP_FOOTPRINT;
  return group_advantage_tick(c, t, stream);
}

// ---- off-road flags for the whole footprint (include/rift_offroad.h; offroad_params.h, offroad_extent.h) -----------------------------
extern "C" int riftof_params_default(RiftOffRoadParams* out) {
  if (!out) return RIFT_ERR_ARG;
  riftof_params_set_default(out);
  return RIFT_OK;
}

extern "C" int riftof_off_road_matrix(RiftCtx* c, const float* center, const float* vertices, int n, const uint8_t* mask, int H, int W, double ox,
                                      double oy, double heading, const RiftEvalParams* params, const RiftOffRoadParams* offroad,
                                      uint8_t* off_road, uint8_t* which, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  const char* who = "riftof_off_road_matrix";
  if (const char* why = riftof_matrix_refusal(offroad, vertices, which)) return refuse(c, who, why);
  if (n <= 0 || !center || !off_road) return refuse(c, who, "n <= 0 or a null pointer");
  DrivableMapDev m; RasterPose q;
  memset(&m, 0, sizeof(m));
  if (mask) {                                      // the raster source: rift_off_road_matrix's refusals, the pose as riftdm_off_road_matrix forms it
    if (const char* why = rift_eval_params_refusal(params)) return refuse(c, who, why);
    if (H <= 0 || W <= 0) return refuse(c, who, "H or W <= 0");
    const double res = (double)(float)params->resolution;
    q = RasterPose{ox, oy, std::cos(heading), std::sin(heading), res, (double)(float)(H / 2.0), (double)(float)(W / 2.0), drivable_inv_res(res)};
  }
  else TRY(drivable_call(c, who, H, W, ox, oy, heading, params, stream, &m, &q));
  TRY(call_open(c, stream));
  if (offroad->extent == RIFTOF_CENTER && !which) {      // the kernels and the labels of before
    if (mask) launch(c, "off_road_kernel", off_road_kernel, dim3(cdiv(n, 256)), dim3(256), 0, center, n, mask, H, W, q.ox, q.oy, q.c, q.s, q.res, -q.res,
                     q.off_x, q.off_y, off_road);
    else launch(c, "off_road_map_kernel", off_road_map_kernel, dim3(cdiv(n, 256)), dim3(256), 0, center, n, m, q, H, W, off_road);
  }
  else launch(c, "footprint_off_road_kernel", footprint_off_road_kernel, dim3(cdiv((long long)n * 8, 256)), dim3(256), 0, center, vertices, n, mask, m, q,
              H, W, (int)offroad->extent, off_road, which);
  return call_close(c);
}

extern "C" int riftof_group_advantage_tick(RiftCtx* c, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                           float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                           const RiftEvalParams* params, const RiftCollisionParams* collision, const RiftOffRoadParams* offroad,
                                           double* advantage, double* returns, double* terms, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (const char* why = riftof_refusal(offroad)) return refuse(c, "riftof_group_advantage_tick", why);
  if (const char* why = riftfp_refusal(collision)) return refuse(c, "riftof_group_advantage_tick", why);
  if (const char* why = rift_eval_params_refusal(params)) return refuse(c, "riftof_group_advantage_tick", why);
  TickCall t{"riftof_group_advantage_tick", trajectory, Rb, Tfull, cbvs, K, turn_buf, turn_ptr, turn_len, speed_buf,
             speed_ptr, speed_len, *params, true, true, advantage, returns, terms};
  t.footprint = collision->mode == RIFTFP_FOOTPRINT;
  t.offroad_footprint = offroad->extent == RIFTOF_FOOTPRINT;
  return group_advantage_tick(c, t, stream);
}

// ---- the advantage of the update from stored returns (include/rift_advantage.h; adv_params.h) ----------------------
extern "C" int riftga_params_default(RiftAdvantageParams* out) {
  if (!out) return RIFT_ERR_ARG;
  riftga_params_set_default(out);
  return RIFT_OK;
}

extern "C" int riftga_arena_advantage(RiftCtx* c, const double* returns, const int32_t* r_count, const uint8_t* valid_mask, int n, int Rcap,
                                      const RiftAdvantageParams* params, double* advantage, double* stats, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (const char* why = riftga_refusal(returns, n, Rcap, params, advantage)) return refuse(c, "riftga_arena_advantage", why);
  if (n == 0) return RIFT_OK;
  TRY(call_open(c, stream));
  const bool batch = params->scale == RIFTGA_SCALE_BATCH_RMS;
  ArenaAdvP p; memset(&p, 0, sizeof(p));
  p.ret = returns; p.r_count = r_count; p.mask = valid_mask; p.n = n; p.Rcap = Rcap;
  p.baseline = params->baseline; p.scale = params->scale; p.eps = params->eps; p.clip = params->clip;
  p.adv = advantage; p.stats = stats;
  if (batch || stats) {                                        // the partials travel from launch to launch in the context's scratch
    const size_t need = riftga_scratch_doubles(n);
    TRY(grow_behind_wait(c, c->ga_scratch, need, need * 2));
    p.part = c->ga_scratch.get(); p.tot = p.part + (size_t)n * RIFTGA_NPART;
  }
  launch(c, "arena_adv_scene_kernel", arena_adv_scene_kernel, dim3(cdiv(n, 4)), dim3(256), 0, p);
  if (p.part) launch(c, "arena_adv_reduce_kernel", arena_adv_reduce_kernel, dim3(1), dim3(RIFTGA_REDUCE_THREADS), 0, p);
  if (batch) {
    const size_t total = (size_t)n * Rcap * 12;
    const int count = (stats && params->clip > 0.0) ? 1 : 0;
    launch(c, "arena_adv_scale_kernel", arena_adv_scale_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, RIFTGA_SCALE_BLOCKS)), dim3(256), 0, p, total, count);
    if (count) launch(c, "arena_adv_clamped_kernel", arena_adv_clamped_kernel, dim3(1), dim3(64), 0, (const double*)p.tot, stats);
  }
  return call_close(c);
}

// ---- one rollout tick's decisions (rift_hip.h) ------------------------------------------------------------------------
// Every refusal is decided here, on the host, before anything is launched; then one wave per CBV (control.h), RIFT_CTL_CHUNK descriptors
// per launch.  The checks and the descriptor fill are shared by rift_control_tick and riftcs_control_tick (include/rift_select.h): `who` is
// the entry's name in the message; with `sel` in SAMPLE mode the launches are the <MAXPL, true> instantiations and u[k] rides in CBV k's
// descriptor.
template <bool SAMPLE>
static void control_tick_launch(RiftCtx* c, const CtlArr& a) {
  with_logits_per_lane(a.G, [&](auto m) { launch(c, "control_tick_kernel", control_tick_kernel<decltype(m)::value, SAMPLE>, dim3(a.K), dim3(64), 0, a); });
}

static int control_tick(RiftCtx* c, const char* who, const float* trajectory, const float* probability, const float* ref_free_trajectory, int Rb,
                        int Tfull, const RiftControlCBV* cbvs, int K, int topk, int sample_interval, double* pid_state, int n_slots,
                        const RiftSelectParams* sel, const double* u, double* decision, void* stream) {
  if (K < 0) return refuse(c, who, "K < 0");
  if (Rb < 1) return refuse(c, who, "Rb < 1");
  const long long G = (long long)Rb * 12;
  if (topk < 1 || topk > G) return refuse(c, who, "topk outside [1, Rb * 12]");
  if (sample_interval < 1) return refuse(c, who, "sample_interval < 1");
  if (Tfull < 2 * (long long)sample_interval) return refuse(c, who, "Tfull < 2 * sample_interval (the thinned path needs two points)");
  if (G > 64 * 16) return refuse(c, who, "Rb * 12 above 1024 candidates (16 logits per lane)");
  if (n_slots < 0) return refuse(c, who, "n_slots < 0");
  if (K > 0 && (!trajectory || !probability || !cbvs || !pid_state || !decision)) return refuse(c, who, "null pointer");
  std::vector<int> slots((size_t)K);
  for (int k = 0; k < K; ++k) {
    if (cbvs[k].batch_index < 0) return refuse(c, who, "batch_index < 0");
    if (cbvs[k].slot < 0 || cbvs[k].slot >= n_slots) return refuse(c, who, "slot outside [0, n_slots)");
    slots[(size_t)k] = cbvs[k].slot;
  }
  std::sort(slots.begin(), slots.end());
  if (std::adjacent_find(slots.begin(), slots.end()) != slots.end()) return refuse(c, who, "two CBVs with the same slot");
  if (K == 0) return RIFT_OK;
  TRY(call_open(c, stream));
  const bool sample = sel && sel->mode == RIFTCS_SAMPLE;
  for (int k0 = 0; k0 < K; k0 += RIFT_CTL_CHUNK) {
    CtlArr a; memset(&a, 0, sizeof(a));
    a.K = std::min(RIFT_CTL_CHUNK, K - k0); a.G = (int)G; a.Tfull = Tfull; a.topk = topk; a.interval = sample_interval;
    if (sample) a.inv_t = riftcs_inv_temperature(sel);
    for (int j = 0; j < a.K; ++j) {
      const RiftControlCBV& v = cbvs[k0 + j];
      CtlK& d = a.d[j];
      d.traj = trajectory + (size_t)v.batch_index * (size_t)G * Tfull * 6;
      d.prob = probability + (size_t)v.batch_index * (size_t)G;
      d.rf = ref_free_trajectory ? ref_free_trajectory + (size_t)v.batch_index * Tfull * 4 : nullptr;
      d.state = pid_state + (size_t)v.slot * RIFT_CONTROL_STATE;
      d.dec = decision + (size_t)(k0 + j) * 8;
      d.ox = v.x; d.oy = v.y; d.ch = std::cos(v.heading); d.sh = std::sin(v.heading); d.speed = v.speed;
      if (sample) d.u = u[k0 + j];
    }
    if (sample) control_tick_launch<true>(c, a);
    else control_tick_launch<false>(c, a);
    TRY(call_close(c));
  }
  return RIFT_OK;
}

int rift_control_tick(RiftCtx* c, const float* trajectory, const float* probability, const float* ref_free_trajectory, int Rb, int Tfull,
                      const RiftControlCBV* cbvs, int K, int topk, int sample_interval, double* pid_state, int n_slots, double* decision,
                      void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  return control_tick(c, "rift_control_tick", trajectory, probability, ref_free_trajectory, Rb, Tfull, cbvs, K, topk, sample_interval, pid_state,
                      n_slots, nullptr, nullptr, decision, stream);
}

// ---- the choice of the executed candidate at run time (include/rift_select.h; select_params.h, control.h) ----------------------
extern "C" int riftcs_params_default(RiftSelectParams* out) {
  if (!out) return RIFT_ERR_ARG;
  riftcs_params_set_default(out);
  return RIFT_OK;
}

extern "C" int riftcs_control_tick(RiftCtx* c, const float* trajectory, const float* probability, const float* ref_free_trajectory, int Rb, int Tfull,
                                   const RiftControlCBV* cbvs, int K, int topk, int sample_interval, double* pid_state, int n_slots,
                                   const RiftSelectParams* params, const double* u, double* decision, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (const char* why = riftcs_refusal(params, u, K)) return refuse(c, "riftcs_control_tick", why);
  return control_tick(c, "riftcs_control_tick", trajectory, probability, ref_free_trajectory, Rb, Tfull, cbvs, K, topk, sample_interval,
                      pid_state, n_slots, params, u, decision, stream);
}

int rift_collate(RiftCtx* c, const RiftReplayArena* ar, const int32_t* scene_idx, int bs, int R_out,
                 const RiftFeatureBatch* ob, float* out_old_logits, float* out_ref_logits, double* out_advantage,
                 uint8_t* out_valid_mask, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (!ar || !scene_idx || !ob || bs <= 0 || R_out <= 0 || R_out > ar->Rcap) return refuse(c, "rift_collate", "arena, scene_idx or out_batch == NULL, bs <= 0, or R_out outside [1, arena->Rcap]");
  // the arena's rows are stored padded to its capacities (ar->A, Mp, Rcap, S); the batch is padded to the dimensions of `ob`, which
  // may be smaller (a host arena that grows by doubling keeps capacities above the largest stored scene): every ragged dimension
  // leads its per-scene block, so the crop is a prefix copy
  if (ob->A > ar->A || ob->Mp > ar->Mp || ob->S > ar->S || ob->A <= 0 || ob->T != ar->T) return refuse(c, "rift_collate", "out_batch's A, Mp or S above the arena's, A <= 0, or another T");
  TRY(call_open(c, stream));
  const RiftFeatureBatch& s = ar->scenes;
  const int A = ar->A, Mp = ar->Mp, Rc = ar->Rcap, S = ar->S, T = ar->T;
  const int oA = ob->A, oMp = ob->Mp, oS = ob->S;
  CollateP p; memset(&p, 0, sizeof(p));
  int k = 0;
  auto add = [&](const void* src, void* dst, long long src_bytes, long long dst_bytes) {
    if (!src || !dst || dst_bytes <= 0) return;
    p.src[k] = (const unsigned char*)src; p.dst[k] = (unsigned char*)dst; p.src_bytes[k] = (int)src_bytes; p.dst_bytes[k] = (int)dst_bytes; ++k;
  };
#define FIX(field, n_src, n_dst, per) add(s.field, (void*)ob->field, (long long)(n_src) * (per), (long long)(n_dst) * (per))
  FIX(agent_position, A, oA, T * 8); FIX(agent_heading, A, oA, T * 4); FIX(agent_velocity, A, oA, T * 8);
  FIX(agent_shape, A, oA, T * 8); FIX(agent_category, A, oA, 1); FIX(agent_valid_mask, A, oA, T);
  FIX(map_point_position, Mp, oMp, 3 * 20 * 8); FIX(map_point_vector, Mp, oMp, 3 * 20 * 8);
  FIX(map_point_orientation, Mp, oMp, 3 * 20 * 4); FIX(map_polygon_center, Mp, oMp, 12);
  FIX(map_polygon_type, Mp, oMp, 1); FIX(map_polygon_on_route, Mp, oMp, 1); FIX(map_polygon_tl_status, Mp, oMp, 1);
  FIX(map_polygon_has_speed_limit, Mp, oMp, 1); FIX(map_polygon_speed_limit, Mp, oMp, 4); FIX(map_valid_mask, Mp, oMp, 20);
  FIX(static_position, S, oS, 8); FIX(static_heading, S, oS, 4); FIX(static_shape, S, oS, 8);
  FIX(static_category, S, oS, 1); FIX(static_valid_mask, S, oS, 1); FIX(current_state, 1, 1, ar->cs_ld * 4);
#undef FIX
#define RAG(srcp, dstp, per_line) add((srcp), (void*)(dstp), (long long)Rc * (per_line), (long long)R_out * (per_line))
  RAG(s.ref_position, ob->ref_position, 120 * 8); RAG(s.ref_vector, ob->ref_vector, 120 * 8);
  RAG(s.ref_orientation, ob->ref_orientation, 120 * 4); RAG(s.ref_valid_mask, ob->ref_valid_mask, 120);
  RAG(ar->old_group_logits, out_old_logits, 12 * 4); RAG(ar->ref_group_logits, out_ref_logits, 12 * 4);
  RAG(ar->group_advantage, out_advantage, 12 * 8); RAG(ar->group_valid_mask, out_valid_mask, 12);
#undef RAG
  p.nt = k;
  launch(c, "collate_kernel", collate_kernel, dim3(bs, k), dim3(256), 0, p, scene_idx);
  return call_close(c);
}

}}  // namespace rift::abi

// an entry whose signature drifts from the header does not compile: the rift_* ones by this list (their trampolines are abi.cpp's), the
// extensions' by their C linkage (a second declaration of another type is an error)
#define RIFT_SHARED_FN(name) static_assert(std::is_same<decltype(&::name), decltype(&rift::abi::name)>::value, #name);
#include "abi_list.h"
#undef RIFT_SHARED_FN
