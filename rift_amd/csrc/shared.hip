// The entries of include/rift_hip.h that do not depend on the MFMA operand format: the objective and its backward, AdamW and clipping,
// the PPO critic, the advantage scans, the candidate rollout, the drivable-area map, the group-advantage tick, the control tick and collate.  They use no MFMA and
// no operand conversion and touch the format-free half of a context only (ctx_core.h), so they are compiled ONCE per library and serve
// contexts of both engine builds; the exported trampolines (abi.cpp) call them directly.
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

// scratch of pi_backward_kernel: dz per row and one 16897-float partial per workgroup of RIFT_PI_BWD_ROWS rows (grow-only)
static int pi_backward_scratch(RiftCtx* c, int rows, int nwg) {
  DEVCHK(c, c->l_dz.reserve((size_t)rows));
  DEVCHK(c, c->l_partial.reserve((size_t)nwg * RIFT_PI_NPARAM));
  return RIFT_OK;
}

// rift_loss_backward (ob == nullptr: the kernel with the reference's literals) and rift_loss_backward_ex (ob: its accepted settings)
static int loss_backward_impl(RiftCtx* c, const char* who, int kind, const RiftLossIn* in, const RiftObjectiveParams* ob, const RiftLossOut* out,
                              double* terms, void* stream) {
  if (!c->loaded) { c->err = std::string(who) + " before rift_forward" + NOT_LOADED; return RIFT_ERR_STATE; }
  if (!c->last_qfinal) { c->err = std::string(who) + " before rift_forward"; return RIFT_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  const int bs = c->last_bs, R = c->last_R, M = 12, G = R * M, rows = bs * G;
  if (G > 64 * 16) { c->err = "group too large"; return RIFT_ERR_ARG; }
  const int nwg = cdiv(rows, RIFT_PI_BWD_ROWS);
  DEVCHK(c, c->l_S.reserve((size_t)bs)); DEVCHK(c, c->l_cnt.reserve((size_t)bs));
  TRY(pi_backward_scratch(c, rows, nwg));
  LossP p; memset(&p, 0, sizeof(p));
  p.kind = kind; p.bs = bs; p.G = G; p.M = M; p.prob = c->last_prob; p.r_kpm = c->last_rkpm;
  p.old_logits = in->old_group_logits; p.ref_logits = in->ref_group_logits; p.adv64 = in->group_advantage;
  p.valid = in->group_valid_mask; p.action_mode = (const long long*)in->action_mode;
  p.scal_a = kind == RIFT_LOSS_PPO ? in->advantage : in->returns; p.old_log_prob = in->old_log_prob;
  p.clip_eps = in->clip_epsilon; p.lambda_entropy = in->lambda_entropy;
  p.S = c->l_S.get(); p.cnt = c->l_cnt.get(); p.dlogit = c->l_dz.get(); p.argmax_rm = (long long*)out->argmax_rm;
  if ((kind == RIFT_LOSS_RIFT || kind == RIFT_LOSS_GRPO) && (!p.old_logits || !p.adv64 || !p.valid)) { c->err = "missing loss inputs"; return RIFT_ERR_ARG; }
  if (kind == RIFT_LOSS_GRPO && !ob && !p.ref_logits) { c->err = "missing ref logits"; return RIFT_ERR_ARG; }
  if (kind == RIFT_LOSS_PPO && (!p.action_mode || !p.scal_a || !p.old_log_prob)) { c->err = "missing ppo inputs"; return RIFT_ERR_ARG; }
  if (kind == RIFT_LOSS_REINFORCE && !p.scal_a) { c->err = "missing returns"; return RIFT_ERR_ARG; }
  if (kind == RIFT_LOSS_SFT && !p.action_mode) { c->err = "missing teacher mode (action_mode)"; return RIFT_ERR_ARG; }
  const dim3 lgrid(cdiv(bs, 4)), lblock(256);
  if (ob) {
    if (terms) DEVCHK(c, c->l_T.reserve((size_t)bs * LOSS_NTERM));
    p.clip_lo = (float)ob->clip_low; p.clip_hi = (float)ob->clip_high; p.kl_gw = (float)ob->kl_beta; p.ent_gw = (float)ob->entropy_coef;
    p.dual_clip = ob->dual_clip; p.kl_beta = ob->kl_beta; p.ent_coef = ob->entropy_coef; p.T = terms ? c->l_T.get() : nullptr;
    if (G <= 64 * 2) launch(c, "loss_kernel", loss_kernel<2, true>, lgrid, lblock, 0, p);
    else if (G <= 64 * 4) launch(c, "loss_kernel", loss_kernel<4, true>, lgrid, lblock, 0, p);
    else launch(c, "loss_kernel", loss_kernel<16, true>, lgrid, lblock, 0, p);
    if (terms) launch(c, "loss_terms_kernel", loss_terms_kernel, dim3(1), dim3(64), 0, (const double*)c->l_T.get(), (const double*)c->l_cnt.get(), bs, terms);
  }
  else if (G <= 64 * 2) launch(c, "loss_kernel", loss_kernel<2>, lgrid, lblock, 0, p);
  else if (G <= 64 * 4) launch(c, "loss_kernel", loss_kernel<4>, lgrid, lblock, 0, p);
  else launch(c, "loss_kernel", loss_kernel<16>, lgrid, lblock, 0, p);
  launch(c, "pi_backward_kernel", pi_backward_kernel, dim3(nwg), dim3(256), 0, (const float*)c->last_qfinal, (const float*)c->last_hpi,
         (const float*)c->l_dz.get(), rows, c->pi.ln_g, c->pi.ln_b, c->pi.w3, 1e-5f,
         c->l_partial.get());
  launch(c, "loss_reduce_kernel", loss_reduce_kernel, dim3(cdiv(RIFT_PI_NPARAM, 256)), dim3(256), 0, (const float*)c->l_partial.get(), nwg,
         out->flat_grad_sum, (const double*)c->l_S.get(), (const double*)c->l_cnt.get(), bs, out->stats, out->exchange);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_loss_backward(RiftCtx* c, int kind, const RiftLossIn* in, const RiftLossOut* out, void* stream) {
  if (!c || !in || !out || !out->stats || !out->flat_grad_sum) return RIFT_ERR_ARG;
  c->err.clear();
  return loss_backward_impl(c, "rift_loss_backward", kind, in, nullptr, out, nullptr, stream);
}

int rift_loss_backward_ex(RiftCtx* c, int kind, const RiftLossIn* in, const RiftObjectiveParams* params, const RiftLossOut* out, double* terms,
                          void* stream) {
  if (!c || !in || !out || !out->stats || !out->flat_grad_sum) return RIFT_ERR_ARG;
  c->err.clear();
  if (const char* why = rift_objective_params_refusal(kind, params, in->ref_group_logits != nullptr)) {
    c->err = std::string("rift_loss_backward_ex: ") + why;
    return RIFT_ERR_ARG;
  }
  return loss_backward_impl(c, "rift_loss_backward_ex", kind, in, params, out, terms, stream);
}

int rift_head_backward(RiftCtx* c, const float* dlogits, int bs, int R, const RiftLossOut* out, int accumulate, void* stream) {
  if (!c || !dlogits || !out || !out->flat_grad_sum) return RIFT_ERR_ARG;
  c->err.clear();
  if (!c->loaded) { c->err = "rift_head_backward before rift_forward" + NOT_LOADED; return RIFT_ERR_STATE; }
  if (!c->last_qfinal) { c->err = "rift_head_backward before rift_forward"; return RIFT_ERR_STATE; }
  if (bs != c->last_bs || R != c->last_R) {
    c->err = "rift_head_backward: dlogits of (" + std::to_string(bs) + ", " + std::to_string(R) + ", 12) against a forward of (" +
             std::to_string(c->last_bs) + ", " + std::to_string(c->last_R) + ", 12)";
    return RIFT_ERR_ARG;
  }
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  const int M = 12, rows = bs * R * M, nwg = cdiv(rows, RIFT_PI_BWD_ROWS);
  TRY(pi_backward_scratch(c, rows, nwg));
  DEVCHK(c, c->l_sink.reserve(2));
  launch(c, "head_dz_kernel", head_dz_kernel, dim3(cdiv(rows, 256)), dim3(256), 0, dlogits, (const uint8_t*)c->last_rkpm, rows, M, c->l_dz.get());
  launch(c, "pi_backward_kernel", pi_backward_kernel, dim3(nwg), dim3(256), 0, (const float*)c->last_qfinal, (const float*)c->last_hpi,
         (const float*)c->l_dz.get(), rows, c->pi.ln_g, c->pi.ln_b, c->pi.w3, 1e-5f,
         c->l_partial.get());
  // (no objective: zero scenes, the two sums land in the sink)
  launch(c, "loss_reduce_kernel", loss_reduce_kernel, dim3(cdiv(RIFT_PI_NPARAM, 256)), dim3(256), 0, (const float*)c->l_partial.get(), nwg,
         out->flat_grad_sum, (const double*)nullptr, (const double*)nullptr, 0, c->l_sink.get(), (double*)nullptr);
  if (out->grad_w1 || out->grad_b1 || out->grad_ln_w || out->grad_ln_b || out->grad_w2 || out->grad_b2)
    launch(c, "head_scatter_kernel", head_scatter_kernel, dim3(cdiv(RIFT_PI_NPARAM, 256)), dim3(256), 0, (const float*)out->flat_grad_sum,
           out->grad_w1, out->grad_b1, out->grad_ln_w, out->grad_ln_b, out->grad_w2, out->grad_b2, accumulate);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_loss_finalize(RiftCtx* c, const RiftLossOut* out, int accumulate, void* stream) {
  if (!c || !out || !out->stats || !out->flat_grad_sum) return RIFT_ERR_ARG;
  c->stream = (hipStream_t)stream; c->dry = false;
  launch(c, "loss_finalize_kernel", loss_finalize_kernel, dim3(cdiv(RIFT_PI_NPARAM, 256)), dim3(256), 0, (const float*)out->flat_grad_sum,
         (const double*)out->stats, out->grad_w1, out->grad_b1, out->grad_ln_w, out->grad_ln_b, out->grad_w2, out->grad_b2,
         out->loss, accumulate, (const double*)out->exchange, out->stats);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_other_vehicle_rollout(RiftCtx* c, const double* actions, const double* speed, const double* location, const double* yaw_deg,
                               const double* extent, int N, int T, int near_lane_change, double bbox_inflation_ratio, double* vertices,
                               void* stream) {
  if (!c || N < 0 || T <= 0) return RIFT_ERR_ARG;
  if (N == 0) return RIFT_OK;
  if (!actions || !speed || !location || !yaw_deg || !extent || !vertices) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(other_vehicle_rollout_kernel, dim3(cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, actions, speed, location, yaw_deg, extent,
                     N, T, near_lane_change, bbox_inflation_ratio, vertices);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_collision_matrix(RiftCtx* c, const float* center_vertices, int G, int Tc, const double* other_vertices, int N, int Ts,
                          uint8_t* collision, void* stream) {
  if (!c || G <= 0 || Ts <= 0 || Tc < Ts || N < 0 || !center_vertices || !collision || (N > 0 && !other_vertices)) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(collision_matrix_kernel, dim3(cdiv((long long)G * Ts, 256)), dim3(256), 0, (hipStream_t)stream, center_vertices, G, Tc,
                     other_vertices, N, Ts, collision);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_off_road_matrix(RiftCtx* c, const float* rollout_center, int n_points, const uint8_t* off_road_mask, int H, int W,
                         double origin_x, double origin_y, double heading, double res_x, double res_y, double off_x, double off_y,
                         uint8_t* off_road, void* stream) {
  if (!c || n_points <= 0 || H <= 0 || W <= 0 || !rollout_center || !off_road_mask || !off_road || res_x == 0.0 || res_y == 0.0) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(off_road_kernel, dim3(cdiv(n_points, 256)), dim3(256), 0, (hipStream_t)stream, rollout_center, n_points, off_road_mask,
                     H, W, origin_x, origin_y, std::cos(heading), std::sin(heading), res_x, res_y, off_x, off_y, off_road);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_sft_teacher_mode(RiftCtx* c, const float* trajectory, const float* teacher_infos, int bs, int R, int M, int T, int frame_rate,
                          int64_t* mode_rm, void* stream) {
  if (!c || !trajectory || !teacher_infos || !mode_rm || bs <= 0 || R <= 0 || M <= 0 || T <= 0 || frame_rate <= 0) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(sft_teacher_mode_kernel, dim3(bs), dim3(64), 0, (hipStream_t)stream, trajectory, teacher_infos, bs, R * M, M, T, frame_rate,
                     (long long*)mode_rm);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_loss_finalize_clip(RiftCtx* c, const RiftLossOut* out, int accumulate, float max_norm, float* total_norm, void* stream) {
  if (!c || !out || !out->stats || !out->flat_grad_sum || !(max_norm > 0.f)) return RIFT_ERR_ARG;
  if (!out->grad_w1 || !out->grad_b1 || !out->grad_ln_w || !out->grad_ln_b || !out->grad_w2 || !out->grad_b2) return RIFT_ERR_ARG;
  c->stream = (hipStream_t)stream; c->dry = false;
  launch(c, "loss_finalize_clip_kernel", loss_finalize_clip_kernel, dim3(1), dim3(1024), 0, (const float*)out->flat_grad_sum,
         (const double*)out->stats, out->grad_w1, out->grad_b1, out->grad_ln_w, out->grad_ln_b, out->grad_w2, out->grad_b2,
         out->loss, accumulate, (const double*)out->exchange, out->stats, max_norm, total_norm);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_clip_grad_norm(RiftCtx* c, float* const* grads, const int64_t* numels, int n, float max_norm, float* total_norm, void* stream) {
  if (!c || !grads || !numels || n <= 0 || n > 16) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  ClipList L; memset(&L, 0, sizeof(L));
  long long tot = 0;
  for (int i = 0; i < n; ++i) { L.g[i] = grads[i]; L.n[i] = numels[i]; tot += numels[i]; }
  L.count = n;
  const int nb = (int)std::min<long long>(64, (tot + 2047) / 2048);
  DEVCHK(c, c->clip_part.reserve(64));
  launch(c, "clip_norm_partial_kernel", clip_norm_partial_kernel, dim3(nb), dim3(256), 0, L, c->clip_part.get());
  launch(c, "clip_scale_kernel", clip_scale_kernel, dim3(nb), dim3(256), 0, L, (const double*)c->clip_part.get(), nb, max_norm, total_norm);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_adamw_step(RiftCtx* c, int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                    float* const* steps, const int64_t* numels, const double* lr, const double* weight_decay, double step_new,
                    double beta1, double beta2, double eps, void* stream) {
  if (!c || n <= 0 || n > 16 || !params || !grads || !exp_avg || !exp_avg_sq || !steps || !numels || !lr || !weight_decay) return RIFT_ERR_ARG;
  if (!(step_new >= 1.0)) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  AdamList L; memset(&L, 0, sizeof(L));
  const double bc1 = 1.0 - std::pow(beta1, step_new), bc2 = 1.0 - std::pow(beta2, step_new);
  long long tot = 0;
  for (int i = 0; i < n; ++i) {
    if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || !steps[i] || numels[i] <= 0) return RIFT_ERR_ARG;
    L.p[i] = params[i]; L.g[i] = grads[i]; L.m[i] = exp_avg[i]; L.v[i] = exp_avg_sq[i]; L.step[i] = steps[i];
    L.n[i] = numels[i]; L.step_size[i] = (float)(lr[i] / bc1); L.decay[i] = (float)(1.0 - lr[i] * weight_decay[i]); L.step_new[i] = (float)step_new;
    tot += numels[i];
  }
  L.count = n; L.beta1 = (float)beta1; L.beta2 = (float)beta2; L.omb1 = (float)(1.0 - beta1); L.omb2 = (float)(1.0 - beta2);
  L.bc2_sqrt = (float)std::sqrt(bc2); L.eps = (float)eps;
  const int nb = (int)std::min<long long>(256, (tot + 255) / 256);
  launch(c, "adamw_kernel", adamw_kernel, dim3(nb), dim3(256), 0, L);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_update_tail(RiftCtx* c, const RiftLossOut* out, int accumulate, float max_norm, float* total_norm, int n, float* const* params,
                     const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, float* const* steps, const double* lr,
                     const double* weight_decay, double step_new, double beta1, double beta2, double eps, void* stream) {
  if (!c || !out || !out->stats || !out->flat_grad_sum || !(max_norm > 0.f) || n != 6) return RIFT_ERR_ARG;
  if (!params || !grads || !exp_avg || !exp_avg_sq || !steps || !lr || !weight_decay || !(step_new >= 1.0)) return RIFT_ERR_ARG;
  float* const gseg[6] = {out->grad_w1, out->grad_b1, out->grad_ln_w, out->grad_ln_b, out->grad_w2, out->grad_b2};
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  TailAdam A; memset(&A, 0, sizeof(A));
  const double bc1 = 1.0 - std::pow(beta1, step_new), bc2 = 1.0 - std::pow(beta2, step_new);
  for (int sgi = 0; sgi < 6; ++sgi) {
    int j = -1;
    for (int t = 0; t < 6; ++t) if (gseg[sgi] && grads[t] == gseg[sgi]) j = t;
    if (j < 0 || !params[j] || !exp_avg[j] || !exp_avg_sq[j] || !steps[j]) { c->err = "rift_update_tail: the AdamW list does not hold the six pi_head gradient tensors"; return RIFT_ERR_ARG; }
    A.p[sgi] = params[j]; A.m[sgi] = exp_avg[j]; A.v[sgi] = exp_avg_sq[j]; A.step[sgi] = steps[j];
    A.step_size[sgi] = (float)(lr[j] / bc1); A.decay[sgi] = (float)(1.0 - lr[j] * weight_decay[j]);
  }
  A.step_new = (float)step_new; A.beta2 = (float)beta2; A.omb1 = (float)(1.0 - beta1); A.omb2 = (float)(1.0 - beta2);
  A.bc2_sqrt = (float)std::sqrt(bc2); A.eps = (float)eps;
  launch(c, "update_tail_kernel", update_tail_kernel, dim3(1), dim3(1024), 0, (const float*)out->flat_grad_sum, (const double*)out->stats,
         out->grad_w1, out->grad_b1, out->grad_ln_w, out->grad_ln_b, out->grad_w2, out->grad_b2, out->loss, accumulate,
         (const double*)out->exchange, out->stats, max_norm, total_norm, A);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
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
  if (!c || !w || !state || !value || n < 0) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  if (n == 0) return RIFT_OK;
  CriticRowsP p; memset(&p, 0, sizeof(p));
  p.w = critic_w(w); p.state = state; p.n = n; p.value = value;
  launch(c, "critic_rows_kernel", critic_rows_kernel, dim3(cdiv(n, 16)), dim3(256), 0, p);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
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
  launch(c, "critic_outer_sum_kernel", critic_outer_sum_kernel, dim3(cdiv(256 * 128, 256)), dim3(256), 0, (const float*)p.dh1, 256, (const float*)p.sn, 128, n, scale, flat);
  launch(c, "critic_col_sum_kernel", critic_col_sum_kernel, dim3(1), dim3(256), 0, (const float*)p.dh1, 256, n, scale, flat + RIFT_CRITIC_OFF_B0);
  launch(c, "critic_outer_sum_kernel", critic_outer_sum_kernel, dim3(cdiv(256 * 256, 256)), dim3(256), 0, (const float*)p.dh2, 256, (const float*)p.h1, 256, n, scale, flat + RIFT_CRITIC_OFF_W1);
  launch(c, "critic_col_sum_kernel", critic_col_sum_kernel, dim3(1), dim3(256), 0, (const float*)p.dh2, 256, n, scale, flat + RIFT_CRITIC_OFF_B1);
  launch(c, "critic_outer_sum_kernel", critic_outer_sum_kernel, dim3(1), dim3(256), 0, (const float*)p.dout, 1, (const float*)p.h2, 256, n, scale, flat + RIFT_CRITIC_OFF_W2);
  launch(c, "critic_col_sum_kernel", critic_col_sum_kernel, dim3(1), dim3(64), 0, (const float*)p.dout, 1, n, scale, flat + RIFT_CRITIC_OFF_B2);
  launch(c, "critic_col_sum_kernel", critic_col_sum_kernel, dim3(1), dim3(128), 0, (const float*)p.gsa, 128, n, scale, flat + RIFT_CRITIC_OFF_SAVG);
  launch(c, "critic_col_sum_kernel", critic_col_sum_kernel, dim3(1), dim3(128), 0, (const float*)p.gss, 128, n, scale, flat + RIFT_CRITIC_OFF_SSTD);
  launch(c, "critic_col_sum_kernel", critic_col_sum_kernel, dim3(1), dim3(64), 0, (const float*)p.gva, 1, n, scale, flat + RIFT_CRITIC_OFF_VAVG);
  launch(c, "critic_col_sum_kernel", critic_col_sum_kernel, dim3(1), dim3(64), 0, (const float*)p.gvs, 1, n, scale, flat + RIFT_CRITIC_OFF_VSTD);
  return RIFT_OK;
}

int rift_critic_loss_backward(RiftCtx* c, const RiftCritic* w, const float* state, const float* reward_sum, int n, double* stats,
                              float* flat, void* stream) {
  if (!c || !w || !state || !reward_sum || !stats || !flat || n <= 0) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  // flat = -sum_rows d SmoothL1 / d theta
  TRY(critic_backward_sums(c, w, state, reward_sum, nullptr, n, -1.f, flat));
  launch(c, "critic_stats_kernel", critic_stats_kernel, dim3(1), dim3(64), 0, (const double*)c->cr_part.get(), cdiv(n, 16), stats);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_critic_backward(RiftCtx* c, const RiftCritic* w, const float* state, const float* dvalue, int n, float* flat, void* stream) {
  if (!c || !w || !state || !dvalue || !flat || n <= 0) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  TRY(critic_backward_sums(c, w, state, nullptr, dvalue, n, 1.f, flat));
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_critic_finalize(RiftCtx* c, const float* flat, const double* stats, float* g_w0, float* g_b0, float* g_w1, float* g_b1,
                         float* g_w2, float* g_b2, float* g_savg, float* g_sstd, float* g_vavg, float* g_vstd, void* stream) {
  if (!c || !flat || !stats) return RIFT_ERR_ARG;
  c->stream = (hipStream_t)stream; c->dry = false;
  launch(c, "critic_finalize_kernel", critic_finalize_kernel, dim3(cdiv(RIFT_CRITIC_NPARAM, 256)), dim3(256), 0, flat, stats, g_w0, g_b0,
         g_w1, g_b1, g_w2, g_b2, g_savg, g_sstd, g_vavg, g_vstd);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

// An empty buffer is a valid (no-op) input of the three scans below, as it is for the reference's loops.
int rift_gae(RiftCtx* c, const double* rewards, const float* undones, const float* values, const float* next_values,
             const float* unterminated, float gamma, float lambda_, int n, float* advantages, void* stream) {
  if (!c || n < 0) return RIFT_ERR_ARG;
  if (n == 0) return RIFT_OK;
  GaeCoef k{rewards, undones, values, next_values, unterminated, gamma, lambda_};
  hipLaunchKernelGGL((affine_scan_reverse_kernel<GaeCoef, float>), dim3(1), dim3(RIFT_SCAN_THREADS), 0, (hipStream_t)stream, k, n, advantages);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_discounted_return(RiftCtx* c, const double* rewards, const float* dones, double gamma, int n, double* returns,
                           void* stream) {
  if (!c || n < 0) return RIFT_ERR_ARG;
  if (n == 0) return RIFT_OK;
  ReturnCoef k{rewards, dones, gamma};
  hipLaunchKernelGGL((affine_scan_reverse_kernel<ReturnCoef, double>), dim3(1), dim3(RIFT_SCAN_THREADS), 0, (hipStream_t)stream, k, n, returns);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_normalize_advantage(RiftCtx* c, float* x, int n, void* stream) {
  if (!c || n < 0) return RIFT_ERR_ARG;
  if (n == 0) return RIFT_OK;
  hipLaunchKernelGGL(normalize_unbiased_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, n);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_group_advantage(RiftCtx* c, const double* returns, int n_groups, int G, double* advantage, void* stream) {
  if (!c || n_groups <= 0 || G <= 0) return RIFT_ERR_ARG;
  hipLaunchKernelGGL(group_zscore_kernel, dim3(cdiv(n_groups, 4)), dim3(256), 0, (hipStream_t)stream, returns, n_groups, G, advantage);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

// The reward half of RiftEvalParams as the kernels take it (adv.h)
static RewardP reward_of(const RiftEvalParams& e) {
  return RewardP{e.alpha_collision, e.alpha_boundary, e.alpha_comfort, e.alpha_l_align, e.alpha_vel_align, e.alpha_l_center, e.alpha_center_bias,
                 e.alpha_velocity, e.alpha_timestep, e.reward_model == RIFT_REWARD_SPARSE ? 1 : 0};
}

int rift_eval_params_default(RiftCtx* c, RiftEvalParams* out) {
  if (!c || !out) return RIFT_ERR_ARG;
  rift_eval_params_set_default(out);
  return RIFT_OK;
}

template <bool TERMS, class RP>
static void launch_rollout_return(const float* delta_dis, const float* delta_angle, const float* speed, const float* acc, const float* ang_vel,
                                  const float* ang_acc, const uint8_t* collision, int collision_ld, const uint8_t* off_road, int off_road_ld,
                                  int G, int Ts, double gamma, const RP& rp, double* returns, double* terms, void* stream) {
  hipLaunchKernelGGL((rollout_return_kernel<TERMS, RP>), dim3(cdiv(G, 4)), dim3(256), 0, (hipStream_t)stream, delta_dis, delta_angle, speed,
                     acc, ang_vel, ang_acc, collision, collision_ld, off_road, off_road_ld, G, Ts, gamma, rp, returns, Ts, terms);
}

int rift_rollout_return(RiftCtx* c, const float* delta_dis, const float* delta_angle, const float* speed, const float* acc,
                        const float* ang_vel, const float* ang_acc, const uint8_t* collision, int collision_ld,
                        const uint8_t* off_road, int off_road_ld, int G, int Ts, double gamma, double* returns, void* stream) {
  if (!c || G <= 0 || Ts <= 0) return RIFT_ERR_ARG;
  launch_rollout_return<false>(delta_dis, delta_angle, speed, acc, ang_vel, ang_acc, collision, collision_ld, off_road, off_road_ld, G, Ts, gamma,
                               RewardDefaults(), returns, nullptr, stream);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_rollout_return_ex(RiftCtx* c, const float* delta_dis, const float* delta_angle, const float* speed, const float* acc,
                           const float* ang_vel, const float* ang_acc, const uint8_t* collision, int collision_ld,
                           const uint8_t* off_road, int off_road_ld, int G, int Ts, const RiftEvalParams* params, double* returns,
                           double* terms, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  if (const char* why = rift_eval_params_refusal(params)) { c->err = std::string("rift_rollout_return_ex: ") + why; return RIFT_ERR_ARG; }
  if (G <= 0 || Ts <= 0 || !returns) { c->err = "rift_rollout_return_ex: G <= 0, Ts <= 0 or returns == NULL"; return RIFT_ERR_ARG; }
  const RewardP rp = reward_of(*params);
  const double g = params->gamma;
#define RIFT_RR(TERMS, RP) launch_rollout_return<TERMS>(delta_dis, delta_angle, speed, acc, ang_vel, ang_acc, collision, collision_ld, off_road, off_road_ld, G, Ts, g, RP, returns, terms, stream)
  if (reward_is_default(rp)) { if (terms) RIFT_RR(true, RewardDefaults()); else RIFT_RR(false, RewardDefaults()); }      // the default weights: the old entry's instance
  else { if (terms) RIFT_RR(true, rp); else RIFT_RR(false, rp); }
#undef RIFT_RR
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_ref_line_info(RiftCtx* c, const float* traj, int G, int Tfull, int Ts, int M, const float* ref_pos, const float* ref_ang,
                       const int32_t* ref_len, int Pmax, float* delta_dis, float* delta_angle, int32_t* closest_idx, void* stream) {
  if (!c || !traj || !ref_pos || !ref_ang || !ref_len || G <= 0 || Ts <= 0 || M <= 0) return RIFT_ERR_ARG;
  hipLaunchKernelGGL(ref_line_info_kernel, dim3(cdiv((long long)G * Ts, 128)), dim3(128), 0, (hipStream_t)stream, traj, G, Tfull, Ts, M,
                     ref_pos, ref_ang, (const int*)ref_len, Pmax, delta_dis, delta_angle, (int*)closest_idx);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_rollout(RiftCtx* c, const RiftRolloutIO* io, void* stream) {
  if (!c || !io || !io->trajectories || !io->center_state || io->G <= 0 || io->Tfull < 40 || io->G_per_group <= 0) return RIFT_ERR_ARG;
  RolloutP p; memset(&p, 0, sizeof(p));
  p.traj = io->trajectories; p.G = io->G; p.Tfull = io->Tfull; p.Gper = io->G_per_group; p.state = io->center_state;
  p.turn_buf = io->turn_buf; p.turn_ptr = (int*)io->turn_ptr; p.turn_len = (int*)io->turn_len;
  p.speed_buf = io->speed_buf; p.speed_ptr = (int*)io->speed_ptr; p.speed_len = (int*)io->speed_len;
  p.center = io->center; p.angle = io->angle; p.speed = io->speed; p.acc = io->acc; p.ang_vel = io->ang_vel; p.ang_acc = io->ang_acc;
  p.vertices = io->vertices; p.closest_index = (int*)io->closest_index; p.aim_idx = (int*)io->aim_idx;
  const size_t ro_need = (size_t)io->G * RIFT_RO_LEN;          // the raw speed history between the two kernels (grown behind a device-wide wait)
  if (ro_need > c->ro_raw.cap() && c->ro_raw.get()) HIPCHK(c, hipDeviceSynchronize());
  DEVCHK(c, c->ro_raw.reserve(ro_need, std::max((size_t)io->G * 2, (size_t)256) * RIFT_RO_LEN));
  p.raw_speed = c->ro_raw.get();
  if (!p.center || !p.angle || !p.speed || !p.acc || !p.ang_vel || !p.ang_acc || !p.vertices || !p.closest_index || !p.aim_idx) return RIFT_ERR_ARG;
  if (c->ro8) hipLaunchKernelGGL(rollout8_kernel, dim3(cdiv(io->G, 8)), dim3(64), (size_t)RIFT_RO_LDS_BYTES, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(rollout_kernel, dim3(cdiv(io->G, 64)), dim3(64), (size_t)RIFT_RO_LDS_BYTES, (hipStream_t)stream, p);
  hipLaunchKernelGGL(rollout_kinematics_kernel, dim3(cdiv(io->G * RIFT_RO_LEN, 256)), dim3(256), 0, (hipStream_t)stream, p);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

// ---- the drivable-area map (include/rift_drivable.h; drivable_grid.h, drivable_map.h) ------------------------------
// the images are released only after the stream that last read them has been waited for
static int drivable_map_release(RiftCtx* c) {
  if (c->dmap.used) { HIPCHK(c, hipSetDevice(c->device)); HIPCHK(c, hipStreamSynchronize(c->dmap.used_on)); }
  c->dmap.img.reset(); c->dmap.grid = DrivableGrid(); c->dmap.loaded = false; c->dmap.used = false; c->dmap.used_on = nullptr;
  return RIFT_OK;
}

int riftdm_load(RiftCtx* c, const double* vertices, const int32_t* poly_start, int n_polys, double cell, double margin, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  DrivableGrid g;
  if (const char* why = drivable_grid_build(vertices, poly_start, n_polys, cell, margin, &g)) { c->err = std::string("riftdm_load: ") + why; return RIFT_ERR_ARG; }
  TRY(drivable_map_release(c));
  HIPCHK(c, hipSetDevice(c->device));
  DrivableImages& im = c->dmap.img;
  DEVCHK(c, im.reserve(g));
  const hipStream_t st = (hipStream_t)stream;
  auto up = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
  hipError_t e = up(im.vertices.get(), vertices, (size_t)g.n_vertices * 2 * sizeof(double));
  if (e == hipSuccess) e = up(im.aabb.get(), g.aabb.data(), g.aabb.size() * sizeof(double));
  if (e == hipSuccess) e = up(im.poly_start.get(), poly_start, n_polys ? ((size_t)n_polys + 1) * sizeof(int32_t) : 0);
  if (e == hipSuccess) e = up(im.cell_start.get(), g.cell_start.data(), g.cell_start.size() * sizeof(int32_t));
  if (e == hipSuccess) e = up(im.cell_poly.get(), g.cell_poly.data(), g.cell_poly.size() * sizeof(int32_t));
  if (e == hipSuccess) e = hipStreamSynchronize(st);         // the host arrays are the caller's and this function's: done with them on return (once per town)
  if (e != hipSuccess) { im.reset(); c->err = std::string("riftdm_load: ") + hipGetErrorString(e); return RIFT_ERR_HIP; }
  g.aabb = {}; g.cell_start = {}; g.cell_poly = {};          // (the numbers stay: riftdm_info)
  c->dmap.grid = std::move(g); c->dmap.loaded = true;
  return RIFT_OK;
}

int riftdm_clear(RiftCtx* c) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  return drivable_map_release(c);
}

int riftdm_info(RiftCtx* c, RiftDrivableInfo* out) {
  if (!c || !out) return RIFT_ERR_ARG;
  c->err.clear();
  if (!c->dmap.loaded) { c->err = "riftdm_info: no drivable-area map is loaded (riftdm_load)"; return RIFT_ERR_STATE; }
  const DrivableGrid& g = c->dmap.grid;
  memset(out, 0, sizeof(*out));
  out->n_polys = g.n_polys; out->n_vertices = g.n_vertices; out->nx = g.nx; out->ny = g.ny; out->max_cell_list = g.max_list;
  out->cell = g.cell; out->margin = g.margin; out->x0 = g.x0; out->y0 = g.y0; out->device_bytes = (int64_t)c->dmap.img.bytes();
  return RIFT_OK;
}

// Every refusal of a call that reads the map, on the host and ahead of any launch; then the images as a kernel takes them, and the stream noted
static int drivable_map_use(RiftCtx* c, const char* who, double resolution, void* stream, DrivableMapDev* m) {
  if (!c->dmap.loaded) { c->err = std::string(who) + ": no drivable-area map is loaded (riftdm_load)"; return RIFT_ERR_STATE; }
  const DrivableGrid& g = c->dmap.grid;
  if (const char* why = drivable_res_refusal(g.margin, (double)(float)resolution)) { c->err = std::string(who) + ": " + why; return RIFT_ERR_ARG; }
  const DrivableImages& im = c->dmap.img;
  m->vertices = im.vertices.get(); m->aabb = im.aabb.get(); m->poly_start = im.poly_start.get(); m->cell_start = im.cell_start.get(); m->cell_poly = im.cell_poly.get();
  m->x0 = g.x0; m->y0 = g.y0; m->cell = g.cell; m->margin = g.margin; m->nx = g.nx; m->ny = g.ny;
  c->dmap.used = true; c->dmap.used_on = (hipStream_t)stream;
  return RIFT_OK;
}

static int drivable_call(RiftCtx* c, const char* who, int H, int W, double ox, double oy, double heading, const RiftEvalParams* params, void* stream,
                         DrivableMapDev* m, RasterPose* q) {
  c->err.clear();
  if (const char* why = rift_eval_params_refusal(params)) { c->err = std::string(who) + ": " + why; return RIFT_ERR_ARG; }
  if (H <= 0 || W <= 0 || (long long)H * W > (1LL << 30)) { c->err = std::string(who) + ": H or W <= 0 (or H * W above 2^30)"; return RIFT_ERR_ARG; }
  if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(heading)) { c->err = std::string(who) + ": a pose that is not finite"; return RIFT_ERR_ARG; }
  TRY(drivable_map_use(c, who, params->resolution, stream, m));
  *q = RasterPose{ox, oy, std::cos(heading), std::sin(heading), (double)(float)params->resolution, (double)(float)(H / 2.0), (double)(float)(W / 2.0),
                  drivable_inv_res((double)(float)params->resolution)};
  return RIFT_OK;
}

int riftdm_off_road_matrix(RiftCtx* c, const float* rollout_center, int n_points, int H, int W, double ox, double oy, double heading,
                             const RiftEvalParams* params, uint8_t* off_road, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  if (n_points <= 0 || !rollout_center || !off_road) { c->err = "riftdm_off_road_matrix: n_points <= 0 or a null pointer"; return RIFT_ERR_ARG; }
  DrivableMapDev m; RasterPose q;
  TRY(drivable_call(c, "riftdm_off_road_matrix", H, W, ox, oy, heading, params, stream, &m, &q));
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(off_road_map_kernel, dim3(cdiv(n_points, 256)), dim3(256), 0, (hipStream_t)stream, rollout_center, n_points, m, q, H, W, off_road);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int riftdm_raster(RiftCtx* c, int H, int W, double ox, double oy, double heading, const RiftEvalParams* params, uint8_t* mask, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  if (!mask) { c->err = "riftdm_raster: mask == NULL"; return RIFT_ERR_ARG; }
  DrivableMapDev m; RasterPose q;
  TRY(drivable_call(c, "riftdm_raster", H, W, ox, oy, heading, params, stream, &m, &q));
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(drivable_raster_kernel, dim3(cdiv((long long)H * W, 256)), dim3(256), 0, (hipStream_t)stream, m, q, H, W, mask);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

// One rollout tick's group advantages (rift_hip.h).  Everything but the candidate rollouts is independent between the CBVs: one launch per
// stage serves a chunk of up to RIFT_TICK_CHUNK of them (tick_multi.h) -- reference-line deviations and neighbour forecasts first, then the
// rollouts CBV by CBV in list order (the shared PID state), then kinematics, flags, returns and z-scores: K + 7 launches instead of 9 K.
// (own_offset: the pixel offset of a CBV comes from its own raster -- the _ex entry; else 200, 200 whatever the raster)
static int group_advantage_tick(RiftCtx* c, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                const RiftEvalParams& ev, bool own_offset, double* advantage, double* returns, double* terms, void* stream,
                                bool use_map = false) {
  if (!c || !trajectory || !cbvs || K <= 0 || Rb <= 0 || Tfull < 80 || !advantage || !turn_buf || !turn_ptr || !turn_len || !speed_buf || !speed_ptr || !speed_len) return RIFT_ERR_ARG;
  c->err.clear();
  constexpr int M = 12, Ts = 40, TR = RIFT_RO_LEN;
  int Gmax = 0, Nmax = 0;
  bool any_map = false;
  for (int k = 0; k < K; ++k) {
    const RiftTickCBV& v = cbvs[k];
    if (v.R <= 0 || v.R > Rb || v.batch_index < 0 || v.Pmax <= 0 || v.n_actors < 0 || !v.center_state || !v.ref_pos || !v.ref_angle || !v.ref_len ||
        (v.n_actors > 0 && !v.actors) || (v.off_road_mask && (v.H <= 0 || v.W <= 0))) { c->err = "rift_group_advantage_tick: bad entry"; return RIFT_ERR_ARG; }
    if (use_map && !v.off_road_mask) {             // (the map entry: NULL mask and H, W > 0 -- from the map; H == W == 0 -- no flags)
      if (v.H < 0 || v.W < 0 || (v.H == 0) != (v.W == 0)) { c->err = "riftdm_group_advantage_tick: H or W <= 0 where the map is asked for"; return RIFT_ERR_ARG; }
      any_map = any_map || v.H > 0;
    }
    Gmax = std::max(Gmax, v.R * M); Nmax = std::max(Nmax, v.n_actors);
  }
  DrivableMapDev dmap; memset(&dmap, 0, sizeof(dmap));
  if (any_map) TRY(drivable_map_use(c, "riftdm_group_advantage_tick", ev.resolution, stream, &dmap));
  HIPCHK(c, hipSetDevice(c->device));
  // per-CBV scratch (bytes, 256-aligned pieces), one set per CBV of a chunk
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  const size_t G = (size_t)Gmax;
  const size_t o_dd = take(G * Ts * 4), o_da = take(G * Ts * 4), o_ci = take(G * Ts * 4);
  const size_t o_center = take(G * TR * 2 * 4), o_angle = take(G * TR * 4), o_speed = take(G * TR * 4), o_acc = take(G * TR * 4), o_av = take(G * TR * 4),
               o_aa = take(G * TR * 4), o_vert = take(G * TR * 8 * 4), o_cl = take(G * 79 * 4), o_aim = take(G * 79 * 4), o_raw = take(G * TR * 4);
  const size_t o_ov = take((size_t)std::max(Nmax, 1) * Ts * 8 * 8), o_col = take(G * Ts), o_offr = take(G * TR), o_ret = take(G * 8);
  const size_t per = off, need = per * (size_t)std::min(K, RIFT_TICK_CHUNK);
  if (need > c->tick_scratch.cap() && c->tick_scratch.get()) HIPCHK(c, hipDeviceSynchronize());
  DEVCHK(c, c->tick_scratch.reserve(need, need * 2));
  const hipStream_t st = (hipStream_t)stream;
  for (int k0 = 0; k0 < K; k0 += RIFT_TICK_CHUNK) {
    TickArr a; memset(&a, 0, sizeof(a));
    a.K = std::min(RIFT_TICK_CHUNK, K - k0); a.gamma = ev.gamma; a.near_lane_change = ev.near_lane_change ? 1 : 0; a.inflation = ev.bbox_inflation_ratio;
    a.res = (double)(float)ev.resolution;                       // resolution_hw is a float32 array in the reference (traj_evaluator.py:102)
    a.reward = reward_of(ev); a.reward_default = reward_is_default(a.reward) ? 1 : 0;
    int gmax = 0, nmax = 0;
    bool chunk_map = false;
    a.map = dmap; a.map_inv_res = drivable_inv_res(a.res);
    for (int j = 0; j < a.K; ++j) {
      const RiftTickCBV& v = cbvs[k0 + j];
      chunk_map = chunk_map || (any_map && !v.off_road_mask && v.H > 0);
      char* S = c->tick_scratch.get() + per * (size_t)j;
      TickK& d = a.d[j];
      d.traj = trajectory + (size_t)v.batch_index * Rb * M * Tfull * 6; d.G = v.R * M; d.Tfull = Tfull; d.Pmax = v.Pmax; d.N = v.n_actors; d.H = v.H; d.W = v.W;
      d.ref_pos = v.ref_pos; d.ref_ang = v.ref_angle; d.ref_len = (const int*)v.ref_len;
      d.dd = (float*)(S + o_dd); d.da = (float*)(S + o_da); d.ci = (int*)(S + o_ci);
      d.actors = v.actors; d.ov = (double*)(S + o_ov);
      RolloutP& p = d.ro;
      p.traj = d.traj; p.G = d.G; p.Tfull = Tfull; p.Gper = d.G; p.state = v.center_state;
      p.turn_buf = turn_buf; p.turn_ptr = (int*)turn_ptr; p.turn_len = (int*)turn_len; p.speed_buf = speed_buf; p.speed_ptr = (int*)speed_ptr; p.speed_len = (int*)speed_len;
      p.center = (float*)(S + o_center); p.angle = (float*)(S + o_angle); p.speed = (float*)(S + o_speed); p.acc = (float*)(S + o_acc);
      p.ang_vel = (float*)(S + o_av); p.ang_acc = (float*)(S + o_aa); p.vertices = (float*)(S + o_vert);
      p.closest_index = (int*)(S + o_cl); p.aim_idx = (int*)(S + o_aim); p.raw_speed = (float*)(S + o_raw);
      d.mask = v.off_road_mask; d.ox = v.pose[0]; d.oy = v.pose[1]; d.ch = std::cos(v.pose[2]); d.sh = std::sin(v.pose[2]);
      d.off_x = own_offset ? (double)(float)(v.H / 2.0) : 200.0; d.off_y = own_offset ? (double)(float)(v.W / 2.0) : 200.0;   // x gets H / 2: the reference's quirk (rift_hip.h)
      d.col = (uint8_t*)(S + o_col); d.offr = (uint8_t*)(S + o_offr);
      d.ret = returns ? returns + (size_t)(k0 + j) * Rb * M : (double*)(S + o_ret);       // straight to the caller's tensor when asked for
      d.terms = terms ? terms + (size_t)(k0 + j) * Rb * M * 8 : nullptr;
      d.adv = advantage + (size_t)(k0 + j) * Rb * M;
      gmax = std::max(gmax, d.G); nmax = std::max(nmax, d.N);
    }
    const dim3 gy((unsigned)1, (unsigned)a.K);
    hipLaunchKernelGGL(tick_multi_kernel<0>, dim3(cdiv(gmax * Ts, 128), a.K), dim3(128), 0, st, a);
    if (nmax > 0) hipLaunchKernelGGL(tick_multi_kernel<1>, dim3(cdiv(nmax, 64), a.K), dim3(64), 0, st, a);
    for (int j = 0; j < a.K; ++j) {
      if (c->ro8) hipLaunchKernelGGL(rollout8_kernel, dim3(cdiv(a.d[j].G, 8)), dim3(64), (size_t)RIFT_RO_LDS_BYTES, st, a.d[j].ro);
      else hipLaunchKernelGGL(rollout_kernel, dim3(cdiv(a.d[j].G, 64)), dim3(64), (size_t)RIFT_RO_LDS_BYTES, st, a.d[j].ro);
    }
    hipLaunchKernelGGL(tick_multi_kernel<2>, dim3(cdiv(gmax * TR, 256), a.K), dim3(256), 0, st, a);
    hipLaunchKernelGGL(tick_multi_kernel<3>, dim3(cdiv(gmax * Ts, 256), a.K), dim3(256), 0, st, a);
    if (chunk_map) hipLaunchKernelGGL(tick_multi_kernel<7>, dim3(cdiv(gmax * TR, 256), a.K), dim3(256), 0, st, a);      // (in place of stage 4: masks, the map and "no flags" in one launch)
    else hipLaunchKernelGGL(tick_multi_kernel<4>, dim3(cdiv(gmax * TR, 256), a.K), dim3(256), 0, st, a);
    hipLaunchKernelGGL(tick_multi_kernel<5>, dim3(cdiv(gmax, 4), a.K), dim3(256), 0, st, a);
    hipLaunchKernelGGL(tick_multi_kernel<6>, dim3(1, a.K), dim3(256), 0, st, a);
    (void)gy;
    HIPCHK(c, hipGetLastError());
  }
  return RIFT_OK;
}

int rift_group_advantage_tick(RiftCtx* c, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                              float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                              double gamma, double* advantage, void* stream) {
  RiftEvalParams ev;
  rift_eval_params_set_default(&ev);
  ev.gamma = gamma;
  return group_advantage_tick(c, trajectory, Rb, Tfull, cbvs, K, turn_buf, turn_ptr, turn_len, speed_buf, speed_ptr, speed_len, ev, false,
                              advantage, nullptr, nullptr, stream);
}

int rift_group_advantage_tick_ex(RiftCtx* c, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                 float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                 const RiftEvalParams* params, double* advantage, double* returns, double* terms, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  if (const char* why = rift_eval_params_refusal(params)) { c->err = std::string("rift_group_advantage_tick_ex: ") + why; return RIFT_ERR_ARG; }
  return group_advantage_tick(c, trajectory, Rb, Tfull, cbvs, K, turn_buf, turn_ptr, turn_len, speed_buf, speed_ptr, speed_len, *params, true,
                              advantage, returns, terms, stream);
}

int riftdm_group_advantage_tick(RiftCtx* c, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                  float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                  const RiftEvalParams* params, double* advantage, double* returns, double* terms, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  if (const char* why = rift_eval_params_refusal(params)) { c->err = std::string("riftdm_group_advantage_tick: ") + why; return RIFT_ERR_ARG; }
  return group_advantage_tick(c, trajectory, Rb, Tfull, cbvs, K, turn_buf, turn_ptr, turn_len, speed_buf, speed_ptr, speed_len, *params, true,
                              advantage, returns, terms, stream, true);
}

// ---- the advantage of the update from stored returns (include/rift_advantage.h; adv_params.h) ----------------------
int riftga_params_default(RiftAdvantageParams* out) {
  if (!out) return RIFT_ERR_ARG;
  riftga_params_set_default(out);
  return RIFT_OK;
}

int riftga_arena_advantage(RiftCtx* c, const double* returns, const int32_t* r_count, const uint8_t* valid_mask, int n, int Rcap,
                           const RiftAdvantageParams* params, double* advantage, double* stats, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  c->err.clear();
  if (const char* why = riftga_refusal(returns, n, Rcap, params, advantage)) { c->err = std::string("riftga_arena_advantage: ") + why; return RIFT_ERR_ARG; }
  if (n == 0) return RIFT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  const bool batch = params->scale == RIFTGA_SCALE_BATCH_RMS;
  ArenaAdvP p; memset(&p, 0, sizeof(p));
  p.ret = returns; p.r_count = r_count; p.mask = valid_mask; p.n = n; p.Rcap = Rcap;
  p.baseline = params->baseline; p.scale = params->scale; p.eps = params->eps; p.clip = params->clip;
  p.adv = advantage; p.stats = stats;
  if (batch || stats) {                                        // the partials travel from launch to launch in the context's scratch
    const size_t need = riftga_scratch_doubles(n);
    if (need > c->ga_scratch.cap() && c->ga_scratch.get()) HIPCHK(c, hipDeviceSynchronize());      // (grown behind a device-wide wait, as ro_raw)
    DEVCHK(c, c->ga_scratch.reserve(need, need * 2));
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
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

// One rollout tick's decisions (rift_hip.h): every refusal is decided here, on the host, before anything is launched; then one wave per CBV
// (control.h), RIFT_CTL_CHUNK descriptors per launch.  The logits of a row are held MAXPL per lane: dispatched as loss_kernel<MAXPL> is.
// The checks and the descriptor fill are shared by rift_control_tick and riftcs_control_tick (include/rift_select.h): `who` is the entry's
// name in the message; with `sel` in SAMPLE mode the launches are the <MAXPL, true> instantiations and u[k] rides in CBV k's descriptor.
template <bool SAMPLE>
static void control_tick_launch(const CtlArr& a, hipStream_t st) {
  if (a.G <= 64 * 2) hipLaunchKernelGGL((control_tick_kernel<2, SAMPLE>), dim3(a.K), dim3(64), 0, st, a);
  else if (a.G <= 64 * 4) hipLaunchKernelGGL((control_tick_kernel<4, SAMPLE>), dim3(a.K), dim3(64), 0, st, a);
  else hipLaunchKernelGGL((control_tick_kernel<16, SAMPLE>), dim3(a.K), dim3(64), 0, st, a);
}

static int control_tick(RiftCtx* c, const char* who, const float* trajectory, const float* probability, const float* ref_free_trajectory, int Rb,
                        int Tfull, const RiftControlCBV* cbvs, int K, int topk, int sample_interval, double* pid_state, int n_slots,
                        const RiftSelectParams* sel, const double* u, double* decision, void* stream) {
  auto refuse = [&](const char* why) { c->err = std::string(who) + ": " + why; return (int)RIFT_ERR_ARG; };
  if (K < 0) return refuse("K < 0");
  if (Rb < 1) return refuse("Rb < 1");
  const long long G = (long long)Rb * 12;
  if (topk < 1 || topk > G) return refuse("topk outside [1, Rb * 12]");
  if (sample_interval < 1) return refuse("sample_interval < 1");
  if (Tfull < 2 * (long long)sample_interval) return refuse("Tfull < 2 * sample_interval (the thinned path needs two points)");
  if (G > 64 * 16) return refuse("Rb * 12 above 1024 candidates (16 logits per lane)");
  if (n_slots < 0) return refuse("n_slots < 0");
  if (K > 0 && (!trajectory || !probability || !cbvs || !pid_state || !decision)) return refuse("null pointer");
  std::vector<int> slots((size_t)K);
  for (int k = 0; k < K; ++k) {
    if (cbvs[k].batch_index < 0) return refuse("batch_index < 0");
    if (cbvs[k].slot < 0 || cbvs[k].slot >= n_slots) return refuse("slot outside [0, n_slots)");
    slots[(size_t)k] = cbvs[k].slot;
  }
  std::sort(slots.begin(), slots.end());
  if (std::adjacent_find(slots.begin(), slots.end()) != slots.end()) return refuse("two CBVs with the same slot");
  c->err.clear();
  if (K == 0) return RIFT_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t st = (hipStream_t)stream;
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
    if (sample) control_tick_launch<true>(a, st);
    else control_tick_launch<false>(a, st);
    HIPCHK(c, hipGetLastError());
  }
  return RIFT_OK;
}

int rift_control_tick(RiftCtx* c, const float* trajectory, const float* probability, const float* ref_free_trajectory, int Rb, int Tfull,
                      const RiftControlCBV* cbvs, int K, int topk, int sample_interval, double* pid_state, int n_slots, double* decision,
                      void* stream) {
  if (!c) return RIFT_ERR_ARG;
  return control_tick(c, "rift_control_tick", trajectory, probability, ref_free_trajectory, Rb, Tfull, cbvs, K, topk, sample_interval, pid_state,
                      n_slots, nullptr, nullptr, decision, stream);
}

// ---- the choice of the executed candidate at run time (include/rift_select.h; select_params.h, control.h) ----------------------
int riftcs_params_default(RiftSelectParams* out) {
  if (!out) return RIFT_ERR_ARG;
  riftcs_params_set_default(out);
  return RIFT_OK;
}

int riftcs_control_tick(RiftCtx* c, const float* trajectory, const float* probability, const float* ref_free_trajectory, int Rb, int Tfull,
                        const RiftControlCBV* cbvs, int K, int topk, int sample_interval, double* pid_state, int n_slots,
                        const RiftSelectParams* params, const double* u, double* decision, void* stream) {
  if (!c) return RIFT_ERR_ARG;
  if (const char* why = riftcs_refusal(params, u, K)) { c->err = std::string("riftcs_control_tick: ") + why; return RIFT_ERR_ARG; }
  return control_tick(c, "riftcs_control_tick", trajectory, probability, ref_free_trajectory, Rb, Tfull, cbvs, K, topk, sample_interval,
                      pid_state, n_slots, params, u, decision, stream);
}

int rift_collate(RiftCtx* c, const RiftReplayArena* ar, const int32_t* scene_idx, int bs, int R_out,
                 const RiftFeatureBatch* ob, float* out_old_logits, float* out_ref_logits, double* out_advantage,
                 uint8_t* out_valid_mask, void* stream) {
  if (!c || !ar || !scene_idx || !ob || bs <= 0 || R_out <= 0 || R_out > ar->Rcap) return RIFT_ERR_ARG;
  // the arena's rows are stored padded to its capacities (ar->A, Mp, Rcap, S); the batch is padded to the dimensions of `ob`, which
  // may be smaller (a host arena that grows by doubling keeps capacities above the largest stored scene): every ragged dimension
  // leads its per-scene block, so the crop is a prefix copy
  if (ob->A > ar->A || ob->Mp > ar->Mp || ob->S > ar->S || ob->A <= 0 || ob->T != ar->T) return RIFT_ERR_ARG;
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
  hipLaunchKernelGGL(collate_kernel, dim3(bs, k), dim3(256), 0, (hipStream_t)stream, p, scene_idx);
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

}}  // namespace rift::abi

// an entry whose signature drifts from the header does not compile
#define RIFT_SHARED_FN(name) static_assert(std::is_same<decltype(&::name), decltype(&rift::abi::name)>::value, #name);
#include "abi_list.h"
#undef RIFT_SHARED_FN

// The drivable-area-map extension (include/rift_drivable.h): operand-format free, so its six exported symbols are defined here, once per
// library, and forward to the entries above without a table; an entry whose signature drifts from its header does not compile.
#define RIFT_DM_FN(name) static_assert(std::is_same<decltype(&::name), decltype(&rift::abi::name)>::value, #name);
RIFT_DM_FN(riftdm_load) RIFT_DM_FN(riftdm_clear) RIFT_DM_FN(riftdm_info) RIFT_DM_FN(riftdm_off_road_matrix) RIFT_DM_FN(riftdm_raster)
RIFT_DM_FN(riftdm_group_advantage_tick)
#undef RIFT_DM_FN
extern "C" {
int riftdm_load(RiftCtx* ctx, const double* vertices, const int32_t* poly_start, int n_polys, double cell, double margin, void* stream) {
  return rift::abi::riftdm_load(ctx, vertices, poly_start, n_polys, cell, margin, stream);
}
int riftdm_clear(RiftCtx* ctx) { return rift::abi::riftdm_clear(ctx); }
int riftdm_info(RiftCtx* ctx, RiftDrivableInfo* out) { return rift::abi::riftdm_info(ctx, out); }
int riftdm_off_road_matrix(RiftCtx* ctx, const float* rollout_center, int n_points, int H, int W, double ox, double oy, double heading,
                           const RiftEvalParams* params, uint8_t* off_road, void* stream) {
  return rift::abi::riftdm_off_road_matrix(ctx, rollout_center, n_points, H, W, ox, oy, heading, params, off_road, stream);
}
int riftdm_raster(RiftCtx* ctx, int H, int W, double ox, double oy, double heading, const RiftEvalParams* params, uint8_t* mask, void* stream) {
  return rift::abi::riftdm_raster(ctx, H, W, ox, oy, heading, params, mask, stream);
}
int riftdm_group_advantage_tick(RiftCtx* ctx, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                const RiftEvalParams* params, double* advantage, double* returns, double* terms, void* stream) {
  return rift::abi::riftdm_group_advantage_tick(ctx, trajectory, Rb, Tfull, cbvs, K, turn_buf, turn_ptr, turn_len, speed_buf, speed_ptr, speed_len,
                                                params, advantage, returns, terms, stream);
}
}  // extern "C"

// The arena-advantage extension (include/rift_advantage.h), layered the same way: two exported symbols, defined once per library.
#define RIFT_GA_FN(name) static_assert(std::is_same<decltype(&::name), decltype(&rift::abi::name)>::value, #name);
RIFT_GA_FN(riftga_params_default) RIFT_GA_FN(riftga_arena_advantage)
#undef RIFT_GA_FN
extern "C" {
int riftga_params_default(RiftAdvantageParams* out) { return rift::abi::riftga_params_default(out); }
int riftga_arena_advantage(RiftCtx* ctx, const double* returns, const int32_t* r_count, const uint8_t* valid_mask, int n, int Rcap,
                           const RiftAdvantageParams* params, double* advantage, double* stats, void* stream) {
  return rift::abi::riftga_arena_advantage(ctx, returns, r_count, valid_mask, n, Rcap, params, advantage, stats, stream);
}
}  // extern "C"

// The candidate-selection extension (include/rift_select.h), layered the same way: two exported symbols, defined once per library.
#define RIFT_CS_FN(name) static_assert(std::is_same<decltype(&::name), decltype(&rift::abi::name)>::value, #name);
RIFT_CS_FN(riftcs_params_default) RIFT_CS_FN(riftcs_control_tick)
#undef RIFT_CS_FN
extern "C" {
int riftcs_params_default(RiftSelectParams* out) { return rift::abi::riftcs_params_default(out); }
int riftcs_control_tick(RiftCtx* ctx, const float* trajectory, const float* probability, const float* ref_free_trajectory, int Rb, int Tfull,
                        const RiftControlCBV* cbvs, int K, int topk, int sample_interval, double* pid_state, int n_slots,
                        const RiftSelectParams* params, const double* u, double* decision, void* stream) {
  return rift::abi::riftcs_control_tick(ctx, trajectory, probability, ref_free_trajectory, Rb, Tfull, cbvs, K, topk, sample_interval, pid_state,
                                        n_slots, params, u, decision, stream);
}
}  // extern "C"
