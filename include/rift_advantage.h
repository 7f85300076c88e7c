/*
 * librift_hip.so -- the group advantage of the policy update, formed from stored returns: an extension of the C-ABI of include/rift_hip.h
 * with a header and a symbol prefix of its own (`riftga_`), layered as include/rift_drivable.h is.  The two entries depend on no MFMA
 * operand format, need no trampoline and are defined once per library (csrc/shared.hip; kernels in csrc/adv_params.h).  Conventions, error
 * codes and RiftCtx are rift_hip.h's.
 */
#ifndef RIFT_ADVANTAGE_H
#define RIFT_ADVANTAGE_H

#include "rift_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RIFTGA_BASELINE_MEAN = 0, RIFTGA_BASELINE_LEAVE_ONE_OUT = 1, RIFTGA_BASELINE_NONE = 2 };
enum { RIFTGA_SCALE_GROUP_STD = 0, RIFTGA_SCALE_BATCH_RMS = 1, RIFTGA_SCALE_NONE = 2 };
typedef struct RiftAdvantageParams {
  int32_t baseline, scale;
  double  eps;    /* added to the scale's denominator; 1e-5 */
  double  clip;   /* advantage clamped to [-clip, clip]; 0 = off */
} RiftAdvantageParams;   /* 24 bytes */

/* MEAN, GROUP_STD, 1e-5, 0: the reference's z-score (rift_group_advantage).  No context, no device. */
int riftga_params_default(RiftAdvantageParams* out);

/* The advantage of every candidate of a replay arena, once per policy update and on the device: rift_group_advantage_tick freezes
 * (ret - mean) / (std + 1e-5) at rollout time; this entry forms the advantage from the returns kept with the transition, under `params`.
 * THE RULE.  The group of scene i is its candidates (r, m) with r < r_count[i] and a non-zero byte in valid_mask.  G is their number, x_j
 * their returns, mean the mean of the x_j.
 *   centred value   MEAN: c_j = x_j - mean.   LEAVE_ONE_OUT: c_j = (x_j - mean) * G / (G - 1), which is x_j minus the mean of the others in
 *                   the form that does not cancel; 0 for G < 2.   NONE: c_j = x_j.
 *   scale           GROUP_STD: c_j / (sd + eps), sd the ddof-0 standard deviation of the group's RETURNS, whatever the baseline.
 *                   BATCH_RMS: c_j / (rms + eps), rms = sqrt(sum of c_j^2 over every valid candidate of the arena / their number N); with
 *                   the MEAN baseline this is the pooled within-group standard deviation.   NONE: c_j.
 *   clip            the result is clamped to [-clip, clip] when clip > 0.
 * Every element of `advantage` that belongs to no group (padded lines, masked candidates, a scene with G == 0) is written as 0.
 * stats (8 doubles on the DEVICE, or NULL): [0] N; [1] scenes with G > 0; [2] scenes with G > 0 whose sd is exactly 0; [3] rms (0 unless
 * BATCH_RMS); [4] candidates clamped; [5]-[7] 0.
 * With the default parameters a scene whose valid lines are a fully valid prefix receives the bits rift_group_advantage gives its
 * (1, r_count * 12) returns.  The same inputs give the same bits on every run and every rank: no floating-point atomic is used; the arena-wide
 * sums go through per-scene partials in the context's scratch and one workgroup that adds them in a fixed order.
 * Launches: one in the group modes (GROUP_STD, NONE); three with BATCH_RMS (per scene, the arena-wide sum, scale and clamp).  `stats` adds one
 * launch (with BATCH_RMS and clip > 0: two).
 * returns, advantage: DEVICE (n, Rcap, 12) f64; r_count: DEVICE (n) i32 or NULL (every scene has Rcap lines); valid_mask: DEVICE (n, Rcap, 12)
 * u8 or NULL (all valid).  RIFT_ERR_ARG with a message (rift_last_error), decided on the host before any launch: params == NULL, an
 * enumerator out of range, eps or clip not finite or < 0, n < 0, Rcap < 1, returns or advantage NULL with n > 0, advantage == returns.
 * n == 0 is RIFT_OK without a launch. */
int riftga_arena_advantage(RiftCtx* ctx, const double* returns, const int32_t* r_count, const uint8_t* valid_mask, int n, int Rcap,
                           const RiftAdvantageParams* params, double* advantage, double* stats, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RIFT_ADVANTAGE_H */
