/*
 * librift_hip.so -- which candidate a CBV executes at the rollout tick, chosen at run time: an extension of the C-ABI of
 * include/rift_hip.h with a header and a symbol prefix of its own (`riftcs_`), layered as include/rift_advantage.h and
 * include/rift_drivable.h are.  The two entries depend on no MFMA operand format, need no trampoline and are defined once per library
 * (csrc/shared.hip; the stage itself in csrc/control.h, defaults and refusals in csrc/select_params.h).  Conventions, error codes and
 * RiftCtx are rift_hip.h's.
 */
#ifndef RIFT_SELECT_H
#define RIFT_SELECT_H

#include "rift_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RIFTCS_GREEDY = 0, RIFTCS_SAMPLE = 1 };
typedef struct RiftSelectParams {
  int32_t mode, reserved;   /* reserved: 0 */
  double  temperature;      /* T > 0, read in SAMPLE only */
} RiftSelectParams;         /* 16 bytes */

/* GREEDY, 0, 1.0: the choice of rift_control_tick.  No context, no device. */
int riftcs_params_default(RiftSelectParams* out);

/* rift_control_tick with the choice of the executed candidate under `params`.  Every argument up to n_slots means what it means there, and
 * so do the decision row, pid_state and the launches (one wave per CBV, RIFT_CTL_CHUNK CBVs per launch).  GREEDY launches the kernels of
 * rift_control_tick and gives its bits; `u` is not read.
 * THE RULE of SAMPLE, for one CBV with flat logits z[0..G) (G = Rb * 12), `topk`, temperature T and one uniform number u in [0, 1).  The
 * host statement (sample_candidate, rift_amd/planning/pluto/inference.py) and the device stage (csrc/control.h) implement this text.
 *   kept set     the `topk` largest logits, exact ties to the lower flat index: rift_control_tick's.
 *   ref-free     first and unchanged: s_top = 1 / sum over kept j of expf(z_j - z_top) in fp32, at T = 1.  With a ref-free trajectory and
 *                0.25 > s_top the ref-free candidate is executed as in rift_control_tick: decision elements 3, 4, 5 are -1, topk, 0.25.
 *                Neither u nor T enters this choice.
 *   weights      otherwise w_j = expf((z_j - z_top) * r) in fp32 for kept j, r = (float)(1.0 / T) (at most FLT_MAX) formed ONCE on the host and
 *                multiplied in fp32 on both sides (the same product, no contraction); 0 for every other candidate.  A padded line (-1e6, for T below a few
 *                thousand) or a -inf logit underflows to exactly 0 and is never drawn; the top candidate has weight 1, so the total is not 0.
 *   draw         c_j = the inclusive prefix sums of the kept weights in ascending flat-index order, accumulated in fp64 from the fp32
 *                weights; W = the last one.  Chosen: the first kept j in that order with w_j > 0 and u * W < c_j; if rounding leaves none,
 *                the last kept j with w_j > 0.  (The device adds each 64-candidate plane with a parallel scan and carries the plane totals:
 *                the same sums in another order, equal to fp64 rounding.  A u closer to an edge c_j / W than that rounding and the few ulp
 *                between two expf may fall on either side.)
 *   reported     element 3 = the chosen flat index; element 4 = its position in the kept list ordered by descending logit, ties to the lower
 *                flat index first (the number of kept candidates that precede it); element 5 = (double)w_j / W, the probability it was
 *                drawn with.
 *   non-finite   a NaN or +inf logit is outside the contract, as for the greedy choice (rift_check_finite); the kernel still terminates and
 *                element 3 is a flat index in [0, G): with no drawable candidate, the greedy top.
 * With topk == 1, or as T -> 0, the draw is the greedy candidate.
 * u: HOST array of K doubles, u[k] for cbvs[k]; NULL is allowed in GREEDY.  It travels with the CBV descriptors as a kernel argument: no
 * device buffer, no upload.
 * RIFT_ERR_ARG with a message (rift_last_error), decided on the host before any launch and ahead of rift_control_tick's own refusals,
 * which apply unchanged: params == NULL; mode outside {GREEDY, SAMPLE}; reserved != 0; temperature not finite or <= 0; SAMPLE with
 * u == NULL and K > 0; a u[k] that is NaN or outside [0, 1).  K == 0 is RIFT_OK without a launch. */
int riftcs_control_tick(RiftCtx* ctx, const float* trajectory /*(bs,Rb,12,Tfull,6)*/, const float* probability /*(bs,Rb,12) logits*/,
                        const float* ref_free_trajectory /*(bs,Tfull,4) or NULL*/, int Rb, int Tfull, const RiftControlCBV* cbvs, int K,
                        int topk, int sample_interval, double* pid_state /*(n_slots,RIFT_CONTROL_STATE) f64, in/out*/, int n_slots,
                        const RiftSelectParams* params, const double* u /*HOST (K), or NULL in GREEDY*/, double* decision /*(K,8) f64*/,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RIFT_SELECT_H */
