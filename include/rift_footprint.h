/*
 * librift_hip.so -- collision flags from the footprints themselves, chosen at run time: an extension of the C-ABI of include/rift_hip.h
 * with a header and a symbol prefix of its own (`riftfp_`), layered as include/rift_select.h, include/rift_advantage.h and
 * include/rift_drivable.h are.  The three entries depend on no MFMA operand format, need no trampoline and are defined once per library
 * (csrc/shared.hip; the kernel in csrc/footprint.h, defaults and refusals in csrc/collision_params.h).  Conventions, error codes, RiftCtx,
 * RiftEvalParams and RiftTickCBV are rift_hip.h's.
 */
#ifndef RIFT_FOOTPRINT_H
#define RIFT_FOOTPRINT_H

#include "rift_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RIFTFP_ENVELOPE = 0, RIFTFP_FOOTPRINT = 1 };
typedef struct RiftCollisionParams {
  int32_t mode, reserved;   /* reserved: 0 */
} RiftCollisionParams;      /* 8 bytes */

/* ENVELOPE, 0: the test of rift_collision_matrix.  No context, no device. */
int riftfp_params_default(RiftCollisionParams* out);

/* rift_collision_matrix with the test of one candidate footprint against one neighbour footprint under `params`.  ENVELOPE is the
 * reference's test: its STRtree query carries no predicate, so it compares axis-aligned envelopes -- a vehicle heading 45 degrees
 * "collides" with a neighbour a whole lane away.  FOOTPRINT tests the oriented quadrilaterals themselves.
 * THE RULE of FOOTPRINT, for one candidate footprint P at step j and one neighbour footprint Q at step j, four vertices each in the given
 * order.  The host statement (collision_matrix, rift_amd/planning/fine_tuner/rlft/traj_eval/footprint.py) and the kernel (csrc/footprint.h)
 * implement this text.
 *   inputs       every fp32 coordinate of P is widened to fp64 (exact); Q is fp64.
 *   envelope     first: the envelopes of P and Q are the [min, max] of their four x and of their four y.  If they are apart by the test of
 *                rift_collision_matrix (closed intervals, touching counts: apart iff minQx > maxPx or maxQx < minPx or minQy > maxPy or
 *                maxQy < minPy) the pair does not collide.  A FOOTPRINT flag therefore never exceeds the ENVELOPE flag, by construction
 *                and not only up to rounding.
 *   origin       otherwise every vertex of P and of Q is taken relative to vertex 0 of P: one rounded fp64 subtraction per coordinate.
 *   axes         each of the eight edges a -> b (b the cyclically next vertex of the same quadrilateral; P's four edges, then Q's) gives the
 *                axis n = (b.y - a.y, a.x - b.x), each component one rounded subtraction of relative coordinates.  No normalisation.
 *   projection   a relative vertex v projects to s(v) = add_rn(mul_rn(n.x, v.x), mul_rn(n.y, v.y)): two rounded products and one rounded
 *                sum, no fused multiply-add (the kernel: __dmul_rn / __dadd_rn; numpy does not contract).
 *   separation   P and Q each give the interval [min, max] of s over their four vertices; the axis separates iff minP > maxQ or
 *                minQ > maxP.  The comparison is strict: touching counts as colliding, like the envelope's closed intervals.
 *   decision     the pair collides iff the envelope test passed and none of the eight axes separates.
 *   outputs      collision[g][j] = 1 iff some neighbour n collides with candidate g at step j, else 0; first_actor[g][j] = the lowest such
 *                n, or -1.  In ENVELOPE mode "collides" is the envelope test alone, and first_actor means the same.
 * For convex quadrilaterals of non-zero area the rule is the exact "the closed sets share a point", up to the rounding of the operations
 * stated.  A quadrilateral degenerated to a line or a point gets whatever the axes say -- two collinear segments are not told apart, an
 * edge of length 0 gives the axis (0, 0), which separates nothing: outside the contract.  A NaN coordinate is outside the contract, as for
 * the envelope test; the kernel still terminates.  The rule does not depend on the winding of either quadrilateral, and exchanging P and Q
 * changes only the origin.
 * This is not the reference's test: where the two differ the reference says "collision" and this rule says "clear".  FOOTPRINT is
 * therefore opt-in.
 *
 * center_vertices: DEVICE (G, Tc, 4, 2) f32, of which steps [0, Ts) are read; other_vertices: DEVICE (N, Ts, 4, 2) f64, NULL with N == 0
 * (every flag 0, every first_actor -1); collision: DEVICE (G, Ts) u8; first_actor: DEVICE (G, Ts) i32, or NULL.
 * ENVELOPE with first_actor == NULL launches the kernel of rift_collision_matrix and gives its bits; every other combination launches
 * footprint_collision_kernel, one thread per (candidate, step).
 * RIFT_ERR_ARG with a message (rift_last_error), decided on the host before any launch and ahead of rift_collision_matrix's own refusals,
 * which apply unchanged: params == NULL; mode outside {ENVELOPE, FOOTPRINT}; reserved != 0. */
int riftfp_collision_matrix(RiftCtx* ctx, const float* center_vertices, int G, int Tc, const double* other_vertices, int N, int Ts,
                            const RiftCollisionParams* params, uint8_t* collision, int32_t* first_actor, void* stream);

/* riftdm_group_advantage_tick with the collision flags under `collision`.  Every argument up to and including `params` means what it means
 * there, per CBV the off-road flags come from a mask, from the loaded map or not at all as they do there, and the refusals of that entry
 * apply unchanged, behind those of `collision` (as for riftfp_collision_matrix).  ENVELOPE issues exactly the launches of
 * riftdm_group_advantage_tick and gives its bits.  FOOTPRINT launches stage 8 of the tick (tick_multi_kernel_8: THE RULE above, same grid,
 * one thread per candidate and step) IN PLACE of stage 3; everything behind the flags -- returns, terms, z-score -- is untouched. */
int riftfp_group_advantage_tick(RiftCtx* ctx, const float* trajectory, int Rb, int Tfull, const RiftTickCBV* cbvs, int K,
                                float* turn_buf, int32_t* turn_ptr, int32_t* turn_len, float* speed_buf, int32_t* speed_ptr, int32_t* speed_len,
                                const RiftEvalParams* params, const RiftCollisionParams* collision, double* advantage, double* returns,
                                double* terms, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RIFT_FOOTPRINT_H */
