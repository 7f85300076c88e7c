// The rollout tick's last step on the device (rift_control_tick, shared.hip): per CBV, keep the top-k candidates by logit, score them with
// a softmax over the kept logits, choose (the ref-free candidate joins last with score 0.25), move the chosen path into the CBV's frame and
// step the waypoint PID -- what PLUTO._decide does on the host with trim_candidates + global_to_local (planning/pluto/inference.py;
// reference pluto.py:142-279) and PIDController.control_pid (planning/pluto/controller/pid_controller.py; reference
// controller/pid_controller.py:13-100).  One 64-lane wave per CBV; the CBV descriptors travel as kernel arguments in chunks, as TickArr does.
//
// The softmax is monotonic, so the best learned candidate is the largest logit; the remaining top-k rounds only feed the denominator.
// The path arithmetic is the host's, operation for operation, in fp64 without contraction (rotate + translate to the global frame,
// re-anchor on the rear axle, rotate back): the two frames cancel only to rounding, and the host result is the statement of the interface.
// One sum is not numpy's tree: the segment lengths behind the target speed are added in path order, which is what np.mean does below eight
// segments (the default: 80 frames, interval 10, seven segments); from eight segments on numpy sums pairwise and the two agree to rounding.
// Which candidate is executed is a stage selected at compile time: the largest logit (rift_control_tick, and GREEDY of riftcs_control_tick),
// or a draw from the softmax over the kept logits at a temperature (SAMPLE; include/rift_select.h states the rule).  Path, PID and decision
// row are shared.
#pragma once
#include "../../include/rift_hip.h"
#include "lanes.h"

namespace rift {

#define RIFT_CTL_CHUNK 16                        // CBVs per launch
#define RIFT_CTL_RING 20
// a pid_state row (RIFT_CONTROL_STATE doubles, rift_hip.h): turn ring [0,20) | speed ring [20,40) | turn head, last | speed head, last
static_assert(2 * RIFT_CTL_RING + 4 == RIFT_CONTROL_STATE, "the pid_state row and RIFT_CONTROL_STATE of rift_hip.h disagree");

struct CtlK {                                    // one CBV
  const float* traj;                             // (G, Tfull, 6) candidates of the CBV's batch row
  const float* prob;                             // (G) logits of that row
  const float* rf;                               // (Tfull, 4) ref-free trajectory of that row, or nullptr
  double* state;                                 // (44) this CBV's pid_state row
  double* dec;                                   // (8) this CBV's decision row
  double ox, oy, ch, sh, speed;                  // rear axle, cos / sin of the heading, speed
  double u;                                      // this CBV's uniform number in [0, 1) (the SAMPLE stage only)
};
struct CtlArr { CtlK d[RIFT_CTL_CHUNK]; int K, G, Tfull, topk, interval; float inv_t; };      // inv_t: (float)(1 / temperature), formed on the host (SAMPLE)

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// WindowedPID.step: the ring's oldest slot takes the error, the mean runs over the window in chronological order with numpy's summation
// tree for 20 values (eight running sums over the first 16, combined pairwise, the last four added in order).
__device__ inline double ctl_pid_step(double* ring, double* head_last, double kp, double ki, double kd, double e) {
#pragma clang fp contract(off)
  constexpr int N = RIFT_CTL_RING;
  int head = (int)head_last[0];
  head = head < 0 ? 0 : (head >= N ? N - 1 : head);                   // (a row the caller filled with something else must not index outside the ring)
  const double last = head_last[1];
  ring[head] = e;
  head = head + 1 == N ? 0 : head + 1;
  double w[N];
#pragma unroll
  for (int i = 0; i < N; ++i) { const int j = head + i; w[i] = ring[j >= N ? j - N : j]; }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = w[j] + w[8 + j];
  double sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
  for (int i = 16; i < N; ++i) sum += w[i];
  const double out = kp * e + ki * (sum / (double)N) + kd * (e - last);
  head_last[0] = (double)head;
  head_last[1] = e;
  return out;
}

// The SAMPLE stage (include/rift_select.h states the rule; sample_candidate of planning/pluto/inference.py is its host statement): on what the
// wave holds after the top-k rounds -- z[MAXPL] per lane, candidate g = lane + 64 i, the kept candidates in `taken`.  Plane i holds the flat
// indices [64 i, 64 i + 64) in lane order, so the prefix sums in flat order are an inclusive 64-lane scan per plane (fp64, six shuffle steps)
// plus the running total of the planes before it; a plane without a drawable candidate is skipped (wave-uniform).  No LDS, no atomics.
// Whatever the logits hold, `chosen` leaves as a flat index in [0, G): a kept candidate or the greedy top.
template <int MAXPL>
__device__ __forceinline__ void ctl_sample(const float (&z)[MAXPL], unsigned taken, float ztop, int top, float inv_t, double u, int lane,
                                           int& chosen, int& pos, double& prob) {
#pragma clang fp contract(off)
  float w[MAXPL];
  double c[MAXPL];
  double carry = 0.0;
#pragma unroll
  for (int i = 0; i < MAXPL; ++i) {
    w[i] = ((taken >> i) & 1u) ? expf((z[i] - ztop) * inv_t) : 0.f;
    const bool live = w[i] > 0.f;                                      // (false for a NaN)
    double s = live ? (double)w[i] : 0.0;
    if (__ballot(live) != 0ull) {
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(s, o, 64); if (lane >= o) s += t; }
      c[i] = carry + s;
      carry += __shfl(s, 63, 64);
    } else {
      c[i] = carry;
    }
  }
  const double W = carry, thr = u * W;
  int hit = 0x7fffffff, last = -1;                                     // per lane: the first drawable candidate past u * W, the last drawable one
#pragma unroll
  for (int i = 0; i < MAXPL; ++i)
    if (w[i] > 0.f) { const int g = lane + i * 64; if (hit == 0x7fffffff && thr < c[i]) hit = g; last = g; }
  int sel = wave_min_i(hit);
  if (sel == 0x7fffffff) { last = -wave_min_i(-last); sel = last >= 0 ? last : top; }
  float zc = 0.f, wc = 0.f;
#pragma unroll
  for (int i = 0; i < MAXPL; ++i) if (i == (sel >> 6)) { zc = z[i]; wc = w[i]; }
  zc = __shfl(zc, sel & 63, 64); wc = __shfl(wc, sel & 63, 64);
  int before = 0;                                                      // kept candidates ahead of it by descending logit, ties to the lower index
#pragma unroll
  for (int i = 0; i < MAXPL; ++i)
    if ((taken >> i) & 1u) { const int g = lane + i * 64; if (z[i] > zc || (z[i] == zc && g < sel)) ++before; }
  chosen = sel; pos = (int)wave_sum((float)before); prob = (double)wc / W;
}

// SAMPLE = false is the choice of rift_control_tick (the largest logit); SAMPLE = true adds the stage above between the score and the path.
template <int MAXPL, bool SAMPLE>
__global__ __launch_bounds__(64) void control_tick_kernel(const CtlArr a) {
#pragma clang fp contract(off)
  if ((int)blockIdx.x >= a.K) return;
  const CtlK& d = a.d[blockIdx.x];
  const int lane = threadIdx.x, G = a.G, Tfull = a.Tfull, kint = a.interval;

  // ---- top-k by logit (ties: the lower flat index), softmax over the kept logits in fp32
  float z[MAXPL];
#pragma unroll
  for (int i = 0; i < MAXPL; ++i) { const int g = lane + i * 64; z[i] = g < G ? d.prob[g] : 0.f; }
  unsigned taken = 0u;
  int top = 0; float ztop = 0.f;
  for (int r = 0; r < a.topk; ++r) {
    float bv = 0.f; int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < MAXPL; ++i) {
      const int g = lane + i * 64;
      if (g < G && !((taken >> i) & 1u) && (bi == 0x7fffffff || z[i] > bv)) { bv = z[i]; bi = g; }
    }
    const bool has = bi != 0x7fffffff;
    const float mv = wave_max(has ? bv : -3.402823466e38f);
    const int wi = wave_min_i(has && bv == mv ? bi : 0x7fffffff);
    if (wi == 0x7fffffff) break;                                       // (topk <= G: not reached with ordinary logits)
    if ((wi & 63) == lane) taken |= 1u << (wi >> 6);
    if (r == 0) { top = wi; ztop = mv; }
  }
  float e = 0.f;
#pragma unroll
  for (int i = 0; i < MAXPL; ++i) if ((taken >> i) & 1u) e += expf(z[i] - ztop);
  const float score = 1.0f / wave_sum(e);
  const bool ref_free = d.rf != nullptr && 0.25f > score;              // first maximum: a learned candidate wins a tie with 0.25
  int chosen = top, pos = 0;                                           // (read in the SAMPLE instantiation only: the greedy one keeps its own expressions)
  double prob = 0.0;
  if constexpr (SAMPLE) {
    prob = (double)score;
    if (!ref_free) ctl_sample<MAXPL>(z, taken, ztop, top, a.inv_t, d.u, lane, chosen, pos, prob);
  }

  // ---- the chosen path in the vehicle frame: point 0 and the thinned points path[k-1::k], lane j transforms thinned point j
  const float* path = ref_free ? d.rf : d.traj + (size_t)(SAMPLE ? chosen : top) * Tfull * 6;
  const int stride = ref_free ? 4 : 6;
  const double ox = d.ox, oy = d.oy, ch = d.ch, sh = d.sh, v = d.speed;
  const double x0 = (double)path[0], y0 = (double)path[1];
  const double dx0 = ox - ((x0 * ch - y0 * sh) + ox), dy0 = oy - ((x0 * sh + y0 * ch) + oy);      // origin - global[0]
  const int n = Tfull / kint;                                          // thinned points (>= 2: checked on the host)
  double aim = 0.5 * v + 2.5;
  aim = fmin(fmax(aim, 5.0), 8.0);
  double seg_sum = 0.0, best = 0.0, ax = 0.0, ay = 0.0, px = 0.0, py = 0.0;
  for (int base = 0; base < n; base += 64) {
    const int j = base + lane;
    double lx = 0.0, ly = 0.0;
    if (j < n) {
      const float* p = path + (size_t)((j + 1) * kint - 1) * stride;
      const double x = (double)p[0], y = (double)p[1];
      const double gx = (x * ch - y * sh) + ox, gy = (x * sh + y * ch) + oy;      // trim_candidates: [x y] . [[c, s], [-s, c]] + origin
      const double qx = (gx + dx0) - ox, qy = (gy + dy0) - oy;                    // global_to_local: re-anchored, relative to the rear axle
      lx = qx * ch + qy * sh; ly = qy * ch - qx * sh;                              //                  . [[c, -s], [s, c]]
    }
    const int cnt = min(64, n - base);
    for (int t = 0; t < cnt; ++t) {                                    // in path order, the same in every lane
      const double x = __shfl(lx, t, 64), y = __shfl(ly, t, 64);
      const int jj = base + t;
      if (jj > 0) { const double sx = x - px, sy = y - py; seg_sum += sqrt(sx * sx + sy * sy); }
      if (jj < n - 1) {                                                // aim point: the last thinned point is excluded, first minimum
        const double dist = fabs(sqrt(x * x + y * y) - aim);
        if (jj == 0 || dist < best) { best = dist; ax = x; ay = y; }
      }
      px = x; py = y;
    }
  }
  if (lane != 0) return;

  // ---- PIDController.control_pid, serial
  const double target = seg_sum / (double)(n - 1);
  const bool brake = target < 0.4 || v / target > 1.1;                 // (short circuit: a zero target never divides)
  double* st = d.state;
  const double gas = ctl_pid_step(st + RIFT_CTL_RING, st + 42, 5.0, 0.5, 1.0, fmin(fmax(target - v, 0.0), 1.0));
  const double throttle = brake ? 0.0 : fmin(fmax(gas, 0.0), 1.0);
  const double bearing = (brake || v < 0.01) ? 0.0 : (-atan2(ay, ax) * (180.0 / 3.141592653589793)) / 90.0;
  const double steer = fmin(fmax(ctl_pid_step(st, st + 40, 1.25, 0.75, 0.3, bearing), -1.0), 1.0);
  double* o = d.dec;
  o[0] = throttle; o[1] = steer; o[2] = brake ? 1.0 : 0.0;
  if constexpr (SAMPLE) {
    o[3] = ref_free ? -1.0 : (double)chosen; o[4] = ref_free ? (double)a.topk : (double)pos; o[5] = ref_free ? 0.25 : prob;
  } else {
    o[3] = ref_free ? -1.0 : (double)top; o[4] = ref_free ? (double)a.topk : 0.0; o[5] = ref_free ? 0.25 : (double)score;
  }
  o[6] = target; o[7] = bearing;
}

}  // namespace rift
