// The group advantage of the policy update from stored returns (include/rift_advantage.h states the rule): baseline, scale and clip are
// run-time parameters, the arena of a replay is one call.  First the host half -- defaults and refusals, free of HIP types, so that a
// stand-alone program built by a plain C++ compiler can run it (tests/test_advantage_param_cases.py) -- then the kernels, for hipcc only.
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/rift_advantage.h"

static inline void riftga_params_set_default(RiftAdvantageParams* p) {
  p->baseline = RIFTGA_BASELINE_MEAN; p->scale = RIFTGA_SCALE_GROUP_STD; p->eps = 1e-5; p->clip = 0.0;
}

// nullptr: the call is accepted; else the reason, a string literal.  Everything riftga_arena_advantage refuses, ahead of any launch.
static inline const char* riftga_refusal(const double* returns, int n, int Rcap, const RiftAdvantageParams* p, const double* advantage) {
  if (!p) return "params == NULL";
  if (p->baseline < RIFTGA_BASELINE_MEAN || p->baseline > RIFTGA_BASELINE_NONE) return "baseline outside {0, 1, 2}";
  if (p->scale < RIFTGA_SCALE_GROUP_STD || p->scale > RIFTGA_SCALE_NONE) return "scale outside {0, 1, 2}";
  if (!isfinite(p->eps) || p->eps < 0.0) return "eps not finite or < 0";
  if (!isfinite(p->clip) || p->clip < 0.0) return "clip not finite or < 0";
  if (n < 0) return "n < 0";
  if (Rcap < 1) return "Rcap < 1";
  if (n > 0 && (!returns || !advantage)) return "returns or advantage == NULL";
  if (n > 0 && advantage == returns) return "advantage == returns (the call is not in place)";
  return nullptr;
}

// Scratch of one call, in doubles (grow-only, RiftCtxCore::ga_scratch): four per-scene partials, then the arena's totals.
#define RIFTGA_NPART 4      // per scene: sum c^2 | G | 1 where G > 0 and sd == 0 | candidates clamped
#define RIFTGA_NTOT 4       // rms | N | the element-wise kernel's clamp counter (a 64-bit integer in the slot) | unused
static inline size_t riftga_scratch_doubles(int n) { return (size_t)n * RIFTGA_NPART + RIFTGA_NTOT; }

#if defined(__HIPCC__)
#include "lanes.h"

namespace rift {

struct ArenaAdvP {
  const double* ret; const int32_t* r_count; const uint8_t* mask; int n, Rcap;
  int baseline, scale; double eps, clip;
  double* adv;
  double* part;           // [RIFTGA_NPART][n], or nullptr: nobody reads the partials (a group mode without stats)
  double* tot;            // [RIFTGA_NTOT]
  double* stats;          // the caller's [8], or nullptr
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ bool arena_adv_valid(const ArenaAdvP& p, int scene, int rc, int i) {
  return i / 12 < rc && (!p.mask || p.mask[(size_t)scene * p.Rcap * 12 + i] != 0);
}

// One wave per scene, four waves per workgroup, the Rcap * 12 flat indices of the scene lane-strided -- the order of group_zscore_body
// (adv.h), so that a fully valid prefix under the default parameters is that kernel's arithmetic bit for bit: the same lane sums, the same
// wave_sum_d, (x - mean) / (sd + eps).  The group modes write the finished advantage; BATCH_RMS writes c_j and leaves the division to
// arena_adv_scale_kernel, behind the arena-wide sum.
__global__ __launch_bounds__(256) void arena_adv_scene_kernel(ArenaAdvP p) {
  const int g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= p.n) return;
  const int L = p.Rcap * 12;
  const int rc = p.r_count ? p.r_count[g] : p.Rcap;
  const double* __restrict__ ret = p.ret + (size_t)g * L;
  double* __restrict__ adv = p.adv + (size_t)g * L;
  double s = 0.0;
  int cnt = 0;
  for (int i = lane; i < L; i += 64)
    if (arena_adv_valid(p, g, rc, i)) { s += ret[i]; ++cnt; }
  const int G = wave_sum_i(cnt);
  const double mean = G > 0 ? wave_sum_d(s) / (double)G : 0.0;
  double q = 0.0;
  for (int i = lane; i < L; i += 64)
    if (arena_adv_valid(p, g, rc, i)) { const double d = ret[i] - mean; q += d * d; }
  const double sd0 = G > 0 ? sqrt(wave_sum_d(q) / (double)G) : 0.0;
  const double sd = sd0 + p.eps;
  const double loo = G > 1 ? (double)G / (double)(G - 1) : 0.0;
  double c2 = 0.0;
  int clamped = 0;
  for (int i = lane; i < L; i += 64) {
    double a = 0.0;
    if (arena_adv_valid(p, g, rc, i)) {
      a = p.baseline == RIFTGA_BASELINE_NONE ? ret[i] : ret[i] - mean;
      if (p.baseline == RIFTGA_BASELINE_LEAVE_ONE_OUT) a *= loo;
      if (p.scale == RIFTGA_SCALE_GROUP_STD) a = a / sd;
      if (p.scale == RIFTGA_SCALE_BATCH_RMS) c2 += a * a;
      else if (p.clip > 0.0) {
        if (a > p.clip) { a = p.clip; ++clamped; }
        else if (a < -p.clip) { a = -p.clip; ++clamped; }
      }
    }
    adv[i] = a;
  }
  if (!p.part) return;
  c2 = wave_sum_d(c2);
  clamped = wave_sum_i(clamped);
  if (lane == 0) {
    p.part[g] = c2;
    p.part[(size_t)p.n + g] = (double)G;
    p.part[(size_t)2 * p.n + g] = (G > 0 && sd0 == 0.0) ? 1.0 : 0.0;
    p.part[(size_t)3 * p.n + g] = (double)clamped;
  }
}

// The arena-wide sums, by ONE workgroup and in a fixed order: thread-strided over the n scenes, wave_sum_d, the sixteen wave results through
// LDS and added in wave order.  The partials were written by an earlier launch on the same stream.  tot: rms, N, and the clamp counter of
// the element-wise kernel set to zero; stats when asked for ([4]: the group modes' clamped candidates -- BATCH_RMS counts them later).
#define RIFTGA_REDUCE_THREADS 1024
__global__ __launch_bounds__(RIFTGA_REDUCE_THREADS) void arena_adv_reduce_kernel(ArenaAdvP p) {
  constexpr int NWV = RIFTGA_REDUCE_THREADS / 64;
  __shared__ double sm[RIFTGA_NPART][NWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double a[RIFTGA_NPART];
#pragma unroll
  for (int k = 0; k < RIFTGA_NPART; ++k) a[k] = 0.0;
  double scenes = 0.0;
  for (int i = tid; i < p.n; i += RIFTGA_REDUCE_THREADS) {
#pragma unroll
    for (int k = 0; k < RIFTGA_NPART; ++k) a[k] += p.part[(size_t)k * p.n + i];
    scenes += p.part[(size_t)p.n + i] > 0.0 ? 1.0 : 0.0;
  }
#pragma unroll
  for (int k = 0; k < RIFTGA_NPART; ++k) {
    a[k] = wave_sum_d(a[k]);
    if (lane == 0) sm[k][wave] = a[k];
  }
  scenes = wave_sum_d(scenes);              // (a count: exact in any order)
  __shared__ double s_scenes[NWV];
  if (lane == 0) s_scenes[wave] = scenes;
  __syncthreads();
  if (tid != 0) return;
  double t[RIFTGA_NPART], sc = 0.0;
#pragma unroll
  for (int k = 0; k < RIFTGA_NPART; ++k) { t[k] = 0.0; for (int w = 0; w < NWV; ++w) t[k] += sm[k][w]; }
  for (int w = 0; w < NWV; ++w) sc += s_scenes[w];
  const bool batch = p.scale == RIFTGA_SCALE_BATCH_RMS;
  const double rms = (batch && t[1] > 0.0) ? sqrt(t[0] / t[1]) : 0.0;
  p.tot[0] = rms; p.tot[1] = t[1];
  *reinterpret_cast<unsigned long long*>(p.tot + 2) = 0ull;
  if (p.stats) {
    p.stats[0] = t[1]; p.stats[1] = sc; p.stats[2] = t[2]; p.stats[3] = rms; p.stats[4] = batch ? 0.0 : t[3];
    p.stats[5] = p.stats[6] = p.stats[7] = 0.0;
  }
}

// BATCH_RMS, behind the sum: advantage = clamp(c / (rms + eps)) element by element; what belongs to no group stays 0 whatever the
// denominator.  Clamped candidates are counted, when somebody asks, with an INTEGER atomic per workgroup that clamped any (tot[2]); the grid
// is capped and strides, so there are at most RIFTGA_SCALE_BLOCKS of them (one per wave cost 50 us of contention at 4096 scenes).
#define RIFTGA_SCALE_BLOCKS 1024
__global__ __launch_bounds__(256) void arena_adv_scale_kernel(ArenaAdvP p, size_t total, int count) {
  const double den = p.tot[0] + p.eps;
  const int L = p.Rcap * 12;
  int clamped = 0;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const int g = (int)(e / (size_t)L), i = (int)(e - (size_t)g * L);
    const int rc = p.r_count ? p.r_count[g] : p.Rcap;
    double a = 0.0;
    if (arena_adv_valid(p, g, rc, i)) {
      a = p.adv[e] / den;
      if (p.clip > 0.0) {
        if (a > p.clip) { a = p.clip; ++clamped; }
        else if (a < -p.clip) { a = -p.clip; ++clamped; }
      }
    }
    p.adv[e] = a;
  }
  if (!count) return;
  __shared__ int s_clamped[4];
  clamped = wave_sum_i(clamped);
  if ((threadIdx.x & 63) == 0) s_clamped[threadIdx.x >> 6] = clamped;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = s_clamped[0] + s_clamped[1] + s_clamped[2] + s_clamped[3];
    if (c > 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.tot + 2), (unsigned long long)c);
  }
}

// (BATCH_RMS with stats and a clip: the integer counter becomes stats[4])
__global__ void arena_adv_clamped_kernel(const double* __restrict__ tot, double* __restrict__ stats) {
  if (threadIdx.x == 0 && blockIdx.x == 0) stats[4] = (double)*reinterpret_cast<const unsigned long long*>(tot + 2);
}

}  // namespace rift
#endif  // __HIPCC__
