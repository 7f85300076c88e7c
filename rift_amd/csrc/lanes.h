// Operand-format-free device helpers of the gfx950 kernels (wave64): the LDS-only barrier, cross-lane reductions, the counter-based RNG,
// finiteness by bit pattern.  Nothing here depends on the MFMA operand format: each engine build makes these names visible inside its own namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rift {

// counter-based RNG for dropout / drop-path / state-dropout: one 32-bit hash per element
// (two rounds of the lowbias32 integer finaliser over (seed, stream, element index); 32-bit multiplies only).
__device__ __forceinline__ uint32_t hash32(uint32_t seed, uint32_t stream, uint32_t idx) {
  uint32_t x = idx * 0x9E3779B1u + (seed ^ (stream * 0x85EBCA6Bu));
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  x += seed * 0xC2B2AE35u + stream;
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
// Element-wise dropout decisions: ONE lowbias32 round per counter and two 16-bit uniforms out of every hash (probability resolution
// 2^-16); the decision is an integer compare against thr16 = p * 65536.  Four times cheaper per element than uniform01, which the
// decoder kernel's dropout epilogues (attention weights, residual branches, FFN hidden layer) were paying 70 us a step for.
__device__ __forceinline__ uint32_t hash1(uint32_t seed, uint32_t stream, uint32_t idx) {
  uint32_t x = idx * 0x9E3779B1u + (seed ^ (stream * 0x85EBCA6Bu));
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}

__device__ __forceinline__ float uniform01(uint32_t seed, uint32_t stream, uint32_t idx) {
  return (float)(hash32(seed, stream, idx) >> 8) * (1.0f / 16777216.0f);
}

// Workgroup barrier for phases that hand data over through LDS only.  __syncthreads() makes hipcc drain EVERY outstanding memory
// operation first (s_waitcnt vmcnt(0) lgkmcnt(0)), which ends the flight of the weight / parameter / next-tile loads these kernels
// issue a phase ahead; here only the LDS counter is drained, so global loads stay in flight across the barrier until their first use.
// Not for phases that exchange data through global memory.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Cross-lane sums.  __shfl_xor lowers to ds_bpermute_b32 (an LDS-crossbar round trip, ~100 cycles of dependent
// latency per step); within a 16-lane row the same exchange is a DPP modifier on a VALU op (a few cycles):
// quad_perm[1,0,3,2], quad_perm[2,3,0,1], row_half_mirror, row_mirror.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float sum4(float v) { v += dpp_f<0xB1>(v); v += dpp_f<0x4E>(v); return v; }
__device__ __forceinline__ float sum8(float v) { v = sum4(v); v += dpp_f<0x141>(v); return v; }
__device__ __forceinline__ float sum16(float v) { v = sum8(v); v += dpp_f<0x140>(v); return v; }
// Across the four 16-lane rows gfx950 has half-exchange instructions: v_permlane16_swap (odd rows of vdst <-> even rows of src)
// and v_permlane32_swap (upper half of vdst <-> lower half of src).  With vdst = src = v the two results hold v[lane] and
// v[lane ^ 16] (resp. v[lane ^ 32]) in some order in every lane, so a commutative combine of them is the xor exchange -- one
// VALU-rate instruction instead of a ds_bpermute round trip.
__device__ __forceinline__ float xadd16(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xadd32(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xmax16(float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xmax32(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float rows_sum(float v) { return xadd32(xadd16(v)); }   // over the 4 lanes {l, l^16, l^32, l^48}

__device__ __forceinline__ float rows_max(float v) { return xmax32(xmax16(v)); }
__device__ __forceinline__ float sum32(float v) { v = sum16(v); return xadd16(v); }
// sum over groups of LPR consecutive lanes (LPR = 8, 16, 32, 64), result in every lane of the group
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
  if (LPR == 4) return sum4(v);
  if (LPR == 8) return sum8(v);
  if (LPR == 16) return sum16(v);
  v = sum32(v);
  if (LPR == 64) v = xadd32(v);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) { return group_sum<64>(v); }
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Finiteness by bit pattern: a float is NaN / +-Inf iff its exponent field is all ones.  Integer compares, so the test also holds in the
// translation units built with -fno-honor-nans (where x != x folds to false) -- used for the device flag behind the reference's
// `assert torch.isfinite(q).all()` (planning_decoder.py:175).  exp_or accumulates the largest exponent field seen; nonfinite_exp tests it.
__device__ __forceinline__ uint32_t exp_max(uint32_t acc, float v) { const uint32_t e = __float_as_uint(v) & 0x7f800000u; return acc > e ? acc : e; }
__device__ __forceinline__ bool nonfinite_exp(uint32_t acc) { return acc == 0x7f800000u; }

}  // namespace rift
