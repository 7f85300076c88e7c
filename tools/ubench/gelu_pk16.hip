// VALU-rate microbenchmark for the GELU epilogue at its real interface: one MFMA accumulator fragment (4 fp32) + bias -> 4 operand words.
//   V0  rational erf in packed fp32 (the packed form of csrc/common.h: gelu_fast), bf16 operand words      (round 2 .. 4)
//   V1  relu(x) - h(|x|) with the bump h(a) = a Phi(-a) as a degree-7 polynomial in PACKED FP16 (v_pk_fma_f16: two elements per full-rate
//       instruction), result converted to bf16 operand words                            (round 5, bf16 build)
//   V2  V0 with fp16 operand words
//   V3  V1 leaving its result as fp16 operand words (no conversion)
// 8 waves per workgroup, one workgroup per CU, values in registers.
// build: hipcc --offload-arch=gfx950 -O3 tools/ubench/gelu_pk16.hip -o tools/ubench/gelu_pk16.bin ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cmath>
#include <vector>
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

#define P0 1.12838531f
#define P1 0.153424003f
#define P2 0.0432474986f
#define P3 0.000753648848f
#define Q1 0.469360935f
#define Q2 0.0945981576f
#define Q3 0.00932609519f
__device__ __forceinline__ f2 gelu_rat2(f2 x) {
  f2 z = x * 0.70710678118654752440f;
  z.x = __builtin_amdgcn_fmed3f(z.x, -3.3f, 3.3f); z.y = __builtin_amdgcn_fmed3f(z.y, -3.3f, 3.3f);
  const f2 t = z * z;
  const f2 p = __builtin_elementwise_fma(t, __builtin_elementwise_fma(t, __builtin_elementwise_fma(t, (f2)P3, (f2)P2), (f2)P1), (f2)P0);
  const f2 q = __builtin_elementwise_fma(t, __builtin_elementwise_fma(t, __builtin_elementwise_fma(t, (f2)Q3, (f2)Q2), (f2)Q1), (f2)1.0f);
  f2 r; r.x = __builtin_amdgcn_rcpf(q.x); r.y = __builtin_amdgcn_rcpf(q.y);
  const f2 e = z * p * r;
  const f2 hx = x * 0.5f;
  return __builtin_elementwise_fma(hx, e, hx);
}
template <bool F16>
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
  unsigned r;
  if (F16) asm("v_cvt_pk_f16_f32 %0, %1, %2\n\ts_nop 0" : "=v"(r) : "v"(lo), "v"(hi));
  else asm("v_cvt_pk_bf16_f32 %0, %1, %2\n\ts_nop 0" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
// h(a) = a Phi(-a) on [0, 4] in u = a / 2 - 1 (Chebyshev fit at 4000 nodes, monomial form; |error| <= 2.2e-4 in exact arithmetic)
#define H0 0.04531748f
#define H1 -0.17138292f
#define H2 0.22257517f
#define H3 0.01231068f
#define H4 -0.32790318f
#define H5 0.24358234f
#define H6 0.05996109f
#define H7 -0.08454493f
// two pairs in lock step: a v_pk_*_f16 result read by the NEXT instruction costs a wait state (hipcc pads an s_nop), so the two Horner chains alternate
__device__ __forceinline__ void gelu_pk16x2(float x0, float x1, float x2, float x3, h2& g0, h2& g1) {
  const h2 xa = __builtin_bit_cast(h2, pack2<true>(x0, x1)), xb = __builtin_bit_cast(h2, pack2<true>(x2, x3));
  const h2 FOUR = (h2)(_Float16)4.0f, HALF = (h2)(_Float16)0.5f, M1 = (h2)(_Float16)-1.0f, ZERO = (h2)(_Float16)0.0f;
  h2 aa, ab, ra, rb;
  asm("v_and_b32 %0, 0x7fff7fff, %1" : "=v"(aa) : "v"(xa));
  asm("v_and_b32 %0, 0x7fff7fff, %1" : "=v"(ab) : "v"(xb));
  asm("v_pk_min_f16 %0, %1, %2" : "=v"(aa) : "v"(aa), "v"(FOUR));
  asm("v_pk_min_f16 %0, %1, %2" : "=v"(ab) : "v"(ab), "v"(FOUR));
  asm("v_pk_max_f16 %0, %1, %2" : "=v"(ra) : "v"(xa), "v"(ZERO));
  asm("v_pk_max_f16 %0, %1, %2" : "=v"(rb) : "v"(xb), "v"(ZERO));
  const h2 ua = __builtin_elementwise_fma(aa, HALF, M1), ub = __builtin_elementwise_fma(ab, HALF, M1);
  h2 pa = __builtin_elementwise_fma(ua, (h2)(_Float16)H7, (h2)(_Float16)H6), pb = __builtin_elementwise_fma(ub, (h2)(_Float16)H7, (h2)(_Float16)H6);
#define STEP(C) pa = __builtin_elementwise_fma(pa, ua, (h2)(_Float16)C); pb = __builtin_elementwise_fma(pb, ub, (h2)(_Float16)C);
  STEP(H5) STEP(H4) STEP(H3) STEP(H2) STEP(H1) STEP(H0)
#undef STEP
  g0 = ra - pa; g1 = rb - pb;
}

template <int V>
__device__ __forceinline__ uint2 gelu4_pack(const f32x4 a, const float4 b) {
  uint2 o;
  if (V == 0 || V == 2) {
    f2 lo, hi, bl, bh;
    lo.x = a[0]; lo.y = a[1]; hi.x = a[2]; hi.y = a[3];
    bl.x = b.x; bl.y = b.y; bh.x = b.z; bh.y = b.w;
    lo = gelu_rat2(lo + bl); hi = gelu_rat2(hi + bh);
    o.x = pack2<V == 2>(lo.x, lo.y); o.y = pack2<V == 2>(hi.x, hi.y);
  } else {
    h2 g0, g1;
    gelu_pk16x2(a[0] + b.x, a[1] + b.y, a[2] + b.z, a[3] + b.w, g0, g1);
    if (V == 3) { o.x = __builtin_bit_cast(unsigned, g0); o.y = __builtin_bit_cast(unsigned, g1); }
    else { o.x = pack2<false>((float)g0[0], (float)g0[1]); o.y = pack2<false>((float)g1[0], (float)g1[1]); }
  }
  return o;
}

template <int V>
__global__ __launch_bounds__(512) void k(unsigned* out, const float* in, int iters, long long* cyc) {
  f32x4 v[8];
  float4 bias;
  for (int i = 0; i < 8; ++i) for (int j = 0; j < 4; ++j) v[i][j] = in[(threadIdx.x * 32 + i * 4 + j) % 8192];
  bias = make_float4(in[threadIdx.x], in[threadIdx.x + 1], in[threadIdx.x + 2], in[threadIdx.x + 3]);
  __syncthreads();
  unsigned acc = 0;
  const long long t0 = clock64();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint2 r = gelu4_pack<V>(v[i], bias);
      acc ^= r.x + r.y;
      v[i][0] += 0.001f; v[i][2] -= 0.001f;      // keep the loop body from being hoisted
    }
  }
  __syncthreads();
  const long long t1 = clock64();
  out[blockIdx.x * 512 + threadIdx.x] = acc;
  if (threadIdx.x == 0 && blockIdx.x == 0) cyc[V] = t1 - t0;
}
template <int V>
__global__ void accuracy(float* o) {   // o[2 V], o[2 V + 1] = max / mean-square error of the operand word against erf GELU in double, x in [-8, 8]
  __shared__ double sq[1024];
  __shared__ float mx[1024];
  double s = 0; float m = 0.f;
  for (int i = threadIdx.x; i < 160001; i += blockDim.x) {
    const float x = -8.f + i * 1e-4f;
    const double ref = 0.5 * (double)x * (1.0 + erf((double)x * 0.70710678118654752440));
    const f32x4 a = {x, x, x, x};
    const uint2 r = gelu4_pack<V>(a, make_float4(0.f, 0.f, 0.f, 0.f));
    float got;
    if (V >= 2) got = (float)__builtin_bit_cast(h2, r.x)[1]; else got = __uint_as_float(r.x & 0xffff0000u);
    const float e = fabsf((float)((double)got - ref));
    m = fmaxf(m, e); s += (double)e * e;
  }
  sq[threadIdx.x] = s; mx[threadIdx.x] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)blockDim.x; ++i) { s += sq[i]; m = fmaxf(m, mx[i]); }
    o[2 * V] = m; o[2 * V + 1] = (float)sqrt(s / 160001.0);
  }
}
int main() {
  float *in, *eo; unsigned* out; long long* cyc;
  hipMalloc(&in, 8200 * 4); hipMalloc(&out, 256 * 512 * 4); hipMalloc(&cyc, 64); hipMalloc(&eo, 64);
  std::vector<float> h(8200);
  for (size_t i = 0; i < h.size(); ++i) h[i] = -3.f + 6.f * (float)(i % 977) / 977.f;
  hipMemcpy(in, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  const int iters = 2000;
  for (int rep = 0; rep < 2; ++rep) {
    k<0><<<256, 512>>>(out, in, iters, cyc); k<1><<<256, 512>>>(out, in, iters, cyc);
    k<2><<<256, 512>>>(out, in, iters, cyc); k<3><<<256, 512>>>(out, in, iters, cyc);
  }
  accuracy<0><<<1, 1024>>>(eo); accuracy<1><<<1, 1024>>>(eo); accuracy<2><<<1, 1024>>>(eo); accuracy<3><<<1, 1024>>>(eo);
  hipDeviceSynchronize();
  long long c[4]; float e[8];
  hipMemcpy(c, cyc, 32, hipMemcpyDeviceToHost); hipMemcpy(e, eo, 32, hipMemcpyDeviceToHost);
  const char* nm[4] = {"rational pk-f32 -> bf16", "bump pk-f16 -> bf16", "rational pk-f32 -> fp16", "bump pk-f16 -> fp16"};
  for (int i = 0; i < 4; ++i)
    printf("%-26s %.2f cycles per element (wave-level, 2 waves/SIMD)  operand word vs erf GELU on [-8, 8]: max %.2e rms %.2e\n", nm[i],
           (double)c[i] / (iters * 32.0), e[2 * i], e[2 * i + 1]);
  return 0;
}
