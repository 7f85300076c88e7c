// Launch bookkeeping, error macros and the call protocol of an entry on the format-free core of a context (ctx_core.h), for the units
// that launch kernels: the engine builds and shared.hip.
#pragma once
#include "ctx_core.h"

#define HIPCHK(ctx, expr)                                                                 \
  do {                                                                                    \
    hipError_t e__ = (expr);                                                              \
    if (e__ != hipSuccess) {                                                              \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                    \
      return RIFT_ERR_HIP;                                                                \
    }                                                                                     \
  } while (0)
#define DEVCHK(ctx, expr) HIPCHK(ctx, (hipError_t)(expr))      // DevBuf::reserve: the allocation hook hands the runtime's error through
#define TRY(x) do { int rc__ = (x); if (rc__ != RIFT_OK) return rc__; } while (0)

namespace rift {

// shared.hip: the dynamic-LDS attributes of the kernels it launches (a hipError_t as int); every rift_ctx_create calls it
int shared_set_attributes();

// Launch bookkeeping on the core.  Internal to each translation unit that launches (the engine builds, shared.hip): the two diagnostic
// kernels are a few instructions and each unit sets the LDS attribute of its own copy.
namespace {

// what the entries that launch on the model's images answer while there is none (RIFT_ERR_STATE, ahead of any launch or allocation)
const std::string NOT_LOADED = ": no model is loaded (rift_model_load is missing, or the last one failed)";

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// The call protocol of an entry that launches, allocates or copies (every one of shared.hip): `if (!c) return RIFT_ERR_ARG;`, the message
// cleared, its refusals (host only, each with a message that names the entry called), call_open, its work, call_close -- in that order.  So a
// refused call leaves its own message, an accepted one an empty message, and every launch is on the context's device and the call's stream.
// (c->stream is the call's alone: no entry of the library launches on a value an earlier call left there -- profiles/NOTES_r28.md has the list.)
inline int refuse(RiftCtxCore* c, const char* entry, const std::string& why, int code = RIFT_ERR_ARG) { c->err = std::string(entry) + ": " + why; return code; }
inline int call_open(RiftCtxCore* c, void* stream) {
  c->err.clear(); c->stream = (hipStream_t)stream; c->dry = false;
  HIPCHK(c, hipSetDevice(c->device));
  return RIFT_OK;
}
inline int call_close(RiftCtxCore* c) { HIPCHK(c, hipGetLastError()); return RIFT_OK; }

inline void prof_events(RiftCtxCore* c, hipEvent_t* e0, hipEvent_t* e1) {
  while (c->prof_pool.size() < c->prof_used + 2) { hipEvent_t e; (void)hipEventCreate(&e); c->prof_pool.push_back(e); }
  *e0 = c->prof_pool[c->prof_used++]; *e1 = c->prof_pool[c->prof_used++];
}
inline void prof_push(RiftCtxCore* c, const char* label, hipEvent_t e0, hipEvent_t e1, double flops) {
  c->prof_recs.push_back(RiftCtxCore::Rec{label, e0, e1, flops});
}

// diagnostic (RIFT_POISON_LDS=<byte>): LDS keeps its contents between kernels, so a kernel that reads LDS it never wrote sees whatever
// the previous kernel on that CU left there.  With the switch set every launch is preceded by a kernel that fills all 160 KB of every
// CU's LDS with the byte (0xFF = NaN pattern): such a read then shows up in the parity tests instead of depending on history.
__global__ __launch_bounds__(256) void lds_poison_kernel(unsigned int pattern) {
  extern __shared__ unsigned int lds_all[];
  for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 256) lds_all[i] = pattern;
  __syncthreads();
  if (lds_all[threadIdx.x] != pattern) asm volatile("s_nop 0");      // keep the stores
}

// diagnostic (RIFT_DELAY=<launch label>:<microseconds>): one lane spins for that long on the stream right behind every launch of that
// label -- the successors of the kernel start later, no CU is taken from anybody.  d(step time) / d(delay) is the kernel's share of the
// step's critical path: ~1 on it, ~0 where the step pipeline has slack (tools/critical_path.py).
__global__ void delay_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
inline void delay_behind(RiftCtxCore* c, const char* label) {
  if (c->dg.delay_ticks > 0 && c->dg.delay_label == label) hipLaunchKernelGGL(delay_kernel, dim3(1), dim3(1), 0, c->stream, c->dg.delay_ticks);
}

// the bookkeeping around one launch (the callable) on c->stream: LDS poison ahead of it, profiling events around it, the diagnostic delay behind it
template <class F>
void launch_call(RiftCtxCore* c, const char* label, F&& f) {
  if (c->dry) return;
  if (c->poison_lds >= 0) {
    const unsigned int b = (unsigned int)c->poison_lds & 0xffu;
    hipLaunchKernelGGL(lds_poison_kernel, dim3(2048), dim3(256), 160 * 1024, c->stream, b | (b << 8) | (b << 16) | (b << 24));
  }
  if (c->prof_on) {
    hipEvent_t e0, e1;
    prof_events(c, &e0, &e1);
    (void)hipEventRecord(e0, c->stream);
    f();
    (void)hipEventRecord(e1, c->stream);
    prof_push(c, label, e0, e1, c->prof_flops);
    c->prof_flops = 0.0;
    return;
  }
  f();
  delay_behind(c, label);
}

// every kernel launch of shared.hip and the single-kernel launches of the engine; `label` is the kernel's name, one per kernel whatever the
// instantiation.  (arguments by reference: the ticks' descriptor arrays are a few KB)
template <class... KArgs, class... Args>
void launch(RiftCtxCore* c, const char* label, void (*kern)(KArgs...), dim3 grid, dim3 block, size_t shmem, const Args&... args) {
  if (grid.x == 0 || grid.y == 0) return;
  launch_call(c, label, [&] { hipLaunchKernelGGL(kern, grid, block, shmem, c->stream, static_cast<KArgs>(args)...); });
}

}  // namespace
}  // namespace rift
