// librift_hip.so : host orchestration + C-ABI of the MI355X-native RIFT policy-update path.
// See include/rift_hip.h for the interface and DESIGN.md for the kernel inventory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <unordered_map>
#include <dlfcn.h>
#include <vector>

#include "engine_ctx.h"
#include "gemm.h"
#include "kernels.h"
#include "nat_l0w.h"
#include "nat_l1w.h"
#include "enc_fused.h"
#include "dec_w.h"
#include "dec_kv.h"
#include "nat_l2w.h"
#include "enc_w.h"
#include "pe_w.h"
#include "fo_w.h"
#include "pe_fused.h"
#include "fourier_fused.h"
#include "fpn_fused.h"
#include "fwd_plan.h"
#include "ego_fused.h"
#include "heads_fused.h"
#include "pi_fused.h"
#include "model_load.h"

#define ENC_NW 8

using namespace RIFT_NS;

namespace {

template <class... KArgs>
void launch_gemm(Ctx* c, const char* label, void (*kern)(KArgs...), dim3 grid, dim3 block, size_t shmem, const GemmP& g) {
  c->prof_flops = 2.0 * (double)g.M * (double)g.N * (double)g.K;
  if (c->prof_on && c->prof_shapes) {   // RIFT_PROF_SHAPES=1: one label per GEMM shape (interned)
    char tmp[160];
    snprintf(tmp, sizeof(tmp), "%s:%dx%dx%d%s%s%s", label, g.M, g.N, g.K, g.pro == PRO_LN ? ":ln" : (g.pro == PRO_AFFINE ? ":bn" : ""),
             g.amode == AMODE_CONV3 ? ":conv" : "", g.stage == 0 ? ":scalar" : "");
    label = c->prof_names.insert(tmp).first->c_str();
  }
  launch(c, label, kern, grid, block, shmem, g);
}

// Weight-only products (mode embeddings through q_proj / m2m in-projection, the ego query projection): input
// independent, so they are computed by the first forward after rift_model_load and kept (per precision mode).
// Returns the buffer and whether the caller must fill it now.
float* wconst_get(Ctx* c, Ctx::WConst& slot, size_t n, bool fp32, bool* fill) {
  Ctx::WConst::V& w = slot.v[fp32 ? 0 : 1];
  if (w.p.reserve(n) != 0) { *fill = false; return nullptr; }
  *fill = !w.ready && !c->dry;
  if (!c->dry) w.ready = true;
  return w.p.get();
}

// ---- GEMM dispatch -----------------------------------------------------------------------
GemmP mk(const float* X, int ldx, int M, const PWShape& w, float* Y, int ldy) {
  GemmP g;
  memset(&g, 0, sizeof(g));
  g.X = X; g.ldx = ldx; g.M = M; g.N = w.N; g.K = w.K; g.Kp = w.Kp; g.bias = w.bias; g.Y = Y; g.ldy = ldy;
  g.ln_eps = 1e-5f; g.gb_div = 1; g.dp_div = 1; g.rz_div = 1;
  return g;
}

// Tile shapes (64 rows per workgroup, 4 waves):
//   m1n8 : wave = 16 rows x 128 cols   -- small K (B fragments are few, A fragments read once)
//   m4n2 : wave = 64 rows x  32 cols   -- N <= 128 with K >= 128 (each weight fragment feeds 4 MFMAs)
//   m2n6 : wave = 32 rows x  96 cols   -- 128 < N <= 192
//   m4n4 : wave = 64 rows x  64 cols   -- N > 192, 256 columns per pass
template <bool BF16>
void gemm_launch(Ctx* c, GemmP g) {
  const size_t a_bytes = (((size_t)64 * (g.Kp + Prec<BF16>::PAD) * sizeof(typename Prec<BF16>::lds_t)) + 15) & ~(size_t)15;
  int variant;   // 0 m1n8, 1 m4n2, 2 m2n6, 3 m4n4
  if (g.N <= 128) variant = (g.Kp >= 128 && g.N > 32) ? 1 : 0;
  else if (g.N <= 192) variant = 2;
  else variant = 3;
  static const int NTs[4] = {8, 2, 6, 4}, WNs[4] = {1, 4, 2, 4};
  const int NT = NTs[variant], WN = WNs[variant];
  const size_t c_bytes = (size_t)4 * 16 * (16 * NT + 4) * 4;
  const bool single = g.N <= 16 * NT * WN;
  g.cs_off = single ? 0 : (int)a_bytes;
  const size_t lds = single ? (a_bytes > c_bytes ? a_bytes : c_bytes) : a_bytes + c_bytes;
  const dim3 grid(cdiv(g.M, 64)), block(256);
  switch (variant) {
    case 0: launch_gemm(c, BF16 ? "gemm_bf16_m1n8" : "gemm_fp32_m1n8", gemm_rows_kernel<BF16, 1, 8, 4, 1>, grid, block, lds, g); break;
    case 1: launch_gemm(c, BF16 ? "gemm_bf16_m4n2" : "gemm_fp32_m4n2", gemm_rows_kernel<BF16, 4, 2, 1, 4>, grid, block, lds, g); break;
    case 2: launch_gemm(c, BF16 ? "gemm_bf16_m2n6" : "gemm_fp32_m2n6", gemm_rows_kernel<BF16, 2, 6, 2, 2>, grid, block, lds, g); break;
    default: launch_gemm(c, BF16 ? "gemm_bf16_m4n4" : "gemm_fp32_m4n4", gemm_rows_kernel<BF16, 4, 4, 1, 4>, grid, block, lds, g); break;
  }
}

void gemm(Ctx* c, GemmP g, const void* W, bool fp32) {      // W: the image of the precision (PW::f32 / PW::bf)
  if (g.M <= 0) return;
  // vectorised A staging needs 16-byte aligned rows: dense conv windows (C % 4 == 0) or ldx % 4 == 0, K % 4 == 0
  const bool conv = g.amode == AMODE_CONV3;
  const bool al = (((uintptr_t)g.X) & 15) == 0 && (g.K % 4 == 0) && (conv ? (g.cv_C % 4 == 0 && g.ldx == g.cv_C) : (g.ldx % 4 == 0)) &&
                  (g.pro == PRO_NONE || ((((uintptr_t)g.pg) | ((uintptr_t)g.pb)) & 15) == 0);
  const int KV = g.Kp / 4;
  g.dbg = c->sw.gemm_dbg;
  g.stage = !al ? 0 : (KV <= 8 ? 1 : KV <= 16 ? 2 : KV <= 32 ? 3 : KV <= 64 ? 4 : 5);
  g.evec = (g.N % 4 == 0) && (g.ldy % 4 == 0) && ((((uintptr_t)g.Y) & 15) == 0) &&
           (!g.bias || (((uintptr_t)g.bias) & 15) == 0) && (!g.gbias || (((uintptr_t)g.gbias) & 15) == 0) &&
           (!g.residual || ((g.ldr % 4 == 0) && (((uintptr_t)g.residual) & 15) == 0));
  g.W = W;
  if (fp32) gemm_launch<false>(c, g);
  else gemm_launch<true>(c, g);
}
void gemm(Ctx* c, const GemmP& g, const PW& w, bool fp32) { gemm(c, g, fp32 ? (const void*)w.f32.get() : (const void*)w.bf.get(), fp32); }

int set_lds_attrs(Ctx* c) {
  const int big = 160 * 1024;
#define SETATTR(K) HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, big))
  HIPCHK(c, (hipError_t)shared_set_attributes());      // (rollout_kernel; shared.hip)
  SETATTR(enc_fused_kernel<ENC_NW>);
  HIPCHK(c, (hipError_t)enc112_set_attributes());
  HIPCHK(c, (hipError_t)decw_set_attributes());
  HIPCHK(c, (hipError_t)l2w_set_attributes());
  HIPCHK(c, (hipError_t)encw_set_attributes());
  HIPCHK(c, (hipError_t)pew_set_attributes());
  HIPCHK(c, (hipError_t)fow_set_attributes());
  SETATTR((gemm_rows_kernel<true, 1, 8, 4, 1>));
  SETATTR((gemm_rows_kernel<true, 4, 2, 1, 4>));
  SETATTR((gemm_rows_kernel<false, 4, 2, 1, 4>));
  SETATTR((gemm_rows_kernel<true, 2, 6, 2, 2>));
  SETATTR((gemm_rows_kernel<true, 4, 4, 1, 4>));
  SETATTR((gemm_rows_kernel<false, 1, 8, 4, 1>));
  SETATTR((gemm_rows_kernel<false, 2, 6, 2, 2>));
  SETATTR((gemm_rows_kernel<false, 4, 4, 1, 4>));
#undef SETATTR
#define SETATTR_N(K, N) HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(N)))
  SETATTR_N(lds_poison_kernel, 160 * 1024);
  SETATTR_N(dec_kv_frag_kernel, DEC_KV_LDS);
  SETATTR_N(pe_mid_kernel, PE_MID_LDS);   // these kernels also hold a few hundred bytes of static LDS
  SETATTR_N(pe_out_kernel, PE_OUT_LDS);
  SETATTR_N(fourier_fused_kernel, FO_LDS);
  SETATTR_N(fpn_tail_kernel, FPN_LDS);
  SETATTR_N(heads3_fused_kernel, HD_LDS);
  SETATTR_N(pi_forward_kernel, PI_LDS);
  HIPCHK(c, (hipError_t)l0w_set_attributes());
  HIPCHK(c, (hipError_t)l1w_set_attributes());
#undef SETATTR_N
  return RIFT_OK;
}

// RCCL through dlopen (rift_comm_*): the library has no link-time dependency on a communication library; an RCCL that is already in the
// process (torch's) is reused so that one process does not run two of them.
struct RcclApi {
  struct UniqueId { char internal[128]; };
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
static RcclApi& rccl_api(std::string* why) {
  static RcclApi api;
  static bool tried = false;
  static std::string err;
  if (!tried) {
    tried = true;
    void* h = nullptr;
    const char* names[] = {getenv("RIFT_RCCL_LIB"), "librccl.so", "librccl.so.1"};
    for (const char* n : names) if (n && !h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL);      // one that is loaded already
    for (const char* n : names) if (n && !h) h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) err = std::string("librccl.so not found (set RIFT_RCCL_LIB): ") + (dlerror() ? dlerror() : "");
    else {
      api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(h, "ncclGetUniqueId");
      api.CommInitRank = (decltype(api.CommInitRank))dlsym(h, "ncclCommInitRank");
      api.AllReduce = (decltype(api.AllReduce))dlsym(h, "ncclAllReduce");
      api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
      api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
      api.ok = api.GetUniqueId && api.CommInitRank && api.AllReduce && api.CommDestroy;
      if (!api.ok) err = "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy";
    }
  }
  if (why) *why = err;
  return api;
}
static int comm_sum_f64(Ctx* c, double* buf, long long count, hipStream_t stream) {
  RcclApi& r = rccl_api(nullptr);
  if (!c->comm || !r.ok) return -1;
  return r.AllReduce(buf, buf, (size_t)count, /*ncclDouble*/ 8, /*ncclSum*/ 0, c->comm, stream);
}

// All-reduce xchg[kb, kb + n) over the ranks (BatchNorm sums); the first exchange of a forward also carries the mask slots [0, kb)
// and is followed by their conversion into the gathered padding mask.  Dry (arena sizing) passes exchange nothing.
void dp_exchange(Fwd& f, long long n) {
  Ctx* c = f.c;
  if (!f.dp) return;
  const bool with_kpm = f.kpm_pending;
  f.kpm_pending = false;
  if (c->dry) return;
  const long long off = with_kpm ? 0 : f.kb, cnt = with_kpm ? f.kb + n : n;
  if (cnt > 0) {
    const int rc = c->dp.fn ? c->dp.fn(c->dp.user, off, cnt, (void*)c->stream) : comm_sum_f64(c, c->dp.xchg + off, cnt, c->stream);      // (no callback: the library's own communicator)
    if (rc != 0 && c->err.empty()) c->err = c->dp.fn ? "data-parallel exchange callback failed" : "data-parallel exchange over the library communicator failed";
  }
  if (with_kpm) launch(c, "dp_kpm_read_kernel", dp_kpm_read_kernel, dim3(cdiv(f.kb, 256)), dim3(256), 0, (const double*)c->dp.xchg, f.kb, f.g_rkpm);
}

void layernorm(Fwd& f, const float* X, int ldx, float* Y, int ldy, int rows, int C, const LayerNormW& ln, int relu = 0) {
  Ctx* c = f.c;
  launch(c, "layernorm_kernel", layernorm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, X, ldx, Y, ldy, rows, C, ln.g,
         ln.b, 1e-5f, relu);
}

// FourierEmbedding (fourier_embedding.py:45-55): in (rows, D) -> out (rows, 128), a new buffer; add: added into the (rows, 128) buffer `to` instead
// (`add` and not the pointer says which: the sizing pass has no pointers)
FourierP fourier_desc(Fwd& f, const float* in, int in_ld, int rows, const FourierW& p, int wrap_dim, bool add, float* to) {
  Ctx* c = f.c;
  const int D = p.D;
  FourierP q; memset(&q, 0, sizeof(q));
  q.in = in; q.in_ld = in_ld; q.rows = rows; q.D = D; q.wrap_dim = wrap_dim; q.freqs = p.freqs;
  for (int d = 0; d < D; ++d) {
    const FourierW::Dim& m = p.mlps[d];
    const PW &lo = *m.lo, &last = *m.last, &w3 = *m.l3;
    q.w0[d] = lo.bf.get(); q.b0[d] = lo.bias; q.wl[d] = last.f32.get(); q.wl_ld = last.Kp;
    q.lng[d] = m.ln.g; q.lnb[d] = m.ln.b;
    q.w3[d] = w3.bf.get(); q.b3[d] = w3.bias;
  }
  q.og = p.out_ln.g; q.ob = p.out_ln.b;
  q.wo = p.out->bf.get(); q.bo = p.out->bias;
  q.Y = add ? to : A_alloc<float>(c, (size_t)rows * 128);
  q.accumulate = add ? 1 : 0;
  return q;
}

// DropPath rates and level shapes of the history encoder (linspace(0, 0.2, 6), embedding.py:30) and of the scene encoder (linspace(0, 0.2, 4),
// pluto_model.py:80-83): read by the fused and the layer-wise path alike
static const float NAT_DPR[6] = {0.f, 0.04f, 0.08f, 0.12f, 0.16f, 0.2f};
static const int NAT_L[3] = {20, 10, 5}, NAT_C[3] = {32, 64, 128};
static const float ENC_DPR[4] = {0.f, 0.2f / 3.f, 0.4f / 3.f, 0.2f};

#include "fwd_layerwise.h"      // the reference forward: the *_layerwise functions the stages below fall to by the kernel plan

// one embedding on its own; returns the buffer it wrote or added into
float* fourier(Fwd& f, const float* in, int in_ld, int rows, const FourierW& p, int wrap_dim, bool add = false, float* to = nullptr) {
  Ctx* c = f.c;
  const int D = p.D;
  if (f.kp.fourier == FO_LAYERWISE || D > 3) return fourier_layerwise(f, in, in_ld, rows, p, wrap_dim, add, to);      // (FourierP holds three dimensions)
  FourierP3 q3; memset(&q3, 0, sizeof(q3));
  q3.e[0] = fourier_desc(f, in, in_ld, rows, p, wrap_dim, add, to);
  q3.nblk[0] = cdiv(rows, FO_ROWS); q3.count = 1;
  c->prof_flops = 2.0 * rows * 128.0 * (D * (129.0 + 128.0) + 128.0);
  launch(c, "fourier_fused_kernel", fourier_fused_kernel, dim3(q3.nblk[0]), dim3(256), (size_t)FO_LDS, q3);
  return q3.e[0].Y;
}

// The two PointsEncoders (map polygons 10 -> 128 with 20 points, reference lines 6 -> 128 with 120 points) in the fused
// three-pass form (pe_fused.h), side by side: five launches for both (statistics, BN finalize, mid, BN finalize, out).
static void pe_fill(Fwd& f, PeP& q, const float* F, int Cin, int groups, int n, const uint8_t* valid, const PointsEncoderW& p) {
  Ctx* c = f.c;
  memset(&q, 0, sizeof(q));
  const int rows = groups * n;
  q.F = F; q.Cin = Cin; q.valid = valid; q.rows = rows; q.ntiles = cdiv(rows, 120);
  const PW &w1 = *p.first0, &w2 = *p.first3, &w3a = *p.feat, &w3b = *p.pool, &w4 = *p.second3;
  q.w1 = w1.bf.get(); q.w2 = w2.bf.get(); q.w3a = w3a.bf.get();
  q.w3b = w3b.bf.get(); q.w4 = w4.bf.get();
  q.b1 = w1.bias; q.b2 = w2.bias; q.b3 = w3a.bias; q.b4 = w4.bias;
  q.s1 = A_alloc<float>(c, 128); q.t1 = A_alloc<float>(c, 128); q.s2 = A_alloc<float>(c, 256); q.t2 = A_alloc<float>(c, 256);
  q.part1 = A_alloc<float>(c, (size_t)2 * 128 * q.ntiles);
  q.part2 = A_alloc<float>(c, (size_t)2 * 256 * q.ntiles);
  q.cnt = A_alloc<int>(c, q.ntiles);
  q.Fmid = A_alloc<unsigned short>(c, (size_t)rows * 256);
  q.gp = A_alloc<float>(c, (size_t)groups * 256);
  q.out = A_alloc<float>(c, (size_t)groups * 128);
  q.do_stats = f.train ? 1 : 0;
  { if (c->sw.pe_ts == n) { q.ts = A_alloc<long long>(c, 64); q.ts_tile = 0; tap(c, "pe_ts", (float*)q.ts, 128); } }
}

static BnFinP bn_fin(const PeP& q, const BatchNormW& bn, int C, const float* part, const float* sc, const float* sh,
                     double* sums = nullptr, int sums_mode = 0) {
  BnFinP b; memset(&b, 0, sizeof(b));
  b.sums = sums; b.sums_mode = sums_mode;
  b.part = part; b.cnt = q.cnt; b.nblk = q.ntiles; b.C = C; b.gamma = bn.g; b.beta = bn.b;
  b.running_mean = bn.mean; b.running_var = bn.var;
  b.num_batches = bn.num_batches; b.scale = (float*)sc; b.shift = (float*)sh;
  return b;
}

void points_encoder_pair(Fwd& f, const float* Fm, int gm, const uint8_t* vm, const PointsEncoderW& pm, const float* Fr, int gr,
                         const uint8_t* vr, const PointsEncoderW& pr, float** out_m, float** out_r) {
  Ctx* c = f.c;
  PeP2 q;
  pe_fill(f, q.a, Fm, 10, gm, 20, vm, pm);
  pe_fill(f, q.b, Fr, 6, gr, 120, vr, pr);
  const int nt = q.a.ntiles + q.b.ntiles;
  const bool pe_w = f.kp.pe == PE_PAIR_W;
  const double rows = (double)q.a.rows + q.b.rows, groups = (double)gm + gr;
  {   // what the passes hand to one another (tests/test_gpu_points_encoder.py): _a map polygons, _b reference lines; g in fp16 words
    static const char* const nm[2][6] = {{"pe_s1_a", "pe_t1_a", "pe_s2_a", "pe_t2_a", "pe_gp_a", "pe_g_a"}, {"pe_s1_b", "pe_t1_b", "pe_s2_b", "pe_t2_b", "pe_gp_b", "pe_g_b"}};
    const PeP* sd[2] = {&q.a, &q.b};
    const int grp[2] = {gm, gr};
    for (int i = 0; i < 2; ++i) {
      tap(c, nm[i][0], (float*)sd[i]->s1, 128); tap(c, nm[i][1], (float*)sd[i]->t1, 128);
      tap(c, nm[i][2], (float*)sd[i]->s2, 256); tap(c, nm[i][3], (float*)sd[i]->t2, 256);
      if (!pe_w) tap(c, nm[i][4], sd[i]->gp, (int64_t)grp[i] * 256);      // (pe_w_kernel keeps gp in registers: only pe_mid_kernel writes it)
      tap(c, nm[i][5], (float*)sd[i]->Fmid, (int64_t)sd[i]->rows * 128);
    }
  }
  const bool stats_p = f.kp.pe_stats_persistent;       // persistent pass A: one partial per workgroup (pe_fused.h)
  // reference lines packed at tile granularity (pe_fused.h: pe_pack_body): table + round count in device memory, built by one extra block
  // of pass A's launch (eval mode: a launch of its own)
  const bool packb = f.kp.pe_pack;
  int* pk_tab = nullptr; int* pk_hdr = nullptr;
  PePackP pk; memset(&pk, 0, sizeof(pk));
  // (the packing's own bound, not the ceil(lines / 2) rounds of the unpacked walk: segments of an odd number of long lines end on a
  // one-line round each -- 99 lines of six or more tiles fill 3 * 17 = 51 records, not 50)
  const int maxr = pe_pack_max_rounds(gr);
  if (packb) {
    pk_tab = A_alloc<int>(c, (size_t)std::max(maxr, 1) * PEW_TAB_INTS); pk_hdr = A_alloc<int>(c, 4);
    pk.tiles = f.r_tiles; pk.nlines = gr; pk.tab = pk_tab; pk.hdr = pk_hdr; pk.max_rounds = maxr; pk.fail = c->nonfinite.get();
    tap(c, "pe_pack_hdr", (float*)pk_hdr, 4); tap(c, "pe_pack_tab", (float*)pk_tab, (int64_t)std::max(maxr, 1) * PEW_TAB_INTS);
    if (!stats_p) { c->prof_flops = 0.0; launch(c, "pe_pack_lines_kernel", pe_pack_lines_kernel, dim3(1), dim3(256), (size_t)gr * 2 * sizeof(int), pk); }
  }
  if (stats_p) {
    int g = std::min(nt, 4 * c->sw.nat_grid);          // four 256-thread workgroups per CU
    int ga = (int)(((long long)g * q.a.ntiles + nt / 2) / nt);
    if (q.a.ntiles > 0 && ga < 1) ga = 1;
    if (q.b.ntiles > 0 && ga > g - 1) ga = g - 1;
    if (q.b.ntiles == 0) ga = g;
    ga = std::min(ga, q.a.ntiles);
    q.a.nwg1 = ga; q.b.nwg1 = std::min(g - ga, q.b.ntiles);
    PeP* sd[2] = {&q.a, &q.b};
    for (int i = 0; i < 2; ++i) { sd[i]->part1w = A_alloc<float>(c, (size_t)2 * 128 * std::max(sd[i]->nwg1, 1)); sd[i]->cnt1w = A_alloc<int>(c, std::max(sd[i]->nwg1, 1)); }
    c->prof_flops = 2.0 * 128.0 * (q.a.rows * 10.0 + q.b.rows * 6.0);
    launch(c, "pe_stats1_kernel", pe_stats1p_kernel, dim3(q.a.nwg1 + q.b.nwg1 + (packb ? 1 : 0)), dim3(256), packb ? (size_t)gr * 2 * sizeof(int) : 0, q, pk);
  } else if (f.train) {
    c->prof_flops = 2.0 * 128.0 * (q.a.rows * 10.0 + q.b.rows * 6.0);
    launch(c, "pe_stats1_kernel", pe_stats1_kernel, dim3(nt), dim3(256), 0, q);
  }
  const bool dpx = f.dp && f.train;      // data parallel: the four BatchNorms see the statistics of the GLOBAL minibatch
  double* xs = dpx ? c->dp.xchg + f.kb : nullptr;
  // pass B's live rounds and workgroup split, from pass A's counts (pe_fused.h: PeLiveP): one extra block of the BatchNorm-1 finalize
  PeLiveP lv; memset(&lv, 0, sizeof(lv));
  const bool live = f.kp.pe_live;
  int pew_grid = std::max(c->sw.nat_grid, 2), pew_ga = 0;      // (two sides: at one workgroup the split below leaves the polygons none -- RIFT_NAT_GRID=1)
  // (the two-line round counts only size the grid and its first split here: with packing or a live list the split is remade on the device)
  if (pe_w) pew_split(cdiv(q.a.rows, PEW_ROUND_ROWS), cdiv(q.b.rows, PEW_ROUND_ROWS), &pew_grid, &pew_ga);
  if (live || packb) {
    const PeP* sd[2] = {&q.a, &q.b};
    for (int i = 0; i < 2; ++i) {
      lv.cnt[i] = live ? sd[i]->cnt : nullptr; lv.nt[i] = sd[i]->ntiles; lv.nr[i] = cdiv(sd[i]->rows, PEW_ROUND_ROWS);
      lv.live[i] = A_alloc<int>(c, std::max(lv.nr[i], 1));
    }
    lv.grid = pew_grid; lv.hdr = A_alloc<int>(c, 4);
    lv.packed_b = pk_hdr;
    tap(c, "pe_live_hdr", (float*)lv.hdr, 4);
    tap(c, "pe_live_a", (float*)lv.live[0], std::max(lv.nr[0], 1)); tap(c, "pe_live_b", (float*)lv.live[1], std::max(lv.nr[1], 1));      // (written in train mode only)
  }
  const bool lvblock = live || packb;       // the extra block of the BatchNorm-1 finalize launch
  for (int mode = dpx ? 1 : 0; mode <= (dpx ? 2 : 0); ++mode) {
    BnFinP f1a = bn_fin(q.a, pm.bn1, 128, q.a.part1, q.a.s1, q.a.t1, xs, mode);
    BnFinP f1b = bn_fin(q.b, pr.bn1, 128, q.b.part1, q.b.s1, q.b.t1, xs ? xs + 257 : nullptr, mode);
    if (stats_p) { f1a.part = q.a.part1w; f1a.cnt = q.a.cnt1w; f1a.nblk = q.a.nwg1; f1b.part = q.b.part1w; f1b.cnt = q.b.cnt1w; f1b.nblk = q.b.nwg1; }
    const bool with_lv = lvblock && mode == (dpx ? 2 : 0);
    PeLiveP none; memset(&none, 0, sizeof(none));
    launch(c, "bn_finalize_t_kernel", bn_finalize_t_kernel, dim3(256 + (with_lv ? 1 : 0)), dim3(256), 0, f1a, f1b, f.train ? 1 : 0, f.bn_update ? 1 : 0, 1e-5f,
           with_lv ? lv : none);
    if (mode == 1) dp_exchange(f, 2 * 257);
  }
  c->prof_flops = 2.0 * rows * (128.0 * 8 + 128.0 * 256 + (f.train ? 256.0 * 256 : 0.0)) + 2.0 * groups * 256.0 * 256;
  BnFinP fa, fb;
  if (pe_w) {     // wave-private pass B: rounds of 240 rows, one statistics partial per workgroup
    PeWP w; memset(&w, 0, sizeof(w));
    const PeP* src[2] = {&q.a, &q.b};
    PeWSide* dst[2] = {&w.a, &w.b};
    const int npts[2] = {20, 120};
    const int grid = pew_grid, ga = pew_ga;
    const int nwg[2] = {lvblock ? grid : ga, lvblock ? grid : grid - ga};       // (live / packed: the split is made on the device; room for either extreme)
    for (int i = 0; i < 2; ++i) {
      const PeP& o = *src[i]; PeWSide& d = *dst[i];
      d.F = o.F; d.Cin = o.Cin; d.valid = o.valid; d.rows = o.rows; d.npts = npts[i];
      d.nrounds = (i == 1 && packb) ? maxr : cdiv(o.rows, PEW_ROUND_ROWS);      // (packed: the kernel's end mark has to lie beyond every record)
      d.img = c->img.pew_img[i].get(); d.w3b = o.w3b; d.b1 = o.b1; d.b2 = o.b2; d.b3 = o.b3; d.s1 = o.s1; d.t1 = o.t1;
      d.live = (live && !(i == 1 && packb)) ? lv.live[i] : nullptr;
      if (i == 1) { d.ptab = pk_tab; d.phdr = pk_hdr; }
      d.part2 = A_alloc<float>(c, (size_t)2 * 256 * std::max(nwg[i], 1)); d.cnt2 = A_alloc<int>(c, std::max(nwg[i], 1));
      d.Fmid = o.Fmid;
    }
    w.ga = ga; w.hdr = lvblock ? lv.hdr : nullptr;
    w.do_stats = f.train ? 1 : 0;
    w.dbg = c->sw.pew_dbg;
    { if (c->sw.pew_ts) { w.ts = A_alloc<long long>(c, 128); tap(c, "pew_ts", (float*)w.ts, 256); } }
    launch_call(c, "pe_w_kernel", [&] { pew_launch(w, grid, c->stream); });
    fa = bn_fin(q.a, pm.bn2, 256, w.a.part2, q.a.s2, q.a.t2, xs, 0); fa.cnt = w.a.cnt2; fa.nblk = nwg[0]; fa.nblk_dev = lvblock ? lv.hdr + 2 : nullptr;
    fb = bn_fin(q.b, pr.bn2, 256, w.b.part2, q.b.s2, q.b.t2, xs ? xs + 513 : nullptr, 0); fb.cnt = w.b.cnt2; fb.nblk = nwg[1]; fb.nblk_dev = lvblock ? lv.hdr + 3 : nullptr;
  } else {
    launch(c, "pe_mid_kernel", pe_mid_kernel, dim3(nt), dim3(512), (size_t)PE_MID_LDS, q);
    fa = bn_fin(q.a, pm.bn2, 256, q.a.part2, q.a.s2, q.a.t2, xs, 0);
    fb = bn_fin(q.b, pr.bn2, 256, q.b.part2, q.b.s2, q.b.t2, xs ? xs + 513 : nullptr, 0);
  }
  for (int mode = dpx ? 1 : 0; mode <= (dpx ? 2 : 0); ++mode) {
    fa.sums_mode = mode; fb.sums_mode = mode;
    PeLiveP none; memset(&none, 0, sizeof(none));
    launch(c, "bn_finalize_t_kernel", bn_finalize_t_kernel, dim3(512), dim3(256), 0, fa, fb, f.train ? 1 : 0, f.bn_update ? 1 : 0, 1e-5f, none);
    if (mode == 1) dp_exchange(f, 2 * 513);
  }
  c->prof_flops = 2.0 * rows * (256.0 * 256 + 256.0 * 128);
  launch(c, "pe_out_kernel", pe_out_kernel, dim3(nt), dim3(512), (size_t)PE_OUT_LDS, q);
  *out_m = q.a.out; *out_r = q.b.out;
}

// three MLPLayer(128, 256, 160) heads -> interleaved (rows, 80, 6), one launch (heads_fused.h); bf16 mode
void heads3_fused(Fwd& f, const float* X, int ldx, int rows, int g_per, int g_stride, int g_off, const MLPLayerW heads[3], float* out) {
  Ctx* c = f.c;
  Heads3P q; memset(&q, 0, sizeof(q));
  q.X = X; q.ldx = ldx; q.rows = rows; q.gather_per = g_per; q.gather_stride = g_stride; q.gather_off = g_off; q.out = out;
  for (int i = 0; i < 3; ++i) {
    const PW &w1 = *heads[i].l0, &w2 = *heads[i].l3;
    q.w1[i] = w1.bf.get(); q.b1[i] = w1.bias; q.w2[i] = w2.bf.get(); q.b2[i] = w2.bias;
    q.lng[i] = heads[i].ln.g; q.lnb[i] = heads[i].ln.b;
  }
  c->prof_flops = 3.0 * 2.0 * rows * (128.0 * 256 + 256.0 * 160);
  launch(c, "heads3_fused_kernel", heads3_fused_kernel, dim3(24 * cdiv(cdiv(rows, HD_ROWS), 8)), dim3(512), (size_t)HD_LDS, q);      // (groups of 8 tiles x 3 heads: heads_fused.h)
}

// The policy head of a forward: cat_x_proj -> pi_head (read LIVE: the only trainable parameters) -> masked logits, then the trajectory
// heads on its q_final.  Launched on c->stream; leaves what rift_loss_backward consumes.
int head_impl(Ctx* c, const Ctx::Head& h) {
  const int nQ = h.nQ, R = h.R, M = 12;
  Fwd f; f.c = c; f.fp32 = h.fp32; f.need_traj = h.need_traj; f.train = f.drop = f.bn_update = false; f.seed = 0;
  // Everything before reads frozen, load-time-packed weights only; pi_head.* is read LIVE from here on.  A host that updates pi_head on
  // another stream (all-reduce + clip + AdamW of the previous step) hands over the event that marks the update's end.
  if (c->st.param_event && !c->dry) HIPCHK(c, hipStreamWaitEvent(c->stream, c->st.param_event, 0));
  if (h.pi_fused) {
    // cat_x_proj (bf16) -> pi_head first Linear (exact fp32, live parameters) -> LayerNorm -> ReLU -> Linear -> masked logits: one launch
    PiFwdP q; memset(&q, 0, sizeof(q));
    q.Q = h.Q; q.rows = nQ; q.rows_per_scene = R * M;
    q.wq = c->m.dec.cat_x_proj_q->bf.get(); q.bq = c->m.dec.cat_x_proj_q->bias; q.x0p = h.x0p;
    q.w1 = c->pi.w0; q.b1 = c->pi.b0;
    q.lng = c->pi.ln_g; q.lnb = c->pi.ln_b;
    q.w2 = c->pi.w3; q.b2 = c->pi.b3;
    q.r_kpm = h.r_kpm; q.M = M; q.eps = 1e-5f; q.QF = h.QF; q.Hpi = h.Hpi; q.prob = h.prob; q.nonfinite = c->nonfinite.get();
    c->prof_flops = 2.0 * nQ * (2.0 * 128 * 128 + 128);
    launch(c, "pi_forward_kernel", pi_forward_kernel, dim3(cdiv(nQ, PI_ROWS)), dim3(512), (size_t)PI_LDS, q);
  } else policy_head_layerwise(c, h);
  tap(c, "q_final", h.QF, (int64_t)nQ * 128);
  if (h.need_traj && h.heads_fused) heads3_fused(f, h.QF, 128, nQ, 0, 0, 0, c->m.dec.head, h.traj);
  else if (h.need_traj) traj_heads_layerwise(c, h);
  if (!c->dry) {
    c->last_qfinal = h.QF; c->last_hpi = h.Hpi; c->last_prob = h.prob; c->last_rkpm = h.r_kpm; c->last_bs = h.bs; c->last_R = h.R;
  }
  return RIFT_OK;
}

// ================= agent encoder (agent_encoder.py:54-96, embedding.py:62-87) =================
// ---- input-only preparation: one launch (prep_kernel) for the seven feature / mask / position builders
// (on the plan's stream: the caller's prepare stream if there is one, rift_set_prepare_stream)
int prepare_inputs(Fwd& f) {
  Ctx* c = f.c;
  const RiftFeatureBatch* B = f.B;
  const int bs = f.bs, A = f.A, Mp = f.Mp, S = f.S, T = f.T, nA = f.nA, nP = f.nP, nL = f.nL, nT = f.nT;
  (void)A_alloc<float>(c, 64);          // front padding: the level-0 NAT kernel's window loads start up to 9 floats before a sequence's first row
  f.F9 = A_alloc<float>(c, (size_t)nA * 20 * 9 + 64);
  f.valid_agent = A_alloc<uint8_t>(c, nA);
  // the fused history encoder runs on the sequences its output is read of -- valid agents other than the ego (agent_encoder.py:77-87) -- in
  // compacted order (nat_l0w.h ranks them); the layer-wise / fp32 path keeps all nA sequences
  const bool compact = f.kp.nat_compact, rank_in_prep = f.kp.rank_in_prep;
  uint8_t* hist_agent = compact ? A_alloc<uint8_t>(c, nA) : nullptr;
  f.nat_aidx = compact ? A_alloc<int>(c, nA) : nullptr;
  f.nat_cnt = compact ? A_alloc<int>(c, 4) : nullptr;
  f.F10 = A_alloc<float>(c, (size_t)nP * 20 * 10);
  f.F6 = A_alloc<float>(c, (size_t)nL * 120 * 6);
  f.kpm = A_alloc<uint8_t>(c, nT);
  f.pos = A_alloc<float>(c, (size_t)nT * 3);
  f.r_pos = A_alloc<float>(c, (size_t)nL * 3);
  f.r_kpm = A_alloc<uint8_t>(c, nL);
  f.r_tiles = A_alloc<uint8_t>(c, (size_t)std::max(nL, 1));
  PrepP q; memset(&q, 0, sizeof(q));
  q.agent_pos = B->agent_position; q.agent_head = B->agent_heading; q.agent_vel = B->agent_velocity; q.agent_shape = B->agent_shape;
  q.agent_valid = B->agent_valid_mask; q.nA = nA; q.Tfull = T; q.F9 = f.F9; q.valid_agent = f.valid_agent; q.hist_agent = hist_agent;
  q.map_pp = B->map_point_position; q.map_pv = B->map_point_vector; q.map_po = B->map_point_orientation; q.map_center = B->map_polygon_center;
  q.nPoly = nP; q.F10 = f.F10;
  q.ref_pos = B->ref_position; q.ref_vec = B->ref_vector; q.ref_ori = B->ref_orientation; q.ref_valid = B->ref_valid_mask; q.nLine = nL;
  q.F6 = f.F6; q.r_pos = f.r_pos; q.r_kpm = f.r_kpm; q.r_tiles = f.r_tiles;
  q.map_valid = B->map_valid_mask; q.static_valid = B->static_valid_mask; q.st_pos = B->static_position; q.st_head = B->static_heading;
  q.bs = bs; q.A = A; q.Mp = Mp; q.S = S; q.kpm = f.kpm; q.pos = f.pos;
  q.nb[0] = cdiv((long long)nA * 20, 256); q.nb[1] = cdiv((long long)nP * 20, 256); q.nb[2] = cdiv((long long)nL * 120, 256);
  q.nb[3] = cdiv(nL, 256); q.nb[4] = cdiv(nL, 256); q.nb[5] = cdiv(nT, 256); q.nb[6] = cdiv(nT, 256);
  int tot = 0;
  for (int i = 0; i < 7; ++i) tot += q.nb[i];
  // (round 6) the ranking as the first bs blocks of this launch (kernels.h: rank_scene_body): no launch of its own on the history chain
  if (rank_in_prep) {
    const int sl = c->parity;
    DevBuf<unsigned long long>& pub = c->slots[sl].rk_pub;
    bool fresh = false;                                // (a batch beyond the arrays of rift_ctx_create: a fresh zeroed array, epochs start over)
    if (pub.cap() < (size_t)bs) HIPCHK(c, hipDeviceSynchronize());      // nothing in flight reads the old array; and the zeros below are in place before ANY stream's launch
    DEVCHK(c, pub.reserve((size_t)bs, (size_t)std::max(2 * bs, 4096), &fresh));
    if (fresh) {
      HIPCHK(c, hipMemset(pub.get(), 0, pub.cap() * sizeof(unsigned long long)));
      HIPCHK(c, hipDeviceSynchronize());               // (hipMemset of device memory may return before the fill has run, and the preparation is launched on a non-blocking stream)
      c->slots[sl].rk_epoch = 0;
    }
    q.nrk = bs; q.rk_pub = c->slots[sl].rk_pub.get(); q.aidx = f.nat_aidx; q.cnt = f.nat_cnt; q.fail = c->nonfinite.get(); q.rk_fault = c->sw.rank_fault ? 1 : 0;
    if (!c->dry) { if (++c->slots[sl].rk_epoch == 0u) c->slots[sl].rk_epoch = 1u; }      // (epoch 0 = "never written")
    q.rk_epoch = c->slots[sl].rk_epoch;
    q.hist_agent = nullptr;                            // (the scene blocks derive the marks themselves)
    tot += bs;
  }
  launch(c, "prep_kernel", prep_kernel, dim3(tot), dim3(256), 0, q);
  if (compact && !rank_in_prep) launch(c, "nat_rank_kernel", nat_rank_kernel, dim3(1), dim3(NAT_RANK_THREADS), 0, (const uint8_t*)hist_agent, nA, f.nat_aidx, f.nat_cnt);
  return RIFT_OK;
}

void dp_kpm_fill(Fwd& f) {
  Ctx* c = f.c;
  launch(c, "dp_kpm_fill_kernel", dp_kpm_fill_kernel, dim3(cdiv(f.kb, 256)), dim3(256), 0, (const uint8_t*)f.r_kpm, f.nL, c->dp.off * f.R, f.kb, c->dp.xchg);
}

int dp_mask_and_drop_counters(Fwd& f) {
  Ctx* c = f.c;
  const int bs = f.bs, R = f.R, nA = f.nA;
  // data parallel: the r2r mask quirk indexes padding rows of the GLOBAL minibatch -> gather them (slots in the exchange buffer; the
  // first BatchNorm exchange carries them, an eval forward exchanges them on their own before the decoder)
  f.q_kpm = f.r_kpm; f.q_bs = bs; f.q_off = 0;
  if (c->dp.on) {
    f.dp = true; f.kb = c->dp.gbs * R; f.kpm_pending = true;
    f.g_rkpm = A_alloc<uint8_t>(c, (size_t)f.kb);
    if ((long long)f.kb + 2 * 513 > c->dp.len || c->dp.off < 0 || c->dp.off + bs > c->dp.gbs) { c->err = "rift_set_dp: exchange buffer too small or shard outside the global minibatch"; return RIFT_ERR_ARG; }
    if (!f.plan.dp_fill_late) dp_kpm_fill(f);      // (late: behind the history chain's hand-back, forward_impl)
    f.q_kpm = f.g_rkpm; f.q_bs = c->dp.gbs; f.q_off = c->dp.off;
  }
#if RIFT_DROP_STATS      // diagnostic build (dropstats.h): the counters of this forward's stochastic decisions, readable as taps afterwards
  if (f.drop) {
    f.ds.nmax = std::max(nA, bs * 6);
    const size_t n = (size_t)RIFT_DS_SITES * f.ds.nmax;
    f.ds.cnt = A_alloc<unsigned int>(c, n); f.ds.any = A_alloc<unsigned int>(c, n); f.ds.all = A_alloc<unsigned int>(c, n);
    f.ds.scale = A_alloc<float>(c, RIFT_DS_SITES + RIFT_DS_DEC_SITES); f.ds.elem = A_alloc<unsigned long long>(c, 2 * RIFT_DS_DEC_SITES);
    if (!c->dry) {
      HIPCHK(c, hipMemsetAsync(f.ds.cnt, 0, n * 4, c->stream)); HIPCHK(c, hipMemsetAsync(f.ds.any, 0, n * 4, c->stream));
      HIPCHK(c, hipMemsetAsync(f.ds.all, 0xff, n * 4, c->stream));
      HIPCHK(c, hipMemsetAsync(f.ds.scale, 0, (RIFT_DS_SITES + RIFT_DS_DEC_SITES) * 4, c->stream));
      HIPCHK(c, hipMemsetAsync(f.ds.elem, 0, 2 * RIFT_DS_DEC_SITES * 8, c->stream));
    }
    tap(c, "drop_cnt", (float*)f.ds.cnt, (int64_t)n); tap(c, "drop_any", (float*)f.ds.any, (int64_t)n); tap(c, "drop_all", (float*)f.ds.all, (int64_t)n);
    tap(c, "drop_scale", f.ds.scale, RIFT_DS_SITES + RIFT_DS_DEC_SITES); tap(c, "drop_elem", (float*)f.ds.elem, 4 * RIFT_DS_DEC_SITES);
    f.ds.skip = A_alloc<unsigned int>(c, 8);      // half-blocks the DropPath grouping of NAT levels 1 and 2 skipped
    if (!c->dry) HIPCHK(c, hipMemsetAsync(f.ds.skip, 0, 8 * 4, c->stream));
    tap(c, "nat_skip", (float*)f.ds.skip, 8);
  }
#endif
  if (f.kp.nat_compact) { tap(c, "nat_aidx", (float*)f.nat_aidx, nA); tap(c, "nat_cnt", (float*)f.nat_cnt, 3); }      // (int32 words read back through the float tap)
  tap(c, "nat_f9", f.F9, (int64_t)nA * 20 * 9);      // the prepared 9-channel rows, all nA slots (prep_kernel)
  return RIFT_OK;
}

// ---- agent-history chain: the three NAT levels (one launch each, or layer-wise) and the FPN tail
void history_encoder(Fwd& f) {
  Ctx* c = f.c;
  const auto& he = c->m.agent;
  const int nA = f.nA;
  static const int Kl[3] = {3, 3, 5};
  float* Oc[3];   // LayerNorm(norm_i) of the last 3 steps of level i: all that out[:, :, -1] of the FPN depends on
  for (int i = 0; i < 3; ++i) Oc[i] = A_alloc<float>(c, (size_t)nA * 3 * NAT_C[i]);
  // the wave-private level kernels hand these rows to fpn_tail_kernel as bf16 (it rounds them to bf16 first thing anyway): same values, half the bytes
  const bool oc_bf16 = f.kp.fpn_fused;
  unsigned short* Ocb[3] = {nullptr, nullptr, nullptr};
  if (oc_bf16) for (int i = 0; i < 3; ++i) Ocb[i] = A_alloc<unsigned short>(c, (size_t)nA * 3 * NAT_C[i]);
  if (f.kp.hist_wave) {
    // one launch per level: [ConvTokenizer ->] 2 NAT blocks -> {FPN LayerNorm of the last 3 steps, downsample conv + LN}
    float* Xin[3] = {nullptr, A_alloc<float>(c, (size_t)nA * 10 * 64), A_alloc<float>(c, (size_t)nA * 5 * 128)};
    // DropPath grouping: the two lists block 0 of level 0's launch makes for levels 1 and 2 (nat_l0w.h: nat_group_body), -1 = no sequence
    const bool group = f.kp.nat_group;
    const int cap1 = 4 * cdiv(nA + 2, 4), cap2 = 3 * cdiv(nA, 3);
    int* perm1 = group ? A_alloc<int>(c, cap1) : nullptr;
    int* perm2 = group ? A_alloc<int>(c, cap2) : nullptr;
    if (group) { tap(c, "nat_perm1", (float*)perm1, cap1); tap(c, "nat_perm2", (float*)perm2, cap2); }      // (int32 words read back through the float tap)
    for (int lv = 0; lv < 3; ++lv) {
      const int C = NAT_C[lv], ksz = Kl[lv], L = NAT_L[lv], rows = nA * L;
      if (lv == 0) {   // level 0 as wave-private, register-resident tiles (no workgroup barriers): nat_l0w.h
        NatL0WP q; memset(&q, 0, sizeof(q));
        q.aidx = f.nat_aidx; q.cnt = f.nat_cnt;
        q.F9 = f.F9; q.nseq = nA; q.img = c->img.l0w_img.get(); q.par = c->img.l0w_par.get(); q.Oc = Oc[0]; q.Ocb = Ocb[0]; q.Xnext = Xin[1];
        { if (c->sw.nat_ts == 1) { q.ts = A_alloc<long long>(c, 64); tap(c, "nat_ts", (float*)q.ts, 128); } }
        q.droppath[0] = f.drop ? NAT_DPR[0] : 0.f; q.droppath[1] = f.drop ? NAT_DPR[1] : 0.f; q.seed = f.seed; q.stream = f.next_stream(); f.stream_id += 4;
        q.ds = f.ds;
        if (group) {      // (levels 1 and 2 take the next two stream numbers: four each)
          q.perm1 = perm1; q.perm2 = perm2; q.cap1 = cap1; q.cap2 = cap2; q.gstream[0] = q.stream + 5; q.gstream[1] = q.stream + 10;
          for (int i = 0; i < 4; ++i) q.gdpr[i] = NAT_DPR[2 + i];
        }
        c->prof_flops = 2.0 * rows * (20.0 * C * C + 4.0 * ksz * C) + 2.0 * rows * 27 * 32 + (rows / 2) * 2.0 * 3 * C * 2 * C;
        // (grouped: one block more, the lists', inside the same bound on the launch's workgroups)
        { const int g0 = std::min(cdiv(cdiv(nA, 4), L0W_NWV), std::max(c->sw.nat_grid - (group ? 1 : 0), 1)) + (group ? 1 : 0); launch_call(c, "nat_l0w_kernel", [&] { l0w_launch(q, g0, c->stream); }); }
        continue;
      }
      if (lv == 1) {   // level 1 likewise (weights swapped through LDS between the two layers): nat_l1w.h
        NatL1WP q; memset(&q, 0, sizeof(q));
        q.cnt = f.nat_cnt; q.perm = perm1;
        q.X = Xin[1]; q.nseq = nA; q.img = c->img.l1w_img.get(); q.par = c->img.l1w_par.get(); q.Oc = Oc[1]; q.Ocb = Ocb[1]; q.Xnext = Xin[2];
        q.droppath[0] = f.drop ? NAT_DPR[2] : 0.f; q.droppath[1] = f.drop ? NAT_DPR[3] : 0.f; q.seed = f.seed; q.stream = f.next_stream(); f.stream_id += 4;
        q.ds = f.ds;
        c->prof_flops = 2.0 * rows * (20.0 * C * C + 4.0 * ksz * C) + (rows / 2) * 2.0 * 3 * C * 2 * C;
        { const int g1 = std::min(cdiv(cdiv(nA, 4), L1W_NWV), c->sw.nat_grid); launch_call(c, "nat_l1w_kernel", [&] { l1w_launch(q, g1, c->stream); }); }
        continue;
      }
      {   // level 2: wave-private tiles of 3 agents, the two layers' weights streamed through LDS (nat_l2w.h)
        NatL2WP q; memset(&q, 0, sizeof(q));
        q.cnt = f.nat_cnt; q.perm = perm2;
        q.X = Xin[2]; q.nseq = nA; q.img = c->img.l2w_img.get(); q.par = c->img.l2w_par.get(); q.Oc = Oc[2]; q.Ocb = Ocb[2];
        q.droppath[0] = f.drop ? NAT_DPR[4] : 0.f; q.droppath[1] = f.drop ? NAT_DPR[5] : 0.f; q.seed = f.seed; q.stream = f.next_stream(); f.stream_id += 4;
        q.ds = f.ds;
        { if (c->sw.nat_ts == 3) { q.ts = A_alloc<long long>(c, 64); tap(c, "nat_ts", (float*)q.ts, 128); } }
        c->prof_flops = 2.0 * rows * (20.0 * C * C + 4.0 * ksz * C);
        // (round 6: up to one tile per workgroup -- a launch that does not fill the chip deals its tiles wave-major and waves without a tile skip
        // the arithmetic, so a small batch runs two or three waves on each of many CUs instead of eight on a few; nat_l2w.hip)
        const int l2grid = std::min(cdiv(nA, 3), c->sw.nat_grid);
        launch_call(c, "nat_l2w_kernel", [&] { l2w_launch(q, l2grid, c->stream); });
        continue;
      }
    }
    // level boundaries of the fused path, rows in the launch's own (compacted) order: the downsampled inputs of levels 1 and 2
    tap(c, "nat_x1", Xin[1], (int64_t)nA * 10 * 64); tap(c, "nat_x2", Xin[2], (int64_t)nA * 5 * 128);
  } else history_levels_layerwise(f, Oc);
  // the FPN inputs (LayerNorm of the last three steps of level i): as the 16-bit operand words the fused tail receives (two per float of
  // the tap, in the launch's compacted order), else fp32 rows of all nA slots
  static const char* const oc_tap[3] = {"nat_oc0", "nat_oc1", "nat_oc2"};
  for (int i = 0; i < 3; ++i) {
    if (oc_bf16) tap(c, oc_tap[i], (float*)Ocb[i], (int64_t)nA * 3 * NAT_C[i] / 2);
    else tap(c, oc_tap[i], Oc[i], (int64_t)nA * 3 * NAT_C[i]);
  }
  // FPN restricted to what out[:, :, -1] depends on
  f.nat_out = A_alloc<float>(c, (size_t)nA * 128);
  if (f.kp.fpn_fused) {
    FpnP q; memset(&q, 0, sizeof(q));
    for (int i = 0; i < 3; ++i) {
      const PW& w = *he.levels[i].lateral;
      q.oc[i] = Oc[i]; q.ocb[i] = Ocb[i]; q.wl[i] = w.bf.get(); q.bl[i] = w.bias;
    }
    q.wf = he.fpn_last->bf.get(); q.bf_ = he.fpn_last->bias;
    q.out = f.nat_out; q.nA = nA; q.cnt = f.nat_cnt; q.aidx = f.nat_aidx;
    c->prof_flops = 2.0 * nA * (2.0 * 128 * (96 + 192 + 384) + 256.0 * 128);
    launch(c, "fpn_tail_kernel", fpn_tail_kernel, dim3(cdiv(nA, FPN_AG)), dim3(512), (size_t)FPN_LDS, q);
  } else fpn_layerwise(f, Oc);
  tap(c, "nat_out", f.nat_out, (int64_t)nA * 128);
}

// ego state token (StateAttentionEncoder, agent_encoder.py:99-140)
void ego_token(Fwd& f) {
  Ctx* c = f.c;
  const RiftFeatureBatch* B = f.B;
  const int bs = f.bs;
  const auto& eg = c->m.agent.ego;
  bool fill_eq;
  float* eq = wconst_get(c, c->wc.ego_q, 128, f.fp32, &fill_eq);
  if (fill_eq) gemm(c, mk(eg.query, 128, 1, *eg.q, eq, 128), *eg.q, f.fp32);
  f.x_ego = A_alloc<float>(c, (size_t)bs * 128);
  if (f.kp.ego_fused) {
    EgoP q; memset(&q, 0, sizeof(q));
    q.cs = B->current_state; q.cs_ld = B->cs_ld; q.lw = c->img.ego_w.get(); q.lb = c->img.ego_b.get(); q.pos = eg.pos_embed;
    q.wkv = eg.kv->bf.get(); q.bkv = eg.kv->bias; q.q = eq;
    q.wo = eg.out_proj->bf.get(); q.bo = eg.out_proj->bias;
    q.out = f.x_ego; q.bs = bs; q.drop_p = f.drop ? 0.75f : 0.f; q.seed = f.seed; q.stream = f.drop ? f.next_stream() : 0;
    q.ds = f.ds;
    c->prof_flops = 2.0 * bs * (6.0 * 128 * 256 + 128.0 * 128);
    launch(c, "ego_fused_kernel", ego_fused_kernel, dim3(bs), dim3(256), 0, q);
  } else ego_token_layerwise(f, eq);
  tap(c, "x_ego", f.x_ego, (int64_t)bs * 128);
}

// decoder queries q0 = q_proj(cat[r_emb, m_emb]) (planning_decoder.py:149-154): they depend on the reference-line embedding only, so with the fused
// embeddings done they are launched here, ahead of the join, and run beside the tail of the agent-history chain instead of between encoder and decoder
int build_q0(Fwd& f) {
  Ctx* c = f.c;
  const auto& pd = c->m.dec;
  const int M = f.M, nL = f.nL, nQ = f.nQ;
  bool fill;
  float* Mb = wconst_get(c, c->wc.Mb, (size_t)M * 128, f.fp32, &fill);
  if (fill) gemm(c, mk(pd.m_emb, 128, M, *pd.q_proj_m, Mb, 128), *pd.q_proj_m, f.fp32);
  f.Q = A_alloc<float>(c, (size_t)nQ * 128);
  if (f.kp.pi_fused) {
    Q0P q; memset(&q, 0, sizeof(q));
    q.r_emb = f.r_emb; q.nL = nL; q.M = M; q.wr = pd.q_proj_r->bf.get(); q.br = pd.q_proj_r->bias;
    q.Mb = Mb; q.Q = f.Q;
    c->prof_flops = 2.0 * nL * 128.0 * 128;
    launch(c, "q0_fused_kernel", q0_fused_kernel, dim3(cdiv(nL, 16)), dim3(256), 0, q);
  } else build_q0_layerwise(f, Mb);
  return RIFT_OK;
}

// ---- map chain: both PointsEncoders, the three Fourier embeddings, the decoder queries
int map_and_embeddings(Fwd& f) {
  Ctx* c = f.c;
  const RiftFeatureBatch* B = f.B;
  const int nP = f.nP, nL = f.nL, nT = f.nT;
  // map encoder (map_encoder.py:31-93)
  // reference-line features are input-only too: both PointsEncoders run side by side (fused path)
  if (f.kp.pe != PE_LAYERWISE) points_encoder_pair(f, f.F10, nP, B->map_valid_mask, c->m.map.polygon_encoder, f.F6, nL, B->ref_valid_mask, c->m.dec.r_encoder, &f.poly, &f.r_emb);
  else f.poly = points_encoder_layerwise(f, f.F10, 10, nP, 20, B->map_valid_mask, c->m.map.polygon_encoder);
  tap(c, "poly_pe", f.poly, (int64_t)nP * 128);
  // the three Fourier embeddings (token positions, speed limits, reference-line positions) depend on inputs only: with both
  // PointsEncoders done they run as ONE launch, and the token kernels add the positional embedding on the way
  if (f.kp.fourier == FO_THREE || f.kp.fourier == FO_THREE_W) {
    tap(c, "r_pe", f.r_emb, (int64_t)nL * 128);
    FourierP3 q3; memset(&q3, 0, sizeof(q3));
    q3.e[0] = fourier_desc(f, f.pos, 3, nT, c->m.pos_emb, 2, false, nullptr);
    q3.e[1] = fourier_desc(f, B->map_polygon_speed_limit, 1, nP, c->m.map.speed_limit_emb, -1, false, nullptr);
    q3.e[2] = fourier_desc(f, f.r_pos, 3, nL, c->m.dec.r_pos_emb, -1, true, f.r_emb);
    q3.nblk[0] = cdiv(nT, FO_ROWS); q3.nblk[1] = cdiv(nP, FO_ROWS); q3.nblk[2] = cdiv(nL, FO_ROWS); q3.count = 3;
    c->prof_flops = 2.0 * 128.0 * ((nT + nL) * (3 * 257.0 + 128.0) + nP * (257.0 + 128.0));
    if (f.kp.fourier == FO_THREE_W) {          // wave-private form: one 16-row tile per wave, 8 tiles per pass, the one-dimensional embedding two passes per workgroup
      FoWP w; memset(&w, 0, sizeof(w));
      w.count = 3;
      for (int i = 0; i < 3; ++i) {
        const FourierP& o = q3.e[i]; FoWSide& d = w.e[i];
        d.in = o.in; d.in_ld = o.in_ld; d.rows = o.rows; d.D = o.D; d.wrap_dim = o.wrap_dim; d.img = c->img.fow_img[i].get(); d.par = c->img.fow_par[i].get();
        d.Y = o.Y; d.accumulate = o.accumulate; d.rep = o.D == 1 ? 2 : 1; d.nwg = cdiv(cdiv(o.rows, 16), 8 * d.rep);
      }
      launch_call(c, "fo_w_kernel", [&] { fow_launch(w, c->stream); });
    } else
    launch(c, "fourier_fused_kernel", fourier_fused_kernel, dim3(q3.nblk[0] + q3.nblk[1] + q3.nblk[2]), dim3(256), (size_t)FO_LDS, q3);
    f.PEtok = q3.e[0].Y; f.speed_emb = q3.e[1].Y;
    tap(c, "fo_pos", f.PEtok, (int64_t)nT * 128);
  } else {
    f.speed_emb = fourier(f, B->map_polygon_speed_limit, 1, nP, c->m.map.speed_limit_emb, -1);
  }
  tap(c, "fo_speed", f.speed_emb, (int64_t)nP * 128);
  if (f.kp.q0_early) TRY(build_q0(f));      // ahead of the join
  return RIFT_OK;
}

// ================= tokens =================
void assemble_tokens(Fwd& f) {
  Ctx* c = f.c;
  const RiftFeatureBatch* B = f.B;
  const int bs = f.bs, A = f.A, Mp = f.Mp, S = f.S, N = f.N, nA = f.nA, nP = f.nP, nT = f.nT;
  f.X = A_alloc<float>(c, (size_t)nT * 128);
  TokenP q; memset(&q, 0, sizeof(q));
  q.nat = f.nat_out; q.x_ego = f.x_ego; q.valid_agent = (const uint8_t*)f.valid_agent; q.category = B->agent_category; q.a_type_emb = c->m.agent.type_emb;
  q.pooled = f.poly; q.ptype = B->map_polygon_type; q.on_route = B->map_polygon_on_route; q.tl = B->map_polygon_tl_status; q.has_sl = B->map_polygon_has_speed_limit;
  q.speed_emb = f.speed_emb; q.p_type_emb = c->m.map.type_emb; q.route_emb = c->m.map.on_route_emb;
  q.tl_emb = c->m.map.traffic_light_emb; q.unk_emb = c->m.map.unknown_speed_emb;
  q.bs = bs; q.A = A; q.Mp = Mp; q.N = N; q.X = f.X; q.pe = f.PEtok;
  q.nblk_a = cdiv((long long)nA * 32, 256);
  launch(c, "token_kernel", token_kernel, dim3(q.nblk_a + cdiv((long long)nP * 32, 256)), dim3(256), 0, q);
  if (S > 0) {
    float* semb = fourier(f, B->static_shape, 2, bs * S, c->m.stat.obj_encoder, -1);
    tap(c, "fo_static", semb, (int64_t)bs * S * 128);
    launch(c, "static_token_kernel", static_token_kernel, dim3(cdiv((long long)bs * S * 128, 256)), dim3(256), 0, (const float*)semb, B->static_category,
           B->static_valid_mask, c->m.stat.type_emb, bs, A, Mp, S, N, f.X);
  }
  if (f.kp.fourier != FO_THREE && f.kp.fourier != FO_THREE_W) fourier(f, f.pos, 3, nT, c->m.pos_emb, 2, true, f.X);      // (else token_kernel added it on the way)
  tap(c, "x_tokens", f.X, (int64_t)nT * 128);
}

// ================= encoder blocks (transformer.py:73-94) =================
void scene_encoder(Fwd& f) {
  Ctx* c = f.c;
  const int bs = f.bs, N = f.N, nT = f.nT;
  f.ENC = A_alloc<float>(c, (size_t)nT * 128);
  const bool wide = f.kp.enc == ENC_FUSED112;      // the fused kernel on its 112-row layout (enc_fused.h: EncLay<112>)
  if (f.kp.enc == ENC_FUSED96 || wide) {
    EncFusedP ep; memset(&ep, 0, sizeof(ep));
    ep.X = f.X; ep.Y = f.ENC; ep.kpm = f.kpm; ep.bs = bs; ep.N = N; ep.seed = f.seed; ep.stream = f.next_stream(); f.stream_id += 8;
    for (int i = 0; i < 4; ++i) {
      const SceneBlockW& p = c->m.encoder_blocks[i];
      EncBlockW& w = ep.blk[i];
      w.ln1_g = p.norm1.g; w.ln1_b = p.norm1.b;
      w.ln2_g = p.norm2.g; w.ln2_b = p.norm2.b;
      w.wqkv = c->img.enc_wqkv[i].get(); w.bqkv = c->img.enc_bqkv[i].get();
      w.wo = p.out_proj->bf.get(); w.bo = p.out_proj->bias;
      w.w1 = p.fc1->bf.get(); w.b1 = p.fc1->bias;
      w.w2 = p.fc2->hid.get(); w.b2 = p.fc2->bias;      // (hidden-layer operand words: pack_hid)
      w.droppath = f.drop ? ENC_DPR[i] : 0.f;
    }
    ep.norm_g = c->m.norm.g; ep.norm_b = c->m.norm.b; ep.nonfinite = c->nonfinite.get();
    ep.ds = f.ds; ep.dbg = c->sw.no_skip ? 1 : 0;
    if (c->sw.enc_ts) { ep.ts = A_alloc<long long>(c, 256); tap(c, "enc_ts", (float*)ep.ts, 512); }
    c->prof_flops = 4.0 * bs * N * (2.0 * 128 * 384 + 4.0 * N * 128 + 2.0 * 128 * 128 + 4.0 * 128 * 512);
    if (f.kp.enc_image != IMG_NONE) {   // the decoder kernel will run: emit its cross-attention K | V operand fragments here
      f.enc_KT = A_alloc<unsigned short>(c, (size_t)bs * 4 * (f.kp.enc_image == IMG_DENSE ? 96 : DECW_KV_FRAGS) * 512);      // (dense: the per-head image, dec_kv.h)
      ep.wkv = c->m.dec.kv_all->bf.get(); ep.bkv = c->m.dec.kv_all->bias;
      ep.KT = f.enc_KT;
      f.kpm_c = A_alloc<uint8_t>(c, (size_t)bs * (wide ? 112 : 96)); ep.kpm_c = f.kpm_c;
      f.enc_x0p = A_alloc<float>(c, (size_t)bs * 128);
      ep.wx0 = c->m.dec.cat_x_proj_x->bf.get(); ep.x0p = f.enc_x0p;
      c->prof_flops += 2.0 * bs * N * 128.0 * 1024;
    }
    if (wide) launch_call(c, "enc_fused112_kernel", [&] { enc112_launch(ep, c->stream); });
    else launch(c, "enc_fused_kernel", enc_fused_kernel<ENC_NW>, dim3(bs), dim3(64 * ENC_NW), (size_t)RIFT_ENC_LDS_BYTES, ep);
  } else if (f.kp.enc == ENC_W) {   // dense-traffic shapes: the wave-private, weight-streaming encoder (two passes per layer)
    EncWP eq; memset(&eq, 0, sizeof(eq));
    eq.X = f.X; eq.Y = f.ENC; eq.kpm = f.kpm; eq.bs = bs; eq.N = N; eq.seed = f.seed; eq.stream = f.next_stream(); f.stream_id += 8;
    eq.KVs = A_alloc<unsigned short>(c, (size_t)bs * 96 * 512);
    eq.img = c->img.encw_img.get(); eq.par = c->img.encw_par.get(); eq.nonfinite = c->nonfinite.get();
    if (f.kp.enc_image == IMG_DENSE) { f.enc_KT = A_alloc<unsigned short>(c, (size_t)bs * 4 * 96 * 512); eq.DKV = f.enc_KT; }   // the decoder's (dense-variant) operands
    for (int i = 0; i < 4; ++i) eq.droppath[i] = f.drop ? ENC_DPR[i] : 0.f;
    eq.ds = f.ds;
    c->prof_flops = 4.0 * bs * N * (2.0 * 128 * 384 + 4.0 * N * 128 + 2.0 * 128 * 128 + 4.0 * 128 * 512);
    launch_call(c, "enc_w_kernel", [&] { encw_launch(eq, c->stream); });
  } else scene_encoder_layerwise(f);
  tap(c, "enc_out", f.ENC, (int64_t)nT * 128);
}

// ================= agent predictor (agent_predictor.py:17-29) =================
void agent_predictor(Fwd& f) {
  Ctx* c = f.c;
  const RiftOutputs* out = f.out;
  const int bs = f.bs, A = f.A, N = f.N;
  if (f.need_traj && out->prediction && A > 1) {
    const int rows = bs * (A - 1);
    if (f.kp.heads_fused) heads3_fused(f, f.ENC, 128, rows, A - 1, N, 1, c->m.predictor, out->prediction);
    else agent_predictor_layerwise(f, rows);
  }
}

// ================= planning decoder (planning_decoder.py:135-188) =================
int planning_decoder(Fwd& f) {
  Ctx* c = f.c;
  const RiftFeatureBatch* B = f.B;
  const KernelPlan& kp = f.kp;
  const int bs = f.bs, R = f.R, N = f.N, M = f.M, nL = f.nL, nQ = f.nQ;
  if (kp.pe == PE_LAYERWISE) f.r_emb = points_encoder_layerwise(f, f.F6, 6, nL, 120, B->ref_valid_mask, c->m.dec.r_encoder);
  if (kp.fourier != FO_THREE && kp.fourier != FO_THREE_W) {
    tap(c, "r_pe", f.r_emb, (int64_t)nL * 128);
    fourier(f, f.r_pos, 3, nL, c->m.dec.r_pos_emb, -1, true, f.r_emb);
  }
  tap(c, "r_emb", f.r_emb, (int64_t)nL * 128);
  if (!kp.q0_early) TRY(build_q0(f));
  tap(c, "q0", f.Q, (int64_t)nQ * 128);

  f.dec_deferred = false; memset(&f.dec_later, 0, sizeof(f.dec_later));
  dp_exchange(f, 0);                      // (eval forward under data parallelism: the mask slots have not travelled yet)
  const float dp = f.drop ? 0.1f : 0.f;   // pluto_model.py:35,93
  if (kp.dec_kv_frag) {   // the dense variant's K | V^T operand fragments from the output of an encoder that emitted none
    f.enc_KT = A_alloc<unsigned short>(c, (size_t)bs * 4 * 96 * 512);
    DecKvP kq; memset(&kq, 0, sizeof(kq));
    kq.ENC = f.ENC; kq.bs = bs; kq.N = N; kq.wkv = c->m.dec.kv_all->bf.get(); kq.bkv = c->m.dec.kv_all->bias; kq.KV = f.enc_KT;
    c->prof_flops = 2.0 * bs * N * 128.0 * 1024;
    launch(c, "dec_kv_frag_kernel", dec_kv_frag_kernel, dim3(bs), dim3(512), (size_t)DEC_KV_LDS, kq);
  }
  if (kp.dec != DEC_LAYERWISE) {
    DecWP dq; memset(&dq, 0, sizeof(dq));
    dq.Q = f.Q; dq.kpm = f.kpm; dq.r_kpm = f.r_kpm; dq.q_kpm = f.q_kpm; dq.q_bs = f.q_bs; dq.q_off = f.q_off; dq.bs = bs; dq.N = N; dq.R = R; dq.dropout = dp; dq.seed = f.seed;
    if (kp.enc_kpm_x0p) { dq.kpm = f.kpm_c; dq.N = kp.enc == ENC_FUSED112 ? 112 : 96; dq.compact = 1; }      // (the encoder compacted its rows: its own key padding, valid keys a prefix)
    dq.stream = f.next_stream(); f.stream_id += 64;
    dq.KV = f.enc_KT; dq.img = c->img.decw_img.get(); dq.par = c->img.decw_par.get(); dq.nonfinite = c->nonfinite.get();
    dq.ds = f.ds;
    if (c->sw.dec_ts) { dq.ts = A_alloc<long long>(c, 1024); tap(c, "dec_ts", (float*)dq.ts, 2048); }      // [0, 128): boundaries of wave 0; [128 + 112 w, ...): arrivals of wave w
    dq.dbg = c->sw.dec_dbg | (c->sw.no_skip ? 64 : 0);
    dq.prob_only = f.need_traj ? 0 : 1;      // no trajectory heads: the policy head and the objectives mask the rows of padded reference lines, nobody else reads them
    c->prof_flops = 4.0 * bs * (R * M) * (2.0 * 128 * (384 + 128) * 2 + 2.0 * 128 * 128 * 2 + 4.0 * 128 * 512 + 4.0 * 128 * (N + R + M));
    // which layers run here and which with the deferred head: the plan's (fwd_kernels.h).  The rows travel through Q between two launches;
    // the dropout streams of a deferred second half carry on from the states the first one leaves (rng_io): the draws are a single launch's
    dq.rng_io = kp.dec_split ? A_alloc<uint32_t>(c, (size_t)bs * 512 * 4) : nullptr;
    for (int i = 0; i < kp.dec_n_now; ++i) {
      dq.l0 = kp.dec_now[i].l0; dq.l1 = kp.dec_now[i].l1;
      launch_call(c, "dec_w_kernel", [&] { decw_launch(dq, c->stream); });
    }
    f.dec_deferred = kp.dec_defer;
    if (kp.dec_defer) { f.dec_later = dq; f.dec_later.l0 = kp.dec_later.l0; f.dec_later.l1 = kp.dec_later.l1; }
  } else decoder_layerwise(f, dp);
  tap(c, "dec3", f.Q, (int64_t)nQ * 128);
  return RIFT_OK;
}

// ================= policy head, hidden_proj / ref_free_decoder =================
int policy_and_ego_heads(Fwd& f) {
  Ctx* c = f.c;
  const RiftOutputs* out = f.out;
  const int flags = f.flags;
  const int bs = f.bs, R = f.R, N = f.N, nQ = f.nQ;
  // cat_x_proj(cat[q, enc_emb[:, 0]]) (planning_decoder.py:177-179): ego-token part is a per-scene bias
  float* x0p = f.enc_x0p;
  if (!f.kp.enc_kpm_x0p) {      // (the encoder's tail did not emit it)
    x0p = A_alloc<float>(c, (size_t)bs * 128);
    gemm(c, mk(f.ENC, N * 128, bs, *c->m.dec.cat_x_proj_x, x0p, 128), *c->m.dec.cat_x_proj_x, f.fp32);
  }
  // ---- the policy head (and the trajectory heads that read its q_final): right here, or -- RIFT_F_DEFER_HEAD -- later through
  // rift_forward_head on a stream of the caller's choice, so that it (and the loss / backward / update behind it) runs beside the next
  // forward's frozen trunk
  Ctx::Head hs;
  hs.valid = true; hs.fp32 = f.fp32; hs.need_traj = f.kp.head_traj; hs.pi_fused = f.kp.pi_fused; hs.heads_fused = f.kp.heads_fused; hs.Q = f.Q; hs.x0p = x0p; hs.r_kpm = f.r_kpm;
  hs.bs = bs; hs.R = R; hs.nQ = nQ; hs.traj = out->trajectory;
  hs.QF = A_alloc<float>(c, (size_t)nQ * 128);
  hs.Hpi = A_alloc<float>(c, (size_t)nQ * 128);
  hs.prob = out->probability ? out->probability : A_alloc<float>(c, nQ);
  if (hs.need_traj && !hs.heads_fused) traj_heads_reserve(c, hs);      // layer-wise trajectory heads: their buffers come out of this forward's arena
  hs.dec_pending = f.dec_deferred; hs.dec = f.dec_later;
  if (flags & RIFT_F_DEFER_HEAD) { if (!c->dry) c->slots[c->parity].head = hs; }
  else TRY(head_impl(c, hs));
  // hidden_proj / ref_free_decoder on the ego token (pluto_model.py:173-180)
  if (!f.kp.heads_fused) ego_heads_layerwise(f);
  else if (out->hidden || (f.need_traj && out->ref_free_trajectory)) {      // one launch (heads_fused.h: ego_heads_kernel)
    const PW &h0 = *c->m.hidden_proj0, &h2 = *c->m.hidden_proj2, &r0 = *c->m.ref_free_decoder.l0, &r3 = *c->m.ref_free_decoder.l3;
    EgoHeadsP q; memset(&q, 0, sizeof(q));
    q.X = f.ENC; q.ldx = N * 128; q.rows = bs;
    q.wh0 = h0.bf.get(); q.wh2 = h2.bf.get(); q.wr0 = r0.bf.get(); q.wr3 = r3.bf.get();
    q.bh0 = h0.bias; q.bh2 = h2.bias; q.br0 = r0.bias; q.br3 = r3.bias;
    q.lng = c->m.ref_free_decoder.ln.g; q.lnb = c->m.ref_free_decoder.ln.b;
    q.hidden = out->hidden; q.ref = (f.need_traj && out->ref_free_trajectory) ? out->ref_free_trajectory : nullptr;
    c->prof_flops = 2.0 * bs * (2.0 * 128 * 128 + 128.0 * 256 + 256.0 * 320);
    launch(c, "ego_heads_kernel", ego_heads_kernel, dim3(cdiv(bs, 16)), dim3(256), 0, q);
  }
  return RIFT_OK;
}

// The streams and events the plan needs, made on first use.
int plan_resources(Ctx* c, const StreamPlan& p) {
  if (p.prefetched && !c->st.ev_prep) HIPCHK(c, hipEventCreateWithFlags(&c->st.ev_prep, hipEventDisableTiming));
  if (p.forked && !c->st.side) { HIPCHK(c, hipStreamCreateWithFlags(&c->st.side, hipStreamNonBlocking)); c->st.side_owned = true; }
  if (p.forked && !c->st.ev_fork) { HIPCHK(c, hipEventCreateWithFlags(&c->st.ev_fork, hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&c->st.ev_join, hipEventDisableTiming)); }
  if (p.nat_aside && !c->st.ev_join2) HIPCHK(c, hipEventCreateWithFlags(&c->st.ev_join2, hipEventDisableTiming));
  return RIFT_OK;
}

// What the kernel plan may depend on (fwd_kernels.h), but for `forked`, which forward_impl takes from the stream plan.
KernelIn kernel_in(const Ctx* c, const RiftFeatureBatch* B, const RiftOutputs* out, int flags) {
  const Ctx::Switches& sw = c->sw;
  KernelIn in;
  in.nat_fused = sw.nat_fused; in.dec_fused = sw.dec_fused; in.enc_fused = sw.enc_fused; in.pe_fused = sw.pe_fused; in.fo_fused = sw.fo_fused;
  in.fpn_fused = sw.fpn_fused; in.ego_fused = sw.ego_fused; in.heads_fused = sw.heads_fused; in.pi_fused = sw.pi_fused;
  in.fo_w = sw.fo_w; in.pe_w = sw.pe_w; in.nat_compact = sw.nat_compact; in.pe_live = sw.pe_live; in.pe_pack = sw.pe_pack;
  in.rank_in_prep = sw.rank_in_prep; in.enc112 = sw.enc112; in.nat_group = sw.nat_group; in.no_skip = sw.no_skip;
  in.dec_defer_max = sw.dec_defer_max; in.dec_split = sw.dec_split; in.dec_layers = sw.dec_layers; in.dec_ts = sw.dec_ts != 0;
  in.fp32 = (flags & RIFT_F_FP32) != 0; in.train = (flags & RIFT_F_TRAIN) != 0; in.drop = in.train && !(flags & RIFT_F_NO_DROP);
  in.need_traj = (flags & RIFT_F_NEED_TRAJ) != 0; in.want_traj = out->trajectory != nullptr;
  in.defer_head = (flags & RIFT_F_DEFER_HEAD) != 0; in.prof_on = c->prof_on;
  in.forked = false;
  in.bs = B->bs; in.A = B->A; in.Mp = B->Mp; in.S = B->S; in.R = B->R; in.enc_nw = ENC_NW;
  return in;
}

PlanIn plan_in(const Ctx* c, const KernelIn& k) {
  PlanIn in;
  in.two_streams = c->sw.two_streams; in.nat_fused = plan_hist_wave(k); in.nat_aside = c->sw.nat_aside; in.side_gate = c->sw.side_gate;
  in.fp32 = k.fp32; in.prof_on = k.prof_on; in.dry = c->dry; in.prep_set = c->st.prep_set; in.dp_on = c->dp.on; in.bs = k.bs;
  return in;
}

// One forward on c->stream (the caller's), in the arena of c->parity; with c->dry set, the sizing pass: the same stages under the same
// kernel plan, so the same allocations, and no launch (rift_forward checks the two passes' arena use against each other).  The
// stages switch c->stream by the plan (fwd_plan.h) and an early error return leaves it switched: rift_forward restores it.
int forward_impl(Ctx* c, const RiftFeatureBatch* B, const RiftOutputs* out, int flags, uint32_t seed) {
  Fwd f;
  f.c = c; f.train = (flags & RIFT_F_TRAIN) != 0; f.drop = f.train && !(flags & RIFT_F_NO_DROP);
  f.fp32 = (flags & RIFT_F_FP32) != 0; f.need_traj = (flags & RIFT_F_NEED_TRAJ) != 0;
  f.bn_update = f.train && !(flags & RIFT_F_NO_BN_UPDATE); f.seed = seed;
  f.B = B; f.out = out; f.flags = flags;
  f.bs = B->bs; f.A = B->A; f.Mp = B->Mp; f.R = B->R; f.S = B->S; f.T = B->T;
  f.N = f.A + f.Mp + f.S;
  f.nA = f.bs * f.A; f.nP = f.bs * f.Mp; f.nL = f.bs * f.R; f.nQ = f.nL * f.M; f.nT = f.bs * f.N;
  KernelIn kin = kernel_in(c, B, out, flags);
  PlanIn pin = plan_in(c, kin);
  const StreamPlan& p = f.plan = plan_streams(pin);
  TRY(plan_resources(c, p));
  pin.dry = false; kin.forked = plan_streams(pin).forked;      // (the launch pass's streams: the sizing pass forks nothing, and gets the same kernel plan)
  f.kp = plan_kernels(kin);
  f.on[ON_CALLER] = c->stream; f.on[ON_PREPARE] = c->st.prep_stream; f.on[ON_SIDE] = c->st.side;

  c->stream = f.on[p.prep_on];
  TRY(prepare_inputs(f));
  c->stream = f.on[ON_CALLER];
  if (p.prefetched) HIPCHK(c, hipEventRecord(c->st.ev_prep, f.on[ON_PREPARE]));
  if (p.main_waits_prep) HIPCHK(c, hipStreamWaitEvent(f.on[ON_CALLER], c->st.ev_prep, 0));
  TRY(dp_mask_and_drop_counters(f));
  if (p.side_waits_prep) HIPCHK(c, hipStreamWaitEvent(f.on[ON_SIDE], c->st.ev_prep, 0));
  if (p.fork_from_main) {
    HIPCHK(c, hipEventRecord(c->st.ev_fork, f.on[ON_CALLER]));
    HIPCHK(c, hipStreamWaitEvent(f.on[ON_SIDE], c->st.ev_fork, 0));
  }

  c->stream = f.on[p.history_on];
  history_encoder(f);
  if (p.nat_aside) HIPCHK(c, hipEventRecord(c->st.ev_join2, f.on[ON_PREPARE]));

  c->stream = f.on[p.dp_fill_on];
  if (p.dp_fill_late) dp_kpm_fill(f);      // (behind the previous forward's exchanges)
  c->stream = f.on[p.map_on];
  ego_token(f);
  TRY(map_and_embeddings(f));

  // join: the agent tokens need both chains
  if (p.join_once) HIPCHK(c, hipStreamWaitEvent(f.on[ON_SIDE], c->st.ev_join2, 0));
  if (p.forked) {
    HIPCHK(c, hipEventRecord(c->st.ev_join, f.on[ON_SIDE]));
    HIPCHK(c, hipStreamWaitEvent(f.on[ON_CALLER], c->st.ev_join, 0));
  }
  if (p.nat_aside && !p.join_once) HIPCHK(c, hipStreamWaitEvent(f.on[ON_CALLER], c->st.ev_join2, 0));

  c->stream = f.on[ON_CALLER];
  assemble_tokens(f);
  scene_encoder(f);
  agent_predictor(f);
  TRY(planning_decoder(f));
  return policy_and_ego_heads(f);
}

}  // namespace

// ============================================================================================
// C-ABI of this build (one per operand format).  The exported `rift_*` symbols of include/rift_hip.h are trampolines (abi.cpp, generated
// from the header) that route a call through the table at the end of this file to the build that owns the context.
// ============================================================================================
namespace RIFT_NS { namespace abi {

// The environment switches, read ONCE when the context is made.  Three idioms, kept as they grew: env_is (the first character decides),
// env_flag (set: atoi != 0), env_int (set: the number).
static bool env_is(const char* name, char ch) { const char* ev = getenv(name); return ev && ev[0] == ch; }
static void env_flag(const char* name, bool* v) { const char* ev = getenv(name); if (ev) *v = atoi(ev) != 0; }
static bool env_int(const char* name, int* v, int base = 10) { const char* ev = getenv(name); if (ev) *v = (int)strtol(ev, nullptr, base); return ev != nullptr; }

static void read_switches(Ctx* c) {
  c->sw.nat_fused = !env_is("RIFT_NAT_UNFUSED", '1');        // 1: the history encoder's NAT levels layer-wise (GEMM / attention launches)
  c->sw.dec_fused = !env_is("RIFT_DEC_UNFUSED", '1');        // 1: the planning decoder layer-wise
  c->sw.enc_fused = !env_is("RIFT_ENC_UNFUSED", '1');        // 1: the scene encoder layer-wise
  c->sw.pe_fused = !env_is("RIFT_PE_UNFUSED", '1');          // 1: the PointsEncoders layer-wise, one after the other
  c->sw.fpn_fused = !env_is("RIFT_FPN_UNFUSED", '1');        // 1: the FPN tail as lateral GEMMs + merge
  c->sw.ego_fused = !env_is("RIFT_EGO_UNFUSED", '1');        // 1: the ego state token as five launches
  c->sw.heads_fused = !env_is("RIFT_HEADS_UNFUSED", '1');    // 1: trajectory / prediction / ego heads as MLPLayer GEMMs
  c->sw.pi_fused = !env_is("RIFT_PI_UNFUSED", '1');          // 1: cat_x_proj -> pi_head and the decoder queries as separate launches
  c->sw.fo_fused = !env_is("RIFT_FOURIER_UNFUSED", '1');     // 1: the Fourier embeddings layer-wise
  c->sw.pe_w = !env_is("RIFT_PE_W", '0');                    // 0: PointsEncoder pass B as the workgroup-tiled pe_mid_kernel
  c->sw.fo_w = !env_is("RIFT_FO_W", '0');                    // 0: the three Fourier embeddings through fourier_fused_kernel
  c->sw.two_streams = !env_is("RIFT_TWO_STREAMS", '0');      // 0: history and map chains one after the other on the caller's stream
  { int g = 0; env_int("RIFT_NAT_GRID", &g); if (g > 0) c->sw.nat_grid = g; }      // workgroups of the persistent launches (default 256: one per CU)
  env_flag("RIFT_NAT_COMPACT", &c->sw.nat_compact);          // 0: the history encoder on all agent slots, not the compacted valid ones
  env_flag("RIFT_PE_LIVE", &c->sw.pe_live);                  // 0: pass B over all rounds instead of the live ones of pass A's counts
  env_flag("RIFT_PE_PACK", &c->sw.pe_pack);                  // 0: reference lines of pass B in two-line rounds instead of packed valid-prefix tiles
  env_flag("RIFT_RANK_IN_PREP", &c->sw.rank_in_prep);        // 0: the ranking as its own launch behind the preparation (nat_rank_kernel)
  env_flag("RIFT_NO_SKIP", &c->sw.no_skip);                  // 1: compute, then discard (dropped encoder branches, padded reference lines of the decoder)
  env_flag("RIFT_NAT_GROUP", &c->sw.nat_group);              // 0: NAT levels 1 and 2 in rank order, no DropPath grouping
  env_flag("RIFT_ENC112", &c->sw.enc112);                    // 0: scenes of 97 .. 112 token slots on enc_w_kernel
  env_flag("RIFT_RANK_FAULT", &c->sw.rank_fault);            // 1 (diagnostic): the first scene block of the in-launch ranking never publishes
  env_int("RIFT_SIDE_GATE", &c->sw.side_gate);               // 1: both front chains behind the caller's queue (fwd_plan.h)
  env_flag("RIFT_NAT_ASIDE", &c->sw.nat_aside);              // 0: the history chain on the caller's stream, not behind the preparation
  env_int("RIFT_DEC_DEFER", &c->sw.dec_defer_max);           // <n>: the decoder goes with the deferred head for bs <= n (0: never; unset: the measured table)
  env_flag("RIFT_DEC_SPLIT", &c->sw.dec_split);              // 0: the deferred decoder as one launch
  env_int("RIFT_DEC_LAYERS", &c->sw.dec_layers);             // (diagnostic) 0 / 2: the non-deferred decoder stops after that many layers and `dec3` taps that boundary; 22: an eval forward's layers as two launches
  env_flag("RIFT_RO8", &c->ro8);                          // 0: candidate rollout with one lane per candidate
  if (env_int("RIFT_POISON_LDS", &c->poison_lds, 0)) c->poison_lds &= 0xff;                // <byte>: every CU's LDS filled ahead of every launch
  if (env_int("RIFT_POISON_ARENA", &c->sw.poison_arena, 0)) c->sw.poison_arena &= 0xff;    // <byte>: the arena filled ahead of every forward
  { const char* ev = getenv("RIFT_DELAY"); const char* col = ev ? strrchr(ev, ':') : nullptr;      // <launch label>:<us> (wall_clock64: 100 MHz)
    if (col) { c->dg.delay_label.assign(ev, col - ev); c->dg.delay_ticks = (long long)(atof(col + 1) * 100.0); } }
  env_int("RIFT_PE_TS", &c->sw.pe_ts);                    // the *_TS taps: phase timestamps of one workgroup
  c->sw.pew_ts = env_is("RIFT_PEW_TS", '1');
  env_int("RIFT_NAT_TS", &c->sw.nat_ts);
  c->sw.enc_ts = getenv("RIFT_ENC_TS") != nullptr;
  c->sw.dec_ts = getenv("RIFT_DEC_TS") != nullptr;
  env_int("RIFT_PEW_DBG", &c->sw.pew_dbg);                // the *_DBG words: handed to the kernel as they are
  env_int("RIFT_DEC_DBG", &c->sw.dec_dbg);
  env_int("RIFT_GEMM_DBG", &c->sw.gemm_dbg);
}

int rift_ctx_create(int device, RiftCtx** ctx) {
  if (!ctx) return RIFT_ERR_ARG;
  Ctx* c = new Ctx();
  c->opfmt = RIFT_OP_F16;
  c->device = device;
  if (hipSetDevice(device) != hipSuccess) { delete c; return RIFT_ERR_HIP; }
  read_switches(c);
  if (c->nonfinite.reserve(1) != 0 || hipMemset(c->nonfinite.get(), 0, sizeof(int)) != hipSuccess) { delete c; return RIFT_ERR_HIP; }
  for (int i = 0; i < RIFT_DEFER_SLOTS; ++i) {      // the in-launch ranking's published counts (kernels.h: rank_scene_body): zero = "never written"
    if (c->slots[i].rk_pub.reserve(4096) != 0 || hipMemset(c->slots[i].rk_pub.get(), 0, 4096 * sizeof(unsigned long long)) != hipSuccess) { delete c; return RIFT_ERR_HIP; }
  }
  if (hipDeviceSynchronize() != hipSuccess) { delete c; return RIFT_ERR_HIP; }      // (the zeros are in place before any stream launches a kernel that reads them)
  int rc = set_lds_attrs(c);
  if (rc != RIFT_OK) { fprintf(stderr, "rift_ctx_create: %s\n", c->err.c_str()); delete c; return rc; }
  *ctx = c;
  return RIFT_OK;
}

void rift_ctx_destroy(RiftCtx* h) {      // (this build's entry: its own context type's destructor runs)
  Ctx* c = static_cast<Ctx*>(h);
  if (!c) return;
  if (c->comm) { (void)rccl_api(nullptr).CommDestroy(c->comm); c->comm = nullptr; }
  delete c;
}

const char* rift_last_error(RiftCtx* h) { return h ? h->err.c_str() : "null context"; }

int rift_model_load(RiftCtx* h, const RiftTensorDesc* params, int n, void* stream) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c || !params) return RIFT_ERR_ARG;
  c->err.clear();
  c->stream = (hipStream_t)stream;
  HIPCHK(c, hipSetDevice(c->device));
  c->loaded = false;                    // (until this load has succeeded there is no model: the entries that launch refuse to run)
  c->pw.clear(); c->m = Model(); c->pi = RiftCtxCore::PiHead(); c->wc = Ctx::WeightOnly();      // (frees the images and the weight-only products; the table pointed at the images)
  c->dry_need = 0;                      // (the first forward on new weights sizes its arena again: it also computes the weight-only products)
  Load load(c, params, n);              // (model_load.h) the descriptors by name, for this call only
  load.walk();                          // every tensor looked up once: GEMM images packed, c->m and c->pi written
  if (load.rc != RIFT_OK) return load.rc;
  TRY(load.pack_streams());             // the wave-private kernels' images, from the raw tensors the walk found
  HIPCHK(c, hipGetLastError());
  c->loaded = true;
  return RIFT_OK;
}

int rift_forward(RiftCtx* h, const RiftFeatureBatch* B, const RiftOutputs* out, int flags, uint32_t seed, void* stream) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c || !B || !out) return RIFT_ERR_ARG;
  c->err.clear();
  if (!c->loaded) { c->err = "rift_forward before rift_model_load" + NOT_LOADED; return RIFT_ERR_STATE; }
  if (B->bs <= 0 || B->A <= 0 || B->Mp <= 0 || B->R <= 0 || B->S < 0 || B->T < 21) { c->err = "bad batch dims"; return RIFT_ERR_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream;
  // deferred-head forwards cycle through the arenas (the caller guarantees that the head / loss of the forward RIFT_DEFER_SLOTS calls back is
  // over, i.e. that this arena is free again); every other forward runs in arena 0
  c->parity = (flags & RIFT_F_DEFER_HEAD) ? (c->parity + 1) % RIFT_DEFER_SLOTS : 0;
  DevBuf<char>& slot = c->slots[c->parity].arena;
  c->arena = slot.get(); c->arena_cap = slot.cap();
  // pass 1 (dry): size the activation arena; pass 2: launch.  The sizes depend on the batch dimensions, the flags and the data-parallel
  // descriptor only: a forward like the previous one skips pass 1 (it is half of the call's host time, which bounds a small-batch step)
  long long omask = 0;      // which outputs are wanted
  { const void* const* op = reinterpret_cast<const void* const*>(out); for (size_t i = 0; i < sizeof(RiftOutputs) / sizeof(void*); ++i) omask |= (long long)(op[i] != nullptr) << i; }
  // (everything forward_impl's A_alloc sequence depends on, besides the switches fixed when the context is made: batch dimensions, flags, the
  // data-parallel descriptor, the wanted outputs and the profiler switch.  The kernel plan (fwd_kernels.h: KernelIn) is a function of this
  // key and of those switches, and so are the diagnostic timestamp buffers: the launch pass allocates exactly what the sizing pass
  // counted, which is checked below)
  const long long dkey[11] = {B->bs, B->A, B->Mp, B->R, B->S, B->T, flags, c->dp.on ? 1 : 0, c->dp.on ? c->dp.gbs : 0, omask, c->prof_on ? 1 : 0};
  int rc = RIFT_OK;
  if (c->dry_need == 0 || memcmp(dkey, c->dry_key, sizeof(dkey)) != 0) {
    c->dry = true; c->arena_off = 0; c->dry_need = 0;
    rc = forward_impl(c, B, out, flags, seed);
    c->stream = (hipStream_t)stream;              // (forward_impl forks onto its side stream; an early error return leaves it selected)
    if (rc != RIFT_OK) { c->dry = false; return rc; }
    memcpy(c->dry_key, dkey, sizeof(dkey)); c->dry_need = c->arena_off;
  }
  const size_t need = c->dry_need;
  if (need > slot.cap()) {
    // (the whole device: with the deferred head and the prepare stream the arena's last readers sit on streams other than the caller's)
    HIPCHK(c, hipDeviceSynchronize());
    const int grown = slot.reserve(need, need + (need >> 3));
    c->arena = slot.get(); c->arena_cap = slot.cap();      // (also when it failed: the view never outlives the block)
    DEVCHK(c, grown);
  }
  c->dry = false; c->arena_off = 0; c->taps.clear();
  // diagnostic: RIFT_POISON_ARENA=<byte> fills the scratch arena before every forward (0xFF = NaN pattern), so that a kernel reading
  // scratch it never wrote shows up as NaN / as run-to-run differences instead of depending on what the memory held before
  // (on the prepare stream if the preparation runs there: every other stream of the forward waits for the preparation)
  if (c->sw.poison_arena >= 0 && c->arena) { HIPCHK(c, hipMemsetAsync(c->arena, c->sw.poison_arena, c->arena_cap, plan_streams(plan_in(c, kernel_in(c, B, out, flags))).prefetched ? c->st.prep_stream : c->stream)); }
  rc = forward_impl(c, B, out, flags, seed);
  c->stream = (hipStream_t)stream;
  if (rc != RIFT_OK) return rc;
  if (!c->err.empty()) return RIFT_ERR_ARG;
  if (c->arena_off != need) {     // the launch pass did not walk the allocations of the sizing pass it was matched with: past the count, kernels were given scratch beyond the arena
    c->dry_need = 0;
    char msg[160];
    snprintf(msg, sizeof(msg), "activation arena: the forward allocated %zu B, its sizing pass counted %zu B (stale or diverging sizing pass)", c->arena_off, need);
    c->err = msg;
    (void)hipDeviceSynchronize();
    return RIFT_ERR_STATE;
  }
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_forward_head_back(RiftCtx* h, int back, void* stream) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c || back < 0 || back >= RIFT_DEFER_SLOTS) return RIFT_ERR_ARG;
  c->err.clear();
  if (!c->loaded) { c->err = "rift_forward_head without a RIFT_F_DEFER_HEAD forward" + NOT_LOADED; return RIFT_ERR_STATE; }
  const int slot = (c->parity - back + RIFT_DEFER_SLOTS) % RIFT_DEFER_SLOTS;
  if (!c->slots[slot].head.valid) { c->err = "rift_forward_head without a RIFT_F_DEFER_HEAD forward"; return RIFT_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  const hipStream_t trunk_stream = c->stream;
  c->stream = (hipStream_t)stream; c->dry = false;
  if (c->slots[slot].head.dec_pending) {          // (the forward left its planning decoder to this call: dec_defer_max)
    const DecWP dq = c->slots[slot].head.dec;
    launch_call(c, "dec_w_kernel", [&] { decw_launch(dq, c->stream); });
    c->slots[slot].head.dec_pending = false;
  }
  const int rc = head_impl(c, c->slots[slot].head);
  c->slots[slot].head.valid = false;
  c->stream = trunk_stream;
  if (rc != RIFT_OK) return rc;
  if (!c->err.empty()) return RIFT_ERR_ARG;
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

int rift_forward_head(RiftCtx* h, void* stream) { return abi::rift_forward_head_back(h, 0, stream); }

int rift_set_dp(RiftCtx* h, const RiftDp* dp) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c) return RIFT_ERR_ARG;
  if (!dp || dp->global_bs <= 0) { c->dp = Ctx::Dp(); return RIFT_OK; }
  if (!dp->xchg || dp->scene_offset < 0 || dp->xchg_len <= 0) { c->err = "rift_set_dp: bad descriptor"; return RIFT_ERR_ARG; }
  if (!dp->exchange && !c->comm) { c->err = "rift_set_dp: no exchange callback and no library communicator (rift_comm_init)"; return RIFT_ERR_ARG; }
  c->dp.on = true; c->dp.off = dp->scene_offset; c->dp.gbs = dp->global_bs; c->dp.xchg = dp->xchg; c->dp.len = dp->xchg_len;
  c->dp.fn = dp->exchange; c->dp.user = dp->user;
  return RIFT_OK;
}

int rift_comm_unique_id(RiftCtx* h, void* unique_id_out) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c || !unique_id_out) return RIFT_ERR_ARG;
  std::string why;
  RcclApi& r = rccl_api(&why);
  if (!r.ok) { c->err = "rift_comm_unique_id: " + why; return RIFT_ERR_STATE; }
  RcclApi::UniqueId id;
  const int rc = r.GetUniqueId(&id);
  if (rc != 0) { c->err = std::string("ncclGetUniqueId: ") + (r.GetErrorString ? r.GetErrorString(rc) : "failed"); return RIFT_ERR_HIP; }
  memcpy(unique_id_out, &id, sizeof(id));
  return RIFT_OK;
}

int rift_comm_init(RiftCtx* h, const void* unique_id, int rank, int world) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c || !unique_id || world < 1 || rank < 0 || rank >= world) return RIFT_ERR_ARG;
  if (c->comm) { c->err = "rift_comm_init: the context has a communicator already (rift_comm_destroy first)"; return RIFT_ERR_STATE; }
  std::string why;
  RcclApi& r = rccl_api(&why);
  if (!r.ok) { c->err = "rift_comm_init: " + why; return RIFT_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  RcclApi::UniqueId id;
  memcpy(&id, unique_id, sizeof(id));
  void* comm = nullptr;
  const int rc = r.CommInitRank(&comm, world, id, rank);
  if (rc != 0 || !comm) { c->err = std::string("ncclCommInitRank: ") + (r.GetErrorString ? r.GetErrorString(rc) : "failed"); return RIFT_ERR_HIP; }
  c->comm = comm; c->comm_rank = rank; c->comm_world = world;
  return RIFT_OK;
}

int rift_comm_all_reduce(RiftCtx* h, double* buf, int64_t count, void* stream) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c || !buf || count <= 0) return RIFT_ERR_ARG;
  if (!c->comm) { c->err = "rift_comm_all_reduce before rift_comm_init"; return RIFT_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = comm_sum_f64(c, buf, count, (hipStream_t)stream);
  if (rc != 0) { RcclApi& r = rccl_api(nullptr); c->err = std::string("ncclAllReduce: ") + (r.GetErrorString ? r.GetErrorString(rc) : "failed"); return RIFT_ERR_HIP; }
  return RIFT_OK;
}

int rift_comm_destroy(RiftCtx* h) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c) return RIFT_ERR_ARG;
  if (c->comm) {
    if (c->dp.on && !c->dp.fn) c->dp = Ctx::Dp();      // (forwards must not reach for a communicator that is gone)
    (void)rccl_api(nullptr).CommDestroy(c->comm);
    c->comm = nullptr; c->comm_world = 1; c->comm_rank = 0;
  }
  return RIFT_OK;
}

int rift_set_prepare_stream(RiftCtx* h, void* prepare_stream) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c) return RIFT_ERR_ARG;
  c->st.prep_stream = (hipStream_t)prepare_stream; c->st.prep_set = prepare_stream != nullptr;
  return RIFT_OK;
}

int rift_set_side_stream(RiftCtx* h, void* side_stream) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c) return RIFT_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->st.side && c->st.side_owned) { HIPCHK(c, hipStreamSynchronize(c->st.side)); (void)hipStreamDestroy(c->st.side); }
  else if (c->st.side) HIPCHK(c, hipStreamSynchronize(c->st.side));
  c->st.side = (hipStream_t)side_stream; c->st.side_owned = false;
  return RIFT_OK;
}

int rift_check_finite(RiftCtx* h, void* stream) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c) return RIFT_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int flag = 0;
  HIPCHK(c, hipMemcpyAsync(&flag, c->nonfinite.get(), sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
  if (!flag) return RIFT_OK;
  HIPCHK(c, hipMemsetAsync(c->nonfinite.get(), 0, sizeof(int), (hipStream_t)stream));
  c->err = (flag & 4) ? "the reference-line packing of the PointsEncoder wanted more rounds than its table holds (pe_fused.h: pe_pack_body): the forward's "
                        "results are invalid; non-finite flag raised"
         : (flag & 2) ? "the in-launch ranking of the history encoder's sequences gave up waiting for a predecessor (kernels.h: rank_scene_body): the forward's "
                        "results are invalid; non-finite flag raised"
                      : "non-finite decoder queries (the reference asserts torch.isfinite(q).all(), planning_decoder.py:175)";
  return RIFT_ERR_NONFINITE;
}

int rift_set_param_event(RiftCtx* h, void* event) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c) return RIFT_ERR_ARG;
  c->st.param_event = (hipEvent_t)event;
  return RIFT_OK;
}

int rift_prof_enable(RiftCtx* h, int on) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c) return RIFT_ERR_ARG;
  c->prof_on = on != 0;
  c->dry_need = 0;                      // the next forward sizes its arena again
  const char* ev = getenv("RIFT_PROF_SHAPES");
  c->prof_shapes = ev && ev[0] == '1';
  if (on) { c->prof_recs.clear(); c->prof_used = 0; }
  return RIFT_OK;
}

// JSON: {"label": {"count": n, "ms": total_ms, "flops": total_flops}, ...}; synchronises the device.
int rift_prof_report(RiftCtx* h, char* buf, int buflen) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c || !buf || buflen <= 0) return RIFT_ERR_ARG;
  HIPCHK(c, hipDeviceSynchronize());
  struct Agg { long n = 0; double ms = 0, fl = 0; };
  std::unordered_map<std::string, Agg> agg;
  for (auto& r : c->prof_recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) continue;
    Agg& a = agg[r.label]; a.n++; a.ms += ms; a.fl += r.flops;
  }
  std::string js = "{";
  bool first = true;
  for (auto& kv : agg) {
    char tmp[256];
    snprintf(tmp, sizeof(tmp), "%s\"%s\": {\"count\": %ld, \"ms\": %.6f, \"flops\": %.6e}", first ? "" : ", ", kv.first.c_str(), kv.second.n, kv.second.ms, kv.second.fl);
    js += tmp; first = false;
  }
  js += "}";
  if ((int)js.size() + 1 > buflen) { c->err = "prof buffer too small"; return RIFT_ERR_ARG; }
  memcpy(buf, js.c_str(), js.size() + 1);
  return RIFT_OK;
}

int rift_tap(RiftCtx* h, const char* name, float* dst, int64_t* numel, void* stream) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c || !name) return RIFT_ERR_ARG;
  auto it = c->taps.find(name);
  if (it == c->taps.end()) { c->err = std::string("unknown tap ") + name; return RIFT_ERR_ARG; }
  if (numel) *numel = it->second.numel;
  if (dst && it->second.numel > 0)
    HIPCHK(c, hipMemcpyAsync(dst, it->second.p, it->second.numel * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RIFT_OK;
}

int rift_op_linear(RiftCtx* h, const float* X, int M, int K, const float* W, const float* bias, int N,
                   const float* ln_w, const float* ln_b, int act, int fp32, float* Y, void* stream) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c || !X || !W || !Y || K > 512) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  PW w;      // transient images of its own (test entry point; not on the hot path): freed on every way out, the model's are not touched
  TRY(pack_image(c, w, W, N, N, K, 0, 0, K, 0, 0, 0, bias));
  GemmP g = mk(X, K, M, w, Y, N);
  if (ln_w) { g.pro = PRO_LN; g.pg = ln_w; g.pb = ln_b; }
  g.act = act;
  gemm(c, g, w, fp32 != 0);
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (the images outlive the GEMM)
  HIPCHK(c, hipGetLastError());
  return RIFT_OK;
}

// Diagnostic: pack once, launch the GEMM `reps` times back to back, return the average milliseconds per launch.
int rift_op_linear_bench(RiftCtx* h, const float* X, int M, int K, const float* W, const float* bias, int N,
                         const float* ln_w, const float* ln_b, int act, const float* residual, float* Y, int reps,
                         float* ms_out, void* stream) {
  Ctx* c = static_cast<Ctx*>(h);
  if (!c || !X || !W || !Y || K > 512 || reps <= 0) return RIFT_ERR_ARG;
  c->err.clear();
  HIPCHK(c, hipSetDevice(c->device));
  c->stream = (hipStream_t)stream; c->dry = false;
  PW w;
  TRY(pack_image(c, w, W, N, N, K, 0, 0, K, 0, 0, 0, bias));
  GemmP g = mk(X, K, M, w, Y, N);
  if (ln_w) { g.pro = PRO_LN; g.pg = ln_w; g.pb = ln_b; }
  g.act = act;
  if (residual) { g.residual = residual; g.ldr = N; }
  hipEvent_t e0, e1;
  HIPCHK(c, hipEventCreate(&e0)); HIPCHK(c, hipEventCreate(&e1));
  for (int i = 0; i < 3; ++i) gemm(c, g, w, false);
  HIPCHK(c, hipEventRecord(e0, c->stream));
  for (int i = 0; i < reps; ++i) gemm(c, g, w, false);
  HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
  if (ms_out) *ms_out = ms / reps;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return RIFT_OK;
}

}}  // namespace RIFT_NS::abi

#include "abi_table.h"
#if RIFT_OP_F16
#define RIFT_VT_SYM rift_vtable_fp16
#else
#define RIFT_VT_SYM rift_vtable_bf16
#endif
#if !defined(__HIP_DEVICE_COMPILE__)      // host data: the device pass of this file must not see pointers to host functions
extern "C" const RiftVTable RIFT_VT_SYM = {
#define RIFT_FN(name) &RIFT_NS::abi::name,
#include "abi_list.h"
#undef RIFT_FN
};
#endif
