// The reference forward: every stage as GEMM / attention / element-wise launches, layer by layer.  It is what RIFT_F_FP32 runs, what the
// RIFT_*_UNFUSED switches select stage by stage (the GPU tests' oracle for the fused kernels) and what shapes outside a fused kernel's
// take.  Which stage runs it is the kernel plan's decision (fwd_kernels.h); the stages of engine.hip call the *_layerwise functions below.
// Included by engine.hip only, inside its unnamed namespace, behind the helpers both paths use (mk, gemm, wconst_get, dp_exchange,
// layernorm, the DropPath rate tables).
#pragma once

// BatchNorm1d folded to an affine (scale, shift) for the next GEMM prologue.
void batchnorm_affine(Fwd& f, const float* X, int rows, int C, const uint8_t* valid, const BatchNormW& bn,
                      float** scale, float** shift) {
  Ctx* c = f.c;
  *scale = A_alloc<float>(c, C); *shift = A_alloc<float>(c, C);
  const int rows_per_blk = 128;
  const int nblk = cdiv(rows, rows_per_blk);
  double* part = A_alloc<double>(c, (size_t)nblk * 2 * C);
  int* cnt = A_alloc<int>(c, nblk);
  if (f.train) launch(c, "bn_partial_kernel", bn_partial_kernel, dim3(nblk), dim3(C), 0, X, C, rows, C, valid, part, cnt, rows_per_blk);
  const bool dpx = f.dp && f.train;      // data parallel: batch statistics over the GLOBAL minibatch (sums all-reduced between two launches)
  double* sums = dpx ? c->dp.xchg + f.kb : nullptr;
  for (int mode = dpx ? 1 : 0; mode <= (dpx ? 2 : 0); ++mode) {
    launch(c, "bn_finalize_kernel", bn_finalize_kernel, dim3(cdiv(C, 4)), dim3(256), 0, (const double*)part, (const int*)cnt, nblk, C,
           bn.g, bn.b, bn.mean,
           bn.var, bn.num_batches, f.train ? 1 : 0,
           f.bn_update ? 1 : 0, 1e-5f, *scale, *shift, sums, mode);
    if (mode == 1) dp_exchange(f, 2 * C + 1);
  }
}

// PointsEncoder (embedding.py:271-296): F (groups*n, Cin) -> (groups, 128)
float* points_encoder_layerwise(Fwd& f, const float* F, int Cin, int groups, int n, const uint8_t* valid, const PointsEncoderW& p) {
  Ctx* c = f.c;
  const int rows = groups * n;
  float* H1 = A_alloc<float>(c, (size_t)rows * 128);
  gemm(c, mk(F, Cin, rows, *p.first0, H1, 128), *p.first0, f.fp32);
  float *s1, *t1;
  batchnorm_affine(f, H1, rows, 128, valid, p.bn1, &s1, &t1);
  float* F256 = A_alloc<float>(c, (size_t)rows * 256);
  GemmP g = mk(H1, 128, rows, *p.first3, F256, 256);
  g.pro = PRO_AFFINE; g.pg = s1; g.pb = t1; g.pro_relu = 1;
  gemm(c, g, *p.first3, f.fp32);
  float* pooled = A_alloc<float>(c, (size_t)groups * 256);
  launch(c, "masked_maxpool_kernel", masked_maxpool_kernel, dim3(cdiv((long long)groups * 256, 256)), dim3(256), 0, (const float*)F256, 256, groups, n, 256,
         valid, pooled);
  float* G1 = A_alloc<float>(c, (size_t)groups * 256);
  gemm(c, mk(pooled, 256, groups, *p.pool, G1, 256), *p.pool, f.fp32);
  float* H2 = A_alloc<float>(c, (size_t)rows * 256);
  GemmP g2 = mk(F256, 256, rows, *p.feat, H2, 256);
  g2.gbias = G1; g2.gb_div = n; g2.gb_mod = 0;
  gemm(c, g2, *p.feat, f.fp32);
  float *s2, *t2;
  batchnorm_affine(f, H2, rows, 256, valid, p.bn2, &s2, &t2);
  float* O = A_alloc<float>(c, (size_t)rows * 128);
  GemmP g3 = mk(H2, 256, rows, *p.second3, O, 128);
  g3.pro = PRO_AFFINE; g3.pg = s2; g3.pb = t2; g3.pro_relu = 1;
  gemm(c, g3, *p.second3, f.fp32);
  float* out = A_alloc<float>(c, (size_t)groups * 128);
  launch(c, "masked_maxpool_kernel", masked_maxpool_kernel, dim3(cdiv((long long)groups * 128, 256)), dim3(256), 0, (const float*)O, 128, groups, n, 128,
         valid, out);
  {   // the fused pair's taps, as far as this path has them: g here in fp32; no gp (G1 is without second_mlp.0's bias, which rides on `feat`)
    static const char* const nm[2][5] = {{"pe_s1_a", "pe_t1_a", "pe_s2_a", "pe_t2_a", "pe_g_a"}, {"pe_s1_b", "pe_t1_b", "pe_s2_b", "pe_t2_b", "pe_g_b"}};
    const char* const* t = nm[n == 20 ? 0 : 1];
    tap(c, t[0], s1, 128); tap(c, t[1], t1, 128); tap(c, t[2], s2, 256); tap(c, t[3], t2, 256); tap(c, t[4], H2, (int64_t)rows * 256);
  }
  return out;
}

template <int NKT>
void run_mha_mfma(Ctx* c, const MhaP& p) {
  const int nqt = (p.Lq + 15) / 16;
  const int waves = nqt < 4 ? nqt : 4;
  const size_t lds = (size_t)NKT * 16 * 40 * 2 + (size_t)32 * (NKT * 16 + 8) * 2 + NKT * 16;
  launch(c, "mha_mfma_kernel", mha_mfma_kernel<NKT>, dim3(p.nb_outer * p.nb_inner * p.H), dim3(64 * waves), lds, p);
}

// bf16 mode: MFMA attention; fp32 mode (or unaligned / very long inputs): exact-fp32 VALU kernel
void run_mha(Ctx* c, const MhaP& p, bool fp32) {
  const bool al = ((((uintptr_t)p.Q) | ((uintptr_t)p.K) | ((uintptr_t)p.V)) & 15) == 0 && p.ldq % 4 == 0 && p.ldkv % 4 == 0;
  if (!fp32 && al && p.Lk <= 192) {
    if (p.Lk <= 32) run_mha_mfma<2>(c, p);
    else if (p.Lk <= 96) run_mha_mfma<6>(c, p);
    else run_mha_mfma<12>(c, p);
    return;
  }
  const long long total = (long long)p.nb_outer * p.nb_inner * p.H * p.Lq;
  launch(c, "mha_kernel", mha_kernel, dim3(cdiv(total, 64)), dim3(64), 0, p);
}

// NAT block (embedding.py:196-202) on X (rows, C) in place
void nat_layer(Fwd& f, float* X, int rows, int C, int H, int ksz, int L, const NatBlockW& p, float droppath) {
  Ctx* c = f.c;
  float* QKV = A_alloc<float>(c, (size_t)rows * 3 * C);
  GemmP g = mk(X, C, rows, *p.qkv, QKV, 3 * C);
  g.pro = PRO_LN; g.pg = p.norm1.g; g.pb = p.norm1.b;
  gemm(c, g, *p.qkv, f.fp32);
  float* AO = A_alloc<float>(c, (size_t)rows * C);
  const int nthreads = rows * H;
  if (ksz == 3) launch(c, "nat_attention_kernel", nat_attention_kernel<3>, dim3(cdiv(nthreads, 256)), dim3(256), 0, (const float*)QKV, p.rpb, rows / L, L, H, AO);
  else launch(c, "nat_attention_kernel", nat_attention_kernel<5>, dim3(cdiv(nthreads, 256)), dim3(256), 0, (const float*)QKV, p.rpb, rows / L, L, H, AO);
  GemmP g2 = mk(AO, C, rows, *p.proj, X, C);
  g2.residual = X; g2.ldr = C;
  if (f.drop && droppath > 0.f) { g2.droppath_p = droppath; g2.dp_div = L; g2.seed = f.seed; g2.stream = f.next_stream(); }
  gemm(c, g2, *p.proj, f.fp32);
  float* Hh = A_alloc<float>(c, (size_t)rows * 3 * C);
  GemmP g3 = mk(X, C, rows, *p.fc1, Hh, 3 * C);
  g3.pro = PRO_LN; g3.pg = p.norm2.g; g3.pb = p.norm2.b; g3.act = ACT_GELU;
  gemm(c, g3, *p.fc1, f.fp32);
  GemmP g4 = mk(Hh, 3 * C, rows, *p.fc2, X, C);
  g4.residual = X; g4.ldr = C;
  if (f.drop && droppath > 0.f) { g4.droppath_p = droppath; g4.dp_div = L; g4.seed = f.seed; g4.stream = f.next_stream(); }
  gemm(c, g4, *p.fc2, f.fp32);
}

// the three NAT levels on all nA sequences -> Oc[i]: LayerNorm(norm_i) of the last 3 steps of level i, fp32 rows
void history_levels_layerwise(Fwd& f, float* const Oc[3]) {
  Ctx* c = f.c;
  const auto& he = c->m.agent;
  const int nA = f.nA;
  float* X0 = A_alloc<float>(c, (size_t)nA * 20 * 32);
  {
    GemmP g = mk(f.F9, 9, nA * 20, *he.embed_proj, X0, 32);
    g.amode = AMODE_CONV3; g.cv_C = 9; g.cv_Lin = 20; g.cv_nout = 20; g.cv_t0 = 0; g.cv_stride = 1;
    gemm(c, g, *he.embed_proj, f.fp32);
  }
  auto nat_level = [&](float* Xl, int lv, int rows, int C, int H, int ksz, int L) {
    nat_layer(f, Xl, rows, C, H, ksz, L, he.levels[lv].blocks[0], NAT_DPR[2 * lv]);
    nat_layer(f, Xl, rows, C, H, ksz, L, he.levels[lv].blocks[1], NAT_DPR[2 * lv + 1]);
  };
  nat_level(X0, 0, nA * 20, 32, 2, 3, 20);
  float* X1 = A_alloc<float>(c, (size_t)nA * 10 * 64);
  {
    GemmP g = mk(X0, 32, nA * 10, *he.levels[0].reduction, X1, 64);
    g.amode = AMODE_CONV3; g.cv_C = 32; g.cv_Lin = 20; g.cv_nout = 10; g.cv_t0 = 0; g.cv_stride = 2;
    gemm(c, g, *he.levels[0].reduction, f.fp32);
    layernorm(f, X1, 64, X1, 64, nA * 10, 64, he.levels[0].ds_norm);
  }
  nat_level(X1, 1, nA * 10, 64, 4, 3, 10);
  // level outputs are the PRE-downsample activations (NATBlock returns (downsample(x), x)); X0/X1 are
  // still needed below, so the downsample writes new buffers.
  float* X2 = A_alloc<float>(c, (size_t)nA * 5 * 128);
  {
    GemmP g = mk(X1, 64, nA * 5, *he.levels[1].reduction, X2, 128);
    g.amode = AMODE_CONV3; g.cv_C = 64; g.cv_Lin = 10; g.cv_nout = 5; g.cv_t0 = 0; g.cv_stride = 2;
    gemm(c, g, *he.levels[1].reduction, f.fp32);
    layernorm(f, X2, 128, X2, 128, nA * 5, 128, he.levels[1].ds_norm);
  }
  nat_level(X2, 2, nA * 5, 128, 8, 5, 5);
  tap(c, "nat_level2", X2, (int64_t)nA * 5 * 128);
  float* Xl[3] = {X0, X1, X2};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)   // rows (a, j) <- level rows (a*L + L-3 + j): 3 strided LN calls
      launch(c, "layernorm_kernel", layernorm_kernel, dim3(cdiv(nA, 4)), dim3(256), 0, (const float*)(Xl[i] + (size_t)(NAT_L[i] - 3 + j) * NAT_C[i]),
             NAT_L[i] * NAT_C[i], Oc[i] + (size_t)j * NAT_C[i], 3 * NAT_C[i], nA, NAT_C[i],
             he.levels[i].norm.g, he.levels[i].norm.b,
             1e-5f, 0);
}

// FPN restricted to what out[:, :, -1] depends on: lateral convolutions, merge, fpn_conv -> f.nat_out
void fpn_layerwise(Fwd& f, float* const Oc[3]) {
  Ctx* c = f.c;
  const auto& he = c->m.agent;
  const int nA = f.nA;
  float* lat[3];
  for (int i = 0; i < 3; ++i) {
    lat[i] = A_alloc<float>(c, (size_t)nA * 2 * 128);
    const PW& lc = *he.levels[i].lateral;
    GemmP g = mk(Oc[i], NAT_C[i], nA * 2, lc, lat[i], 128);
    g.amode = AMODE_CONV3; g.cv_C = NAT_C[i]; g.cv_Lin = 3; g.cv_nout = 2; g.cv_t0 = 1; g.cv_stride = 1;
    gemm(c, g, lc, f.fp32);
  }
  float* Z = A_alloc<float>(c, (size_t)nA * 256);
  launch(c, "fpn_merge_kernel", fpn_merge_kernel, dim3(cdiv((long long)nA * 128, 256)), dim3(256), 0, (const float*)lat[0], (const float*)lat[1],
         (const float*)lat[2], nA, Z);
  gemm(c, mk(Z, 256, nA, *he.fpn_last, f.nat_out, 128), *he.fpn_last, f.fp32);
}

// ego state token (StateAttentionEncoder, agent_encoder.py:99-140) as five launches; eq: the projected query -> f.x_ego
void ego_token_layerwise(Fwd& f, const float* eq) {
  Ctx* c = f.c;
  const RiftFeatureBatch* B = f.B;
  const int bs = f.bs;
  const auto& eg = c->m.agent.ego;
  float* E = A_alloc<float>(c, (size_t)bs * 6 * 128);
  launch(c, "ego_token_kernel", ego_token_kernel, dim3(cdiv((long long)bs * 6 * 128, 256)), dim3(256), 0, B->current_state, B->cs_ld,
         (const float*)c->img.ego_w.get(), (const float*)c->img.ego_b.get(), eg.pos_embed, bs, E);
  float* EKV = A_alloc<float>(c, (size_t)bs * 6 * 256);
  gemm(c, mk(E, 128, bs * 6, *eg.kv, EKV, 256), *eg.kv, f.fp32);
  uint8_t* edrop = nullptr;
  if (f.drop) {
    edrop = A_alloc<uint8_t>(c, (size_t)bs * 6);
    launch(c, "ego_dropmask_kernel", ego_dropmask_kernel, dim3(cdiv(bs * 6, 256)), dim3(256), 0, bs, 0.75f, f.seed, f.next_stream(), edrop);
  }
  float* EAO = A_alloc<float>(c, (size_t)bs * 128);
  {
    MhaP p; memset(&p, 0, sizeof(p));
    p.Q = eq; p.ldq = 128; p.K = EKV; p.V = EKV + 128; p.ldkv = 256; p.O = EAO; p.ldo = 128;
    p.nb_outer = bs; p.nb_inner = 1; p.H = 4; p.Lq = 1; p.Lk = 6;
    p.q_outer = 0; p.q_inner = 0; p.q_stride = 0; p.kv_outer = 6; p.kv_inner = 0; p.kv_stride = 1;
    p.o_outer = 1; p.o_inner = 0; p.o_stride = 0; p.mask = edrop; p.mask_quirk = 0; p.mask_mod = 1;
    run_mha(c, p, f.fp32);
  }
  gemm(c, mk(EAO, 128, bs, *eg.out_proj, f.x_ego, 128), *eg.out_proj, f.fp32);
}

// FourierEmbedding (fourier_embedding.py:45-55): in (rows, D) -> out (rows, 128); add: added into the buffer `to`, which is returned
float* fourier_layerwise(Fwd& f, const float* in, int in_ld, int rows, const FourierW& p, int wrap_dim, bool add, float* to) {
  Ctx* c = f.c;
  const int D = p.D;
  float* FF = A_alloc<float>(c, (size_t)D * rows * 129);
  launch(c, "fourier_feature_kernel", fourier_feature_kernel, dim3(cdiv((long long)D * rows * 65, 256)), dim3(256), 0, in, in_ld, rows, D,
         p.freqs, wrap_dim, FF);
  float* T1 = A_alloc<float>(c, (size_t)rows * 128);
  float* acc = A_alloc<float>(c, (size_t)rows * 128);
  for (int d = 0; d < D; ++d) {
    const FourierW::Dim& m = p.mlps[d];
    GemmP g = mk(FF + (size_t)d * rows * 129, 129, rows, *m.l0, T1, 128);
    gemm(c, g, *m.l0, f.fp32);
    GemmP g2 = mk(T1, 128, rows, *m.l3, acc, 128);
    g2.pro = PRO_LN; g2.pg = m.ln.g; g2.pb = m.ln.b; g2.pro_relu = 1;
    if (d > 0) { g2.residual = acc; g2.ldr = 128; }
    gemm(c, g2, *m.l3, f.fp32);
  }
  float* out = A_alloc<float>(c, (size_t)rows * 128);
  GemmP g3 = mk(acc, 128, rows, *p.out, out, 128);
  g3.pro = PRO_LN; g3.pg = p.out_ln.g; g3.pb = p.out_ln.b; g3.pro_relu = 1;
  gemm(c, g3, *p.out, f.fp32);
  if (add) {
    launch(c, "add_inplace_kernel", add_inplace_kernel, dim3(cdiv((long long)rows * 128, 256)), dim3(256), 0, to, (const float*)out, (size_t)rows * 128);
    return to;
  }
  return out;
}

// decoder queries: q_proj's reference-line half as a GEMM, then the broadcast sum with the modes' half Mb -> f.Q
void build_q0_layerwise(Fwd& f, const float* Mb) {
  Ctx* c = f.c;
  const auto& pd = c->m.dec;
  float* Ra = A_alloc<float>(c, (size_t)f.nL * 128);
  gemm(c, mk(f.r_emb, 128, f.nL, *pd.q_proj_r, Ra, 128), *pd.q_proj_r, f.fp32);
  launch(c, "build_q0_kernel", build_q0_kernel, dim3(cdiv((long long)f.nQ * 128, 256)), dim3(256), 0, (const float*)Ra, Mb, f.nL, f.M, f.Q);
}

// the four encoder blocks (transformer.py:73-94) on f.X in place, then the final norm -> f.ENC
void scene_encoder_layerwise(Fwd& f) {
  Ctx* c = f.c;
  const int bs = f.bs, N = f.N, nT = f.nT;
  float* QKV = A_alloc<float>(c, (size_t)nT * 384);
  float* AO = A_alloc<float>(c, (size_t)nT * 128);
  float* H512 = A_alloc<float>(c, (size_t)nT * 512);
  for (int i = 0; i < 4; ++i) {
    const SceneBlockW& p = c->m.encoder_blocks[i];
    GemmP g = mk(f.X, 128, nT, *p.qkv, QKV, 384);
    g.pro = PRO_LN; g.pg = p.norm1.g; g.pb = p.norm1.b;
    gemm(c, g, *p.qkv, f.fp32);
    MhaP m; memset(&m, 0, sizeof(m));
    m.Q = QKV; m.ldq = 384; m.K = QKV + 128; m.V = QKV + 256; m.ldkv = 384; m.O = AO; m.ldo = 128;
    m.nb_outer = bs; m.nb_inner = 1; m.H = 4; m.Lq = N; m.Lk = N;
    m.q_outer = N; m.q_stride = 1; m.kv_outer = N; m.kv_stride = 1; m.o_outer = N; m.o_stride = 1;
    m.mask = f.kpm; m.mask_mod = 1;
    run_mha(c, m, f.fp32);
    GemmP g2 = mk(AO, 128, nT, *p.out_proj, f.X, 128);
    g2.residual = f.X; g2.ldr = 128;
    if (f.drop && ENC_DPR[i] > 0.f) { g2.droppath_p = ENC_DPR[i]; g2.dp_div = N; g2.seed = f.seed; g2.stream = f.next_stream(); }
    gemm(c, g2, *p.out_proj, f.fp32);
    GemmP g3 = mk(f.X, 128, nT, *p.fc1, H512, 512);
    g3.pro = PRO_LN; g3.pg = p.norm2.g; g3.pb = p.norm2.b; g3.act = ACT_GELU;
    gemm(c, g3, *p.fc1, f.fp32);
    GemmP g4 = mk(H512, 512, nT, *p.fc2, f.X, 128);
    g4.residual = f.X; g4.ldr = 128;
    if (f.drop && ENC_DPR[i] > 0.f) { g4.droppath_p = ENC_DPR[i]; g4.dp_div = N; g4.seed = f.seed; g4.stream = f.next_stream(); }
    gemm(c, g4, *p.fc2, f.fp32);
  }
  layernorm(f, f.X, 128, f.ENC, 128, nT, 128, c->m.norm);
}

// MLPLayer (mlp_layer.py:8-16): X (rows,128) -> out (rows, Nout) with hidden width Hd
void mlp_layer(Fwd& f, const float* X, int ldx, int rows, const MLPLayerW& p, float* out, int ldo, bool fp32) {
  Ctx* c = f.c;
  const PW& w0 = *p.l0;
  float* T = A_alloc<float>(c, (size_t)rows * w0.N);
  gemm(c, mk(X, ldx, rows, w0, T, w0.N), w0, fp32);
  const PW& w3 = *p.l3;
  GemmP g = mk(T, w0.N, rows, w3, out, ldo);
  g.pro = PRO_LN; g.pg = p.ln.g; g.pb = p.ln.b; g.pro_relu = 1;
  gemm(c, g, w3, fp32);
}

__global__ void interleave_traj_kernel(const float* __restrict__ loc, const float* __restrict__ yaw,
                                       const float* __restrict__ vel, int rows, float* __restrict__ out) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // (row, t, c6)
  if (idx >= rows * 480) return;
  const int c6 = idx % 6, t = (idx / 6) % 80, r = idx / 480;
  const float* src = c6 < 2 ? loc : (c6 < 4 ? yaw : vel);
  out[idx] = src[(size_t)r * 160 + t * 2 + (c6 & 1)];
}

// agent predictor (agent_predictor.py:17-29): the agents' encoder rows gathered, three MLPLayer heads, interleaved -> out->prediction
void agent_predictor_layerwise(Fwd& f, int rows) {
  Ctx* c = f.c;
  float* Xa = A_alloc<float>(c, (size_t)rows * 128);
  launch(c, "gather_rows_kernel", gather_rows_kernel, dim3(cdiv((long long)rows * 128, 256)), dim3(256), 0, (const float*)f.ENC, 128, Xa, 128, rows, 128,
         f.A - 1, f.N, 1);
  float* o3[3];
  for (int i = 0; i < 3; ++i) {
    o3[i] = A_alloc<float>(c, (size_t)rows * 160);
    mlp_layer(f, Xa, 128, rows, c->m.predictor[i], o3[i], 160, f.fp32);
  }
  launch(c, "interleave_traj_kernel", interleave_traj_kernel, dim3(cdiv((long long)rows * 480, 256)), dim3(256), 0, (const float*)o3[0], (const float*)o3[1],
         (const float*)o3[2], rows, f.out->prediction);
}

// the decoder blocks as GEMM / attention launches on f.Q in place (fp32 mode, RIFT_DEC_UNFUSED=1, shapes outside the fused kernel's)
void decoder_layerwise(Fwd& f, float dp) {
  Ctx* c = f.c;
  const int bs = f.bs, R = f.R, N = f.N, M = f.M, nL = f.nL, nQ = f.nQ, nT = f.nT;
  float* DQKV = A_alloc<float>(c, (size_t)nQ * 384);
  float* DAO = A_alloc<float>(c, (size_t)nQ * 128);
  float* DQc = A_alloc<float>(c, (size_t)nQ * 128);
  float* DH = A_alloc<float>(c, (size_t)nQ * 512);
  float* KVm = A_alloc<float>(c, (size_t)nT * 256);
  const int n_layers = f.kp.dec_now[0].l1;      // (RIFT_DEC_LAYERS)
  for (int i = 0; i < n_layers; ++i) {
    const DecoderBlockW& p = c->m.dec.decoder_blocks[i];
    // ---- r2r self attention over the R reference lines of each (scene, mode), with the mask quirk
    GemmP g = mk(f.Q, 128, nQ, *p.r2r_qkv, DQKV, 384);
    g.pro = PRO_LN; g.pg = p.norm[0].g; g.pb = p.norm[0].b;
    gemm(c, g, *p.r2r_qkv, f.fp32);
    {
      MhaP m; memset(&m, 0, sizeof(m));
      m.Q = DQKV; m.ldq = 384; m.K = DQKV + 128; m.V = DQKV + 256; m.ldkv = 384; m.O = DAO; m.ldo = 128;
      m.nb_outer = bs; m.nb_inner = M; m.H = 4; m.Lq = R; m.Lk = R;
      m.q_outer = R * M; m.q_inner = 1; m.q_stride = M; m.kv_outer = R * M; m.kv_inner = 1; m.kv_stride = M;
      m.o_outer = R * M; m.o_inner = 1; m.o_stride = M;
      m.mask = f.q_kpm; m.mask_quirk = 1; m.mask_mod = f.q_bs; m.mask_off = f.q_off * M;   // tgt_key_padding_mask.repeat(M, 1), planning_decoder.py:56-60
      if (dp > 0.f) { m.dropout_p = dp; m.seed = f.seed; m.stream = f.next_stream(); }
      run_mha(c, m, f.fp32);
    }
    GemmP g2 = mk(DAO, 128, nQ, *p.r2r_out, f.Q, 128);
    g2.residual = f.Q; g2.ldr = 128;
    if (dp > 0.f) { g2.dropout_p = dp; g2.seed = f.seed; g2.stream = f.next_stream(); }
    gemm(c, g2, *p.r2r_out, f.fp32);
    // ---- m2m self attention over the 12 modes: q = k = (h + m_pos) W + b, v = h W + b
    bool fill_mp;
    float* MP = wconst_get(c, c->wc.mp[i], (size_t)M * 384, f.fp32, &fill_mp);
    if (fill_mp) gemm(c, mk(c->m.dec.m_pos, 128, M, *p.m2m_qk0, MP, 384), *p.m2m_qk0, f.fp32);
    GemmP g3 = mk(f.Q, 128, nQ, *p.m2m_qkv, DQKV, 384);
    g3.pro = PRO_LN; g3.pg = p.norm[1].g; g3.pb = p.norm[1].b;
    g3.gbias = MP; g3.gb_div = 1; g3.gb_mod = M;
    gemm(c, g3, *p.m2m_qkv, f.fp32);
    {
      MhaP m; memset(&m, 0, sizeof(m));
      m.Q = DQKV; m.ldq = 384; m.K = DQKV + 128; m.V = DQKV + 256; m.ldkv = 384; m.O = DAO; m.ldo = 128;
      m.nb_outer = nL; m.nb_inner = 1; m.H = 4; m.Lq = M; m.Lk = M;
      m.q_outer = M; m.q_stride = 1; m.kv_outer = M; m.kv_stride = 1; m.o_outer = M; m.o_stride = 1;
      if (dp > 0.f) { m.dropout_p = dp; m.seed = f.seed; m.stream = f.next_stream(); }
      run_mha(c, m, f.fp32);
    }
    GemmP g4 = mk(DAO, 128, nQ, *p.m2m_out, f.Q, 128);
    g4.residual = f.Q; g4.ldr = 128; g4.rowzero = f.r_kpm; g4.rz_div = M;   // rows of padded ref lines become 0 (:65-72)
    if (dp > 0.f) { g4.dropout_p = dp; g4.seed = f.seed; g4.stream = f.next_stream(); }
    gemm(c, g4, *p.m2m_out, f.fp32);
    // ---- cross attention: R*12 queries per scene against the encoder tokens
    GemmP g5 = mk(f.Q, 128, nQ, *p.cross_q, DQc, 128);
    g5.pro = PRO_LN; g5.pg = p.norm[2].g; g5.pb = p.norm[2].b;
    gemm(c, g5, *p.cross_q, f.fp32);
    gemm(c, mk(f.ENC, 128, nT, *p.cross_kv, KVm, 256), *p.cross_kv, f.fp32);
    {
      MhaP m; memset(&m, 0, sizeof(m));
      m.Q = DQc; m.ldq = 128; m.K = KVm; m.V = KVm + 128; m.ldkv = 256; m.O = DAO; m.ldo = 128;
      m.nb_outer = bs; m.nb_inner = 1; m.H = 4; m.Lq = R * M; m.Lk = N;
      m.q_outer = R * M; m.q_stride = 1; m.kv_outer = N; m.kv_stride = 1; m.o_outer = R * M; m.o_stride = 1;
      m.mask = f.kpm; m.mask_mod = 1;
      if (dp > 0.f) { m.dropout_p = dp; m.seed = f.seed; m.stream = f.next_stream(); }
      run_mha(c, m, f.fp32);
    }
    GemmP g6 = mk(DAO, 128, nQ, *p.cross_out, f.Q, 128);
    g6.residual = f.Q; g6.ldr = 128;
    if (dp > 0.f) { g6.dropout_p = dp; g6.seed = f.seed; g6.stream = f.next_stream(); }
    gemm(c, g6, *p.cross_out, f.fp32);
    // ---- FFN
    GemmP g7 = mk(f.Q, 128, nQ, *p.ffn0, DH, 512);
    g7.pro = PRO_LN; g7.pg = p.norm[3].g; g7.pb = p.norm[3].b; g7.act = ACT_RELU;
    if (dp > 0.f) { g7.dropout_p = dp; g7.seed = f.seed; g7.stream = f.next_stream(); }
    gemm(c, g7, *p.ffn0, f.fp32);
    GemmP g8 = mk(DH, 512, nQ, *p.ffn3, f.Q, 128);
    g8.residual = f.Q; g8.ldr = 128;
    if (dp > 0.f) { g8.dropout_p = dp; g8.seed = f.seed; g8.stream = f.next_stream(); }
    gemm(c, g8, *p.ffn3, f.fp32);
  }
}

// policy head: cat_x_proj -> pi_head's first Linear -> LayerNorm, ReLU, Linear, masked logits as three launches
void policy_head_layerwise(Ctx* c, const Ctx::Head& h) {
  const int nQ = h.nQ, M = 12;
  GemmP g = mk(h.Q, 128, nQ, *c->m.dec.cat_x_proj_q, h.QF, 128);
  g.gbias = h.x0p; g.gb_div = h.R * M; g.gb_mod = 0;
  gemm(c, g, *c->m.dec.cat_x_proj_q, h.fp32);
  // pi head: first Linear straight from the live (trainable) fp32 parameters, exact-fp32 MFMA
  PWShape w; w.N = 128; w.K = 128; w.Kp = 128; w.Npad = 128; w.bias = c->pi.b0;
  gemm(c, mk(h.QF, 128, nQ, w, h.Hpi, 128), (const void*)c->pi.w0, true);
  launch(c, "pi_tail_kernel", pi_tail_kernel, dim3(cdiv(nQ, 4)), dim3(256), 0, (const float*)h.Hpi, nQ, M, c->pi.ln_g,
         c->pi.ln_b, c->pi.w3, c->pi.b3,
         (const uint8_t*)h.r_kpm, 1e-5f, h.prob, c->nonfinite.get());
}

// trajectory heads on q_final: MLPLayer(128, 256, 160) three times as in mlp_layer(), on the buffers the trunk reserved (traj_heads_reserve)
void traj_heads_reserve(Ctx* c, Ctx::Head& h) {
  for (int i = 0; i < 3; ++i) { h.oT[i] = A_alloc<float>(c, (size_t)h.nQ * 256); h.o3[i] = A_alloc<float>(c, (size_t)h.nQ * 160); }
}
void traj_heads_layerwise(Ctx* c, const Ctx::Head& h) {
  const int nQ = h.nQ;
  for (int i = 0; i < 3; ++i) {
    const PW& w0 = *c->m.dec.head[i].l0;
    const PW& w3 = *c->m.dec.head[i].l3;
    float* T = h.oT[i];
    gemm(c, mk(h.QF, 128, nQ, w0, T, w0.N), w0, h.fp32);
    GemmP g = mk(T, w0.N, nQ, w3, h.o3[i], 160);
    g.pro = PRO_LN; g.pg = c->m.dec.head[i].ln.g; g.pb = c->m.dec.head[i].ln.b; g.pro_relu = 1;
    gemm(c, g, w3, h.fp32);
  }
  launch(c, "interleave_traj_kernel", interleave_traj_kernel, dim3(cdiv((long long)nQ * 480, 256)), dim3(256), 0, (const float*)h.o3[0], (const float*)h.o3[1],
         (const float*)h.o3[2], nQ, h.traj);
}

// hidden_proj / ref_free_decoder on the ego token (pluto_model.py:173-180)
void ego_heads_layerwise(Fwd& f) {
  Ctx* c = f.c;
  const RiftOutputs* out = f.out;
  const int bs = f.bs, N = f.N;
  if (out->hidden) {
    float* Th = A_alloc<float>(c, (size_t)bs * 128);
    GemmP g = mk(f.ENC, N * 128, bs, *c->m.hidden_proj0, Th, 128);
    g.act = ACT_RELU;
    gemm(c, g, *c->m.hidden_proj0, f.fp32);
    gemm(c, mk(Th, 128, bs, *c->m.hidden_proj2, out->hidden, 128), *c->m.hidden_proj2, f.fp32);
  }
  if (f.need_traj && out->ref_free_trajectory)
    mlp_layer(f, f.ENC, N * 128, bs, c->m.ref_free_decoder, out->ref_free_trajectory, 320, f.fp32);
}
