// rift_model_load (included by engine.hip inside the build, behind the headers of the kernels it packs for): ONE walk over the module
// tree of the reference.  Each module kind has one function here that names the module's tensors: it looks every raw tensor up once,
// packs the GEMM images, writes the module's fields of Model (model.h) and, where a wave-private kernel packs from the raw fp32 tensors,
// that kernel's *Src fields from the same local pointers.  Parameter names are spelt in this file only, each once; the images have no
// names -- Ctx::pw owns them, the Model field that holds the pointer is the name.
#pragma once
#include <type_traits>

namespace RIFT_NS {
namespace {

// the image of one linear map from (a window of) an fp32 matrix or Conv1d weight, into a PW the caller owns
int pack_image(Ctx* c, PW& w, const float* src, int n_src, int N, int K, int src_row_off, int src_col_off, int src_ld, int conv_C,
               int tap_lo, int tap_n, const float* bias) {
  w.N = N; w.K = K; w.Kp = (K + 31) & ~31; w.Npad = (N + 15) & ~15; w.bias = bias;
  const size_t cnt = (size_t)w.Npad * w.Kp;
  DEVCHK(c, w.bf.reserve(cnt));
  DEVCHK(c, w.f32.reserve(cnt));
  const int blocks = cdiv((long long)cnt, 256);
  hipLaunchKernelGGL(pack_weight_kernel<true>, dim3(blocks), dim3(256), 0, c->stream, src + src_col_off, (void*)w.bf.get(), n_src, K,
                     w.Npad, w.Kp, conv_C, tap_lo, tap_n, src_row_off, src_ld);
  hipLaunchKernelGGL(pack_weight_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, src + src_col_off, (void*)w.f32.get(),
                     n_src, K, w.Npad, w.Kp, conv_C, tap_lo, tap_n, src_row_off, src_ld);
  return RIFT_OK;
}

const std::string HE = "agent_encoder.history_encoder", PD = "planning_decoder";

struct Load {
  Ctx* c;
  std::unordered_map<std::string, const RiftTensorDesc*> by_name;      // the caller's descriptors: they live for the call
  int rc = RIFT_OK;                                                    // the first failure (its message is c->err); the walk goes on without packing
  // what the pack kernels of the wave-private kernels read: raw fp32 tensors, launched on by pack_streams behind a walk that found them all
  NatL0WSrc l0w = {}; NatL1WSrc l1w = {}; NatL2WSrc l2w = {}; EncWSrc encw = {}; DecWSrc decw = {};
  FoWSrc fow[3] = {};      // pos_emb, map_encoder.speed_limit_emb, planning_decoder.r_pos_emb (the three embeddings of the fused launch)
  PeWSrc pew[2] = {};      // map_encoder.polygon_encoder, planning_decoder.r_encoder

  Load(Ctx* ctx, const RiftTensorDesc* params, int n) : c(ctx) {
    by_name.reserve((size_t)n);
    for (int i = 0; i < n; ++i) by_name[params[i].name] = &params[i];
  }
  std::nullptr_t fail(int code, const std::string& msg) { if (rc == RIFT_OK) { rc = code; c->err = msg; } return nullptr; }
  bool hipok(int e, const char* what) {
    if (e != hipSuccess) fail(RIFT_ERR_HIP, std::string(what) + ": " + hipGetErrorString((hipError_t)e));
    return e == hipSuccess;
  }

  // ---- THE lookup: every tensor the load reads is required, with its rank (only a BatchNorm's num_batches_tracked is optional: bn) ----
  const RiftTensorDesc* need(const std::string& name, int ndim) {
    auto it = by_name.find(name);
    if (it == by_name.end()) return fail(RIFT_ERR_ARG, "missing parameter: " + name);
    if (it->second->ndim != ndim) return fail(RIFT_ERR_ARG, "parameter " + name + " has " + std::to_string(it->second->ndim) + " dimensions, not " + std::to_string(ndim));
    return it->second;
  }
  const float* vec(const std::string& name, int ndim = 1) { const RiftTensorDesc* t = need(name, ndim); return t ? (const float*)t->data : nullptr; }
  struct Lin { const float *w = nullptr, *b = nullptr; const int64_t* shape = nullptr; };      // a weight (N, K) or (N, C, 3) and its bias (N)
  Lin matrix(const std::string& wname, const std::string& bname, int ndim = 2) {
    Lin l;
    if (const RiftTensorDesc* t = need(wname, ndim)) { l.w = (const float*)t->data; l.shape = t->shape; }
    if (!bname.empty()) l.b = vec(bname);
    return l;
  }
  Lin linear(const std::string& p) { return matrix(p + ".weight", p + ".bias"); }                        // nn.Linear
  Lin in_proj(const std::string& p) { return matrix(p + ".in_proj_weight", p + ".in_proj_bias"); }       // nn.MultiheadAttention: (384, 128) = q | k | v
  Lin conv(const std::string& p, bool with_bias = true) {                                                // nn.Conv1d, kernel 3
    Lin l = matrix(p + ".weight", with_bias ? p + ".bias" : "", 3);
    if (l.w && l.shape[2] != 3) fail(RIFT_ERR_ARG, "parameter " + p + ".weight is no Conv1d weight of 3 taps");
    return l;
  }

  // ---- packing: null (and rc set) on failure, or behind an earlier one ----
  PW* pack(const float* src, int n_src, int N, int K, int row_off, int col_off, int ld, int conv_C, int tap_lo, int tap_n, const float* bias) {
    if (rc != RIFT_OK) return nullptr;
    c->pw.emplace_back();
    const int e = pack_image(c, c->pw.back(), src, n_src, N, K, row_off, col_off, ld, conv_C, tap_lo, tap_n, bias);
    if (e != RIFT_OK) { rc = e; return nullptr; }
    return &c->pw.back();
  }
  PW* pack_linear(const Lin& l) { return rc ? nullptr : pack(l.w, (int)l.shape[0], (int)l.shape[0], (int)l.shape[1], 0, 0, (int)l.shape[1], 0, 0, 0, l.b); }
  // rows [r0, r0 + n_src) as a GEMM with N output columns (rows beyond n_src are zero)
  PW* pack_rows(const Lin& l, int r0, int n_src, int N, bool with_bias = true) {
    return rc ? nullptr : pack(l.w, n_src, N, (int)l.shape[1], r0, 0, (int)l.shape[1], 0, 0, 0, with_bias ? l.b + r0 : nullptr);
  }
  // columns [c0, c0 + K): the halves of a Linear over a concatenation; the bias goes with one of them
  PW* pack_cols(const Lin& l, int c0, int K, bool with_bias) {
    return rc ? nullptr : pack(l.w, (int)l.shape[0], (int)l.shape[0], K, 0, c0, (int)l.shape[1], 0, 0, 0, with_bias ? l.b : nullptr);
  }
  // taps [tap_lo, tap_lo + tap_n) of a Conv1d, tap-major: [N][tap_n * C]
  PW* pack_conv(const Lin& l, int tap_lo = 0, int tap_n = 3) {
    return rc ? nullptr : pack(l.w, (int)l.shape[0], (int)l.shape[0], tap_n * (int)l.shape[1], 0, 0, 0, (int)l.shape[1], tap_lo, tap_n, l.b);
  }
  // rows [r0, r0 + n) of four (N_src, K) matrices stacked into one (4 n, K) GEMM weight, with the stacked bias (owned by the image)
  PW* pack_stacked_rows(const Lin (&l)[4], int r0, int n) {
    if (rc != RIFT_OK) return nullptr;
    if (n % 16) return fail(RIFT_ERR_ARG, "pack_stacked_rows: n % 16");
    c->pw.emplace_back();
    PW& w = c->pw.back();
    const int K = (int)l[0].shape[1];
    w.N = 4 * n; w.K = K; w.Kp = (K + 31) & ~31; w.Npad = (w.N + 15) & ~15;
    const size_t cnt = (size_t)w.Npad * w.Kp;
    if (!hipok(w.bf.reserve(cnt), "device memory of a packed image") || !hipok(w.f32.reserve(cnt), "device memory of a packed image") || !hipok(w.own_bias.reserve((size_t)w.N), "device memory of a stacked bias")) return nullptr;
    for (int i = 0; i < 4; ++i) {
      if (l[i].shape[1] != K) return fail(RIFT_ERR_ARG, "pack_stacked_rows: matrices of different widths");
      const size_t off = (size_t)i * n * w.Kp;     // a 16-row block of a fragment-major image starts at the row-major offset of its first row
      const int blocks = cdiv((long long)n * w.Kp, 256);
      hipLaunchKernelGGL(pack_weight_kernel<true>, dim3(blocks), dim3(256), 0, c->stream, l[i].w, (void*)(w.bf.get() + off), n, K, n, w.Kp, 0, 0, 0, r0, K);
      hipLaunchKernelGGL(pack_weight_kernel<false>, dim3(blocks), dim3(256), 0, c->stream, l[i].w, (void*)(w.f32.get() + off), n, K, n, w.Kp, 0, 0, 0, r0, K);
      if (!hipok(hipMemcpyAsync(w.own_bias.get() + (size_t)i * n, l[i].b + r0, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream), "copy of a stacked bias")) return nullptr;
    }
    w.bias = w.own_bias.get();
    return &w;
  }
  // + the hidden-layer-operand image of a packed weight (the fused scene encoder's fc2: its A rows are GELU outputs, common.h: gelu4_hid)
  PW* pack_hid(PW* w) {
    if (!w) return nullptr;
    const size_t cnt = (size_t)w->Npad * w->Kp;
    if (!hipok(w->hid.reserve(cnt), "device memory of a hidden-layer image")) return nullptr;
    hipLaunchKernelGGL(pack_weight_hid_kernel, dim3(cdiv((long long)cnt, 256)), dim3(256), 0, c->stream, (const float*)w->f32.get(), w->hid.get(), w->Npad, w->Kp);
    return w;
  }

  // ---- the module kinds ----
  LayerNormW ln(const std::string& p) { return {vec(p + ".weight"), vec(p + ".bias")}; }
  BatchNormW bn(const std::string& p) {
    auto nb = by_name.find(p + ".num_batches_tracked");
    return {vec(p + ".weight"), vec(p + ".bias"), (float*)vec(p + ".running_mean"), (float*)vec(p + ".running_var"), nb == by_name.end() ? nullptr : (long long*)nb->second->data};
  }
  MLPLayerW mlp(const std::string& p) { return {pack_linear(linear(p + ".mlp.0")), pack_linear(linear(p + ".mlp.3")), ln(p + ".mlp.1")}; }

  FourierW fourier(const std::string& p, int D, FoWSrc* src = nullptr) {      // src: the embedding also runs wave-private (fo_w.h)
    FoWSrc none = {}; FoWSrc& q = src ? *src : none;
    FourierW f; f.D = q.D = D; f.freqs = q.freqs = vec(p + ".freqs.weight", 2);
    for (int d = 0; d < D; ++d) {
      const std::string m = p + ".mlps." + std::to_string(d);
      const Lin l0 = linear(m + ".0"), l3 = linear(m + ".3");      // .0 is (128, 129): the fused kernels take it as K = 128 (lo) + a rank-1 term (last)
      f.mlps[d] = {pack_linear(l0), pack_cols(l0, 0, 128, true), pack_cols(l0, 128, 1, false), pack_linear(l3), ln(m + ".1")};
      q.w0[d] = l0.w; q.b0[d] = l0.b; q.lng[d] = f.mlps[d].ln.g; q.lnb[d] = f.mlps[d].ln.b; q.w3[d] = l3.w; q.b3[d] = l3.b;
    }
    const Lin out = linear(p + ".to_out.2");
    f.out_ln = ln(p + ".to_out.0"); f.out = pack_linear(out);
    q.og = f.out_ln.g; q.ob = f.out_ln.b; q.wo = out.w; q.bo = out.b;
    return f;
  }

  PointsEncoderW points_encoder(const std::string& p, PeWSrc& q, int Cin) {
    const Lin f0 = linear(p + ".first_mlp.0"), f3 = linear(p + ".first_mlp.3"), s0 = linear(p + ".second_mlp.0"), s3 = linear(p + ".second_mlp.3");
    q = {f0.w, f3.w, s0.w, Cin};
    return {pack_linear(f0), pack_linear(f3), pack_cols(s0, 0, 256, true), pack_cols(s0, 256, 256, false), pack_linear(s3),      // second_mlp.0 over [feat | pool]
            bn(p + ".first_mlp.1"), bn(p + ".second_mlp.1")};
  }

  void nat_block(const std::string& p, NatBlockW& k, NatBlkSrc& q) {
    const Lin qkv = linear(p + ".attn.qkv"), proj = linear(p + ".attn.proj"), fc1 = linear(p + ".mlp.fc1"), fc2 = linear(p + ".mlp.fc2");
    k = {ln(p + ".norm1"), ln(p + ".norm2"), pack_linear(qkv), pack_linear(proj), pack_linear(fc1), pack_linear(fc2), vec(p + ".attn.rpb", 2)};
    q = {k.norm1.g, k.norm1.b, qkv.w, qkv.b, k.rpb, proj.w, proj.b, k.norm2.g, k.norm2.b, fc1.w, fc1.b, fc2.w, fc2.b};
  }
  template <class Src>      // NatL0WSrc / NatL1WSrc / NatL2WSrc: the level's wave-private kernel
  void nat_level(int lv, Src& q) {
    const std::string n = std::to_string(lv), l = HE + ".levels." + n;
    NatLevelW& k = c->m.agent.levels[lv];
    for (int b = 0; b < 2; ++b) nat_block(l + ".blocks." + std::to_string(b), k.blocks[b], q.blk[b]);
    k.norm = ln(HE + ".norm" + n); q.fn_g = k.norm.g; q.fn_b = k.norm.b;
    k.lateral = pack_conv(conv(HE + ".lateral_convs." + n));
    if constexpr (!std::is_same<Src, NatL2WSrc>::value) {      // levels 0 and 1: downsample (a Conv1d without bias, then LayerNorm)
      const Lin red = conv(l + ".downsample.reduction", false);
      k.reduction = pack_conv(red); k.ds_norm = ln(l + ".downsample.norm");
      q.w_ds = red.w; q.ds_g = k.ds_norm.g; q.ds_b = k.ds_norm.b;
    }
  }
  void history_encoder() {
    const Lin tok = conv(HE + ".embed.proj"), fpn = conv(HE + ".fpn_conv");
    c->m.agent.embed_proj = pack_conv(tok); l0w.w_tok = tok.w; l0w.b_tok = tok.b;
    nat_level(0, l0w); nat_level(1, l1w); nat_level(2, l2w);
    c->m.agent.fpn_last = pack_conv(fpn, 0, 2);      // fpn_conv at the last step: taps 0, 1 only -> [128][256]
  }

  void ego_state_emb() {
    const std::string p = "agent_encoder.ego_state_emb";
    const Lin in = in_proj(p + ".attn");
    c->m.agent.ego = {vec(p + ".query", 3), vec(p + ".pos_embed", 3), pack_rows(in, 0, 128, 128), pack_rows(in, 128, 256, 256), pack_linear(linear(p + ".attn.out_proj"))};
    if (!hipok(c->img.ego_w.reserve(6 * 128), "device memory of the ego tables") || !hipok(c->img.ego_b.reserve(6 * 128), "device memory of the ego tables")) return;
    for (int i = 0; i < 6; ++i) {      // the six Linear(1, 128) of StateAttentionEncoder as one (6, 128) table each
      const Lin l = linear(p + ".linears." + std::to_string(i));
      if (rc != RIFT_OK) return;
      if (!hipok(hipMemcpyAsync(c->img.ego_w.get() + i * 128, l.w, 128 * 4, hipMemcpyDeviceToDevice, c->stream), "copy into the ego tables") ||
          !hipok(hipMemcpyAsync(c->img.ego_b.get() + i * 128, l.b, 128 * 4, hipMemcpyDeviceToDevice, c->stream), "copy into the ego tables")) return;
    }
  }

  void scene_block(int i) {
    const std::string p = "encoder_blocks." + std::to_string(i);
    const Lin in = in_proj(p + ".attn"), out = linear(p + ".attn.out_proj"), fc1 = linear(p + ".mlp.fc1"), fc2 = linear(p + ".mlp.fc2");
    SceneBlockW& k = c->m.encoder_blocks[i];
    k = {ln(p + ".norm1"), ln(p + ".norm2"), pack_rows(in, 0, 384, 384), pack_linear(out), pack_linear(fc1), pack_hid(pack_linear(fc2))};
    encw.l[i] = {k.norm1.g, k.norm1.b, in.w, in.b, out.w, out.b, k.norm2.g, k.norm2.b, fc1.w, fc1.b, fc2.w, fc2.b};
  }

  Lin decoder_block(int i) {      // returns cross_attn's in-projection: its k | v rows also go into kv_all and the encoder kernel's tail
    const std::string p = PD + ".decoder_blocks." + std::to_string(i);
    const Lin r2r = in_proj(p + ".r2r_attn"), r2ro = linear(p + ".r2r_attn.out_proj"), m2m = in_proj(p + ".m2m_attn"), m2mo = linear(p + ".m2m_attn.out_proj");
    const Lin cr = in_proj(p + ".cross_attn"), cro = linear(p + ".cross_attn.out_proj"), f1 = linear(p + ".ffn.0"), f2 = linear(p + ".ffn.3");
    DecoderBlockW& k = c->m.dec.decoder_blocks[i];
    DecWSrc::L& q = decw.l[i];
    for (int j = 0; j < 4; ++j) { k.norm[j] = ln(p + ".norm" + std::to_string(j + 1)); q.ln[2 * j] = k.norm[j].g; q.ln[2 * j + 1] = k.norm[j].b; }
    k.r2r_qkv = pack_rows(r2r, 0, 384, 384); k.r2r_out = pack_linear(r2ro);
    k.m2m_qkv = pack_rows(m2m, 0, 384, 384); k.m2m_qk0 = pack_rows(m2m, 0, 256, 384, false); k.m2m_out = pack_linear(m2mo);      // qk0: q | k of the mode positions, no bias
    k.cross_q = pack_rows(cr, 0, 128, 128); k.cross_kv = pack_rows(cr, 128, 256, 256); k.cross_out = pack_linear(cro);
    k.ffn0 = pack_linear(f1); k.ffn3 = pack_linear(f2);
    q.r2r_w = r2r.w; q.r2r_b = r2r.b; q.r2ro_w = r2ro.w; q.r2ro_b = r2ro.b; q.m2m_w = m2m.w; q.m2m_b = m2m.b; q.m2mo_w = m2mo.w; q.m2mo_b = m2mo.b;
    q.c_w = cr.w; q.c_b = cr.b; q.co_w = cro.w; q.co_b = cro.b; q.f1_w = f1.w; q.f1_b = f1.b; q.f2_w = f2.w; q.f2_b = f2.b;
    encw.dkv_w[i] = cr.w; encw.dkv_b[i] = cr.b;
    return cr;
  }
  void planning_decoder() {
    auto& m = c->m.dec;
    m.r_encoder = points_encoder(PD + ".r_encoder", pew[1], 6);
    m.r_pos_emb = fourier(PD + ".r_pos_emb", 3, &fow[2]);
    const Lin qp = linear(PD + ".q_proj"), cx = linear(PD + ".cat_x_proj");      // each over a concatenation: [r | m], [q | x]
    m.q_proj_r = pack_cols(qp, 0, 128, true); m.q_proj_m = pack_cols(qp, 128, 128, false);
    m.m_emb = vec(PD + ".m_emb", 4); m.m_pos = decw.m_pos = vec(PD + ".m_pos", 3);
    Lin cross[4];
    for (int i = 0; i < 4; ++i) cross[i] = decoder_block(i);
    m.kv_all = pack_stacked_rows(cross, 128, 256);
    m.cat_x_proj_q = pack_cols(cx, 0, 128, true); m.cat_x_proj_x = pack_cols(cx, 128, 128, false);
    const char* three[3] = {"loc", "yaw", "vel"};
    for (int i = 0; i < 3; ++i) {
      c->m.predictor[i] = mlp(std::string("agent_predictor.") + three[i] + "_predictor");
      m.head[i] = mlp(PD + "." + three[i] + "_head");
    }
    const std::string ph = PD + ".pi_head.mlp.";      // (the trainable tensors: the head and both backward entries of shared.hip read them live through these pointers)
    c->pi = {vec(ph + "0.weight", 2), vec(ph + "0.bias"), vec(ph + "1.weight"), vec(ph + "1.bias"), vec(ph + "3.weight", 2), vec(ph + "3.bias")};
  }

  void walk() {      // PlanningModel
    Model& m = c->m;
    history_encoder();
    ego_state_emb();
    m.agent.type_emb = vec("agent_encoder.type_emb.weight", 2);
    m.map.polygon_encoder = points_encoder("map_encoder.polygon_encoder", pew[0], 10);
    m.map.speed_limit_emb = fourier("map_encoder.speed_limit_emb", 1, &fow[1]);
    m.map.type_emb = vec("map_encoder.type_emb.weight", 2); m.map.on_route_emb = vec("map_encoder.on_route_emb.weight", 2);
    m.map.traffic_light_emb = vec("map_encoder.traffic_light_emb.weight", 2); m.map.unknown_speed_emb = vec("map_encoder.unknown_speed_emb.weight", 2);
    m.stat.obj_encoder = fourier("static_objects_encoder.obj_encoder", 2);
    m.stat.type_emb = vec("static_objects_encoder.type_emb.weight", 2);
    m.pos_emb = fourier("pos_emb", 3, &fow[0]);
    for (int i = 0; i < 4; ++i) scene_block(i);
    m.norm = ln("norm"); encw.fn_g = m.norm.g; encw.fn_b = m.norm.b;
    planning_decoder();
    m.hidden_proj0 = pack_linear(linear("hidden_proj.0")); m.hidden_proj2 = pack_linear(linear("hidden_proj.2"));
    m.ref_free_decoder = mlp("ref_free_decoder");
  }

  // behind a walk that found every tensor: the weight streams / parameter blocks of the wave-private kernels, from the raw fp32 tensors
  int pack_streams() {
    Ctx::Images& g = c->img;
    hipStream_t s = c->stream;
    DEVCHK(c, g.l0w_img.reserve((size_t)L0W_NFRAG * 512)); DEVCHK(c, g.l0w_par.reserve(L0W_NPAR));
    l0w_pack(l0w, g.l0w_img.get(), g.l0w_par.get(), s);
    DEVCHK(c, g.l1w_img.reserve((size_t)L1W_NFRAG * 512)); DEVCHK(c, g.l1w_par.reserve(L1W_NPAR));
    l1w_pack(l1w, g.l1w_img.get(), g.l1w_par.get(), s);
    DEVCHK(c, g.l2w_img.reserve((size_t)2 * L2W_BLK_FRAGS * 512)); DEVCHK(c, g.l2w_par.reserve(L2W_NPAR));
    l2w_pack(l2w, g.l2w_img.get(), g.l2w_par.get(), s);
    DEVCHK(c, g.encw_img.reserve((size_t)(4 * ENCW_LAYER_FRAGS + ENCW_TAIL_FRAGS) * 512)); DEVCHK(c, g.encw_par.reserve(ENCW_NPAR));
    encw_pack(encw, g.encw_img.get(), g.encw_par.get(), s);
    for (int i = 0; i < 3; ++i) {
      DEVCHK(c, g.fow_img[i].reserve((size_t)7 * 32 * 512)); DEVCHK(c, g.fow_par[i].reserve(FOW_NPAR));
      fow_pack(fow[i], g.fow_img[i].get(), g.fow_par[i].get(), s);
    }
    for (int i = 0; i < 2; ++i) {      // W1 | W2 | W3a streams of the two PointsEncoders (pass B)
      DEVCHK(c, g.pew_img[i].reserve((size_t)PEW_FRAGS * 512));
      pew_pack(pew[i], g.pew_img[i].get(), s);
    }
    DEVCHK(c, g.decw_img.reserve((size_t)4 * DECW_LAYER_FRAGS * 512)); DEVCHK(c, g.decw_par.reserve((size_t)4 * DECW_PAR_LAYER));
    decw_pack(decw, g.decw_img.get(), g.decw_par.get(), s);
    // chunked in_proj image for the fused encoder kernel: per 2-head chunk (q_h0 | k_h0 | q_h1 | k_h1 | v_h0 | v_h1).  The row table is
    // static data, so the asynchronous copy may read it whenever it runs: no wait on the stream.
    static const std::vector<int> idx = [] {
      std::vector<int> v(384);
      for (int ch = 0; ch < 2; ++ch)
        for (int seg = 0; seg < 6; ++seg) {
          const int part = seg < 4 ? (seg & 1) : 2;                 // 0 q, 1 k, 2 v
          const int head = 2 * ch + (seg < 4 ? (seg >> 1) : (seg - 4));
          for (int d = 0; d < 32; ++d) v[ch * 192 + seg * 32 + d] = part * 128 + head * 32 + d;
        }
      return v;
    }();
    DEVCHK(c, g.enc_idx.reserve(384));
    HIPCHK(c, hipMemcpyAsync(g.enc_idx.get(), idx.data(), 384 * sizeof(int), hipMemcpyHostToDevice, s));
    for (int i = 0; i < 4; ++i) {
      DEVCHK(c, g.enc_wqkv[i].reserve(384 * 128)); DEVCHK(c, g.enc_bqkv[i].reserve(384));
      hipLaunchKernelGGL(pack_rows_indexed_kernel, dim3(cdiv(384 * 128, 256)), dim3(256), 0, s, encw.l[i].w_in, encw.l[i].b_in, (const int*)g.enc_idx.get(),
                         384, 128, g.enc_wqkv[i].get(), g.enc_bqkv[i].get());
    }
    return RIFT_OK;
  }
};

}  // namespace
}  // namespace RIFT_NS
