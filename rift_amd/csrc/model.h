// The model's operands, written ONCE by rift_model_load's walk over the module tree (model_load.h): plain structs of pointers that mirror
// the module tree of the reference.  Parameter names exist at load only; the forward reads these fields.  A `const PW*` points at an
// element of Ctx::pw (packed images), a `const float*` at a tensor of the caller's state dict.
#pragma once
#include "launch.h"
#include "opfmt.h"

namespace RIFT_NS {

struct PWShape { int N = 0, K = 0, Kp = 0, Npad = 0; const float* bias = nullptr; };
struct PW : PWShape {   // packed weight image of one linear map Y = X W^T (+ b); owns its images, lives in Ctx::pw and is handed on by reference
  DevBuf<unsigned short> bf; DevBuf<float> f32;
  DevBuf<unsigned short> hid;   // (fc2 weights of the fused encoder only) the same image in hidden-layer operand words (opfmt.h); pack_hid
  DevBuf<float> own_bias;       // (pack_stacked_rows only) the stacked bias that `bias` points to
};

struct LayerNormW { const float *g = nullptr, *b = nullptr; };
struct BatchNormW {
  const float *g = nullptr, *b = nullptr; float *mean = nullptr, *var = nullptr;      // (the running statistics are written by a train forward)
  long long* num_batches = nullptr;                                                   // num_batches_tracked: the only optional tensor
};
struct MLPLayerW { const PW *l0 = nullptr, *l3 = nullptr; LayerNormW ln; };           // mlp.0 -> mlp.1 (LayerNorm) -> ReLU -> mlp.3
struct FourierW {                                                                       // FourierEmbedding
  int D = 0; const float* freqs = nullptr;
  struct Dim { const PW *l0 = nullptr, *lo = nullptr, *last = nullptr, *l3 = nullptr; LayerNormW ln; } mlps[3];      // .0 (layer-wise) = .0.lo | .0.last (fused)
  LayerNormW out_ln; const PW* out = nullptr;                                           // to_out.0, to_out.2
};
struct PointsEncoderW {
  const PW *first0 = nullptr, *first3 = nullptr, *feat = nullptr, *pool = nullptr, *second3 = nullptr;      // (feat | pool: the column halves of second_mlp.0)
  BatchNormW bn1, bn2;                                                                  // first_mlp.1, second_mlp.1
};
struct NatBlockW { LayerNormW norm1, norm2; const PW *qkv = nullptr, *proj = nullptr, *fc1 = nullptr, *fc2 = nullptr; const float* rpb = nullptr; };
struct NatLevelW {
  NatBlockW blocks[2]; LayerNormW norm;                                                 // levels.i.blocks.*, norm_i
  const PW* reduction = nullptr; LayerNormW ds_norm;                                    // levels.i.downsample (levels 0 and 1)
  const PW* lateral = nullptr;                                                          // lateral_convs.i
};
struct SceneBlockW { LayerNormW norm1, norm2; const PW *qkv = nullptr, *out_proj = nullptr, *fc1 = nullptr, *fc2 = nullptr; };      // encoder_blocks.i
struct DecoderBlockW {                                                                  // planning_decoder.decoder_blocks.i
  LayerNormW norm[4];
  const PW *r2r_qkv = nullptr, *r2r_out = nullptr, *m2m_qkv = nullptr, *m2m_qk0 = nullptr, *m2m_out = nullptr;
  const PW *cross_q = nullptr, *cross_kv = nullptr, *cross_out = nullptr, *ffn0 = nullptr, *ffn3 = nullptr;
};

struct Model {
  struct {      // agent_encoder
    const PW* embed_proj = nullptr; NatLevelW levels[3]; const PW* fpn_last = nullptr;      // history_encoder
    const float* type_emb = nullptr;
    struct { const float *query = nullptr, *pos_embed = nullptr; const PW *q = nullptr, *kv = nullptr, *out_proj = nullptr; } ego;      // ego_state_emb
  } agent;
  struct {      // map_encoder
    PointsEncoderW polygon_encoder; FourierW speed_limit_emb;
    const float *type_emb = nullptr, *on_route_emb = nullptr, *traffic_light_emb = nullptr, *unknown_speed_emb = nullptr;
  } map;
  struct { FourierW obj_encoder; const float* type_emb = nullptr; } stat;      // static_objects_encoder
  FourierW pos_emb;
  SceneBlockW encoder_blocks[4]; LayerNormW norm;
  MLPLayerW predictor[3];      // agent_predictor.{loc,yaw,vel}_predictor
  struct {      // planning_decoder
    PointsEncoderW r_encoder; FourierW r_pos_emb;
    const PW *q_proj_r = nullptr, *q_proj_m = nullptr; const float *m_emb = nullptr, *m_pos = nullptr;
    DecoderBlockW decoder_blocks[4];
    const PW *kv_all = nullptr, *cat_x_proj_q = nullptr, *cat_x_proj_x = nullptr;
    MLPLayerW head[3];         // {loc,yaw,vel}_head
  } dec;
  const PW *hidden_proj0 = nullptr, *hidden_proj2 = nullptr; MLPLayerW ref_free_decoder;
};

}  // namespace RIFT_NS
