// The context of one engine build (included by engine.hip inside the build: one type per MFMA operand format) and the per-forward context.
#pragma once
#include <deque>
#include <unordered_map>

#include "model.h"
#include "dec_w.h"
#include "dropstats.h"
#include "fwd_plan.h"
#include "fwd_kernels.h"

namespace RIFT_NS {

struct Tap { float* p; int64_t numel; };

// The context of this build: the model side on top of the format-free core (ctx_core.h).  One type per operand format (rift_bf::Ctx,
// rift_hf::Ctx); the entries of this build's table cast the C handle down once at the top.
struct Ctx : RiftCtx {
  std::deque<PW> pw;                           // owns the packed images (a deque: its elements never move); cleared and refilled by rift_model_load only
  Model m;                                     // the forward's operands: pointers at `pw` and at the caller's tensors, written by the load's one walk (model_load.h)
  // activations that depend on (frozen) weights only, computed once per model load, each for the fp32 and the 16-bit mode
  struct WConst { struct V { DevBuf<float> p; bool ready = false; } v[2]; };
  struct WeightOnly { WConst ego_q, Mb, mp[4]; } wc;      // the ego query through attn.q, m_emb through q_proj.m, m_pos through the layers' m2m qk0
  // activation arena (bump allocator, reset every forward).  A forward with RIFT_F_DEFER_HEAD alternates between the arenas of `slots`, so
  // that the policy head / loss / backward of step k (rift_forward_head, rift_loss_backward on another stream) read step k's activations
  // while the frozen trunk of step k + 1 already writes its own.
  char* arena = nullptr; size_t arena_cap = 0, arena_off = 0;      // (the arena of the current slot, as A_alloc reads it)
  long long dry_key[11] = {}; size_t dry_need = 0;      // the arena size of the last sized forward and what it depended on
  struct Head {   // what the policy head of a forward needs (pi_forward .. trajectory heads); kept per arena for the deferred form
    bool valid = false, fp32 = false, need_traj = false;
    bool pi_fused = false, heads_fused = false;      // the kernel plan of the forward that made it (fwd_kernels.h): the deferred call runs the same path
    float *Q = nullptr, *x0p = nullptr, *QF = nullptr, *Hpi = nullptr, *prob = nullptr, *traj = nullptr, *o3[3] = {nullptr, nullptr, nullptr}, *oT[3] = {nullptr, nullptr, nullptr};
    uint8_t* r_kpm = nullptr; int bs = 0, R = 0, nQ = 0;
    bool dec_pending = false; DecWP dec;      // the planning decoder deferred along with the head (small batches, see dec_defer_max)
  };
  // the deferred-head slots: an arena, the head left in it, and the in-launch ranking's published per-scene counts (kernels.h:
  // rank_scene_body), which persist between launches (a word is valid when it carries the launch's epoch; zero at allocation, epochs
  // start at 1).  The look-back over these words relies on ONE preparation launch in flight per slot and on an epoch fixed on the host for
  // each launch (prepare_inputs): a captured graph that replays the launch would replay a stale epoch, so that launch is never graph-replayed.
  struct Slot { DevBuf<char> arena; Head head; DevBuf<unsigned long long> rk_pub; unsigned int rk_epoch = 0; } slots[RIFT_DEFER_SLOTS];
  int parity = 0;      // (the slot of the current forward)
  // The switches of the environment (read_switches), read ONCE when the context is made (nine getenv calls per forward were ~10 us of a
  // call whose host time bounds a small-batch step).
  struct Switches {
    bool nat_fused = true, dec_fused = true, enc_fused = true, pe_fused = true, fo_fused = true, fpn_fused = true, ego_fused = true, heads_fused = true, pi_fused = true;
    bool fo_w = true;                   // wave-private Fourier embeddings (fo_w.h): tokens, speed limits, reference-line positions
    bool pe_w = true;                   // wave-private PointsEncoder pass B (pe_w.h)
    bool two_streams = true, nat_compact = true, pe_live = true, pe_pack = true;
    int side_gate = 0; bool nat_aside = true;      // (the history chain behind the preparation on the prepare stream)
    int nat_grid = 256; int gemm_dbg = 0;
    // (round 4) Below a chip-filling batch a step is the LATENCY of token assembly -> encoder -> decoder on the caller's queue (one workgroup per
    // scene whatever the batch) while most CUs idle.  Nothing behind the encoder belongs to the frozen trunk's critical path of the NEXT
    // step, so with the head deferred the decoder goes with it: rift_forward_head_back launches decoder -> head on the caller's update
    // stream, and the caller's queue holds token assembly -> encoder of step k + 1 beside them.  All its operands live in the forward's
    // arena (four slots).  Which batch sizes: forward_impl's measured table, or bs <= RIFT_DEC_DEFER (0 = never).
    // (Measured and not kept: the deferred decoder on a third stream of the engine's own, so that decoder k would also run beside tail k - 1 --
    // 0.21 -> 0.40 ms at 32 scenes, with 4 or 8 hardware queues; every stream beyond the four the step uses has made cross-queue waits slower.)
    int dec_defer_max = -1; bool dec_split = true;   // (-1: the measured table in forward_impl; RIFT_DEC_DEFER=<n>: bs <= n)            // (RIFT_DEC_SPLIT=0: the deferred decoder as one launch)
    int dec_layers = 4;               // (diagnostic, RIFT_DEC_LAYERS) 0 / 2: the non-deferred decoder stops after that many layers -- the `dec3` tap then holds q0 / the
                                      // output of layer 1; 22: layers [0, 2) and [2, 4) of an eval forward as two launches; anything else: all four, one launch
    bool rank_fault = false;               // RIFT_RANK_FAULT=1 (diagnostic): the first scene block of the in-launch ranking never publishes its counts
    bool no_skip = false;                  // RIFT_NO_SKIP=1: the scene encoder computes the branches DropPath drops and the decoder the padded reference lines' discarded
                                           // sub-blocks, as until round 7 (the reference of tests/test_gpu_skip_discarded.py and the "before" leg of the A/B in one binary)
    bool enc112 = true;                    // RIFT_ENC112=0: scenes of 97 .. 112 token slots on enc_w_kernel (rounds 3 - 5) instead of the fused kernel's 112-row layout
    bool nat_group = true;                 // RIFT_NAT_GROUP=0: NAT levels 1 and 2 in rank order, every half-block computed (the path RIFT_NO_SKIP=1 also takes)
    bool rank_in_prep = true;              // RIFT_RANK_IN_PREP=0: the ranking as its own launch behind the preparation (nat_rank_kernel, rounds 3 - 5)
    // the per-call diagnostic switches: RIFT_{PE,PEW,NAT,ENC,DEC}_TS, RIFT_{PEW,DEC}_DBG, RIFT_POISON_ARENA
    int pe_ts = -1, pew_dbg = 0, pew_ts = 0, nat_ts = 0, enc_ts = 0, dec_ts = 0, dec_dbg = 0, poison_arena = -1;
  } sw;
  // streams and events beside the caller's stream (RiftCtxCore::stream)
  struct Streams {
    hipEvent_t param_event = nullptr;      // rift_set_param_event: the trainable parameters are valid once this event has passed
    hipStream_t prep_stream = nullptr; bool prep_set = false; hipEvent_t ev_prep = nullptr;      // rift_set_prepare_stream
    hipEvent_t ev_join2 = nullptr;      // (the history chain behind the preparation on the prepare stream: its join event)
    hipStream_t side = nullptr; bool side_owned = false; hipEvent_t ev_fork = nullptr, ev_join = nullptr;   // (RIFT_TWO_STREAMS=0 switches it off) the agent-history chain (NAT levels + FPN tail) on a second stream beside the map / reference-line chain
  } st;
  // per-kernel weight images (rift_model_load)
  struct Images {
    DevBuf<float> ego_w, ego_b;   // packed (6,128) linears of StateAttentionEncoder
    DevBuf<unsigned short> l0w_img; DevBuf<float> l0w_par;   // wave-private level-0 NAT kernel (nat_l0w.h)
    DevBuf<unsigned short> encw_img; DevBuf<float> encw_par;   // weight stream / parameters of the dense-traffic scene encoder (enc_w.h)
    DevBuf<unsigned short> l2w_img; DevBuf<float> l2w_par;   // wave-private, weight-streaming level-2 NAT kernel (nat_l2w.h)
    DevBuf<unsigned short> l1w_img; DevBuf<float> l1w_par;   // wave-private level-1 NAT kernel (nat_l1w.h)
    DevBuf<unsigned short> enc_wqkv[4];   // chunked (q|k|q|k|v|v) bf16 in_proj images
    DevBuf<float> enc_bqkv[4];
    DevBuf<int> enc_idx;
    DevBuf<unsigned short> fow_img[3]; DevBuf<float> fow_par[3];   // wave-private Fourier embeddings (fo_w.h)
    DevBuf<unsigned short> pew_img[2];   // wave-private PointsEncoder pass B (pe_w.h): weight streams of the map / reference-line encoders
    DevBuf<unsigned short> decw_img; DevBuf<float> decw_par;   // weight stream / parameter blocks of the decoder kernel (dec_w.h)
  } img;
  std::unordered_map<std::string, Tap> taps;
  struct Dp { bool on = false; int off = 0, gbs = 0; double* xchg = nullptr; long long len = 0; RiftExchangeFn fn = nullptr; void* user = nullptr; } dp;   // rift_set_dp
  DevBuf<int> nonfinite;            // device flag set by the policy-head kernels when the decoder output is not finite
  void* comm = nullptr; int comm_rank = 0, comm_world = 1;      // library-owned RCCL communicator (rift_comm_init), or null
  ~Ctx() {      // (the DevBuf members free the device memory)
    if (st.ev_prep) (void)hipEventDestroy(st.ev_prep);
    if (st.ev_join2) (void)hipEventDestroy(st.ev_join2);
    if (st.side && st.side_owned) (void)hipStreamDestroy(st.side);
    if (st.ev_fork) { (void)hipEventDestroy(st.ev_fork); (void)hipEventDestroy(st.ev_join); }
  }
};

template <class T>
T* A_alloc(Ctx* c, size_t n) {
  size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
  char* p = c->dry ? nullptr : c->arena + c->arena_off;
  c->arena_off += bytes;
  return reinterpret_cast<T*>(p);
}

inline void tap(Ctx* c, const char* name, float* p, int64_t numel) {
  if (!c->dry) c->taps[name] = Tap{p, numel};
}

// per-forward context: the flags, the stream plan, the kernel plan, the batch dimensions, and what one stage of forward_impl hands to the next
struct Fwd {
  Ctx* c; bool train, drop, fp32, need_traj, bn_update; uint32_t seed; uint32_t stream_id = 1;
  uint32_t next_stream() { return stream_id++; }
  // data parallel (rift_set_dp): xchg[0, kb) = quirk-mask slots of the global minibatch, xchg[kb, ...) = BatchNorm sums of the current point
  bool dp = false, kpm_pending = false; int kb = 0; uint8_t* g_rkpm = nullptr;
  uint8_t* r_tiles = nullptr;                        // tiles of every reference line up to its last valid point (prep_kernel), for pe_w_kernel's packed rounds
  const RiftFeatureBatch* B = nullptr; const RiftOutputs* out = nullptr; int flags = 0;
  KernelPlan kp;                                     // which kernel every stage runs (fwd_kernels.h): the same in the sizing and the launch pass
  StreamPlan plan; hipStream_t on[3] = {nullptr, nullptr, nullptr};      // (indexed by PlanStream)
  int bs = 0, A = 0, Mp = 0, R = 0, S = 0, T = 0, N = 0, M = 12, nA = 0, nP = 0, nL = 0, nQ = 0, nT = 0;
  DropStats ds = {};                                 // diagnostic build (dropstats.h): this forward's counters; all zero in the product library
  // prepare_inputs
  float *F9 = nullptr, *F10 = nullptr, *F6 = nullptr, *pos = nullptr, *r_pos = nullptr;
  uint8_t *valid_agent = nullptr, *kpm = nullptr, *r_kpm = nullptr;
  int *nat_aidx = nullptr, *nat_cnt = nullptr;      // the history encoder on the compacted sequences (kp.nat_compact; nat_l0w.h ranks them)
  const uint8_t* q_kpm = nullptr; int q_bs = 0, q_off = 0;                    // the r2r mask quirk's rows: this shard's, or the gathered global minibatch's
  // history_encoder, ego_token, map_and_embeddings, assemble_tokens
  float *nat_out = nullptr, *x_ego = nullptr, *poly = nullptr, *r_emb = nullptr, *speed_emb = nullptr, *PEtok = nullptr, *Q = nullptr, *X = nullptr;
  // scene_encoder
  float* ENC = nullptr;
  unsigned short* enc_KT = nullptr;   // the decoder's cross-attention K | V^T operand fragments, written by the encoder kernel's tail
  uint8_t* kpm_c = nullptr;           // the key padding of the compacted encoder rows (bs, 96): what the decoder masks those fragments with
  float* enc_x0p = nullptr;           // cat_x_proj's ego-token half, written by the encoder kernel's tail
  // planning_decoder
  bool dec_deferred = false; DecWP dec_later;
};

}  // namespace RIFT_NS
