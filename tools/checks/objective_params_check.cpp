// The host-side defaults and refusals of RiftObjectiveParams (rift_amd/csrc/objective_params.h) as a stand-alone program, meant for the
// host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/checks/objective_params_check.cpp -o objective_params_check && ./objective_params_check
// Walks every refusal the header lists and every field with NaN / +Inf / -Inf, and prints one line per case; exit status 0 = all as expected.
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <limits>

#include "../../rift_amd/csrc/objective_params.h"

static int failures = 0;
static const int other_kinds[] = {RIFT_LOSS_PPO, RIFT_LOSS_REINFORCE, RIFT_LOSS_SFT, -1, 5};

static void expect(const char* what, int kind, const RiftObjectiveParams* p, bool has_ref, const char* want /* substring of the reason, or NULL = accepted */) {
  const char* got = rift_objective_params_refusal(kind, p, has_ref);
  const bool ok = want ? (got && strstr(got, want)) : got == nullptr;
  printf("%-44s %s%s\n", what, got ? "refused: " : "accepted", got ? got : "");
  if (!ok) { ++failures; printf("  EXPECTED %s\n", want ? want : "acceptance"); }
}

int main() {
  static_assert(sizeof(RiftObjectiveParams) == 40, "RiftObjectiveParams is 40 bytes");
  static_assert(offsetof(RiftObjectiveParams, clip_high) == 8 && offsetof(RiftObjectiveParams, entropy_coef) == 32, "field offsets");
  RiftObjectiveParams r, g, u;
  memset(&r, 0xff, sizeof(r)); memset(&g, 0xff, sizeof(g)); memset(&u, 0x5a, sizeof(u));      // every byte is written by the defaults
  if (!rift_objective_params_set_default(RIFT_LOSS_RIFT, &r) || !rift_objective_params_set_default(RIFT_LOSS_GRPO, &g)) { ++failures; printf("defaults refused\n"); }
  if (r.clip_low != 0.8 || r.clip_high != 1.2 || r.dual_clip != 3.0 || r.kl_beta != 0.0 || r.entropy_coef != 0.0) { ++failures; printf("RIFT defaults\n"); }
  if (g.clip_low != 0.8 || g.clip_high != 1.2 || g.dual_clip != 0.0 || g.kl_beta != 0.2 || g.entropy_coef != 0.0) { ++failures; printf("GRPO defaults\n"); }
  const RiftObjectiveParams before = u;
  for (int kind : other_kinds)
    if (rift_objective_params_set_default(kind, &u) || memcmp(&u, &before, sizeof(u)) != 0) { ++failures; printf("kind %d has defaults\n", kind); }
  expect("RIFT defaults, no reference logits", RIFT_LOSS_RIFT, &r, false, nullptr);
  expect("GRPO defaults", RIFT_LOSS_GRPO, &g, true, nullptr);
  expect("GRPO defaults, no reference logits", RIFT_LOSS_GRPO, &g, false, "ref_group_logits");
  expect("NULL", RIFT_LOSS_RIFT, nullptr, true, "NULL");
  for (int kind : other_kinds) { char w[64]; snprintf(w, sizeof(w), "kind %d", kind); expect(w, kind, &r, true, "kind"); }
  double RiftObjectiveParams::* const fields[] = {&RiftObjectiveParams::clip_low, &RiftObjectiveParams::clip_high, &RiftObjectiveParams::dual_clip,
                                                  &RiftObjectiveParams::kl_beta, &RiftObjectiveParams::entropy_coef};
  const double bad[] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
  RiftObjectiveParams p;
  int k = 0;
  for (auto f : fields) {
    for (double v : bad) { p = r; p.*f = v; char w[64]; snprintf(w, sizeof(w), "field %d = %g", k, v); expect(w, RIFT_LOSS_RIFT, &p, true, "not finite"); }
    ++k;
  }
  p = r; p.clip_low = 0.0; expect("clip_low = 0", RIFT_LOSS_RIFT, &p, true, "clip_low");
  p = r; p.clip_low = -0.8; expect("clip_low = -0.8", RIFT_LOSS_RIFT, &p, true, "clip_low");
  p = r; p.clip_low = 1.0 + 1e-12; expect("clip_low = 1 + 1e-12", RIFT_LOSS_RIFT, &p, true, "clip_low");
  p = r; p.clip_low = 1.0; p.clip_high = 1.0; expect("clip 1 / 1", RIFT_LOSS_RIFT, &p, true, nullptr);
  p = r; p.clip_high = 1.0 - 1e-12; expect("clip_high = 1 - 1e-12", RIFT_LOSS_RIFT, &p, true, "clip_high");
  p = r; p.clip_low = 0.8; p.clip_high = 1.28; expect("clip 0.8 / 1.28", RIFT_LOSS_RIFT, &p, true, nullptr);
  p = r; p.dual_clip = 1.0; expect("dual_clip = 1", RIFT_LOSS_RIFT, &p, true, "dual_clip");
  p = r; p.dual_clip = -3.0; expect("dual_clip = -3", RIFT_LOSS_RIFT, &p, true, "dual_clip");
  p = r; p.dual_clip = 0.0; expect("dual_clip = 0", RIFT_LOSS_RIFT, &p, true, nullptr);
  p = r; p.dual_clip = -0.0; expect("dual_clip = -0", RIFT_LOSS_RIFT, &p, true, nullptr);
  p = r; p.dual_clip = 1.35; expect("dual_clip = 1.35", RIFT_LOSS_GRPO, &p, true, nullptr);
  p = r; p.kl_beta = -1e-300; expect("kl_beta = -1e-300", RIFT_LOSS_RIFT, &p, true, "kl_beta");
  p = r; p.kl_beta = 0.2; expect("RIFT, kl_beta = 0.2", RIFT_LOSS_RIFT, &p, true, nullptr);
  p = r; p.kl_beta = 0.2; expect("RIFT, kl_beta = 0.2, no reference logits", RIFT_LOSS_RIFT, &p, false, "ref_group_logits");
  p = g; p.kl_beta = 0.0; expect("GRPO, kl_beta = 0, no reference logits", RIFT_LOSS_GRPO, &p, false, nullptr);
  p = r; p.entropy_coef = -0.5; expect("entropy_coef = -0.5", RIFT_LOSS_RIFT, &p, true, "entropy_coef");
  p = r; p.entropy_coef = 0.5; expect("entropy_coef = 0.5", RIFT_LOSS_RIFT, &p, true, nullptr);
  printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
