"""The small kernels around the forward path -- optimizer tail, gradient clip, GAE / return scans, z-scores, rollout return, PPO critic,
the PPO objective's hyper-parameters, other-vehicle forecast, SFT teacher label -- against plain fp64 / oracle references, at
hyper-parameters where every term shows and at the sizes where their loops, chunks and tiles end raggedly.  The inputs and the fp64
restatements are in tests/small_kernel_cases.py; tests/test_small_kernel_cases.py checks on the CPU that the inputs make each term
visible (dropping it moves the reference by > 100 bars).  Needs a real MI355X: `pytest -m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import losses, traj_flags as otf
from tests import helpers as H
from tests import small_kernel_cases as K

pytestmark = pytest.mark.gpu

RIFT_ERR_ARG = -1           # include/rift_hip.h


@pytest.fixture(scope="module")
def ffi():
    from rift_amd import _ffi
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    _ffi.load_library()
    return _ffi


def dist(a, b):
    """max |a - b| in fp64; both finite."""
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    d = np.abs(a.reshape(-1) - b.reshape(-1))
    assert np.isfinite(d).all()
    return float(d.max()) if d.size else 0.0


# ---- 1. AdamW and the fused tail ------------------------------------------------------------------------------------------------------
def test_adamw_step_with_per_tensor_lr_decay_and_a_visible_eps(ffi):
    """rift_adamw_step on 16 tensors of 1 .. 70 001 elements (95 493 in all: the 256-workgroup grid-stride loop wraps) from zero state, six
    steps, betas (0.8, 0.95), eps 1e-3, a different lr ~1e-2 per tensor and per step, weight decay cycling 0.1 / 0 / 0.03, gradients of scale
    3.0 and 1e-4 alternating with a tenth of the entries exactly zero -- against the fp64 restatement of torch.optim.AdamW.
    Bar per tensor and quantity: max(4 D, 4 fp32 ulps of the tensor's largest magnitude), D = the distance between torch's own fp32 CPU
    AdamW (foreach=False, one group per tensor) and the fp64 restatement on the same inputs: parameters 4.0e-7, exp_avg 2.5e-7,
    exp_avg_sq 1.4e-6 (bars 1.6e-6 / 9.8e-7 / 5.5e-6 and up).  Measured on MI355X, kernel against fp64: parameters 4.0e-7, exp_avg 2.9e-7,
    exp_avg_sq 1.4e-6; the worst error is 0.29 of its bar."""
    case = K.adam_case()
    ref = K.adamw_ref64(case)
    D, bars = K.adam_bars(ref, K.adamw_torch32(case))
    print(f"AdamW: |torch fp32 CPU - fp64| parameters {D[0]:.3e}, exp_avg {D[1]:.3e}, exp_avg_sq {D[2]:.3e}")
    eng = ffi.Engine("cuda:0")
    n = len(case["init"])
    p = [t.clone().cuda() for t in case["init"]]
    g, m, v = ([torch.zeros_like(t) for t in p] for _ in range(3))
    steps = [torch.zeros(1, device="cuda") for _ in p]
    al = eng.make_adam_list(p, g, m, v, steps)
    for k, row in enumerate(case["grads"]):
        for dst, src in zip(g, row):
            dst.copy_(src)
        eng.adamw_step_raw(al, case["lrs"][k], case["wds"], float(k + 1), *K.ADAM_BETAS, K.ADAM_EPS)
        assert all(float(s) == k + 1 for s in steps)                       # the device step counters equal step_new exactly
    torch.cuda.synchronize()
    got = [[dist(p[i], ref[i][0]), dist(m[i], ref[i][1]), dist(v[i], ref[i][2])] for i in range(n)]
    worst = max(got[i][q] / bars[i][q] for i in range(n) for q in range(3))
    print("AdamW: max |kernel - fp64| parameters %.3e, exp_avg %.3e, exp_avg_sq %.3e; worst error / bar %.2f" %
          (*[max(r[q] for r in got) for q in range(3)], worst))
    for i in range(n):
        for q, what in enumerate(("param", "exp_avg", "exp_avg_sq")):
            assert got[i][q] <= bars[i][q], (K.ADAM_SIZES[i], what, got[i][q], bars[i][q])
    # argument errors: more than 16 tensors, a step number below one -- refused before anything is launched
    before = [t.clone() for t in p]
    vp = C.c_void_p

    def call(cnt, step_new):
        rep = lambda arr: (vp * cnt)(*[arr[i % n] for i in range(cnt)])  # noqa: E731
        return eng.lib.rift_adamw_step(eng.ctx, cnt, rep(al["p"]), rep(al["g"]), rep(al["m"]), rep(al["v"]), rep(al["s"]),
                                       (C.c_int64 * cnt)(*[1] * cnt), (C.c_double * cnt)(*[1e-2] * cnt), (C.c_double * cnt)(*[0.0] * cnt),
                                       step_new, *K.ADAM_BETAS, K.ADAM_EPS, ffi._stream())
    assert call(17, 7.0) == RIFT_ERR_ARG and call(16, 0.0) == RIFT_ERR_ARG
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, p)) and all(float(s) == 6.0 for s in steps)
    eng.close()


@pytest.mark.parametrize("config", range(len(K.TAIL_CONFIGS)))
def test_update_tail_with_a_shuffled_list_and_per_tensor_hyper_parameters(ffi, config):
    """rift_update_tail on the six pi_head tensors, the AdamW list in a shuffled order with its own lr and weight decay per tensor, three
    consecutive steps (accumulate 0 / 1, with and without the f64 exchange buffer, gradient sums that clip and that pass through):
      * bit for bit equal to rift_loss_finalize_clip followed by rift_adamw_step on copies of the same state (parameters, clipped .grad,
        exp_avg, exp_avg_sq, step counters, loss, total norm, stats);
      * parameters / exp_avg / exp_avg_sq within max(4 D, 4 ulps) of the fp64 restatement (finalize, clip, AdamW), D = torch's fp32 CPU
        operations against it on the same inputs (parameters 2.7e-7 .. 3.0e-7).  Measured on MI355X: worst error / bar 0.25 .. 0.32."""
    case = K.tail_case(config)
    ref, ref_steps = K.tail_ref(case)
    t32, _ = K.tail_ref(case, fp32=True)
    D = [max(float(np.max(np.abs(a[q] - b[q]))) for a, b in zip(ref, t32)) for q in range(3)]
    eng = ffi.Engine("cuda:0")
    order = K.TAIL_ORDER

    def run(fused):
        p = [t.clone().cuda() for t in case["init"]]
        g = [t.clone().cuda() for t in case["prev"]]
        m, v = ([torch.zeros_like(t) for t in p] for _ in range(2))
        steps = [torch.zeros(1, device="cuda") for _ in p]
        pick = lambda ts: [ts[s] for s in order]  # noqa: E731
        al = eng.make_adam_list(pick(p), pick(g), pick(m), pick(v), pick(steps))
        trace = []
        for k in range(3):
            flat = case["flat"][k].cuda()
            stats = torch.tensor([K.TAIL_S, K.TAIL_CNT], dtype=torch.float64, device="cuda")
            xchg = torch.cat([flat.double() * 2.0, stats * 2.0]) if case["xchg"] else None
            loss = torch.zeros(1, dtype=torch.float64, device="cuda")
            tn = torch.zeros(1, device="cuda")
            lo = ffi.RiftLossOut()
            lo.loss, lo.stats, lo.flat_grad_sum, lo.exchange = ffi._ptr(loss), ffi._ptr(stats), ffi._ptr(flat), ffi._ptr(xchg)
            lo.grad_w1, lo.grad_b1, lo.grad_ln_w, lo.grad_ln_b, lo.grad_w2, lo.grad_b2 = (ffi._ptr(t) for t in g)
            lrs, wds = [case["lrs"][k][s] for s in order], [case["wds"][s] for s in order]
            if fused:
                eng.update_tail_raw(lo, case["accumulate"], K.TAIL_MAX_NORM, tn, al, lrs, wds, float(k + 1), *K.ADAM_BETAS, K.ADAM_EPS)
            else:
                eng.loss_finalize_clip_raw(lo, case["accumulate"], K.TAIL_MAX_NORM, tn)
                eng.adamw_step_raw(al, lrs, wds, float(k + 1), *K.ADAM_BETAS, K.ADAM_EPS)
            torch.cuda.synchronize()
            trace.append((float(loss), float(tn), stats.cpu()))
        return [[t.cpu() for t in ts] for ts in (p, m, v, g, steps)], trace

    fused, ftrace = run(True)
    two, ttrace = run(False)
    for what, a, b in zip(("param", "exp_avg", "exp_avg_sq", "grad", "step"), fused, two):
        for s in range(6):
            assert torch.equal(a[s], b[s]), (what, s, float((a[s] - b[s]).abs().max()))
    for k, ((l1, n1, s1), (l2, n2, s2), (lr_, nr)) in enumerate(zip(ftrace, ttrace, ref_steps)):
        assert l1 == l2 and n1 == n2 and torch.equal(s1, s2)
        assert abs(l1 - lr_) < 1e-12 and abs(n1 - nr) < 1e-6 * nr, (k, l1, lr_, n1, nr)
    assert all(float(s) == 3.0 for s in fused[4])
    worst = 0.0
    for s in range(6):
        for q, what in enumerate(("param", "exp_avg", "exp_avg_sq")):
            bar = max(4 * D[q], 4 * float(K.ulp32(np.max(np.abs(ref[s][q])))))
            e = dist(fused[q][s], ref[s][q])
            worst = max(worst, e / bar)
            assert e <= bar, (s, what, e, bar)
        assert dist(fused[3][s], ref[s][3]) < 1e-6 * max(1.0, float(np.max(np.abs(ref[s][3]))))
    print(f"update tail {config}: |torch fp32 CPU - fp64| {D[0]:.3e} / {D[1]:.3e} / {D[2]:.3e}; worst kernel error / bar {worst:.2f}")
    eng.close()


# ---- 2. gradient clip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", [None, -1e-3, 1e-3])
def test_clip_grad_norm_on_either_side_of_the_threshold(ffi, rel):
    """rift_clip_grad_norm over 16 tensors of odd sizes against fp64: all-zero gradients (norm 0, nothing touched, nothing non-finite), and
    gradients whose norm is max_norm (1 -+ 1e-3), so that the coefficient lands on either side of one.  Total norm 1e-6 relative, elements
    within two fp32 ulps (measured on MI355X: 1.55 ulps when clipping, 0 when passing through)."""
    grads = K.clip_case(rel)
    total, want = K.clip_ref64(grads)
    eng = ffi.Engine("cuda:0")
    mine = [t.clone().cuda() for t in grads]
    tn = torch.full((1,), -1.0, device="cuda")
    eng.clip_grad_norm_raw(eng.make_clip_list(mine), K.CLIP_MAX_NORM, tn)
    torch.cuda.synchronize()
    assert abs(float(tn) - total) <= 1e-6 * total
    worst = 0.0
    for a, src, w in zip(mine, grads, want):
        a = a.cpu()
        assert torch.isfinite(a).all()
        if rel is None or rel < 0:
            assert torch.equal(a, src)                                        # passed through untouched
        e = np.abs(a.double().numpy() - w) / K.ulp32(w)
        worst = max(worst, float(e.max()))
    print(f"clip rel={rel}: total norm {float(tn):.7f} (fp64 {total:.7f}), worst element error {worst:.2f} ulps")
    assert worst <= 2.0
    eng.close()


# ---- 3. reverse scans -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", K.SCAN_RATES)
def test_reverse_scans_at_every_chunk_shape(ffi, rate):
    """rift_gae (gamma 0.9, lambda 0.6: the two are told apart) and rift_discounted_return (gamma 0.9) against the oracle's sequential
    loops, the WHOLE output, at n = 1 .. 20 011: fewer steps than threads, one per thread, ragged chunks, episode ends on both sides of chunk
    boundaries.  GAE within one fp32 ulp of the oracle's value (both run the recurrence in fp64 and round once on the store); returns within
    1e-9 max(1, max |ref|)."""
    eng = ffi.Engine("cuda:0")
    for n in K.SCAN_NS:
        i = K.scan_inputs(n, rate)
        got = eng.gae(i["rewards"], i["undones"], i["values"], i["next_values"], i["unterminated"], K.SCAN_GAMMA, K.SCAN_LAMBDA).cpu()
        ref = K.gae_ref(n, rate).double().numpy()
        e = np.abs(got.double().numpy() - ref)
        assert np.isfinite(e).all() and (e <= K.ulp32(ref)).all(), (n, float(e.max()), int(np.argmax(e / K.ulp32(ref))))
        ret = eng.discounted_return(i["rewards"], i["dones"], K.SCAN_GAMMA)
        rref = K.return_ref(n, rate)
        assert dist(ret, rref) < 1e-9 * max(1.0, float(rref.abs().max())), n
    if rate == K.SCAN_RATES[0]:
        n = 4097
        i = K.scan_inputs(n, rate)
        for gamma in (1.0, 0.0):
            rref = K.return_ref(n, rate, gamma)
            assert dist(eng.discounted_return(i["rewards"], i["dones"], gamma), rref) < 1e-9 * max(1.0, float(rref.abs().max())), gamma
    eng.close()


# ---- 4. z-scores ----------------------------------------------------------------------------------------------------------------------
def test_normalize_advantage_centred_and_shifted(ffi):
    """rift_normalize_advantage at n = 2 .. 4099 on centred data and on data with mean 8 and spread 0.5 against fp64 on the fp32 inputs.
    Bar (K.normalize_ref64 has the derivation): (ulp32(|mean|) / 2 + 2 ulp32(max |x - mean|)) / (std + 1e-5) + 2 ulp32(result).
    Measured on MI355X: centred 3.4e-7 (0.36 of the bar), mean 8: 1.04e-6 (0.62 of the bar, which the rounded mean dominates there).
    n = 1 is left out: the reference's unbiased standard deviation is NaN there."""
    eng = ffi.Engine("cuda:0")
    for shifted in (False, True):
        worst, worst_abs = 0.0, 0.0
        for n in K.NORM_NS:
            x = K.normalize_input(n, shifted)
            ref, bar = K.normalize_ref64(x)
            got = eng.normalize_advantage_(x.clone().cuda()).cpu().double().numpy()
            e = np.abs(got - ref)
            assert np.isfinite(e).all()
            worst, worst_abs = max(worst, float((e / bar).max())), max(worst_abs, float(e.max()))
            assert (e <= bar).all(), (shifted, n, float(e.max()), float(bar.max()))
        print(f"normalize ({'mean 8' if shifted else 'centred'}): max error {worst_abs:.3e}, worst error / bar {worst:.2f}")
    eng.close()


def test_group_zscore_with_ragged_groups_and_workgroups(ffi):
    """rift_group_advantage for G = 1 .. 193 (below, at and above one and three wave-widths) and 1 .. 9 groups (four per workgroup: ragged
    last one), standard-normal returns and returns around -300 with spread 0.5, against oracle.advantage.group_zscore per group: 1e-9.
    G = 1 gives exactly 0."""
    eng = ffi.Engine("cuda:0")
    worst = 0.0
    for ng in K.GROUP_NS:
        for G in K.GROUP_GS:
            for shifted in (False, True):
                ret = K.group_input(ng, G, shifted)
                got = eng.group_advantage(ret).cpu()
                if G == 1:
                    assert not got.any()
                e = dist(got, K.group_ref(ret))
                worst = max(worst, e)
                assert e < 1e-9, (ng, G, shifted, e)
    print(f"group z-score: max error {worst:.3e}")
    eng.close()


# ---- 5. rollout return ----------------------------------------------------------------------------------------------------------------
def _rollout_return(eng, c):
    T = torch.from_numpy
    return eng.rollout_return(T(c["delta_dis"]), T(c["delta_angle"]), T(c["speed"]), T(c["acc"]), T(c["ang_vel"]), T(c["ang_acc"]),
                              c["collision"], c["off_road"], gamma=K.RR_GAMMA)


def test_rollout_return_over_horizons_past_one_wave(ffi):
    """rift_rollout_return for Ts = 1 .. 130 (one, two and three rounds of 64 steps) and G = 1 .. 9 (four candidates per workgroup), gamma
    0.93, the flags passed as wider arrays whose columns beyond the horizon are all set; collisions at none / 0 / Ts - 1 / 63 / 64 / 65 /
    64 and 70 / 127.  Against oracle.advantage.rollout_return: 1e-5 max(1, max |ref|).  Measured on MI355X at Ts = 130: 1.2e-7 (max |ref| 27.7, bar 2.8e-4);
    over all shapes 1.8e-7."""
    eng = ffi.Engine("cuda:0")
    worst = {}
    for G in K.RR_GS:
        for s, Ts in enumerate(K.RR_TS):
            c = K.rollout_return_case(G, Ts, s)
            assert all(v > K.RR_MARGIN for v in K.rollout_return_margins(c).values())
            ref = K.rollout_return_ref(c)
            e = dist(_rollout_return(eng, c), ref)
            worst[Ts] = max(worst.get(Ts, 0.0), e)
            assert e < 1e-5 * max(1.0, float(np.max(np.abs(ref)))), (G, Ts, e)
    c = K.rollout_return_case(9, 130, 0)                         # every collision placement in one call
    ref = K.rollout_return_ref(c)
    e = dist(_rollout_return(eng, c), ref)
    print(f"rollout return: Ts = 130 error {max(e, worst[130]):.3e} (max |ref| {float(np.max(np.abs(ref))):.1f}); by horizon " +
          ", ".join(f"{t}: {v:.1e}" for t, v in worst.items()))
    assert e < 1e-5 * max(1.0, float(np.max(np.abs(ref))))
    eng.close()


def test_dense_reward_decisions_on_their_thresholds(ffi):
    """One step, inputs exactly on the reward's thresholds (|acc| = 4, |speed| = 3 and 20, standing still, delta_angle 0 and 2.0, negative
    speed, collision with and without off-road) against oracle.advantage.dense_reward: 1e-6."""
    eng = ffi.Engine("cuda:0")
    kat = np.array(K.REWARD_KAT, dtype=np.float64)
    col = lambda j: np.ascontiguousarray(kat[:, j:j + 1].astype(np.float32))  # noqa: E731
    c = {"delta_dis": col(0), "delta_angle": col(1), "speed": col(2), "acc": col(3), "ang_vel": np.zeros((len(kat), 1), np.float32),
         "ang_acc": col(4), "collision": kat[:, 5:6] != 0, "off_road": kat[:, 6:7] != 0}
    got = eng.rollout_return(*[torch.from_numpy(c[k]) for k in ("delta_dis", "delta_angle", "speed", "acc", "ang_vel", "ang_acc")],
                             c["collision"], c["off_road"], gamma=K.RR_GAMMA).cpu().numpy()
    ref = K.reward_kat_ref()
    for row, a, b in zip(K.REWARD_KAT, got, ref):
        assert abs(a - b) < 1e-6, (row, a, b)
    eng.close()


# ---- 6. PPO critic --------------------------------------------------------------------------------------------------------------------
def test_critic_at_ragged_row_counts_on_one_engine(ffi):
    """rift_critic_forward and rift_critic_loss_backward + rift_critic_finalize at n = 1, 15, 17, 50, 257 and then 15 again on ONE engine
    (16 rows per workgroup; the scratch buffer grows and is then reused larger than needed: nothing of the 257-row call may reach the
    15-row sums), targets on both SmoothL1 branches, against oracle.critic with autograd: values 1e-5, gradients 1e-5 + 1e-4 max |ref|,
    the loss through the `stats` convention 1e-5.  (A single row cannot sit on both branches: the n = 1 call takes the linear one.)"""
    sd = {k: v.cuda().contiguous() for k, v in H.critic_weights().items()}
    eng = ffi.Engine("cuda:0")
    w = eng.critic_desc(sd)
    actor = 0.37                                                            # a stand-in for the actor half the objective kernel leaves in stats
    for call, n in enumerate(K.CRITIC_NS):
        c = K.critic_case(call)
        value, vloss, grads_o = K.critic_ref(c)
        e = (value - c["target"]).abs()
        if n >= 4:
            assert float((e < 1).float().mean()) >= 0.25 and float((e > 1).float().mean()) >= 0.25
        assert dist(eng.critic_forward(sd, c["state"]), value) < 1e-5, n
        stats = torch.tensor([-actor * n, float(n)], dtype=torch.float64, device="cuda")
        flat = torch.full((ffi.CRITIC_NPARAM,), 7.0, dtype=torch.float32, device="cuda")      # every entry is written, none accumulated into
        eng.critic_loss_backward_raw(w, c["state"].cuda(), c["target"].cuda(), stats, flat)
        assert abs(float(-stats[0] / stats[1]) - (actor + vloss)) < 1e-5, n
        grads = [torch.full_like(sd[k], 7.0) for k in ffi.CRITIC_KEYS]
        eng.critic_finalize_raw(flat, stats, grads)
        torch.cuda.synchronize()
        for k, g in zip(ffi.CRITIC_KEYS, grads):
            assert dist(g, grads_o[k]) < 1e-5 + 1e-4 * float(grads_o[k].abs().max()), (call, n, k)
    eng.close()


# ---- 7. PPO hyper-parameters ----------------------------------------------------------------------------------------------------------
def test_ppo_objective_at_other_clip_and_entropy_weights(ffi):
    """loss_backward("ppo", clip_epsilon=0.4, lambda_entropy=0.2) on the `small` fixture in fp32 mode, old_log_prob set from the device's own
    probabilities so that the six ratios are 0.5, 0.7, 0.9, 1.1, 1.3, 2.0 (0.7 and 1.3 inside the 0.4 range, outside the default one), mixed
    advantage signs, against the oracle on the tapped q_final with the same two values: loss 1e-5, gradients 1e-5 + 1e-4 max |ref|."""
    _, batch, sd = H.load_case("small")
    data = batch["cur_pluto_feature_torch"]
    eng = ffi.Engine("cuda:0")
    eng.load_state_dict({k: v.clone() for k, v in sd.items()})
    out = eng.forward(data, fp32=True)
    torch.cuda.synchronize()
    r_pad = ~data["reference_line"]["valid_mask"].any(-1)
    b = H.clone_tree(batch)
    b.update(K.ppo_case(out["probability"].cpu(), r_pad))
    stats, flat, _ = eng.loss_backward("ppo", b, clip_epsilon=K.PPO_CLIP, lambda_entropy=K.PPO_ENT)
    grads = {k: torch.zeros_like(sd["planning_decoder.pi_head." + k]).cuda() for k in losses.PI_KEYS}
    loss = float(eng.loss_finalize(stats, flat, grads).item())
    qf = eng.tap("q_final").view(r_pad.shape[0], r_pad.shape[1], 12, 128).cpu()
    want, want_g, prob = losses.pi_head_loss_and_grads(sd, qf, "ppo", H.clone_tree(b), r_pad, clip_epsilon=K.PPO_CLIP, lambda_entropy=K.PPO_ENT)
    lp = torch.log_softmax(prob.masked_fill(r_pad.unsqueeze(-1), -1e8).view(6, -1), dim=1).view(prob.shape)
    ratio = (lp[torch.arange(6), b["action_mode_torch"][:, 0], b["action_mode_torch"][:, 1]] - b["old_log_prob_torch"]).exp()
    assert float((ratio - torch.tensor(K.PPO_RATIOS)).abs().max()) < 1e-3          # the oracle sees the ratios the test set up
    default, _, _ = losses.pi_head_loss_and_grads(sd, qf, "ppo", H.clone_tree(b), r_pad)
    print(f"PPO (0.4, 0.2): |loss - oracle| {abs(loss - float(want)):.3e}; the oracle at the defaults is {abs(float(default) - float(want)):.3e} away")
    assert abs(loss - float(want)) < 1e-5
    for k in grads:
        assert dist(grads[k], want_g[k]) < 1e-5 + 1e-4 * float(want_g[k].abs().max()), k
    eng.close()


# ---- 8. two small neighbours ----------------------------------------------------------------------------------------------------------
def test_other_vehicle_rollout_over_flags_inflations_and_sizes(ffi):
    """rift_other_vehicle_rollout with near_lane_change False / True, bbox_inflation_ratio 1.0 / 1.3, N = 1, 64, 65 (64 actors per
    workgroup), T = 1, 40, braking, coasting, slow and accelerating actors, against oracle.traj_flags.get_other_vehicle_rollout (itself
    pinned bit-exact to the reference's fixture): 1e-9."""
    eng = ffi.Engine("cuda:0")
    worst = 0.0
    for N in K.OV_NS:
        inp = K.other_vehicle_case(N)
        for T in K.OV_TS:
            for lane_change in (False, True):
                for infl in (1.0, 1.3):
                    got = eng.other_vehicle_rollout(**inp, num_future_frames=T, near_lane_change=lane_change, bbox_inflation_ratio=infl)
                    want = otf.get_other_vehicle_rollout(**inp, num_future_frames=T, near_lane_change=lane_change, bbox_inflation_ratio=infl)
                    assert tuple(got.shape) == (N, T, 4, 2) == want.shape
                    e = dist(got, want)
                    worst = max(worst, e)
                    assert e < 1e-9, (N, T, lane_change, infl, e)
    print(f"other-vehicle rollout: max error {worst:.3e}")
    eng.close()


@pytest.mark.parametrize("T", K.SFT_TS)
def test_sft_teacher_mode_breaks_ties_by_the_first_index(ffi, T):
    """rift_sft_teacher_mode with 72 candidates (more than one per lane), T = 7 (below frame_rate), 25 and 80, exact integer target speeds,
    two candidates 64 or more apart sharing the minimum (in neighbouring lanes, and in the same lane): the (r, m) label equals
    oracle.losses.sft_teacher_mode bit for bit -- torch.argmin's first index."""
    eng = ffi.Engine("cuda:0")
    traj, teacher = K.sft_case(T)
    r, m = losses.sft_teacher_mode(traj, teacher, K.SFT_FR)
    got = eng.sft_teacher_mode(traj, teacher, K.SFT_FR).cpu()
    assert torch.equal(got[:, 0], r) and torch.equal(got[:, 1], m), (got.tolist(), r.tolist(), m.tolist())
    assert [int(a) * K.SFT_M + int(b) for a, b in got] == [first for first, _ in K.SFT_TIES]
    eng.close()
