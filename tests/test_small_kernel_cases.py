"""The input conditions of tests/test_gpu_small_kernels.py, checked on the references alone (no GPU): every term the GPU tests are meant
to pin is numerically VISIBLE on their inputs -- the fp64 reference moves by far more than the test's bar when the term is dropped or two
arguments are exchanged -- and no thresholded quantity sits where a last-bit difference of the device's libm could flip a decision."""
import numpy as np
import pytest
import torch

from oracle import losses, pluto_ref
from tests import helpers as H
from tests import small_kernel_cases as K


@pytest.fixture(scope="module")
def adam():
    case = K.adam_case()
    ref = K.adamw_ref64(case)
    dist, bars = K.adam_bars(ref, K.adamw_torch32(case))
    return case, ref, dist, bars


def test_adamw_inputs_are_the_ones_the_issue_names(adam):
    case, ref, dist, bars = adam
    n = len(K.ADAM_SIZES)
    assert n == 16 and sum(K.ADAM_SIZES) > 65536 and {1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 16384, 70001} <= set(K.ADAM_SIZES)
    assert all(len(set(row)) == n and all(5e-3 < lr < 5e-2 for lr in row) for row in case["lrs"]) and len({row[0] for row in case["lrs"]}) == 6
    assert case["wds"][:6] == [0.1, 0.0, 0.03, 0.1, 0.0, 0.03]
    for k, row in enumerate(case["grads"]):
        big = torch.cat(row)
        assert 0.08 < float((big == 0).float().mean()) < 0.12
        assert abs(float(big[big != 0].std()) / (3.0 if k % 2 == 0 else 1e-4) - 1) < 0.05
    # the decay factor the kernels multiply by is not one
    for row in case["lrs"]:
        for lr, wd in zip(row, case["wds"]):
            assert (np.float32(1.0 - lr * wd) != np.float32(1.0)) == (wd != 0.0)
    print(f"AdamW: |torch fp32 - fp64| parameters {dist[0]:.3e}, exp_avg {dist[1]:.3e}, exp_avg_sq {dist[2]:.3e}")
    assert all(0 < d < 1e-5 for d in dist)


@pytest.mark.parametrize("what", ["no_decay", "eps_1e-8", "beta1_0.9", "beta2_0.999", "neighbour_lr", "neighbour_wd"])
def test_adamw_terms_are_visible(adam, what):
    """Each change moves the fp64 parameters by more than 100 bars (the largest per-tensor bar), on at least one tensor."""
    case, ref, dist, bars = adam
    n = len(K.ADAM_SIZES)
    kw = {"no_decay": dict(wds=[0.0] * n), "eps_1e-8": dict(eps=1e-8), "beta1_0.9": dict(betas=(0.9, K.ADAM_BETAS[1])),
          "beta2_0.999": dict(betas=(K.ADAM_BETAS[0], 0.999)), "neighbour_lr": dict(lrs=[row[1:] + row[:1] for row in case["lrs"]]),
          "neighbour_wd": dict(wds=case["wds"][1:] + case["wds"][:1])}[what]
    moved = max(float(np.max(np.abs(a[0] - b[0]))) for a, b in zip(ref, K.adamw_ref64(case, **kw)))
    bar = max(b[0] for b in bars)
    print(f"AdamW {what}: fp64 parameters move by {moved:.3e} = {moved / bar:.0f} bars of {bar:.3e}")
    assert moved > 100 * bar


@pytest.mark.parametrize("config", range(len(K.TAIL_CONFIGS)))
def test_update_tail_cases_clip_and_pass_and_are_visible(config):
    case = K.tail_case(config)
    ref, steps = K.tail_ref(case)
    t32, _ = K.tail_ref(case, fp32=True)
    norms = [s[1] for s in steps]
    assert any(x > K.TAIL_MAX_NORM * 1.05 for x in norms) and any(x < K.TAIL_MAX_NORM * 0.95 for x in norms), norms
    dist = max(float(np.max(np.abs(a[0] - b[0]))) for a, b in zip(ref, t32))
    bar = max(max(4 * dist, 4 * float(K.ulp32(np.max(np.abs(a[0]))))) for a in ref)
    swapped = dict(case, lrs=[row[1:] + row[:1] for row in case["lrs"]], wds=case["wds"][1:] + case["wds"][:1])
    moved = max(float(np.max(np.abs(a[0] - b[0]))) for a, b in zip(ref, K.tail_ref(swapped)[0]))
    print(f"update tail {config}: norms {norms}, |torch fp32 - fp64| {dist:.3e}, neighbour's lr / wd moves the parameters by {moved:.3e}")
    assert moved > 100 * bar and sorted(K.TAIL_ORDER) == list(range(6)) and list(K.TAIL_ORDER) != list(range(6))


def test_clip_cases_land_on_either_side_of_one():
    assert len(K.CLIP_SIZES) == 16 and all(n % 2 for n in K.CLIP_SIZES)
    for rel in (-1e-3, 1e-3):
        total, clipped = K.clip_ref64(K.clip_case(rel))
        assert abs(total / (K.CLIP_MAX_NORM * (1 + rel)) - 1) < 1e-6
        coef = K.CLIP_MAX_NORM / (total + 1e-6)
        assert (coef < 1) == (rel > 0) and abs(coef - 1) > 5e-4
    total, clipped = K.clip_ref64(K.clip_case(None))
    assert total == 0.0 and all(not a.any() for a in clipped)


def test_scan_inputs_cover_the_chunk_edges_and_tell_the_arguments_apart():
    assert {1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 4095, 4097} <= set(K.SCAN_NS) and 15000 < max(K.SCAN_NS) < 25000
    for n in K.SCAN_NS:
        ch = -(-n // 1024)
        ends = K.forced_ends(n)
        assert 0 in ends and n - 1 in ends
        assert all((b - 1 in ends and b in ends) for b in range(97 * ch, n, 97 * ch))
        for rate in K.SCAN_RATES:
            i = K.scan_inputs(n, rate)
            assert all(i["dones"][e] == 1 for e in ends)
            assert bool(((i["unterminated"] == 0) <= (i["undones"] == 0)).all())          # terminated implies done
    n, rate = 1025, 0.05
    i = K.scan_inputs(n, rate)
    assert abs(float(i["dones"].mean()) - rate) < 0.03
    ref = K.gae_ref(n, rate)
    masks = float((ref - K.gae_ref(n, rate, exchange_masks=True)).abs().max())
    coefs = float((ref - K.gae_ref(n, rate, K.SCAN_LAMBDA, K.SCAN_GAMMA)).abs().max())
    print(f"GAE n={n}: exchanging undones / unterminated moves the oracle by {masks:.3f}, exchanging gamma / lambda by {coefs:.3f}")
    assert masks > 0.1 and coefs > 0.1
    r9, r98 = K.return_ref(n, rate), K.return_ref(n, rate, 0.98)
    assert float((r9 - r98).abs().max()) > 0.1


def test_zscore_inputs():
    for n in K.NORM_NS:
        x = K.normalize_input(n, True)
        ref, bar = K.normalize_ref64(x)
        assert abs(float(x.mean()) - 8) < 1.0 and ref.shape == (n,) and np.isfinite(ref).all()
        # the shifted data is where rounding the mean to fp32 shows: its term dominates the bar, and the bar stays far below the result
        assert float(np.max(bar)) < 1e-5
    assert set(K.GROUP_GS) == {1, 2, 12, 13, 63, 64, 65, 127, 192, 193} and set(K.GROUP_NS) == {1, 3, 4, 5, 9}
    ret = K.group_input(3, 13, True)
    assert abs(float(ret.mean()) + 300) < 1 and abs(K.group_ref(ret)).max() > 0.5
    assert not K.group_ref(K.group_input(5, 1, True)).any()


def test_rollout_return_inputs_keep_clear_of_every_threshold():
    worst = {}
    for G in K.RR_GS:
        for s, Ts in enumerate(K.RR_TS):
            c = K.rollout_return_case(G, Ts, s)
            assert c["collision"].shape[1] != Ts and c["off_road"].shape[1] != Ts and c["collision"].shape[1] != c["off_road"].shape[1]
            for k, v in K.rollout_return_margins(c).items():
                worst[k] = min(worst.get(k, 1.0), v)
    print("rollout return: smallest distance to a threshold", {k: f"{v:.2e}" for k, v in worst.items()})
    assert all(v > K.RR_MARGIN for v in worst.values()), worst


def test_rollout_return_second_round_is_visible():
    """Ts = 130, nine rows, every collision placement: clearing the flags from step 64 on moves at least three rows by > 100 bars."""
    c = K.rollout_return_case(9, 130, 0)
    placed = [sorted(np.nonzero(row[:130])[0].tolist()) for row in c["collision"]]
    assert placed[:8] == [[], [0], [129], [63], [64], [65], [64, 70], [127]]
    ref = K.rollout_return_ref(c)
    cleared = c["collision"].copy()
    cleared[:, 64:130] = False
    moved = np.abs(ref - K.rollout_return_ref(c, cleared))
    bar = 1e-5 * max(1.0, float(np.max(np.abs(ref))))
    print(f"rollout return Ts=130: clearing the second-round collisions moves the rows by {np.round(moved, 4).tolist()} (bar {bar:.2e})")
    assert int((moved > 100 * bar).sum()) >= 3


def test_reward_known_answers_by_hand():
    """The decisions of the dense reward exactly on their thresholds, against values worked out by hand from reward_model.py."""
    ref = K.reward_kat_ref()
    kat = K.REWARD_KAT
    align = lambda da, sp: 0.5 * (min(np.cos(np.float32(da)), 0) + 0.05 * min(np.float32(np.cos(np.float32(da))) * np.float32(sp), 0)  # noqa: E731
                                  + 0.25 * (1 - float(np.float32(da)) / (np.pi / 2)))
    center = lambda dd, da: -0.6 * (np.cos(np.float32(da)) > 0.5) * (float(np.float32(dd)) - 0.05 / np.exp(float(np.float32(dd)) - 0.5))  # noqa: E731
    for row, got in zip(kat, ref):
        dd, da, sp, ac, aa, col, off = row
        comfort = -0.8 * ((abs(ac) > 4) + (abs(aa) > 4))
        vel = 0.1 * max(float(np.cos(np.float32(da))), 0) * (3 < abs(sp) < 20) * abs(sp)
        tstep = -0.1 * (abs(sp) > 0 or abs(ac) > 0)
        want = -(20 + abs(sp)) * col - 5.0 * off + comfort + align(da, sp) + center(dd, da) + vel + tstep
        assert abs(got - want) < 1e-6, (row, got, want)
    assert abs(ref[0] - ref[1]) < 1e-12 and abs(ref[0] - ref[2] - 1.6) < 1e-12                 # |acc| = 4 costs nothing, 4.5 twice 0.8
    assert abs((ref[6] - ref[3]) - (0.1 * float(np.cos(np.float32(0.1))) * 12.0 + 0.0)) < 1e-6   # only inside (3, 20) is there a bonus
    assert abs(ref[3] - ref[4]) < 1e-12 and abs(ref[8] - ref[7] + 0.1) < 1e-12


def test_critic_targets_fall_on_both_smooth_l1_branches():
    from oracle import critic as ocr
    for call, n in enumerate(K.CRITIC_NS):
        c = K.critic_case(call)
        e = (ocr.critic_forward(H.critic_weights(), c["state"]) - c["target"]).abs()
        assert c["state"].shape == (n, 128) and float((e - 1).abs().min()) > 0.15
        if n >= 4:
            assert float((e < 1).float().mean()) >= 0.25 and float((e > 1).float().mean()) >= 0.25
    assert K.CRITIC_NS == (1, 15, 17, 50, 257, 15)


def test_ppo_hyper_parameters_are_visible():
    """The oracle at (clip_epsilon, lambda_entropy) = (0.2, 0.01) and at (0.4, 0.2) on the `small` fixture: loss and gradient differ by more
    than 100 bars (1e-5; 1e-5 + 1e-4 max |ref|)."""
    _, batch, sd = H.load_case("small")
    data = batch["cur_pluto_feature_torch"]
    ref, _, taps = pluto_ref.planning_model_forward(sd, H.clone_tree(data), need_traj=False, want_taps=True)
    r_pad = ~data["reference_line"]["valid_mask"].any(-1)
    b = K.ppo_case(ref["probability"], r_pad)
    lp = torch.log_softmax(ref["probability"].masked_fill(r_pad.unsqueeze(-1), -1e8).view(6, -1), dim=1).view(ref["probability"].shape)
    ratio = (lp[torch.arange(6), b["action_mode_torch"][:, 0], b["action_mode_torch"][:, 1]] - b["old_log_prob_torch"]).exp()
    assert float((ratio - torch.tensor(K.PPO_RATIOS)).abs().max()) < 1e-5
    for edge in (0.6, 0.8, 1.2, 1.4):
        assert float((ratio - edge).abs().min()) > 0.09
    assert (b["advantage_torch"] > 0).any() and (b["advantage_torch"] < 0).any()
    l0, g0, _ = losses.pi_head_loss_and_grads(sd, taps["q_final"], "ppo", b, r_pad)
    l1, g1, _ = losses.pi_head_loss_and_grads(sd, taps["q_final"], "ppo", b, r_pad, clip_epsilon=K.PPO_CLIP, lambda_entropy=K.PPO_ENT)
    l0b, g0b, _ = losses.pi_head_loss_and_grads(sd, taps["q_final"], "ppo", b, r_pad, clip_epsilon=0.2, lambda_entropy=0.01)
    assert float(l0) == float(l0b) and all(torch.equal(g0[k], g0b[k]) for k in g0)             # the defaults are unchanged
    # each of the two hyper-parameters on its own as well
    lc, gc, _ = losses.pi_head_loss_and_grads(sd, taps["q_final"], "ppo", b, r_pad, clip_epsilon=K.PPO_CLIP, lambda_entropy=0.01)
    le, ge, _ = losses.pi_head_loss_and_grads(sd, taps["q_final"], "ppo", b, r_pad, clip_epsilon=0.2, lambda_entropy=K.PPO_ENT)
    for la, ga in ((l1, g1), (lc, gc), (le, ge)):
        gd = max(float((ga[k] - g0[k]).abs().max()) / (1e-5 + 1e-4 * float(ga[k].abs().max())) for k in ga)
        print(f"PPO: loss moves by {abs(float(la) - float(l0)):.3e}, gradients by {gd:.0f} bars")
        assert abs(float(la) - float(l0)) > 100 * 1e-5 and gd > 100


def test_other_vehicle_and_sft_cases():
    for N in K.OV_NS:
        c = K.other_vehicle_case(N)
        assert all(len(v) == N for v in c.values())
    c = K.other_vehicle_case(65)
    assert (c["brake"] == 1).sum() > 5 and ((c["brake"] == 0) & (c["throttle"] == 0)).sum() > 5 and (c["speed"] < 1).sum() > 5
    for T in K.SFT_TS:
        traj, teacher = K.sft_case(T)
        assert traj.shape == (4, K.SFT_R, K.SFT_M, T, 6) and K.SFT_R * K.SFT_M == 72
        assert torch.equal(traj, traj.round())
        local = losses.sft_global_to_local(traj, teacher[:, 1:3], teacher[:, 3], K.SFT_FR)
        d = (losses.sft_target_speed(local) - teacher[:, 0][:, None, None]).abs().view(4, -1)
        assert torch.equal(d, d.round())                                       # exact target speeds: the tie is a tie in any arithmetic
        r, m = losses.sft_teacher_mode(traj, teacher, K.SFT_FR)
        for b, (first, second) in enumerate(K.SFT_TIES):
            assert second - first >= 64 and float(d[b, first]) == float(d[b, second]) == 1.0 == float(d[b].min())
            assert int((d[b] == 1.0).sum()) == 2 and (int(r[b]), int(m[b])) == (first // K.SFT_M, first % K.SFT_M)
