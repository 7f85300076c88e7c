"""Weight sets, references and restatements shared by the evaluator-parameter tests (tests/test_eval_params_host.py on the CPU,
tests/test_gpu_eval_params.py on the device) and by tests/golden/gen_reward_params.py.

The reference for non-default weights is oracle.advantage with its module-level dict P patched (monkeypatch.setitem, restored on exit):
with P patched, oracle.advantage.rollout_return restates the reference's DenseRewardModel with edited `params`
(tests/golden/reward_params.npz holds the reference's own numbers)."""
import contextlib

import numpy as np
import pytest

from oracle import advantage as oadv

DEFAULTS = dict(oadv.P)
KEYS = tuple(DEFAULTS)               # the order of RiftEvalParams
# Three sets that together move every one of the nine weights off its default; B carries a centre bias.
SETS = {
    "A": dict(DEFAULTS, alpha_collision=12.0, alpha_boundary=9.0, alpha_comfort=1.7),
    "B": dict(DEFAULTS, alpha_l_align=1.3, alpha_vel_align=0.4, alpha_l_center=1.1, alpha_center_bias=0.35),
    "C": dict(DEFAULTS, alpha_collision=31.0, alpha_velocity=0.37, alpha_timestep=0.45),
}
SPARSE = {"reference": dict(alpha_collision=15.0, alpha_boundary=15.0), "edited": dict(alpha_collision=7.0, alpha_boundary=11.0)}
GAMMAS = (0.98, 0.9)                 # of the fixture
assert all(any(s[k] != DEFAULTS[k] for s in SETS.values()) for k in KEYS)


def moved(weights):
    return [k for k in KEYS if weights[k] != DEFAULTS[k]]


@contextlib.contextmanager
def patched_P(weights):
    """oracle.advantage.P with `weights` for the duration."""
    before = dict(oadv.P)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in weights.items():
            mp.setitem(oadv.P, k, v)
        yield
    assert oadv.P == before


def dense_return(weights, c, gamma, Ts=None):
    """oracle.advantage.rollout_return under `weights` on a dict of inputs (flags possibly wider than the horizon)."""
    Ts = c["delta_angle"].shape[1] if Ts is None else Ts
    with patched_P(weights):
        return oadv.rollout_return(c["delta_dis"], c["delta_angle"], c["speed"], c["acc"], c["ang_vel"], c["ang_acc"],
                                   c["collision"][:, :Ts], c["off_road"][:, :Ts], gamma)


def sparse_return(w, c, gamma):
    """SparseRewardModel inside the loop of get_rollout_return: the discounted infraction penalties up to and including the first collision."""
    G, Ts = c["delta_angle"].shape
    out = np.zeros(G)
    for i in range(G):
        for j in range(Ts):
            out[i] += (-w["alpha_collision"] * int(c["collision"][i, j]) - w["alpha_boundary"] * int(c["off_road"][i, j])) * gamma ** j
            if c["collision"][i, j]:
                break
    return out


def dense_terms(P, delta_dis, delta_angle, speed, acc, ang_acc, collision, offroad):
    """The seven terms of one step's dense reward, (R_collision, R_offroad, R_comfort, R_l_align, R_l_center, R_velocity, R_timestep), with
    the numpy 1.24 promotions written out; inputs np.float32 scalars, |delta_dis| and |delta_angle| already taken."""
    f32, f64 = np.float32, np.float64
    c = np.cos(f32(delta_angle))
    cs = f32(c * f32(speed))
    dd = abs(f64(f32(delta_dis)) - P["alpha_center_bias"])
    asp = abs(f32(speed))
    return np.array([
        -(f64(P["alpha_collision"]) + f64(asp)) * f64(collision),
        -P["alpha_boundary"] * offroad,
        -P["alpha_comfort"] * (int(abs(f32(acc)) > 4) + int(abs(f32(ang_acc)) > 4)),
        P["alpha_l_align"] * (f64(min(c, f32(0))) + P["alpha_vel_align"] * f64(min(cs, f32(0))) + 0.25 * (1 - f64(f32(delta_angle)) / (np.pi / 2))),
        -P["alpha_l_center"] * int(c > 0.5) * (dd - 0.05 / np.exp(dd - 0.5)),
        P["alpha_velocity"] * f64(max(c, f32(0))) * int(3 < asp < 20) * f64(asp),
        -P["alpha_timestep"] * int(asp > 0 or abs(f32(acc)) > 0)], dtype=np.float64)


def terms_ref(weights, c, gamma, sparse=False):
    """(G, 8): the discounted sums of the seven terms over the steps that count, and the number of those steps; also checks, step by
    step, that the restatement's sum IS oracle.advantage.dense_reward (1e-12)."""
    G, Ts = c["delta_angle"].shape
    out = np.zeros((G, 8))
    with patched_P(weights if not sparse else DEFAULTS):
        for i in range(G):
            for j in range(Ts):
                col, off = int(c["collision"][i, j]), int(c["off_road"][i, j])
                a = (abs(c["delta_dis"][i, j]), abs(c["delta_angle"][i, j]), c["speed"][i, j], c["acc"][i, j])
                if sparse:
                    t = np.array([-weights["alpha_collision"] * col, -weights["alpha_boundary"] * off, 0, 0, 0, 0, 0], dtype=np.float64)
                else:
                    t = dense_terms(oadv.P, *a, c["ang_acc"][i, j], col, off)
                    whole = oadv.dense_reward(*a, c["ang_vel"][i, j], c["ang_acc"][i, j], col, off)
                    assert abs(t.sum() - whole) <= 1e-12, (i, j, t.sum(), whole)
                out[i, :7] += t * gamma ** j
                out[i, 7] += 1
                if col:
                    break
    return out
