"""The conditions of tests/test_gpu_objective_params.py on the references alone, and the host side of the objective settings (no GPU):
restated_ex is the fp64 oracle at a kind's defaults; every setting a GPU test uses moves the restatement by at least 100 loss bars and 50
gradient bars (25 for the entropy term at 0.5) on every batch it is used on; no realised ratio lies near an edge a setting introduces, so
the counts of `terms` follow from the placed classes; the struct, its defaults and refusals, objective_params and the policies'
config['objective'].  A case that fails a condition is redesigned, not loosened."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from oracle import pluto_ref
from tests import helpers as H
from tests import objective_cases as O
from tests import objective_param_cases as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def forwards():
    """{(batch, head factor): (r_pad, logits, q_final, state dict)} from the CPU oracle's forward, computed once."""
    out = {}
    for name in P.ALL:
        for w in sorted({O.head_scale(name, kind) for kind in ("rift", "grpo")}):
            sd = O.spread_weights(H.weights(), w)
            b = O.batch(name)
            ref, _, taps = pluto_ref.planning_model_forward(sd, b["cur_pluto_feature_torch"], need_traj=False, want_taps=True)
            out[name, w] = (O.line_padding(b), ref["probability"], taps["q_final"], sd)
    return out


@pytest.fixture(scope="module")
def cases(forwards):
    """{(batch, kind): (case, info, r_pad, q_final, state dict, the restatement at the kind's defaults)}, shared and left unchanged."""
    out = {}
    for name in P.ALL:
        for kind in ("rift", "grpo"):
            r_pad, prob, qf, sd = forwards[name, O.head_scale(name, kind)]
            c, info = P.build_case(name, kind, prob, r_pad)
            info["ratios"] = O.realised_ratios(prob, r_pad, c["old_group_logits_torch"])
            out[name, kind] = (c, info, r_pad, qf, sd, P.reference(sd, qf, kind, c, r_pad, P.DEFAULTS[kind]))
    return out


@pytest.mark.parametrize("kind", ["rift", "grpo"])
@pytest.mark.parametrize("name", P.ALL)
def test_restatement_is_the_oracle_at_the_defaults(cases, name, kind):
    """restated_ex at a kind's defaults = objective_cases.restated bit for bit (the same operations) = the fp64 oracle to 1e-12: the chain
    oracle -> fixtures holds for the new reference.  The other kind's name with this kind's settings gives the same numbers."""
    c, info, r_pad, qf, sd, ref = cases[name, kind]
    old = O.restated(sd, qf, kind, c, r_pad)
    r64 = O.objective_ref64(sd, qf, kind, c, r_pad)
    assert float(ref[0]) == float(old[0]) and all(torch.equal(ref[1][k], old[1][k]) for k in ref[1])
    assert abs(float(ref[0]) - float(r64[0])) < 1e-12 and max(float((ref[1][k] - r64[1][k]).abs().max()) for k in ref[1]) < 1e-12
    other = P.reference(sd, qf, "grpo" if kind == "rift" else "rift", c, r_pad, P.DEFAULTS[kind])
    assert float(other[0]) == float(ref[0]) and all(torch.equal(other[1][k], ref[1][k]) for k in ref[1]) and torch.equal(other[2], ref[2])
    t = ref[2]
    s = P.DEFAULTS[kind]
    assert float(t[5]) == float(c["group_advantage_mask_torch"].sum()) and float(t[6]) == 0.0 and float(t[7]) == 0.0
    assert abs(float(t[0] - s["kl_beta"] * t[1] + s["entropy_coef"] * t[2]) / float(t[5]) + float(ref[0])) < 1e-12


@pytest.mark.parametrize("kind,sname,name", P.CASES)
def test_every_setting_is_visible_on_the_restatement(cases, kind, sname, name):
    c, info, r_pad, qf, sd, ref = cases[name, kind]
    s = P.settings(kind, sname)
    got = P.reference(sd, qf, kind, c, r_pad, s)
    ml, mg = P.moved(ref, got)
    need = P.SETTINGS[kind][sname][1]
    print(f"{kind} {sname} on {name}: loss moves by {ml / O.LOSS_BAR:.0f} loss bars, gradients by {mg:.0f} bars (asked: 100 / {need})")
    assert ml >= 100 * O.LOSS_BAR and mg >= need
    # the sums: the identity with the loss, and the counts from the placed classes alone
    t = got[2]
    assert abs(float(t[0] - s["kl_beta"] * t[1] + s["entropy_coef"] * t[2]) / float(t[5]) + float(got[0])) < 1e-12
    assert (int(t[3]), int(t[4]), int(t[5])) == P.expected_counts(c, info, s)
    assert (float(t[1]) != 0.0) == (s["kl_beta"] != 0.0) and (float(t[2]) != 0.0) == (s["entropy_coef"] != 0.0)


@pytest.mark.parametrize("kind", ["rift", "grpo"])
@pytest.mark.parametrize("name", P.ALL)
def test_no_ratio_lies_near_an_edge_a_setting_uses(cases, name, kind):
    c, info, r_pad, qf, sd, ref = cases[name, kind]
    keep = c["group_advantage_mask_torch"].view(info["ratios"].shape).numpy()
    off, _ = O.ratio_margin(info, info["ratios"])
    assert off < 1e-5
    d = P.edge_distances(info["ratios"], keep)
    print(f"{name} {kind}: placement error {off:.1e}; nearest valid ratio per edge " + ", ".join(f"{e}: {v:.3f}" for e, v in sorted(d.items())))
    for e, margin in P.EDGES.items():
        assert d[e] >= margin - 1e-5, e          # (a target on the margin itself realises within the placement error of it)
    # the counts at the defaults and at the combined settings differ: the settings change which candidates are clamped and floored
    assert P.expected_counts(c, info, P.DEFAULTS[kind]) != P.expected_counts(c, info, dict(P.DEFAULTS[kind], **P.COMBINED))
    assert P.expected_counts(c, info, P.DEFAULTS[kind]) == tuple(int(v) for v in ref[2][3:6])


@pytest.mark.parametrize("kind", ["rift", "grpo"])
def test_settings_that_move_nothing_are_not_used(cases, kind):
    """The asymmetric range on `one` (no 1.26 class there: RIFT's deal holds no A > 0 above 1.2 at all, GRPO's holds (1.5, +1), clamped and
    gradient-free under either range) and dual_clip 3 on GRPO's classes (no ratio above 1.5) leave the gradients, or everything, where
    they are: which is why no test uses them."""
    c, info, r_pad, qf, sd, ref = cases["one", kind]
    ml, mg = P.moved(ref, P.reference(sd, qf, kind, c, r_pad, dict(P.DEFAULTS[kind], clip_high=1.28)))
    assert mg == 0.0 and (ml == 0.0 or kind == "grpo")
    if kind == "grpo":
        for name in P.ALL:
            c, info, r_pad, qf, sd, ref = cases[name, kind]
            assert P.moved(ref, P.reference(sd, qf, kind, c, r_pad, dict(P.DEFAULTS[kind], dual_clip=3.0))) == (0.0, 0.0)


# ---- host only ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_defaults_and_declarations(tmp_path):
    """RiftObjectiveParams as gcc lays it out (the method of test_ctypes_structs_match_the_header_as_a_c_compiler_lays_it_out), the two new
    declarations, and rift_objective_params_default for both kinds and for a refused one -- no context, no device."""
    from rift_amd import _ffi
    assert ctypes.sizeof(_ffi.RiftObjectiveParams) == 40 and tuple(f for f, _ in _ffi.RiftObjectiveParams._fields_) == P.KEYS == _ffi.OBJECTIVE_KEYS
    gcc = shutil.which("gcc")
    if gcc is not None:
        lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rift_hip.h"', 'int main(void) {', '  printf("%zu", sizeof(RiftObjectiveParams));']
        lines += [f'  printf(" %zu", offsetof(RiftObjectiveParams, {f}));' for f in P.KEYS] + ['  return 0;', '}']
        src = tmp_path / "layout.c"
        src.write_text("\n".join(lines))
        subprocess.check_call([gcc, "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "layout")])
        size, *offs = map(int, subprocess.check_output([str(tmp_path / "layout")], text=True).split())
        assert size == ctypes.sizeof(_ffi.RiftObjectiveParams)
        assert [getattr(_ffi.RiftObjectiveParams, f).offset for f in P.KEYS] == offs
    hdr = open(os.path.join(REPO, "include", "rift_hip.h")).read()
    for name in ("rift_objective_params_default", "rift_loss_backward_ex"):
        assert name in _ffi.EXPORTS and f"int {name}(" in hdr
    lib = _ffi.load_library()
    for kind in ("rift", "grpo"):
        p = _ffi.RiftObjectiveParams()
        ctypes.memset(ctypes.byref(p), 0xff, ctypes.sizeof(p))
        assert lib.rift_objective_params_default(_ffi.LOSS_KINDS[kind], ctypes.byref(p)) == 0
        assert {k: getattr(p, k) for k in P.KEYS} == P.DEFAULTS[kind]
    for kind in (_ffi.LOSS_KINDS["ppo"], _ffi.LOSS_KINDS["reinforce"], _ffi.LOSS_KINDS["sft"], -1, 5):
        p = _ffi.RiftObjectiveParams(1.0, 2.0, 3.0, 4.0, 5.0)
        assert lib.rift_objective_params_default(kind, ctypes.byref(p)) == -1
        assert [getattr(p, k) for k in P.KEYS] == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert lib.rift_objective_params_default(0, None) == -1


def test_objective_params_fills_the_defaults_and_refuses_unknown_keys():
    from rift_amd import _ffi
    p = _ffi.objective_params("rift")
    assert {k: getattr(p, k) for k in P.KEYS} == P.DEFAULTS["rift"]
    p = _ffi.objective_params("grpo", dual_clip=1.35, entropy_coef=0.5)
    assert {k: getattr(p, k) for k in P.KEYS} == dict(P.DEFAULTS["grpo"], dual_clip=1.35, entropy_coef=0.5)
    assert bytes(memoryview(_ffi.objective_params("rift", kl_beta=0.2))) == bytes(memoryview(_ffi.objective_params("grpo", dual_clip=3.0)))
    with pytest.raises(ValueError, match="unknown key.*clip_hi.*known.*clip_low.*clip_high.*dual_clip.*kl_beta.*entropy_coef"):
        _ffi.objective_params("rift", clip_hi=1.3)
    for kind in ("ppo", "reinforce", "sft"):
        with pytest.raises(ValueError, match="rift.*grpo"):
            _ffi.objective_params(kind)


def test_policy_objective_configuration():
    """config['objective'] of rift_pluto / grpo_pluto: read like config['traj_eval'] -- an unknown key raises and names the known ones,
    rift_pluto with kl_beta > 0 points to grpo_pluto with dual_clip 3.0, every other policy raises on the key -- and is what train() hands to
    the trainer; without the key there is nothing to hand over."""
    from rift_amd.planning import CBV_POLICY_LIST
    base = {'num_scenario': 1, 'device': 'cpu'}
    with pytest.raises(ValueError, match="unknown key.*clip_hi.*known.*clip_low.*clip_high.*dual_clip.*kl_beta.*entropy_coef"):
        CBV_POLICY_LIST['rift_pluto'](dict(base, objective={'clip_hi': 1.3}), None)
    with pytest.raises(ValueError, match="unknown key.*beta"):
        CBV_POLICY_LIST['grpo_pluto'](dict(base, objective={'beta': 0.1}), None)
    with pytest.raises(ValueError, match=r"kl_beta.*rift_pluto.*reference logits.*grpo_pluto.*'dual_clip': 3\.0"):
        CBV_POLICY_LIST['rift_pluto'](dict(base, objective={'kl_beta': 0.2}), None)
    for name in sorted(set(CBV_POLICY_LIST) - {'rift_pluto', 'grpo_pluto'}):
        with pytest.raises(ValueError, match=r"config\['objective'\].*" + name):
            CBV_POLICY_LIST[name](dict(base, objective={}), None)
    assert len(CBV_POLICY_LIST) == 8
    assert CBV_POLICY_LIST['rift_pluto'](dict(base), None)._objective is None
    assert CBV_POLICY_LIST['rift_pluto'](dict(base, objective={}), None)._objective == {}
    assert CBV_POLICY_LIST['rift_pluto'](dict(base, objective={'kl_beta': 0, 'dual_clip': 2}), None)._objective == {'kl_beta': 0.0, 'dual_clip': 2.0}
    pol = CBV_POLICY_LIST['grpo_pluto'](dict(base, objective=dict(P.COMBINED)), None)
    assert pol._objective == P.COMBINED


def test_trainer_refuses_objective_settings_it_cannot_honour():
    """RLFTTrainer(objective=...) decides before it touches the model or the device: a kind without group objective, an unknown key, and
    the term sums under data parallelism (per-rank sums that nothing all-reduces)."""
    from rift_amd.planning.fine_tuner.rlft.trainer import RLFTTrainer
    with pytest.raises(ValueError, match="rift.*grpo.*reinforce"):
        RLFTTrainer(None, kind="reinforce", objective={})
    with pytest.raises(ValueError, match="unknown key.*clip"):
        RLFTTrainer(None, kind="rift", objective={"clip": 0.3})
    with pytest.raises(ValueError, match="terms.*data parallelism"):
        RLFTTrainer(None, kind="grpo", objective={"terms": True}, exchange=lambda t: None, dp_rank=0, dp_world=2)
