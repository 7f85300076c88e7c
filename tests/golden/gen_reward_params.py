"""Writes tests/golden/reward_params.npz: the reference's own get_rollout_return (traj_eval/traj_evaluator.py:333-370) with
DenseRewardModel.params edited (reward_model.py:16-32) and with SparseRewardModel (:60-91), on tests.helpers.advantage_inputs().

    python tests/golden/gen_reward_params.py          # needs the reference checkout (tests/golden/ref_loader.py)

Per dense weight set S of tests/eval_param_cases.SETS and gamma g: `ret_S_g` (48,) float64 and its group z-score `z_S_g`
(traj_evaluator.py:467-470); `weights_S` (9,) in the order of eval_param_cases.KEYS.  Sparse: `ret_sparse_<name>_g` with the reference
class's own defaults ("reference") and with edited ones; get_rollout_return hands the reward model eight arguments, of which the sparse
model takes the last two -- the adapter below does nothing else.  Data only."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import eval_param_cases as E  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.golden import ref_loader  # noqa: E402
from tests.golden.gen_golden import _ref_function  # noqa: E402


class _SparseAdapter:
    def __init__(self, model):
        self.model = model

    def get_reward(self, delta_dis, delta_angle, speed, acc, angular_speed, angular_acc, collision, offroad):
        return self.model.get_reward(collision, offroad)


def main():
    import types
    ref_loader.install()
    rr = _ref_function("rift/cbv/planning/fine_tuner/rlft/traj_eval/traj_evaluator.py", "get_rollout_return")
    spec = importlib.util.spec_from_file_location("ref_reward_model", os.path.join(ref_loader.REF_ROOT, "rift/gym_carla/reward/reward_model.py"))
    rm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rm)
    i = H.advantage_inputs()
    args = (i["delta_dis"], i["delta_angle"], i["speed"], i["acc"], i["ang_vel"], i["ang_acc"], i["collision"], i["off_road"])
    out = {}
    for name, weights in E.SETS.items():
        model = rm.DenseRewardModel()
        assert tuple(model.get_params()) == E.KEYS and model.get_params() == E.DEFAULTS
        model.params.update(weights)
        out[f"weights_{name}"] = np.array([weights[k] for k in E.KEYS])
        for g in E.GAMMAS:
            ret = rr(types.SimpleNamespace(reward_model=model), *args, gamma=g)
            out[f"ret_{name}_{g}"] = ret
            out[f"z_{name}_{g}"] = (ret - np.mean(ret)) / (np.std(ret) + 1e-5)
    for name, weights in E.SPARSE.items():
        model = rm.SparseRewardModel()
        if name == "reference":
            assert model.get_params() == weights
        model.params.update(weights)
        out[f"weights_sparse_{name}"] = np.array([weights["alpha_collision"], weights["alpha_boundary"]])
        for g in E.GAMMAS:
            out[f"ret_sparse_{name}_{g}"] = rr(types.SimpleNamespace(reward_model=_SparseAdapter(model)), *args, gamma=g)
    path = os.path.join(HERE, "reward_params.npz")
    np.savez_compressed(path, **out)
    print("reward_params ->", path, f"{os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
