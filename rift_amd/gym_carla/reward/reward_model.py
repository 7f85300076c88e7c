"""DenseRewardModel / SparseRewardModel -- the reward models of the rollout return (rift/gym_carla/reward/reward_model.py:11-91) as
parameter containers: `params` is the dict the reference keeps for editing, and what Engine.eval_params copies into RiftEvalParams for the
device (rift_rollout_return_ex, rift_group_advantage_tick_ex).  get_reward is the host statement of one step's reward, for logging and
checks; the rollout return itself runs on the HIP engine.

The dtype promotion is that of the reference environment (numpy 1.24: np.float32 scalar (op) python float -> float64, np.float32 (op)
np.float32 -> float32), written out so that the value does not depend on the installed numpy's promotion rules."""
import numpy as np

DENSE_KEYS = ('alpha_collision', 'alpha_boundary', 'alpha_comfort', 'alpha_l_align', 'alpha_vel_align', 'alpha_l_center',
              'alpha_center_bias', 'alpha_velocity', 'alpha_timestep')          # the order of RiftEvalParams (include/rift_hip.h)
SPARSE_KEYS = ('alpha_collision', 'alpha_boundary')


class DenseRewardModel:
    kind = 'dense'

    def __init__(self, **overrides):
        self.params = self._sample_params()
        _override(self.params, overrides)

    def _sample_params(self):
        return dict(zip(DENSE_KEYS, (20.0, 5.0, 0.8, 0.5, 0.05, 0.6, 0.0, 0.1, 0.1)))

    def get_params(self):
        return self.params

    def get_terms(self, delta_dis, delta_angle, speed, acc, angular_speed, angular_acc, collision, offroad):
        """(R_collision, R_offroad, R_comfort, R_l_align, R_l_center, R_velocity, R_timestep) of one step, float64."""
        p, f32, f64 = self.params, np.float32, np.float64
        delta_dis, delta_angle, speed, acc, angular_acc = (f32(x) for x in (delta_dis, delta_angle, speed, acc, angular_acc))
        a_speed = abs(speed)
        cos = np.cos(delta_angle)                                       # float32
        cos_speed = f32(cos * speed)                                    # float32 * float32
        dis = abs(f64(delta_dis) - p['alpha_center_bias'])
        return (-(f64(p['alpha_collision']) + f64(a_speed)) * f64(collision),
                f64(-p['alpha_boundary'] * offroad),
                f64(-p['alpha_comfort'] * (int(abs(acc) > 4) + int(abs(angular_acc) > 4))),
                p['alpha_l_align'] * (f64(min(cos, f32(0))) + p['alpha_vel_align'] * f64(min(cos_speed, f32(0)))
                                      + 0.25 * (1 - f64(abs(delta_angle)) / (np.pi / 2))),
                -p['alpha_l_center'] * int(cos > 0.5) * (dis - 0.05 / np.exp(dis - 0.5)),
                p['alpha_velocity'] * f64(max(cos, f32(0))) * int(3 < a_speed < 20) * f64(a_speed),
                f64(-p['alpha_timestep'] * int(a_speed > 0 or abs(acc) > 0)))

    def get_reward(self, delta_dis, delta_angle, speed, acc, angular_speed, angular_acc, collision, offroad):
        t = self.get_terms(delta_dis, delta_angle, speed, acc, angular_speed, angular_acc, collision, offroad)
        return t[0] + t[1] + t[2] + t[3] + t[4] + t[5] + t[6]


class SparseRewardModel:
    kind = 'sparse'

    def __init__(self, **overrides):
        self.params = self._sample_params()
        _override(self.params, overrides)

    def _sample_params(self):
        return {'alpha_collision': 15.0, 'alpha_boundary': 15.0}

    def get_params(self):
        return self.params

    def get_terms(self, collision, offroad):
        return (np.float64(-self.params['alpha_collision'] * collision), np.float64(-self.params['alpha_boundary'] * offroad)) + (np.float64(0.0),) * 5

    def get_reward(self, collision, offroad):
        return -self.params['alpha_collision'] * collision + -self.params['alpha_boundary'] * offroad


def _override(params, overrides):
    unknown = sorted(set(overrides) - set(params))
    if unknown:
        raise ValueError(f"unknown reward parameter(s) {unknown}; known: {sorted(params)}")
    params.update({k: float(v) for k, v in overrides.items()})


def rollout_return(model, delta_dis, delta_angle, speed, acc, ang_vel, ang_acc, collision, off_road, gamma=0.98):
    """Host statement of get_rollout_return (traj_eval/traj_evaluator.py:333-370) with either model: the discounted reward of every
    candidate (G,) float64, counting up to and including the first colliding step."""
    G, Ts = np.asarray(delta_angle).shape
    out = np.zeros((G,), dtype=np.float64)
    for i in range(G):
        for j in range(Ts):
            col, off = int(collision[i][j]), int(off_road[i][j])
            if model.kind == 'sparse':
                r = model.get_reward(col, off)
            else:
                r = model.get_reward(abs(delta_dis[i][j]), abs(delta_angle[i][j]), speed[i][j], acc[i][j], ang_vel[i][j], ang_acc[i][j], col, off)
            out[i] += r * gamma ** j
            if col:
                break
    return out
