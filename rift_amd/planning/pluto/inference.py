"""Rollout-side inference helpers: what RIFTPluto.get_action / _get_action does between the model
forward and the CARLA control call (rift_pluto.py:28-161, pluto.py:196-300), without CarlaDataProvider: the caller passes the CBV's
rear-axle pose and speed.  The model forward is the HIP engine in eval mode (all outputs); the per-CBV post-processing is a
few dozen candidates per tick and stays on the host in numpy / float64, as in the reference."""
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from scipy.special import softmax

from rift_amd.planning.pluto.controller.pid_controller import PIDController


def trim_candidates(candidate_trajectories: np.ndarray, probability: np.ndarray, origin: np.ndarray, angle: float,
                    ref_free_trajectory: Optional[np.ndarray] = None, topk: int = 10):
    """pluto.py:196-247: top-k candidates by logit (stable descending argsort), softmax over the kept logits, optional ref-free
    candidate with score 0.25 and index -1, rotation + translation to the global frame, first point duplicated in front.
    Returns (trajectories (k[+1], T+1, 3), scores, original flat indices int64, n_ref, n_mode)."""
    n_ref, n_mode, T, C = candidate_trajectories.shape
    cand = candidate_trajectories.reshape(-1, T, C)
    flat = probability.reshape(-1)
    order = np.argsort(-flat)
    traj = cand[order][:topk]
    score = softmax(flat[order][:topk])
    orig = np.arange(n_ref * n_mode)[order][:topk]
    if ref_free_trajectory is not None:
        traj = np.concatenate([traj, ref_free_trajectory[None, ...]], axis=0)
        score = np.concatenate([score, [0.25]], axis=0)
        orig = np.concatenate([orig, [-1]], axis=0)
    rot = np.array([[np.cos(angle), np.sin(angle)], [-np.sin(angle), np.cos(angle)]])
    traj[..., :2] = np.matmul(traj[..., :2], rot) + origin
    traj[..., 2] += angle
    traj = np.concatenate([traj[..., 0:1, :], traj], axis=-2)
    return traj, score, orig, n_ref, n_mode


def candidate_distribution(flat_logits: np.ndarray, topk: int, temperature: float):
    """The distribution sample_candidate draws from (include/rift_select.h: kept set, weights, prefix sums):
    -> (order, kept, w, c): `order` the `topk` largest logits by descending logit, ties to the lower flat index; `kept` the same flat
    indices in ascending order; `w` (fp32) their weights expf((z - z_top) * r), r the fp32 reciprocal of the temperature; `c` (fp64) the
    inclusive prefix sums of `w` in `kept` order, c[-1] = W."""
    z = np.asarray(flat_logits, dtype=np.float32).reshape(-1)
    order = np.argsort(-z, kind="stable")[:int(topk)]
    kept = np.sort(order)
    inv_t = np.float32(min(1.0 / float(temperature), float(np.finfo(np.float32).max)))
    with np.errstate(under="ignore", invalid="ignore"):
        w = np.exp(((z[kept] - z[order[0]]) * inv_t).astype(np.float32)).astype(np.float32)
    return order, kept, w, np.cumsum(w.astype(np.float64))


def sample_candidate(flat_logits: np.ndarray, topk: int, temperature: float, u: float) -> Tuple[int, int, float]:
    """The host statement of the sampled choice (include/rift_select.h states the rule; the SAMPLE stage of control_tick_kernel is tested
    against this function): among the `topk` largest of the flat logits, draw with weights expf((z - z_top) / T) in fp32 and prefix sums in
    fp64 over ascending flat index -- the first kept candidate with a positive weight and u * W < c, the last such candidate if rounding
    leaves none.  -> (flat index, position in the kept list by descending logit, probability w / W).
    The ref-free rule is the caller's and comes first (PLUTO._decide): this function is asked only when a learned candidate is executed.
    The ordering is a STABLE descending sort (exact ties to the lower flat index, as the device keeps them).  trim_candidates sorts with
    numpy's default kind, which promises no order among equal logits: the two can differ in which of several equal logits at the edge of
    the kept set is kept, and in the positions of equal logits inside it."""
    order, kept, w, c = candidate_distribution(flat_logits, topk, temperature)
    live = w > 0
    hit = np.nonzero(live & (float(u) * c[-1] < c))[0]
    drawable = np.nonzero(live)[0]
    if hit.size == 0 and drawable.size == 0:           # (non-finite logits, outside the contract: the greedy top)
        return int(order[0]), 0, float("nan")
    j = int(hit[0]) if hit.size else int(drawable[-1])
    flat = int(kept[j])
    return flat, int(np.nonzero(order == flat)[0][0]), float(np.float64(w[j]) / c[-1])


def global_to_local(global_trajectory: np.ndarray, origin: np.ndarray, angle: float) -> np.ndarray:
    """pluto.py:262-279: re-anchor the first point on the rear axle, rotate into the vehicle frame."""
    delta = origin - global_trajectory[0, :2]
    pos = global_trajectory[..., :2] + delta
    rot = np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]])
    position = np.matmul(pos - origin, rot)
    heading = global_trajectory[..., 2] - angle
    return np.concatenate([position, heading[..., None]], axis=-1)


def action_mode_of(orig_index: int, n_mode: int) -> Tuple[int, int]:
    """(r_idx, m_idx) of a flat candidate index (rlft_pluto.py:174-176); integer, bit-exact."""
    return int(orig_index) // n_mode, int(orig_index) % n_mode


class ControlSlots:
    """Which row of the device-side controller state (rift_control_tick's `pid_state`) belongs to which CBV.  A key -- (env_id, cbv_id) --
    gets a row that holds zeros, i.e. a freshly constructed PIDController: a row never used before, or a released one the caller has
    zeroed since.  release() only parks a row; it is handed out again after zeroed() has confirmed the memset."""

    def __init__(self):
        self._slot: Dict = {}
        self._free: list = []          # zeroed, reusable
        self._released: list = []      # left by their CBV, still holding its state
        self._rows = 0                 # rows handed out so far (rows beyond them have never been written)

    def slot(self, key) -> int:
        if key not in self._slot:
            if self._free:
                self._slot[key] = self._free.pop()
            else:
                self._slot[key] = self._rows
                self._rows += 1
        return self._slot[key]

    def release(self, key):
        if key in self._slot:
            self._released.append(self._slot.pop(key))

    def pending(self) -> list:
        """Rows released and not zeroed yet."""
        return list(self._released)

    def zeroed(self, slots):
        """The caller has zeroed `slots` (rows reported by pending()): they may be handed out again."""
        for s in slots:
            self._released.remove(s)
            self._free.append(s)

    def keys(self):
        return list(self._slot)

    def __contains__(self, key):
        return key in self._slot

    def __len__(self):
        return len(self._slot)

    @property
    def rows(self) -> int:
        return self._rows


class PlutoInference:
    """Eval-mode policy step for a batch of CBVs: HIP forward with every output, then per-CBV candidate selection and PID control."""

    def __init__(self, model, topk: int = 10, use_ref_free: bool = True):
        self.model, self.topk, self.use_ref_free = model, topk, use_ref_free
        self.controllers: Dict = {}

    @torch.no_grad()
    def forward(self, feature_data: Dict) -> Dict[str, torch.Tensor]:
        was_training, need = self.model.training, self.model.need_traj
        self.model.eval()
        self.model.need_traj = True
        try:
            return self.model(feature_data)
        finally:
            self.model.need_traj = need
            self.model.train(was_training)

    def act(self, outputs: Dict[str, torch.Tensor], index: int, cbv_id, origin: np.ndarray, angle: float, speed: float):
        """-> ((throttle, steer, brake), chosen global trajectory (79, 3), candidates, scores, flat indices)."""
        cand = outputs["candidate_trajectories"][index].cpu().numpy().astype(np.float64)
        prob = outputs["probability"][index].cpu().numpy()
        rf = None
        if self.use_ref_free and "output_ref_free_trajectory" in outputs:
            rf = outputs["output_ref_free_trajectory"][index].cpu().numpy().astype(np.float64)
        cands, score, orig, _, n_mode = trim_candidates(cand, prob, np.asarray(origin, dtype=np.float64), float(angle), rf, self.topk)
        best = int(score.argmax())
        trajectory = cands[best, 1:]
        local = global_to_local(trajectory, np.asarray(origin, dtype=np.float64), float(angle))
        ctrl = self.controllers.setdefault(cbv_id, PIDController())
        return ctrl.control_pid(local[:, :2], float(speed)), trajectory, cands, score, orig
