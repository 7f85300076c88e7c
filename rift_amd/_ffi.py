"""ctypes binding of ``librift_hip.so`` (C-ABI in ``include/rift_hip.h``).

The mirror of the header -- its constants, structs and function signatures -- is ``rift_amd/_abi.py``, which
``tools/gen/abi_trampolines.py`` generates from the header; this module gives those names the spellings the package uses and adds what
the header does not say: the order the feature batch is filled in, the parameter names and sizes behind the flat gradient vectors, and
the Engine.

The product path has NO CPU fallback: if the shared library is missing or fails
to load, importing the engine raises immediately.
"""
import ctypes as C
import threading
import os
from typing import Dict, Optional

import numpy as np
import torch

from rift_amd import _abi, _abi_advantage, _abi_drivable, _abi_footprint, _abi_offroad, _abi_select, tick_pack
from rift_amd._abi import (EXPORTS, RiftControlCBV, RiftCritic, RiftDp, RiftEvalParams, RiftFeatureBatch, RiftLossIn,  # noqa: F401
                           RiftLossOut, RiftObjectiveParams, RiftOutputs, RiftReplayArena, RiftRolloutIO, RiftTensorDesc, RiftTickCBV)
from rift_amd._abi_drivable import RiftDrivableInfo      # the drivable-area-map extension (include/rift_drivable.h)
from rift_amd._abi_advantage import RiftAdvantageParams  # the arena-advantage extension (include/rift_advantage.h)
from rift_amd._abi_select import RiftSelectParams        # the candidate-selection extension (include/rift_select.h)
from rift_amd._abi_footprint import RiftCollisionParams  # the collision-test extension (include/rift_footprint.h)
from rift_amd._abi_offroad import RiftOffRoadParams      # the off-road-extent extension (include/rift_offroad.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librift_hip.so")


def _enum(prefix: str) -> Dict[str, int]:
    """{"rift": 0, ...} from the header's enumerators RIFT_LOSS_RIFT = 0, ..., in header order."""
    return {k[len(prefix):].lower(): v for k, v in vars(_abi).items() if k.startswith(prefix)}


F_TRAIN, F_NEED_TRAJ, F_FP32, F_NO_DROP = _abi.RIFT_F_TRAIN, _abi.RIFT_F_NEED_TRAJ, _abi.RIFT_F_FP32, _abi.RIFT_F_NO_DROP
F_NO_BN_UPDATE, F_DEFER_HEAD = _abi.RIFT_F_NO_BN_UPDATE, _abi.RIFT_F_DEFER_HEAD
DEFER_SLOTS = _abi.RIFT_DEFER_SLOTS        # activation arenas the deferred-head forwards cycle through
LOSS_KINDS = _enum("RIFT_LOSS_")
REWARD_MODELS = _enum("RIFT_REWARD_")
OPERANDS = _enum("RIFT_OPERANDS_")         # the 16-bit MFMA operand format of a context's fused kernels
PI_NPARAM, CRITIC_NPARAM = _abi.RIFT_PI_NPARAM, _abi.RIFT_CRITIC_NPARAM_C
CONTROL_STATE = _abi.RIFT_CONTROL_STATE    # doubles per pid_state row of rift_control_tick: turn ring (20) | speed ring (20) | turn head, last | speed head, last
EXCHANGE_FN = _abi.RiftExchangeFn

vp = C.c_void_p

_FB_PTRS = [
    "agent_position", "agent_heading", "agent_velocity", "agent_shape", "agent_category", "agent_valid_mask",
    "map_point_position", "map_point_vector", "map_point_orientation", "map_polygon_center", "map_polygon_type",
    "map_polygon_on_route", "map_polygon_tl_status", "map_polygon_has_speed_limit", "map_polygon_speed_limit",
    "map_valid_mask", "ref_position", "ref_vector", "ref_orientation", "ref_valid_mask", "static_position",
    "static_heading", "static_shape", "static_category", "static_valid_mask", "current_state",
]
assert _FB_PTRS == [n for n, t in RiftFeatureBatch._fields_ if t is vp], "_FB_PTRS and the pointers of RiftFeatureBatch (include/rift_hip.h) differ"


def eval_params(reward_model=None, gamma: float = 0.98, bbox_inflation_ratio: float = 1.1, resolution: float = 0.5,
                near_lane_change: bool = True) -> RiftEvalParams:
    """RiftEvalParams from a reward model of rift_amd.gym_carla.reward.reward_model (None: DenseRewardModel's defaults) and the reference's
    TrajEvaluator arguments.  The sparse model carries two weights; the other seven stay at the dense defaults (the device does not read
    them).  Refusals (a NaN, gamma < 0, ...) are the library's, at the call that takes the struct."""
    from rift_amd.gym_carla.reward.reward_model import DenseRewardModel
    p = RiftEvalParams()
    weights = DenseRewardModel().get_params()
    kind = "dense"
    if reward_model is not None:
        kind = reward_model.kind
        unknown = sorted(set(reward_model.get_params()) - set(weights))
        if kind not in REWARD_MODELS or unknown:
            raise ValueError(f"reward model {kind!r} with parameter(s) {unknown}: known models {sorted(REWARD_MODELS)}, known parameters {sorted(weights)}")
        weights.update(reward_model.get_params())
    p.reward_model, p.near_lane_change, p.gamma = REWARD_MODELS[kind], 1 if near_lane_change else 0, float(gamma)
    for k, v in weights.items():
        setattr(p, k, float(v))
    p.bbox_inflation_ratio, p.resolution = float(bbox_inflation_ratio), float(resolution)
    return p


OBJECTIVE_KEYS = tuple(n for n, _ in RiftObjectiveParams._fields_)
OBJECTIVE_KINDS = ("rift", "grpo")


def objective_params(kind: str, **settings) -> RiftObjectiveParams:
    """RiftObjectiveParams of kind 'rift' / 'grpo': the library's defaults of that kind (rift_objective_params_default) with `settings`
    (clip_low, clip_high, dual_clip, kl_beta, entropy_coef) on top.  An unknown key or a kind without settings raises ValueError; what a
    value may be (clip_low in (0, 1], ...) is the library's refusal, at the call that takes the struct."""
    if kind not in OBJECTIVE_KINDS:
        raise ValueError(f"objective settings exist for the kinds {list(OBJECTIVE_KINDS)}, not for {kind!r}")
    unknown = sorted(set(settings) - set(OBJECTIVE_KEYS))
    if unknown:
        raise ValueError(f"objective: unknown key(s) {unknown}; known: {list(OBJECTIVE_KEYS)}")
    p = RiftObjectiveParams()
    rc = load_library().rift_objective_params_default(LOSS_KINDS[kind], C.byref(p))
    if rc != 0:
        raise RuntimeError(f"rift_objective_params_default failed ({rc})")
    for k, v in settings.items():
        setattr(p, k, float(v))
    return p


ADVANTAGE_BASELINES = {"mean": _abi_advantage.RIFTGA_BASELINE_MEAN, "leave_one_out": _abi_advantage.RIFTGA_BASELINE_LEAVE_ONE_OUT,
                       "none": _abi_advantage.RIFTGA_BASELINE_NONE}
ADVANTAGE_SCALES = {"group_std": _abi_advantage.RIFTGA_SCALE_GROUP_STD, "batch_rms": _abi_advantage.RIFTGA_SCALE_BATCH_RMS,
                    "none": _abi_advantage.RIFTGA_SCALE_NONE}
ADVANTAGE_KEYS = ("baseline", "scale", "clip", "eps")


def advantage_params(baseline: str = "mean", scale: str = "group_std", clip: float = 0.0, eps: float = 1e-5) -> RiftAdvantageParams:
    """RiftAdvantageParams of Engine.arena_advantage (include/rift_advantage.h states the rule): the baseline and the scale by name; the
    defaults are the reference's z-score.  An unknown name raises ValueError; what a value may be (clip >= 0, ...) is the library's
    refusal, at the call that takes the struct."""
    if baseline not in ADVANTAGE_BASELINES:
        raise ValueError(f"advantage: baseline = {baseline!r}; known: {list(ADVANTAGE_BASELINES)}")
    if scale not in ADVANTAGE_SCALES:
        raise ValueError(f"advantage: scale = {scale!r}; known: {list(ADVANTAGE_SCALES)}")
    p = RiftAdvantageParams()
    p.baseline, p.scale, p.eps, p.clip = ADVANTAGE_BASELINES[baseline], ADVANTAGE_SCALES[scale], float(eps), float(clip)
    return p


SELECT_MODES = {"greedy": _abi_select.RIFTCS_GREEDY, "sample": _abi_select.RIFTCS_SAMPLE}
SELECT_KEYS = ("mode", "temperature")


def select_params(mode: str = "greedy", temperature: float = 1.0) -> RiftSelectParams:
    """RiftSelectParams of Engine.control_tick(select=...) (include/rift_select.h states the rule): the mode by name; the default is the
    greedy choice of rift_control_tick.  An unknown name raises ValueError; what the temperature may be (finite, > 0) is the library's
    refusal, at the call that takes the struct."""
    if mode not in SELECT_MODES:
        raise ValueError(f"select: mode = {mode!r}; known: {list(SELECT_MODES)}")
    p = RiftSelectParams()
    p.mode, p.reserved, p.temperature = SELECT_MODES[mode], 0, float(temperature)
    return p


COLLISION_MODES = {"envelope": _abi_footprint.RIFTFP_ENVELOPE, "footprint": _abi_footprint.RIFTFP_FOOTPRINT}


def collision_params(mode: str = "envelope") -> RiftCollisionParams:
    """RiftCollisionParams of Engine.collision_matrix(mode=...) / Engine.group_advantage_tick(collision=...) (include/rift_footprint.h states
    the rule): the mode by name; the default is the envelope test of rift_collision_matrix.  An unknown name raises ValueError."""
    if mode not in COLLISION_MODES:
        raise ValueError(f"collision: mode = {mode!r}; known: {list(COLLISION_MODES)}")
    p = RiftCollisionParams()
    p.mode, p.reserved = COLLISION_MODES[mode], 0
    return p


OFFROAD_EXTENTS = {"center": _abi_offroad.RIFTOF_CENTER, "footprint": _abi_offroad.RIFTOF_FOOTPRINT}


def offroad_params(extent: str = "center") -> RiftOffRoadParams:
    """RiftOffRoadParams of Engine.off_road_matrix(extent=...) / Engine.off_road_matrix_map(extent=...) / Engine.group_advantage_tick(
    off_road_extent=...) (include/rift_offroad.h states the rule): the extent by name; the default is the footprint centre alone, the flag of
    rift_off_road_matrix.  An unknown name raises ValueError."""
    if extent not in OFFROAD_EXTENTS:
        raise ValueError(f"off_road: extent = {extent!r}; known: {list(OFFROAD_EXTENTS)}")
    p = RiftOffRoadParams()
    p.extent, p.reserved = OFFROAD_EXTENTS[extent], 0
    return p


PI_KEYS = ("mlp.0.weight","mlp.0.bias", "mlp.1.weight", "mlp.1.bias", "mlp.3.weight", "mlp.3.bias")       # flat order of PI_NPARAM
PI_SIZES = (128 * 128, 128, 128, 128, 128, 1)
CRITIC_SIZES = (256 * 128, 256, 256 * 256, 256, 256, 1, 128, 128, 1, 1)                                       # flat order of CRITIC_NPARAM
CRITIC_KEYS = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias",
               "state_avg", "state_std", "value_avg", "value_std")
assert sum(PI_SIZES) == PI_NPARAM and sum(CRITIC_SIZES) == CRITIC_NPARAM, "the flat layouts and the counts of include/rift_hip.h differ"

_libs = {}


def load_library(variant: str = "") -> C.CDLL:
    """Load librift_hip.so (variant "stats": librift_hip_stats.so, the diagnostic twin with the drop-decision counters of
    csrc/dropstats.h); raise loudly when it is absent (no fallback path exists)."""
    if variant in _libs:
        return _libs[variant]
    path = LIB_PATH if not variant else LIB_PATH.replace("librift_hip.so", f"librift_hip_{variant}.so")
    if not variant and os.environ.get("RIFT_LIB"):       # diagnostic: an A/B build of the library (rift_amd.build.build_variant)
        path = os.environ["RIFT_LIB"]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). rift_amd has no CPU fallback.")
    _libs[variant] = lib = _abi_offroad.bind(_abi_footprint.bind(_abi_select.bind(_abi_advantage.bind(_abi_drivable.bind(_abi.bind(C.CDLL(path)))))))
    return lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class _KnownStreams(threading.local):        # per host thread: a policy driven from one thread must not hand its stream to another thread's calls
    def __init__(self):
        self.stack = []


_KNOWN_STREAM = _KnownStreams()


def _stream():
    """The stream handle the C-ABI calls are given: torch's current stream -- or the one a caller has declared current (known_stream)."""
    st = _KNOWN_STREAM.stack
    if st:
        return st[-1]
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_DEBUG_STREAMS = os.environ.get("RIFT_DEBUG_STREAMS") == "1"      # (read once: known_stream is entered two or three times per update step)


class known_stream:
    """`with known_stream(s):` -- the caller states that `s` IS torch's current stream for the duration (it entered `torch.cuda.stream(s)` or
    read `torch.cuda.current_stream()` itself), which saves the ~7 us lookup in every C-ABI call of the block: eight per update step, a
    quarter of the step's host time, and the host time is what bounds a small-batch step."""

    def __init__(self, s: torch.cuda.Stream):
        self.h = C.c_void_p(s.cuda_stream)

    def __enter__(self):
        if _DEBUG_STREAMS:                                    # the declaration must be true
            assert self.h.value == torch.cuda.current_stream().cuda_stream, "known_stream(s): s is not torch's current stream"
        _KNOWN_STREAM.stack.append(self.h)
        return self

    def __exit__(self, *exc):
        _KNOWN_STREAM.stack.pop()
        return False


def _dev(t: torch.Tensor, dtype, device) -> torch.Tensor:
    if t.dtype != dtype or t.device != device or not t.is_contiguous():
        t = t.to(device=device, dtype=dtype).contiguous()
    return t


def feature_batch(data: Dict, device) -> (RiftFeatureBatch, list):
    """Build the POD descriptor of a collated feature dict.
    Returns (struct, keepalive list of the tensors whose pointers it holds)."""
    f32, i8, u8 = torch.float32, torch.int8, torch.bool
    ag, mp, rl = data["agent"], data["map"], data["reference_line"]
    so = data.get("static_objects")
    keep = []

    def put(t, dt):
        t = _dev(t, dt, device)
        keep.append(t)
        return t

    fb = RiftFeatureBatch()
    pos = put(ag["position"], f32)
    bs, A, T = pos.shape[:3]
    Mp = mp["point_position"].shape[1]
    R = rl["position"].shape[1]
    S = so["position"].shape[1] if so is not None else 0
    fb.bs, fb.A, fb.Mp, fb.R, fb.S, fb.T = bs, A, Mp, R, S, T
    t = {
        "agent_position": pos, "agent_heading": put(ag["heading"], f32), "agent_velocity": put(ag["velocity"], f32),
        "agent_shape": put(ag["shape"], f32), "agent_category": put(ag["category"], i8),
        "agent_valid_mask": put(ag["valid_mask"], u8),
        "map_point_position": put(mp["point_position"], f32), "map_point_vector": put(mp["point_vector"], f32),
        "map_point_orientation": put(mp["point_orientation"], f32), "map_polygon_center": put(mp["polygon_center"], f32),
        "map_polygon_type": put(mp["polygon_type"], i8), "map_polygon_on_route": put(mp["polygon_on_route"], u8),
        "map_polygon_tl_status": put(mp["polygon_tl_status"], i8),
        "map_polygon_has_speed_limit": put(mp["polygon_has_speed_limit"], u8),
        "map_polygon_speed_limit": put(mp["polygon_speed_limit"], f32), "map_valid_mask": put(mp["valid_mask"], u8),
        "ref_position": put(rl["position"], f32), "ref_vector": put(rl["vector"], f32),
        "ref_orientation": put(rl["orientation"], f32), "ref_valid_mask": put(rl["valid_mask"], u8),
        "current_state": put(data["current_state"], f32),
    }
    if S > 0:
        t.update({"static_position": put(so["position"], f32), "static_heading": put(so["heading"], f32),
                  "static_shape": put(so["shape"], f32), "static_category": put(so["category"], i8),
                  "static_valid_mask": put(so["valid_mask"], u8)})
    for name in _FB_PTRS:
        setattr(fb, name, t[name].data_ptr() if name in t else None)
    fb.cs_ld = t["current_state"].shape[1]
    return fb, keep


class Engine:
    """One RiftCtx bound to one device + the torch tensors it borrows."""

    def __init__(self, device=None, operands: str = "bf16", variant: str = ""):
        """operands: "bf16" | "fp16" -- the MFMA operand format of the fused kernels (forward(fp32=True) ignores it).
        variant: "" | "stats" (the diagnostic library; bf16 operands only)."""
        if operands not in OPERANDS:
            raise ValueError(f"operands must be one of {sorted(OPERANDS)}, got {operands!r}")
        if not torch.cuda.is_available():
            raise RuntimeError("rift_amd.Engine needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.lib = load_library(variant)
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.ctx = vp()
        self.operands = operands
        rc = self.lib.rift_ctx_create_ex(self.device.index or 0, OPERANDS[operands], C.byref(self.ctx))
        if rc != 0:
            raise RuntimeError(f"rift_ctx_create_ex failed ({rc})")
        self._params = None
        self._names = None
        self._keep = []
        self._stage_host = self._stage_dev = None
        self._stage_off = 0
        self._ctl_state = None         # control_tick: (n_slots, CONTROL_STATE) f64, grow-only
        self.generation = 0            # counts the calls that overwrite the policy head's activations (forward, forward_raw, forward_head):
                                       # head_backward refers to the latest one, a caller that kept a graph compares (rift_amd/autograd.py)

    # ---- small host inputs (the rollout tick's per-CBV readings) ---------------------------------
    _STAGE_BYTES = 8 << 20
    _NP_OF = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8,
              torch.int8: np.int8, torch.bool: np.bool_}

    def stage_tree(self, data):
        """A nested dict of CPU tensors (a collated feature batch) -> the same dict on the device.  Round 6: the leaves are laid side by side
        in the pinned arena and go up in ONE asynchronous copy (a tick's batch is ~34 small tensors: 34 copies of ~8 us of host time each
        were a quarter of the tick, tools/tick_latency.py --profile); leaves the arena cannot take (other dtypes, > 2 MiB, empty, already on
        the device) go through stage() / .to() one by one."""
        leaves = []

        def walk(d):
            if isinstance(d, dict):
                return {k: walk(v) for k, v in d.items()}
            if torch.is_tensor(d):
                leaves.append(d)
                return len(leaves) - 1
            raise NotImplementedError(type(d))

        shape = walk(data)
        out = self.stage_many(leaves)

        def build(d):
            return {k: build(v) for k, v in d.items()} if isinstance(d, dict) else out[d]
        return build(shape)

    def stage_many(self, tensors):
        """[CPU tensor] -> [device tensor], the arena-sized ones through one span of the pinned arena and one asynchronous copy (see stage())."""
        plan, total = [], 0
        for t in tensors:
            if t.is_cuda or t.dtype not in self._NP_OF or t.numel() == 0 or t.numel() * t.element_size() > self._STAGE_BYTES // 4:
                plan.append(None)
                continue
            a = np.ascontiguousarray(t.detach().numpy())
            plan.append((a, total))
            total = (total + a.nbytes + 255) & ~255
        if total > self._STAGE_BYTES // 2:               # (an unusually large batch: leaf by leaf, each with its own wrap check)
            return [self.stage(t, t.dtype) if p is not None else (t if t.is_cuda else t.to(self.device)) for t, p in zip(tensors, plan)]
        off = self._arena_span(total)
        host = self._stage_host.numpy()
        for p in plan:
            if p is not None:
                a, o = p
                host[off + o:off + o + a.nbytes] = a.reshape(-1).view(np.uint8)
        if total:
            self._stage_dev[off:off + total].copy_(self._stage_host[off:off + total], non_blocking=True)
        out = []
        for t, p in zip(tensors, plan):
            if p is None:
                out.append(t if t.is_cuda and t.device == self.device else t.to(self.device))
            else:
                a, o = p
                out.append(self._stage_dev[off + o:off + o + a.nbytes].view(t.dtype).view(a.shape))
        return out

    def _arena_span(self, nbytes: int) -> int:
        """The offset of the next `nbytes` of the pinned arena and its device twin (allocated at the first call): 256-byte aligned, behind
        the span before it; a span that would run past the end starts at 0 again, behind a synchronisation."""
        if self._stage_host is None:
            self._stage_host = torch.empty(self._STAGE_BYTES, dtype=torch.uint8).pin_memory()
            self._stage_dev = torch.empty(self._STAGE_BYTES, dtype=torch.uint8, device=self.device)
        off = (self._stage_off + 255) & ~255
        if off + nbytes > self._STAGE_BYTES:
            torch.cuda.synchronize(self.device)      # every consumer of the slots about to be rewritten is done -- on ANY stream (a staged batch may
                                                     # have been handed to a hook that reads it elsewhere); once per 8 MiB of uploads
            off = 0
        self._stage_off = off + nbytes
        return off

    def stage(self, a, dtype: torch.dtype) -> torch.Tensor:
        """Host array / CPU tensor -> device tensor of `dtype` through a pinned arena and an ASYNCHRONOUS copy on the current stream.
        `tensor.to(device)` from pageable memory waits for everything the stream holds; a tick's evaluation chain makes ~15 such uploads
        per CBV, each between kernel launches, and that wait -- not the copies -- was a third of the tick (tools/tick_latency.py).  The
        arena advances by the call and wraps behind a stream synchronisation, so a staged tensor is valid until 8 MiB of later uploads:
        it is for the inputs of the call at hand, not for keeping (a policy's `data` dict is invalid after its tick), and the arena is one per
        engine: not for concurrent callers.  Large (> 2 MiB) and empty inputs take the ordinary path."""
        if torch.is_tensor(a):
            if a.is_cuda:
                return _dev(a, dtype, self.device)
            a = a.detach().numpy()
        a = np.ascontiguousarray(a, dtype=self._NP_OF[dtype])
        n = a.nbytes
        if n == 0 or n > self._STAGE_BYTES // 4:
            return torch.from_numpy(a).to(self.device)
        off = self._arena_span(n)
        self._stage_host.numpy()[off:off + n] = a.reshape(-1).view(np.uint8)
        d = self._stage_dev[off:off + n]
        d.copy_(self._stage_host[off:off + n], non_blocking=True)
        return d.view(dtype).view(a.shape)

    def close(self):
        if self.ctx:
            self.lib.rift_ctx_destroy(self.ctx)
            self.ctx = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0 and getattr(self, "_dp_error", None) is not None:
            e, self._dp_error = self._dp_error, None
            raise RuntimeError(f"{what}: the data-parallel exchange raised") from e
        if rc != 0:
            msg = self.lib.rift_last_error(self.ctx)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    # ---- parameters -------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Bind views onto `sd`'s tensors (moved to the device if necessary; the engine keeps
        references, pi_head.* and BatchNorm running statistics are read / written in place)."""
        params = {}
        for k, v in sd.items():
            dt = torch.int64 if v.dtype == torch.int64 else torch.float32
            params[k] = _dev(v, dt, self.device)
        descs = (RiftTensorDesc * len(params))()
        names = []
        for i, (k, v) in enumerate(params.items()):
            nb = k.encode()
            names.append(nb)
            descs[i].name = nb
            descs[i].data = v.data_ptr()
            descs[i].numel = v.numel()
            descs[i].ndim = min(v.dim(), 4)
            shp = list(v.shape)[-4:] if v.dim() > 4 else list(v.shape)
            # collapse leading singleton dims of (1,1,12,128)-style parameters to at most 4 dims
            for d in range(4):
                descs[i].shape[d] = shp[d] if d < len(shp) else 1
        self._params, self._names = params, names
        self._check(self.lib.rift_model_load(self.ctx, descs, len(params), _stream()), "rift_model_load")
        return params

    # ---- forward ----------------------------------------------------------------------------
    def forward(self, data: Dict, train=False, need_traj=False, fp32=False, no_drop=False, bn_update=True,
                seed: int = 0) -> Dict[str, torch.Tensor]:
        fb, keep = feature_batch(data, self.device)
        bs, A, R = fb.bs, fb.A, fb.R
        o = RiftOutputs()
        out = {"probability": torch.empty(bs, R, 12, device=self.device),
               "hidden": torch.empty(bs, 128, device=self.device)}
        if need_traj:
            out["trajectory"] = torch.empty(bs, R, 12, 80, 6, device=self.device)
            out["prediction"] = torch.empty(bs, max(A - 1, 0), 80, 6, device=self.device)
            out["ref_free_trajectory"] = torch.empty(bs, 80, 4, device=self.device)
        for k, v in out.items():
            setattr(o, k, v.data_ptr())
        flags = (F_TRAIN if train else 0) | (F_NEED_TRAJ if need_traj else 0) | (F_FP32 if fp32 else 0) | \
                (F_NO_DROP if no_drop else 0) | (0 if bn_update else F_NO_BN_UPDATE)
        self._check(self.lib.rift_forward(self.ctx, C.byref(fb), C.byref(o), flags, C.c_uint32(seed & 0xFFFFFFFF),
                                          _stream()), "rift_forward")
        self.generation += 1
        self._keep = keep + list(out.values())
        self._bs = bs
        return out

    def forward_raw(self, fb: RiftFeatureBatch, out: RiftOutputs, flags: int, seed: int):
        """Hot-loop entry: prebuilt descriptors, no tensor conversion, no allocation."""
        rc = self.lib.rift_forward(self.ctx, C.byref(fb), C.byref(out), flags, C.c_uint32(seed & 0xFFFFFFFF), _stream())
        self.generation += 1
        if rc != 0:
            self._check(rc, "rift_forward")
        self._bs = fb.bs

    def set_side_stream(self, stream: Optional["torch.cuda.Stream"]):
        """rift_set_side_stream: the forward's second chain runs on `stream` instead of a stream of the library's own (a host that places its
        streams on the hardware queues itself: RLFTTrainer); None returns to the library's."""
        self._side_stream = stream                     # keeps the torch stream object alive while the engine holds its handle
        rc = self.lib.rift_set_side_stream(self.ctx, C.c_void_p(stream.cuda_stream if stream is not None else 0))
        if rc != 0:
            self._check(rc, "rift_set_side_stream")

    def set_prepare_stream(self, stream: Optional["torch.cuda.Stream"]):
        """rift_set_prepare_stream: the input-only preparation of the following forwards runs on `stream` (behind the gather of the batch
        the caller queued there) instead of between two steps on the forward's stream; None switches it off."""
        self._prep_stream = stream                     # keeps the torch stream object alive while the engine holds its handle
        rc = self.lib.rift_set_prepare_stream(self.ctx, C.c_void_p(stream.cuda_stream if stream is not None else 0))
        if rc != 0:
            self._check(rc, "rift_set_prepare_stream")

    def forward_head(self, back: int = 0):
        """The policy head of the last F_DEFER_HEAD forward -- or of the one `back` forwards before it -- on the current stream (the caller
        has ordered it behind that forward)."""
        rc = self.lib.rift_forward_head_back(self.ctx, back, _stream())
        self.generation += 1
        if rc != 0:
            self._check(rc, "rift_forward_head")

    def loss_backward_raw(self, kind: int, li: RiftLossIn, lo: RiftLossOut, params: Optional[RiftObjectiveParams] = None,
                          terms: Optional[int] = None):
        """rift_loss_backward; with `params` rift_loss_backward_ex (`terms`: the address of a device [8] f64 buffer, or None)."""
        if params is None:
            rc = self.lib.rift_loss_backward(self.ctx, kind, C.byref(li), C.byref(lo), _stream())
            if rc != 0:
                self._check(rc, "rift_loss_backward")
            return
        rc = self.lib.rift_loss_backward_ex(self.ctx, kind, C.byref(li), C.byref(params), C.byref(lo), terms, _stream())
        if rc != 0:
            self._check(rc, "rift_loss_backward_ex")

    def loss_finalize_raw(self, lo: RiftLossOut, accumulate: int = 0):
        rc = self.lib.rift_loss_finalize(self.ctx, C.byref(lo), accumulate, _stream())
        if rc != 0:
            self._check(rc, "rift_loss_finalize")

    def check_finite(self):
        """Sync point of the reference's `assert torch.isfinite(q).all()` (planning_decoder.py:175): waits for the current stream and
        raises if any forward since the last check produced non-finite decoder queries."""
        self._check(self.lib.rift_check_finite(self.ctx, _stream()), "rift_forward (decoder finiteness check)")

    def set_dp(self, scene_offset: int, global_bs: int, xchg: torch.Tensor, exchange):
        """rift_set_dp: this rank's forwards process scenes [scene_offset, scene_offset + bs) of a `global_bs`-scene minibatch.
        `xchg`: caller-owned device f64 buffer; `exchange(t)`: in-place SUM all-reduce of a slice of it over the ranks, enqueued on the
        current stream.  The BatchNorm statistics and the r2r quirk masks of rift_forward then cover the global minibatch."""
        assert xchg.dtype == torch.float64 and xchg.is_cuda and xchg.is_contiguous()
        if getattr(self, "_dp_key", None) != (xchg.data_ptr(), id(exchange)):
            def _cb(user, offset, count, stream):
                try:
                    # the header's contract: the all-reduce is enqueued on the stream the engine names (it is torch's current stream
                    # unless the caller handed rift_forward another one)
                    if (stream or 0) != torch.cuda.current_stream(xchg.device).cuda_stream:
                        with torch.cuda.stream(torch.cuda.ExternalStream(stream or 0, device=xchg.device)):
                            exchange(xchg[offset:offset + count])
                    else:
                        exchange(xchg[offset:offset + count])
                    return 0
                except BaseException as e:          # an exception must not unwind through the C frames
                    self._dp_error = e
                    return -1
            self._dp_cb = EXCHANGE_FN(_cb)
            self._dp_key = (xchg.data_ptr(), id(exchange))
            self._dp_keep = (xchg, exchange)
        d = RiftDp()
        d.scene_offset, d.global_bs, d.xchg, d.xchg_len, d.exchange, d.user = scene_offset, global_bs, xchg.data_ptr(), xchg.numel(), self._dp_cb, None
        self._check(self.lib.rift_set_dp(self.ctx, C.byref(d)), "rift_set_dp")

    # ---- the library-owned communicator (rift_comm_*: RCCL through dlopen; hosts without torch.distributed) ---------------------------------
    def comm_unique_id(self) -> bytes:
        """128 bytes (an ncclUniqueId) from ONE rank; hand them to every rank out of band."""
        buf = C.create_string_buffer(128)
        self._check(self.lib.rift_comm_unique_id(self.ctx, C.cast(buf, vp)), "rift_comm_unique_id")
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == 128
        buf = C.create_string_buffer(unique_id, 128)
        self._check(self.lib.rift_comm_init(self.ctx, C.cast(buf, vp), rank, world), "rift_comm_init")

    def comm_all_reduce(self, t: torch.Tensor):
        """In-place SUM all-reduce of a device f64 tensor over the library's communicator, on the current stream."""
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous()
        self._check(self.lib.rift_comm_all_reduce(self.ctx, _ptr(t), t.numel(), _stream()), "rift_comm_all_reduce")

    def comm_destroy(self):
        self._check(self.lib.rift_comm_destroy(self.ctx), "rift_comm_destroy")

    def set_dp_library_comm(self, scene_offset: int, global_bs: int, xchg: torch.Tensor):
        """rift_set_dp with exchange = NULL: the forward's exchanges go over the communicator of comm_init()."""
        assert xchg.dtype == torch.float64 and xchg.is_cuda and xchg.is_contiguous()
        d = RiftDp()
        d.scene_offset, d.global_bs, d.xchg, d.xchg_len, d.exchange, d.user = scene_offset, global_bs, xchg.data_ptr(), xchg.numel(), EXCHANGE_FN(0), None
        self._dp_keep = (xchg, None)
        self._dp_key = None
        self._check(self.lib.rift_set_dp(self.ctx, C.byref(d)), "rift_set_dp")

    def clear_dp(self):
        self._check(self.lib.rift_set_dp(self.ctx, None), "rift_set_dp")
        self._dp_key = self._dp_cb = self._dp_keep = None

    def set_param_event(self, event: Optional["torch.cuda.Event"]):
        """rift_set_param_event: forwards wait for `event` (recorded after the optimizer step) right before they read pi_head."""
        self._param_event = event                                   # keep the handle alive
        self._check(self.lib.rift_set_param_event(self.ctx, C.c_void_p(event.cuda_event) if event is not None else None),
                    "rift_set_param_event")

    def loss_finalize_clip_raw(self, lo: RiftLossOut, accumulate: int, max_norm: float, total_norm: Optional[torch.Tensor]):
        """rift_loss_finalize + clip_grad_norm_ over the six pi_head gradients, one launch."""
        rc = self.lib.rift_loss_finalize_clip(self.ctx, C.byref(lo), accumulate, float(max_norm),
                                              _ptr(total_norm) if total_norm is not None else None, _stream())
        if rc != 0:
            self._check(rc, "rift_loss_finalize_clip")

    def make_adam_list(self, params, grads, exp_avg, exp_avg_sq, steps):
        """Host-side argument arrays of rift_adamw_step for a fixed list of tensors (built once, reused every step)."""
        n = len(params)
        arr = lambda ts: (vp * n)(*[t.data_ptr() for t in ts])
        return {"n": n, "p": arr(params), "g": arr(grads), "m": arr(exp_avg), "v": arr(exp_avg_sq), "s": arr(steps),
                "numel": (C.c_int64 * n)(*[t.numel() for t in params]), "keep": (params, grads, exp_avg, exp_avg_sq, steps)}

    def adamw_step_raw(self, al, lrs, wds, step_new: float, beta1: float, beta2: float, eps: float):
        n = al["n"]
        rc = self.lib.rift_adamw_step(self.ctx, n, al["p"], al["g"], al["m"], al["v"], al["s"], al["numel"],
                                      (C.c_double * n)(*lrs), (C.c_double * n)(*wds), float(step_new), float(beta1), float(beta2),
                                      float(eps), _stream())
        if rc != 0:
            self._check(rc, "rift_adamw_step")

    def update_tail_raw(self, lo: RiftLossOut, accumulate: int, max_norm: float, total_norm, al, lrs, wds, step_new: float, beta1: float,
                        beta2: float, eps: float):
        """rift_update_tail: finalize + gradient-norm clip + AdamW of the six pi_head tensors, one launch (al: make_adam_list of exactly those)."""
        n = al["n"]
        rc = self.lib.rift_update_tail(self.ctx, C.byref(lo), accumulate, float(max_norm), _ptr(total_norm) if total_norm is not None else None, n,
                                       al["p"], al["g"], al["m"], al["v"], al["s"], (C.c_double * n)(*lrs), (C.c_double * n)(*wds), float(step_new),
                                       float(beta1), float(beta2), float(eps), _stream())
        if rc != 0:
            self._check(rc, "rift_update_tail")

    def prof_enable(self, on: bool):
        self._check(self.lib.rift_prof_enable(self.ctx, 1 if on else 0), "rift_prof_enable")

    def prof_report(self) -> dict:
        import json
        buf = C.create_string_buffer(1 << 18)
        self._check(self.lib.rift_prof_report(self.ctx, buf, len(buf)), "rift_prof_report")
        return json.loads(buf.value.decode())

    def tap(self, name: str) -> torch.Tensor:
        n = C.c_int64(0)
        self._check(self.lib.rift_tap(self.ctx, name.encode(), None, C.byref(n), _stream()), "rift_tap")
        t = torch.empty(n.value, device=self.device)
        self._check(self.lib.rift_tap(self.ctx, name.encode(), _ptr(t), C.byref(n), _stream()), "rift_tap")
        return t

    # ---- loss + backward ---------------------------------------------------------------------
    def loss_backward(self, kind: str, batch: Dict[str, torch.Tensor], clip_epsilon=0.2, lambda_entropy=0.01, objective=None,
                      terms: bool = False):
        """Phase 1: per-rank sums.  Returns (stats[2] f64, flat_grad_sum[PI_NPARAM] f32, argmax_rm or None).
        objective (kinds 'rift' / 'grpo'): a dict of settings (objective_params' keys; {} = the kind's defaults) or a ready
        RiftObjectiveParams -- the call is rift_loss_backward_ex; None: rift_loss_backward.  terms=True (with `objective`): the device
        [8] f64 term sums of that call join the result as a fourth element."""
        if terms and objective is None:
            raise ValueError("loss_backward: terms=True needs objective= (rift_loss_backward has no term sums)")
        if objective is not None and not isinstance(objective, RiftObjectiveParams):
            objective = objective_params(kind, **objective)
        dev = self.device
        li = RiftLossIn()
        keep = []

        def put(key, dt):
            if key not in batch or batch[key] is None:
                return None
            t = _dev(batch[key], dt, dev)
            keep.append(t)
            return t.data_ptr()

        li.old_group_logits = put("old_group_logits_torch", torch.float32)
        li.ref_group_logits = put("ref_group_logits_torch", torch.float32)
        li.group_advantage = put("group_advantage_torch", torch.float64)
        li.group_valid_mask = put("group_advantage_mask_torch", torch.bool)
        li.action_mode = put("action_mode_torch", torch.int64)
        li.advantage = put("advantage_torch", torch.float32)
        li.old_log_prob = put("old_log_prob_torch", torch.float32)
        li.returns = put("return_torch", torch.float32)
        li.clip_epsilon, li.lambda_entropy = clip_epsilon, lambda_entropy
        lo = RiftLossOut()
        stats = torch.zeros(2, dtype=torch.float64, device=dev)
        flat = torch.zeros(PI_NPARAM, dtype=torch.float32, device=dev)
        lo.stats, lo.flat_grad_sum = stats.data_ptr(), flat.data_ptr()
        argmax = None
        if kind in ("reinforce", "sft"):          # chosen (r, m): REINFORCE's argmax / SFT's target label
            argmax = torch.zeros(self._bs, 2, dtype=torch.int64, device=dev)
            lo.argmax_rm = argmax.data_ptr()
        if objective is not None:
            tsum = torch.zeros(8, dtype=torch.float64, device=dev) if terms else None
            self._check(self.lib.rift_loss_backward_ex(self.ctx, LOSS_KINDS[kind], C.byref(li), C.byref(objective), C.byref(lo), _ptr(tsum), _stream()),
                        "rift_loss_backward_ex")
            self._keep_loss = keep
            return (stats, flat, argmax, tsum) if terms else (stats, flat, argmax)
        self._check(self.lib.rift_loss_backward(self.ctx, LOSS_KINDS[kind], C.byref(li), C.byref(lo), _stream()),
                    "rift_loss_backward")
        self._keep_loss = keep
        return stats, flat, argmax

    def loss_finalize(self, stats, flat, grads: Dict[str, torch.Tensor], accumulate=False) -> torch.Tensor:
        """Phase 2: loss = -S/count and grads = -flat/count into the six pi_head .grad tensors
        (`grads` keyed by 'mlp.0.weight', 'mlp.0.bias', 'mlp.1.weight', 'mlp.1.bias', 'mlp.3.weight', 'mlp.3.bias')."""
        lo = RiftLossOut()
        loss = torch.zeros(1, dtype=torch.float64, device=self.device)
        lo.loss, lo.stats, lo.flat_grad_sum = loss.data_ptr(), stats.data_ptr(), flat.data_ptr()
        lo.grad_w1, lo.grad_b1 = _ptr(grads.get("mlp.0.weight")), _ptr(grads.get("mlp.0.bias"))
        lo.grad_ln_w, lo.grad_ln_b = _ptr(grads.get("mlp.1.weight")), _ptr(grads.get("mlp.1.bias"))
        lo.grad_w2, lo.grad_b2 = _ptr(grads.get("mlp.3.weight")), _ptr(grads.get("mlp.3.bias"))
        self._check(self.lib.rift_loss_finalize(self.ctx, C.byref(lo), 1 if accumulate else 0, _stream()),
                    "rift_loss_finalize")
        return loss

    def head_backward(self, dlogits: torch.Tensor, grads: Optional[Dict[str, torch.Tensor]] = None, accumulate: bool = False) -> torch.Tensor:
        """rift_head_backward: the gradient sums of the six pi_head tensors for an upstream gradient `dlogits` = d loss / d probability
        (bs, R, 12) over the activations of the latest forward.  Returns flat[PI_NPARAM] = sum_rows dz * d logit / d theta (PI_KEYS order, no
        sign, no count; rows of padded reference lines contribute nothing); `grads` (keyed like loss_finalize's) are overwritten with it or,
        with `accumulate`, added to.  A data-parallel host all-reduces `flat` itself."""
        if dlogits.dim() != 3 or dlogits.shape[2] != 12:
            raise ValueError(f"head_backward: dlogits must be (bs, R, 12), got {tuple(dlogits.shape)}")
        dz = _dev(dlogits, torch.float32, self.device)
        flat = torch.empty(PI_NPARAM, dtype=torch.float32, device=self.device)
        lo = RiftLossOut()
        lo.flat_grad_sum = flat.data_ptr()
        g = grads or {}
        lo.grad_w1, lo.grad_b1 = _ptr(g.get("mlp.0.weight")), _ptr(g.get("mlp.0.bias"))
        lo.grad_ln_w, lo.grad_ln_b = _ptr(g.get("mlp.1.weight")), _ptr(g.get("mlp.1.bias"))
        lo.grad_w2, lo.grad_b2 = _ptr(g.get("mlp.3.weight")), _ptr(g.get("mlp.3.bias"))
        self._check(self.lib.rift_head_backward(self.ctx, _ptr(dz), dz.shape[0], dz.shape[1], C.byref(lo), 1 if accumulate else 0, _stream()),
                    "rift_head_backward")
        return flat

    # ---- single ops ---------------------------------------------------------------------------
    def op_linear(self, x, w, b=None, ln_w=None, ln_b=None, act=0, fp32=False):
        x = _dev(x, torch.float32, self.device)
        w = _dev(w, torch.float32, self.device)
        b = None if b is None else _dev(b, torch.float32, self.device)
        ln_w = None if ln_w is None else _dev(ln_w, torch.float32, self.device)
        ln_b = None if ln_b is None else _dev(ln_b, torch.float32, self.device)
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, device=self.device)
        self._check(self.lib.rift_op_linear(self.ctx, _ptr(x), M, K, _ptr(w), _ptr(b), N, _ptr(ln_w), _ptr(ln_b), act,
                                            1 if fp32 else 0, _ptr(y), _stream()), "rift_op_linear")
        return y

    def op_linear_bench(self, x, w, b=None, ln_w=None, ln_b=None, act=0, residual=None, reps=50):
        """Average microseconds per launch of the forward's GEMM kernel on this shape (diagnostic)."""
        dev = self.device
        x, w = _dev(x, torch.float32, dev), _dev(w, torch.float32, dev)
        opt = [None if t is None else _dev(t, torch.float32, dev) for t in (b, ln_w, ln_b, residual)]
        M, K = x.shape
        N = w.shape[0]
        y = torch.empty(M, N, device=dev)
        ms = C.c_float(0)
        self._check(self.lib.rift_op_linear_bench(self.ctx, _ptr(x), M, K, _ptr(w), _ptr(opt[0]), N, _ptr(opt[1]), _ptr(opt[2]),
                                                  act, _ptr(opt[3]), _ptr(y), reps, C.byref(ms), _stream()), "rift_op_linear_bench")
        return ms.value * 1e3

    def ref_line_info(self, trajectories, ref_pos_list, ref_angle_list, Ts=40):
        """TrajEvaluator.get_ref_line_info on device.  trajectories (R, M, Tfull, C>=6 or 4)."""
        dev = self.device
        traj = _dev(trajectories, torch.float32, dev)
        R, M, Tfull, Cc = traj.shape
        assert Cc == 6
        Pmax = max(p.shape[0] for p in ref_pos_list)
        if all(not (torch.is_tensor(p) and p.is_cuda) for p in ref_pos_list):
            # host-side lines (the rollout tick: straight from the observation): padded on the host, ONE upload -- [positions | angles] + lengths
            hp, ha, _ = tick_pack.pad_ref_lines(ref_pos_list, ref_angle_list)
            up = self.stage(np.concatenate([hp.reshape(-1), ha.reshape(-1)]), torch.float32)
            rp, ra = up[:hp.size].view(R, Pmax, 2), up[hp.size:].view(R, Pmax)
        else:
            rp = torch.zeros(R, Pmax, 2, device=dev)
            ra = torch.zeros(R, Pmax, device=dev)
            for r in range(R):
                n = ref_pos_list[r].shape[0]
                rp[r, :n] = ref_pos_list[r].to(dev)
                ra[r, :n] = ref_angle_list[r].to(dev)
        rl = self.stage(np.array([p.shape[0] for p in ref_pos_list], dtype=np.int32), torch.int32)
        G = R * M
        dd = torch.empty(G, Ts, device=dev)
        da = torch.empty(G, Ts, device=dev)
        ci = torch.empty(G, Ts, dtype=torch.int32, device=dev)
        self._check(self.lib.rift_ref_line_info(self.ctx, _ptr(traj), G, Tfull, Ts, M, _ptr(rp), _ptr(ra), _ptr(rl), Pmax, _ptr(dd),
                                                _ptr(da), _ptr(ci), _stream()), "rift_ref_line_info")
        return dd, da, ci

    def new_pid_state(self, capacity: int):
        """Persistent state of the two BatchPIDTorch filters of TrackPropagate (zero-initialised, never reset)."""
        dev = self.device
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        return {"turn_buf": z(capacity, 20), "turn_ptr": z(capacity, dt=torch.int32), "turn_len": z(capacity, dt=torch.int32),
                "speed_buf": z(capacity, 20), "speed_ptr": z(capacity, dt=torch.int32), "speed_len": z(capacity, dt=torch.int32)}

    def rollout(self, trajectories, center_state, pid_state, g_per_group=None):
        """TrajEvaluator.get_center_rollout / TrackPropagate.propagate on device.
        trajectories (G, Tfull, 6); center_state (n_groups, 6) = x, y, heading, speed, width, length."""
        dev = self.device
        traj = _dev(trajectories, torch.float32, dev)
        G, Tfull, _ = traj.shape
        cs = self.stage(center_state, torch.float32).view(-1, 6)
        gper = g_per_group or G // cs.shape[0]
        io = RiftRolloutIO()
        io.trajectories, io.G, io.Tfull, io.G_per_group, io.center_state = traj.data_ptr(), G, Tfull, gper, cs.data_ptr()
        for k in ("turn_buf", "turn_ptr", "turn_len", "speed_buf", "speed_ptr", "speed_len"):
            assert pid_state[k].shape[0] >= G
            setattr(io, k, pid_state[k].data_ptr())
        out = {"center": torch.empty(G, 80, 2, device=dev), "vertices": torch.empty(G, 80, 4, 2, device=dev),
               "closest_index": torch.empty(G, 79, dtype=torch.int32, device=dev),
               "aim_idx": torch.empty(G, 79, dtype=torch.int32, device=dev)}
        for k in ("angle", "speed", "acc", "ang_vel", "ang_acc"):
            out[k] = torch.empty(G, 80, device=dev)
        for k, v in out.items():
            setattr(io, k, v.data_ptr())
        self._check(self.lib.rift_rollout(self.ctx, C.byref(io), _stream()), "rift_rollout")
        self._keep_ro = (traj, cs)
        return out

    def other_vehicle_rollout(self, steer, throttle, brake, speed, location, yaw_deg, extent, num_future_frames: int = 40,
                              near_lane_change: bool = True, bbox_inflation_ratio: float = 1.1):
        """get_other_vehicle_rollout on the device: per-actor arrays (see rift_hip.h) -> (N, T, 4, 2) float64 device tensor."""
        dev = self.device
        N, block = tick_pack.actor_block({"steer": steer, "throttle": throttle, "brake": brake, "speed": speed, "location": location,
                                          "yaw_deg": yaw_deg, "extent": extent})
        out = torch.empty(N, num_future_frames, 4, 2, dtype=torch.float64, device=dev)
        if N:
            # the five per-actor arrays in ONE upload: [controls (N,3) | speed (N) | location (N,3) | yaw (N) | extent (N,2)] as blocks of one buffer
            up = self.stage(block, torch.float64)
            act, sp, loc, yaw, ext = up[:3 * N], up[3 * N:4 * N], up[4 * N:7 * N], up[7 * N:8 * N], up[8 * N:]
            self._check(self.lib.rift_other_vehicle_rollout(self.ctx, _ptr(act), _ptr(sp), _ptr(loc), _ptr(yaw), _ptr(ext), N, num_future_frames,
                                                            1 if near_lane_change else 0, float(bbox_inflation_ratio), _ptr(out), _stream()),
                        "rift_other_vehicle_rollout")
        return out

    def eval_params(self, reward_model=None, gamma: float = 0.98, bbox_inflation_ratio: float = 1.1, resolution: float = 0.5,
                    near_lane_change: bool = True) -> RiftEvalParams:
        """The RiftEvalParams of rollout_return / group_advantage_tick (module-level eval_params)."""
        return eval_params(reward_model, gamma, bbox_inflation_ratio, resolution, near_lane_change)

    def group_advantage_tick(self, trajectory, cbvs, pid_state, gamma: float = 0.98, *, params: Optional[RiftEvalParams] = None,
                             want_returns: bool = False, want_terms: bool = False, collision=None, off_road_extent=None):
        """The group advantages of one tick's CBVs in one C-ABI call (rift_group_advantage_tick): `trajectory` (bs, Rb, 12, Tfull, 6) the tick's
        model output (device), `cbvs` a list of dicts in tick order -- the entries rift_amd/tick_pack.py describes, key by key
        -- whose valid reference lines are a prefix of their rows.  Everything host-side goes up in ONE staged copy.  Returns the (K, Rb, 12) f64
        device tensor; rows r >= R of a CBV are zero.
        `params` (eval_params; its gamma replaces the argument's) sends the call through rift_group_advantage_tick_ex: reward model, gamma,
        bbox_inflation_ratio, near_lane_change, resolution and a pixel offset from each CBV's own raster.  With want_returns / want_terms the
        result is a dict: "advantage" (K, Rb, 12), "returns" (K, Rb, 12), "terms" (K, Rb, 12, 8) -- the ones asked for, views of the ONE device
        tensor "packed" (K * Rb * 12 * 10 doubles, zero where nothing is written), so that a tick reads all of it back in one copy.  With
        params None and nothing wanted the call is rift_group_advantage_tick, as ever.
        A tick with an entry that takes its off-road flags from the loaded drivable-area map ("raster" + "pose", load_drivable_map) goes
        through riftdm_group_advantage_tick (params None: eval_params(gamma=gamma)).
        `collision` ('envelope' | 'footprint', or a ready RiftCollisionParams; include/rift_footprint.h states the rule) sends the tick through
        riftfp_group_advantage_tick, with or without the map: 'envelope' gives the bits of the call made without it, 'footprint' takes the
        collision flags from the footprints themselves.  None: the entry choice above.
        `off_road_extent` ('center' | 'footprint', or a ready RiftOffRoadParams; include/rift_offroad.h states the rule): 'footprint' sends the
        tick through riftof_group_advantage_tick (collision None: the envelope test), which takes the off-road flags from the centre and the
        four corners of every rollout step, against mask or map.  None or 'center': the entry choice above, the call made without it."""
        dev = self.device
        if collision is not None and not isinstance(collision, RiftCollisionParams):
            collision = collision_params(collision)
        if off_road_extent is not None and not isinstance(off_road_extent, RiftOffRoadParams):
            off_road_extent = offroad_params(off_road_extent)
        if off_road_extent is not None and off_road_extent.extent == _abi_offroad.RIFTOF_CENTER and off_road_extent.reserved == 0:
            off_road_extent = None                                                # (the centre alone: the entries of before)
        if off_road_extent is not None and collision is None:
            collision = collision_params("envelope")
        traj = _dev(trajectory, torch.float32, dev)
        bs, Rb, M, Tfull, Cc = traj.shape
        assert M == 12 and Cc == 6
        blob, layout = tick_pack.pack_tick(cbvs)                                  # 1. pack: host arithmetic only
        up = self.stage(blob, torch.uint8)                                        # 2. stage once
        arr = tick_pack.fill_tick_cbvs(layout, up.data_ptr())                     # 3. fill
        K, pid_keys = len(layout), ("turn_buf", "turn_ptr", "turn_len", "speed_buf", "speed_ptr", "speed_len")
        Gmax = 12 * max(c.R for c in layout)
        assert all(pid_state[k].shape[0] >= Gmax for k in pid_keys)
        use_map = any(c.from_map for c in layout)
        plain = params is None and not want_returns and not want_terms and not use_map and collision is None
        if plain:                                                                 # 4. the C entry: plain | _ex | riftdm_ | riftfp_
            res = {"advantage": torch.zeros(K, Rb, 12, dtype=torch.float64, device=dev)}
            name, tail = "rift_group_advantage_tick", (float(gamma), _ptr(res["advantage"]))
        else:
            n = K * Rb * 12
            packed = torch.zeros(n * 10, dtype=torch.float64, device=dev)
            res = {"packed": packed, "advantage": packed[:n].view(K, Rb, 12)}
            if want_returns:
                res["returns"] = packed[n:2 * n].view(K, Rb, 12)
            if want_terms:
                res["terms"] = packed[2 * n:].view(K, Rb, 12, 8)
            name = "riftdm_group_advantage_tick" if use_map else "rift_group_advantage_tick_ex"
            tail = (C.byref(eval_params(gamma=gamma) if params is None else params), _ptr(res["advantage"]), _ptr(res.get("returns")),
                    _ptr(res.get("terms")))
            if collision is not None:                                             # (the map entry's semantics per CBV, the collision params behind `params`)
                name, tail = "riftfp_group_advantage_tick", tail[:1] + (C.byref(collision),) + tail[1:]
            if off_road_extent is not None:                                       # (the off-road params behind the collision params)
                name, tail = "riftof_group_advantage_tick", tail[:2] + (C.byref(off_road_extent),) + tail[2:]
        self._check(getattr(self.lib, name)(self.ctx, _ptr(traj), Rb, Tfull, arr, K, *(_ptr(pid_state[k]) for k in pid_keys), *tail, _stream()),
                    name)
        self._keep_tick = (traj, up)
        return res if want_returns or want_terms else res["advantage"]

    def control_state(self, n_slots: int = 0) -> torch.Tensor:
        """The (n_slots, CONTROL_STATE) f64 controller state of control_tick, owned by the engine and grow-only (a zero row = a fresh PIDController);
        growing copies the rows in use into a NEW tensor, on the current stream: a tensor returned earlier is the state only until the next
        growth (ask again instead of keeping it)."""
        cur = self._ctl_state
        if cur is None or cur.shape[0] < n_slots:
            cap = max(16, n_slots, 2 * (cur.shape[0] if cur is not None else 0))
            new = torch.zeros(cap, CONTROL_STATE, dtype=torch.float64, device=self.device)
            if cur is not None:
                new[:cur.shape[0]].copy_(cur)
            self._ctl_state = new
        return self._ctl_state

    def adopt_control_state(self, other: "Engine"):
        """Take over the controller state of `other` (the engine a model was bound to before a precision / device change): the CBVs' rows
        and their content carry over."""
        if other._ctl_state is not None:
            self._ctl_state = other._ctl_state.to(self.device)
            other._ctl_state = None

    def control_reset(self, slots):
        """Zero the controller state of `slots` (a CBV that left; stream-ordered, so a control_tick issued behind it sees a fresh controller)."""
        if self._ctl_state is not None:
            for s in slots:
                if 0 <= int(s) < self._ctl_state.shape[0]:
                    self._ctl_state[int(s)].zero_()          # (a memset per slot: an index list would be a blocking upload)

    def control_tick(self, trajectory, probability, ref_free_trajectory, cbvs, topk: int = 10, sample_interval: int = 10, select=None, u=None):
        """The decisions of one tick's CBVs in one C-ABI call (rift_control_tick): `trajectory` (bs, Rb, 12, Tfull, 6), `probability`
        (bs, Rb, 12) and `ref_free_trajectory` ((bs, Tfull, 4) or None) are the raw outputs of the tick's forward; `cbvs` is a list of
        (batch_index, slot, x, y, heading, speed).  Returns the (K, 8) f64 device tensor of rift_hip.h: throttle, steer, brake, flat
        index (-1: ref-free), kept position, score, desired_speed, delta_angle.  Enqueued on the current stream; no synchronisation.
        `select` (a RiftSelectParams, or {'mode': 'greedy' | 'sample', 'temperature': float}) makes the call riftcs_control_tick
        (include/rift_select.h states the rule): in 'sample' mode `u` holds one number in [0, 1) per CBV, a host sequence, and elements 3 to 5
        describe the drawn candidate (its flat index, its kept position, the probability it was drawn with)."""
        dev = self.device
        traj = _dev(trajectory, torch.float32, dev)
        prob = _dev(probability, torch.float32, dev)
        rf = None if ref_free_trajectory is None else _dev(ref_free_trajectory, torch.float32, dev)
        bs, Rb, M, Tfull, Cc = traj.shape
        assert M == 12 and Cc == 6 and tuple(prob.shape) == (bs, Rb, 12) and (rf is None or tuple(rf.shape) == (bs, Tfull, 4))
        K = len(cbvs)
        arr = (RiftControlCBV * max(K, 1))()
        for t, (b, slot, x, y, heading, speed) in zip(arr, cbvs):
            if not 0 <= int(b) < bs:
                raise ValueError(f"control_tick: batch_index {b} outside the batch of {bs}")
            t.batch_index, t.slot, t.x, t.y, t.heading, t.speed = int(b), int(slot), float(x), float(y), float(heading), float(speed)
        state = self.control_state(max([int(v[1]) + 1 for v in cbvs if int(v[1]) >= 0], default=0))
        out = torch.empty(K, 8, dtype=torch.float64, device=dev)
        if select is None:
            if u is not None:
                raise ValueError("control_tick: `u` is read with select={'mode': 'sample', ...} only")
            self._check(self.lib.rift_control_tick(self.ctx, _ptr(traj), _ptr(prob), _ptr(rf), Rb, Tfull, arr, K, int(topk), int(sample_interval),
                                                   _ptr(state), state.shape[0], _ptr(out), _stream()), "rift_control_tick")
        else:
            if not isinstance(select, RiftSelectParams):
                unknown = sorted(set(select) - set(SELECT_KEYS))
                if unknown:
                    raise ValueError(f"select: unknown key(s) {unknown}; known: {list(SELECT_KEYS)}")
                select = select_params(**select)
            draws = None
            if u is not None:
                draws = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
                if draws.size != K:
                    raise ValueError(f"control_tick: {draws.size} numbers in `u` for {K} CBVs")
            self._check(self.lib.riftcs_control_tick(self.ctx, _ptr(traj), _ptr(prob), _ptr(rf), Rb, Tfull, arr, K, int(topk), int(sample_interval),
                                                     _ptr(state), state.shape[0], C.byref(select), None if draws is None else C.c_void_p(draws.ctypes.data),
                                                     _ptr(out), _stream()), "riftcs_control_tick")
        self._keep_ctl = (traj, prob, rf)
        return out

    def sft_teacher_mode(self, trajectory, teacher_infos, frame_rate: int = 10):
        """generate_target_label's teacher side: trajectory (bs,R,M,T,6), teacher_infos (bs,5) -> (bs,2) int64 (r, m) of the candidate
        whose PID target speed is closest to the teacher's; feed it as `action_mode_torch` to loss_backward("sft")."""
        dev = self.device
        tr = _dev(trajectory, torch.float32, dev)
        ti = _dev(teacher_infos, torch.float32, dev)
        bs, R, M, T, _ = tr.shape
        out = torch.empty(bs, 2, dtype=torch.int64, device=dev)
        self._check(self.lib.rift_sft_teacher_mode(self.ctx, _ptr(tr), _ptr(ti), bs, R, M, T, frame_rate, _ptr(out), _stream()),
                    "rift_sft_teacher_mode")
        return out

    def collision_matrix(self, center_vertices, other_vertices, Ts: int = 40, mode=None, want_first: bool = False):
        """get_collision_matrix: envelope overlap of candidate footprints (G,Tc,4,2) with forecast neighbours (N,Ts,4,2) -> (G,Ts) bool.
        `mode` ('envelope' | 'footprint', or a ready RiftCollisionParams) or want_first make the call riftfp_collision_matrix
        (include/rift_footprint.h states the rule); with want_first the result is (flags, first_actor (G,Ts) int32: the lowest colliding
        neighbour, or -1).  mode None and no want_first: rift_collision_matrix, as ever."""
        dev = self.device
        cv = _dev(center_vertices, torch.float32, dev)
        G, Tc = cv.shape[:2]
        ov = _dev(torch.as_tensor(other_vertices), torch.float64, dev)
        N = ov.shape[0]
        assert N == 0 or (ov.shape[1] >= Ts and tuple(ov.shape[2:]) == (4, 2))
        if N and ov.shape[1] != Ts:
            ov = ov[:, :Ts].contiguous()
        out = torch.empty(G, Ts, dtype=torch.uint8, device=dev)
        if mode is None and not want_first:
            self._check(self.lib.rift_collision_matrix(self.ctx, _ptr(cv), G, Tc, _ptr(ov) if N else None, N, Ts, _ptr(out), _stream()),
                        "rift_collision_matrix")
            return out.bool()
        p = mode if isinstance(mode, RiftCollisionParams) else collision_params("envelope" if mode is None else mode)
        first = torch.empty(G, Ts, dtype=torch.int32, device=dev) if want_first else None
        self._check(self.lib.riftfp_collision_matrix(self.ctx, _ptr(cv), G, Tc, _ptr(ov) if N else None, N, Ts, C.byref(p), _ptr(out), _ptr(first),
                                                     _stream()), "riftfp_collision_matrix")
        return (out.bool(), first) if want_first else out.bool()

    def _off_road_extent(self, rc, vertices, extent, which, mask, H, W, pose, params):
        """riftof_off_road_matrix for off_road_matrix / off_road_matrix_map: rc (G, T, 2) on the device, mask a device tensor or None (the map)
        -> (G, T) bool, or (flags, which (G, T) uint8: bit k = point k of the rule is off road)."""
        G, T = rc.shape[:2]
        p = extent if isinstance(extent, RiftOffRoadParams) else offroad_params(extent)
        vt = None if vertices is None else _dev(vertices, torch.float32, self.device)
        assert vt is None or tuple(vt.shape) == (G, T, 4, 2)
        out = torch.empty(G, T, dtype=torch.uint8, device=self.device)
        wh = torch.empty(G, T, dtype=torch.uint8, device=self.device) if which else None
        self._check(self.lib.riftof_off_road_matrix(self.ctx, _ptr(rc), _ptr(vt), G * T, _ptr(mask), int(H), int(W), float(pose[0]), float(pose[1]),
                                                    float(pose[2]), C.byref(params), C.byref(p), _ptr(out), _ptr(wh), _stream()), "riftof_off_road_matrix")
        return (out.bool(), wh) if which else out.bool()

    def off_road_matrix(self, rollout_center, off_road_mask, origin, heading: float, resolution_hw=(0.5, -0.5), offset=(200.0, 200.0), vertices=None,
                        extent="center", which: bool = False):
        """get_off_road_matrix lookup: rollout_center (G,T,2), off_road_mask (H,W) uint8 with 1 = not drivable -> (G,T) bool.
        `vertices` (G,T,4,2), `extent` ('center' | 'footprint', or a ready RiftOffRoadParams) and `which` make the call riftof_off_road_matrix
        (include/rift_offroad.h states the rule): 'footprint' flags a step whose centre or one of whose four corners is off road; with `which`
        the result is (flags, which (G,T) uint8: bit k = point k is off road).  That entry takes the resolution as (r, -r) and the offset as
        (H / 2, W / 2) only.  With the defaults: rift_off_road_matrix, as ever."""
        dev = self.device
        rc = _dev(rollout_center, torch.float32, dev)
        G, T = rc.shape[:2]
        m = self.stage(off_road_mask, torch.uint8)
        H, W = m.shape
        if vertices is not None or which or isinstance(extent, RiftOffRoadParams) or extent != "center":
            res = float(resolution_hw[0])
            if float(resolution_hw[1]) != -res or res <= 0 or (float(offset[0]), float(offset[1])) != (float(np.float32(H / 2)), float(np.float32(W / 2))):
                raise ValueError(f"off_road_matrix: with vertices, extent or which the resolution is (r, -r) and the offset (H / 2, W / 2) = "
                                 f"{(H / 2, W / 2)}; got {tuple(resolution_hw)}, {tuple(offset)}")
            return self._off_road_extent(rc, vertices, extent, which, m, H, W, (origin[0], origin[1], heading), eval_params(resolution=res))
        out = torch.empty(G, T, dtype=torch.uint8, device=dev)
        self._check(self.lib.rift_off_road_matrix(self.ctx, _ptr(rc), G * T, _ptr(m), H, W, float(origin[0]), float(origin[1]), float(heading),
                                                  float(resolution_hw[0]), float(resolution_hw[1]), float(offset[0]), float(offset[1]),
                                                  _ptr(out), _stream()), "rift_off_road_matrix")
        return out.bool()

    # ---- the drivable-area map: off-road flags without a raster (include/rift_drivable.h states the rule) ------------
    def load_drivable_map(self, polygons, cell: float = 16.0, margin: float = 1.0) -> dict:
        """The drivable polygons of a town -> the device, once: `polygons` is a list of (n, 2) float64 vertex arrays in the global frame (a ring
        may repeat its first vertex as its last, as shapely's exterior.coords does).  A second call replaces the map.  Returns drivable_map_info()."""
        polys = [np.ascontiguousarray(np.asarray(p, dtype=np.float64)).reshape(-1, 2) for p in polygons]
        start = np.zeros(len(polys) + 1, dtype=np.int32)
        if polys:
            start[1:] = np.cumsum([p.shape[0] for p in polys])
        verts = np.ascontiguousarray(np.concatenate(polys, 0)) if polys else np.zeros((0, 2), dtype=np.float64)
        self._check(self.lib.riftdm_load(self.ctx, verts.ctypes.data_as(vp), start.ctypes.data_as(vp), len(polys), float(cell), float(margin),
                                                    _stream()), "riftdm_load")
        return self.drivable_map_info()

    def clear_drivable_map(self):
        self._check(self.lib.riftdm_clear(self.ctx), "riftdm_clear")

    def drivable_map_info(self) -> Optional[dict]:
        """The loaded map's numbers (RiftDrivableInfo as a dict), or None when no map is loaded."""
        info = RiftDrivableInfo()
        rc = self.lib.riftdm_info(self.ctx, C.byref(info))
        if rc == _abi.RIFT_ERR_STATE:
            return None
        self._check(rc, "riftdm_info")
        return {k: getattr(info, k) for k, _ in RiftDrivableInfo._fields_ if k != "reserved"}

    def off_road_matrix_map(self, rollout_center, pose, raster_size=(400, 400), params: Optional[RiftEvalParams] = None, vertices=None,
                            extent="center", which: bool = False):
        """get_off_road_matrix from the loaded map: rollout_center (G, T, 2), pose (x, y, heading) of the footprint centre, raster_size (H, W) of
        the raster the rule speaks of, params (eval_params: its resolution is read) -> (G, T) bool.  `vertices`, `extent` and `which` as in
        off_road_matrix (riftof_off_road_matrix with a NULL mask); with the defaults: riftdm_off_road_matrix, as ever."""
        dev = self.device
        rc = _dev(rollout_center, torch.float32, dev)
        G, T = rc.shape[:2]
        params = eval_params() if params is None else params
        if vertices is not None or which or isinstance(extent, RiftOffRoadParams) or extent != "center":
            return self._off_road_extent(rc, vertices, extent, which, None, raster_size[0], raster_size[1], pose, params)
        out = torch.empty(G, T, dtype=torch.uint8, device=dev)
        self._check(self.lib.riftdm_off_road_matrix(self.ctx, _ptr(rc), G * T, int(raster_size[0]), int(raster_size[1]), float(pose[0]), float(pose[1]),
                                                      float(pose[2]), C.byref(params), _ptr(out), _stream()), "riftdm_off_road_matrix")
        return out.bool()

    def drivable_raster(self, pose, raster_size=(400, 400), params: Optional[RiftEvalParams] = None) -> torch.Tensor:
        """The (H, W) uint8 device mask the reference would hand to the lookup, drawn by the rule from the loaded map: 1 = off road."""
        H, W = int(raster_size[0]), int(raster_size[1])
        params = eval_params() if params is None else params
        out = torch.empty(max(H, 0), max(W, 0), dtype=torch.uint8, device=self.device)
        self._check(self.lib.riftdm_raster(self.ctx, H, W, float(pose[0]), float(pose[1]), float(pose[2]), C.byref(params), _ptr(out), _stream()),
                    "riftdm_raster")
        return out

    def make_clip_list(self, grads):
        """Pre-build the (pointer, numel) arrays of a fixed list of .grad tensors for clip_grad_norm_raw."""
        n = len(grads)
        ptrs = (vp * n)(*[g.data_ptr() for g in grads])
        nums = (C.c_int64 * n)(*[g.numel() for g in grads])
        return (ptrs, nums, n, list(grads))

    def clip_grad_norm_raw(self, clip_list, max_norm: float, total_norm: Optional[torch.Tensor] = None):
        ptrs, nums, n, _ = clip_list
        rc = self.lib.rift_clip_grad_norm(self.ctx, ptrs, nums, n, max_norm, _ptr(total_norm), _stream())
        if rc != 0:
            self._check(rc, "rift_clip_grad_norm")

    # ---- PPO critic ----------------------------------------------------------------------------
    @staticmethod
    def critic_desc(sd: Dict[str, torch.Tensor]) -> "RiftCritic":
        """Views onto a CriticPPO state_dict (net.{0,2,4}.{weight,bias}, state_avg/std, value_avg/std; device fp32)."""
        w = RiftCritic()
        keep = []
        for f, k in (("w0", "net.0.weight"), ("b0", "net.0.bias"), ("w1", "net.2.weight"), ("b1", "net.2.bias"), ("w2", "net.4.weight"),
                     ("b2", "net.4.bias"), ("state_avg", "state_avg"), ("state_std", "state_std"), ("value_avg", "value_avg"),
                     ("value_std", "value_std")):
            t = sd[k]
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise RuntimeError(f"critic parameter {k} must be a contiguous fp32 device tensor")
            setattr(w, f, t.data_ptr())
            keep.append(t)
        w._keep = keep
        return w

    def critic_forward(self, sd: Dict[str, torch.Tensor], state: torch.Tensor) -> torch.Tensor:
        st = _dev(state, torch.float32, self.device)
        out = torch.empty(st.shape[0], dtype=torch.float32, device=self.device)
        w = self.critic_desc(sd)
        self._check(self.lib.rift_critic_forward(self.ctx, C.byref(w), _ptr(st), st.shape[0], _ptr(out), _stream()), "rift_critic_forward")
        return out

    def critic_backward(self, sd: Dict[str, torch.Tensor], state: torch.Tensor, dvalue: torch.Tensor,
                        grads: Optional[Dict[str, torch.Tensor]] = None, accumulate: bool = False) -> torch.Tensor:
        """rift_critic_backward: flat[CRITIC_NPARAM] = sum_i dvalue[i] * d value_net(state)[i] / d theta over the ten critic tensors (CRITIC_KEYS
        order; no sign, no count) for an upstream gradient `dvalue` = d loss / d value (n).  `grads` (keyed by CRITIC_KEYS, any subset)
        receive their segments of it -- copied, or added with `accumulate`.  The forward is recomputed from `state`: no forward needs to
        have run."""
        st = _dev(state, torch.float32, self.device)
        dv = _dev(dvalue, torch.float32, self.device).reshape(-1)
        if st.dim() != 2 or st.shape[1] != 128 or dv.numel() != st.shape[0]:
            raise ValueError(f"critic_backward: state (n, 128) and dvalue (n), got {tuple(st.shape)} and {tuple(dvalue.shape)}")
        flat = torch.empty(CRITIC_NPARAM, dtype=torch.float32, device=self.device)
        w = self.critic_desc(sd)
        self._check(self.lib.rift_critic_backward(self.ctx, C.byref(w), _ptr(st), _ptr(dv), st.shape[0], _ptr(flat), _stream()), "rift_critic_backward")
        if grads:
            for k, seg in zip(CRITIC_KEYS, flat.split(CRITIC_SIZES)):
                if grads.get(k) is not None:
                    (grads[k].add_ if accumulate else grads[k].copy_)(seg.view_as(grads[k]))
        return flat

    def critic_loss_backward_raw(self, w: "RiftCritic", state: torch.Tensor, reward_sum: torch.Tensor, stats: torch.Tensor, flat: torch.Tensor):
        rc = self.lib.rift_critic_loss_backward(self.ctx, C.byref(w), _ptr(state), _ptr(reward_sum), state.shape[0], _ptr(stats), _ptr(flat), _stream())
        if rc != 0:
            self._check(rc, "rift_critic_loss_backward")

    def critic_finalize_raw(self, flat: torch.Tensor, stats: torch.Tensor, grads):
        rc = self.lib.rift_critic_finalize(self.ctx, _ptr(flat), _ptr(stats), *[_ptr(g) for g in grads], _stream())
        if rc != 0:
            self._check(rc, "rift_critic_finalize")

    def gae(self, rewards, undones, values, next_values, unterminated, gamma=0.98, lambda_=0.98):
        dev = self.device
        r = _dev(rewards, torch.float64, dev)
        a = [_dev(t, torch.float32, dev) for t in (undones, values, next_values, unterminated)]
        n = r.numel()
        out = torch.empty(n, dtype=torch.float32, device=dev)
        self._check(self.lib.rift_gae(self.ctx, _ptr(r), _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), gamma, lambda_, n,
                                      _ptr(out), _stream()), "rift_gae")
        return out

    def discounted_return(self, rewards, dones, gamma=0.98):
        dev = self.device
        r = _dev(rewards, torch.float64, dev)
        d = _dev(dones, torch.float32, dev)
        out = torch.empty(r.numel(), dtype=torch.float64, device=dev)
        self._check(self.lib.rift_discounted_return(self.ctx, _ptr(r), _ptr(d), gamma, r.numel(), _ptr(out), _stream()),
                    "rift_discounted_return")
        return out

    def normalize_advantage_(self, x):
        assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous()
        self._check(self.lib.rift_normalize_advantage(self.ctx, _ptr(x), x.numel(), _stream()), "rift_normalize_advantage")
        return x

    def group_advantage(self, returns):
        r = _dev(returns, torch.float64, self.device)
        ng, G = r.shape
        out = torch.empty_like(r)
        self._check(self.lib.rift_group_advantage(self.ctx, _ptr(r), ng, G, _ptr(out), _stream()), "rift_group_advantage")
        return out

    def arena_advantage(self, returns, r_count=None, valid_mask=None, params: Optional[RiftAdvantageParams] = None, out=None,
                        want_stats: bool = False):
        """The advantage of every candidate of an arena from its stored returns (riftga_arena_advantage; include/rift_advantage.h states the
        rule), on the current stream: `returns` (n, Rcap, 12) f64, `r_count` (n) i32 or None (every scene has Rcap lines), `valid_mask`
        (n, Rcap, 12) bool / u8 or None (all valid), `params` advantage_params(...) (None: the defaults, the reference's z-score), `out` the
        (n, Rcap, 12) f64 device tensor to write (None: a new one; never `returns` itself).  Returns the advantage, or with want_stats
        (advantage, stats): the eight f64 of the header, on the device."""
        dev = self.device
        r = _dev(returns, torch.float64, dev)
        if r.dim() != 3 or r.shape[2] != 12:
            raise ValueError(f"arena_advantage: returns (n, Rcap, 12), got {tuple(r.shape)}")
        n, Rcap = int(r.shape[0]), int(r.shape[1])
        rc = None if r_count is None else _dev(r_count, torch.int32, dev)
        vm = None if valid_mask is None else _dev(valid_mask.view(torch.uint8) if valid_mask.dtype == torch.bool else valid_mask, torch.uint8, dev)
        if (rc is not None and rc.numel() != n) or (vm is not None and tuple(vm.shape) != tuple(r.shape)):
            raise ValueError("arena_advantage: r_count (n) and valid_mask (n, Rcap, 12) go with returns (n, Rcap, 12)")
        if out is None:
            out = torch.empty_like(r)
        elif not (out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == tuple(r.shape)):
            raise ValueError("arena_advantage: out must be a contiguous f64 device tensor of the shape of returns")
        stats = torch.empty(8, dtype=torch.float64, device=dev) if want_stats else None
        p = advantage_params() if params is None else params
        self._check(self.lib.riftga_arena_advantage(self.ctx, _ptr(r), _ptr(rc), _ptr(vm), n, Rcap, C.byref(p), _ptr(out), _ptr(stats), _stream()),
                    "riftga_arena_advantage")
        return (out, stats) if want_stats else out

    def rollout_return(self, delta_dis, delta_angle, speed, acc, ang_vel, ang_acc, collision, off_road, gamma=0.98, *, reward_model=None,
                       terms: bool = False):
        """The discounted return of G candidates, (G,) f64.  reward_model (rift_amd.gym_carla.reward.reward_model) or terms=True send the call
        through rift_rollout_return_ex; terms=True returns (returns, terms (G, 8)): the seven discounted term sums and the steps counted.
        reward_model may also be a ready RiftEvalParams (its gamma then replaces the argument's)."""
        dev = self.device
        f = [_dev(t, torch.float32, dev) for t in (delta_dis, delta_angle, speed, acc, ang_vel, ang_acc)]
        col, off = self.stage(collision, torch.bool), self.stage(off_road, torch.bool)
        G, Ts = f[1].shape
        out = torch.empty(G, dtype=torch.float64, device=dev)
        if reward_model is None and not terms:
            self._check(self.lib.rift_rollout_return(self.ctx, *[_ptr(t) for t in f], _ptr(col), col.shape[1], _ptr(off),
                                                     off.shape[1], G, Ts, gamma, _ptr(out), _stream()), "rift_rollout_return")
            return out
        p = reward_model if isinstance(reward_model, RiftEvalParams) else eval_params(reward_model, gamma)
        tm = torch.empty(G, 8, dtype=torch.float64, device=dev) if terms else None
        self._check(self.lib.rift_rollout_return_ex(self.ctx, *[_ptr(t) for t in f], _ptr(col), col.shape[1], _ptr(off),
                                                    off.shape[1], G, Ts, C.byref(p), _ptr(out), _ptr(tm), _stream()), "rift_rollout_return_ex")
        return (out, tm) if terms else out
