"""Designed batches, the fp64 reference, its 16-bit operand emulation and its mutants for the output heads (heads3_fused_kernel on the planning
rows and on the gathered agent rows, ego_heads_kernel, the layer-wise MLPLayer launches with interleave_traj_kernel): what
tests/test_gpu_heads.py compares the engine's `trajectory`, `prediction`, `hidden` and `ref_free_trajectory` with, and what
tests/test_heads_cases.py checks on the CPU.  No GPU import.

`reference64` restates oracle/pluto_ref.py's `mlp_layer` (loc / yaw / vel heads of the planning decoder, `agent_predictor`,
`ref_free_decoder`) and `hidden_proj` in fp64 from enc_out (bs, N, 128) and q_final (bs, R, 12, 128) on.  Its inputs are arguments, so the
GPU test feeds it the DEVICE's enc_out and q_final taps (device error and E_emu then measure the heads alone) and the CPU test the oracle's.
    trajectory (bs, R, 12, 80, 6), ALL lines | prediction (bs, A - 1, 80, 6), ALL agent slots 1 .. A - 1 | hidden (bs, 128) |
    ref_free_trajectory (bs, 80, 4)
`fmt` = "bf16" / "fp16" rounds BOTH operands of every contraction (the two Linears of every head) to that format and nothing else:
E_emu[case, tap, fmt] = max |emulation - fp64| over the compared part of a tap is the yardstick of the device bars (tests/history_cases.py).
`mut` names ONE wrong restatement (MUTANTS): the CPU test asserts that each moves a compared tap by at least three device bars."""
import torch

from oracle import pluto_ref
from rift_amd import synthetic as syn
from tests import helpers as H

M, D, STEPS = 12, 128, 80
LN_EPS = 1e-5
TILE, EGO_TILE, GROUP_ROWS = 128, 16, 8 * 128       # heads_fused.h: HD_ROWS, the rows of an ego_heads_kernel workgroup, rows of a group of 8 tiles
FMT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TAPS = ("trajectory", "prediction", "hidden", "ref_free_trajectory")
HEADS = ("loc", "yaw", "vel")
# The device bar of a tap is K[fmt] * E_emu[case, tap, fmt]: one factor per format for all taps, cases and builds = twice the worst measured
# device-error / E_emu ratio, rounded up, and never more than 6 (the rule of history_cases.K).  Measured on MI355X over all taps, cases and
# builds: bf16 1.0001 (layer-wise: plan1056, ref_free_trajectory; fused 1.0000), fp16 1.0035 (fused: b17, ref_free_trajectory; layer-wise
# 1.0001) -- the heads are two contractions deep and the device rounds where the emulation does; twice that, rounded up, is 3.
K = {"bf16": 3, "fp16": 3}
# The exact-fp32 path against fp64, every tap: twice the worst measured on MI355X (1.911e-6: p128, prediction), rounded up to one digit;
# tests/test_gpu_heads.py asserts it stays under 1e-4 max(1, max |tap|).
FP32_BAR = 4e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
# name: (first scene seed, scenes bs, agent slots A, polygon slots Mp, line slots R).  What each reaches (test_heads_cases.py asserts it
# from the shapes): planning rows bs R 12 against the 128-row tiles of heads3_fused_kernel and its groups of 8 tiles x 3 heads; prediction
# rows bs (A - 1), gathered from the encoder output at stride N, offset 1; bs against the 16 rows of an ego_heads_kernel workgroup.
SPEC = {
    "one": (9700, 1, 2, 3, 3),              # 36 planning rows (< 128), A = 2: one prediction row, bs = 1
    "b15": (9710, 15, 10, 3, 2),            # 360 = 2 x 128 + 104 planning rows; 135 prediction rows, 9 per scene: tile 1 starts inside scene 14
    "b16": (9730, 16, 9, 4, 2),             # bs R = 32: 384 = 3 x 128 planning rows; 128 prediction rows, 8 per scene; bs = one ego tile
    "b17": (9750, 17, 2, 3, 1),             # 204 planning rows; A = 2 over 17 scenes: every prediction row from another scene; bs = 16 + 1
    "b33": (9770, 33, 6, 3, 1),             # 396 = 3 x 128 + 12 planning rows; 165 prediction rows, 5 per scene (128 = 25 x 5 + 3); bs = 2 x 16 + 1
    "p128": (9810, 2, 65, 3, 1),            # exactly 128 prediction rows
    "plan1056": (9820, 11, 3, 3, 8),        # 1056 planning rows: nine tiles, group 1 holds one (blockIdx / 24 = 1)
    "pred1056": (9840, 24, 45, 3, 1),       # 1056 prediction rows: nine tiles, group 1 holds one; 44 per scene (128 = 2 x 44 + 40)
}
CASES = tuple(SPEC)
_c = {}


def _build(name):
    seed0, bs, A, Mp, R = SPEC[name]
    scenes = [syn.make_scene(seed0 + i, A, Mp, R, R) for i in range(bs)]
    for b, s in enumerate(scenes):
        f = s["feature"]
        f["agent"]["valid_mask"][:] = True
        f["map"]["valid_mask"][:] = True
        # one padded agent slot in every odd scene (A = 2: in every third scene, the only slot there is): its prediction is not compared
        if (A > 2 and b % 2 == 1) or (A == 2 and b % 3 == 1):
            f["agent"]["valid_mask"][1 + b % (A - 1)] = False
        keep = 1 + (7 * b + 1) % R if bs > 1 else R                 # a prefix of valid lines, never empty; a padded line is what the
        rl = f["reference_line"]                                    # collation pads with: zeros, no valid point
        for r in range(keep, R):
            for k in ("position", "vector", "orientation", "valid_mask", "future_projection"):
                rl[k][r] = 0
    return syn.collate_scenes(scenes)["cur_pluto_feature_torch"]


def case(name):
    if name not in _c:
        _c[name] = _build(name)
    return _c[name]


def masks(data):
    """(valid lines (bs, R), valid agents of the slots 1 .. A - 1 (bs, A - 1))."""
    return data["reference_line"]["valid_mask"].any(-1), data["agent"]["valid_mask"][:, 1:, :21].any(-1)


def shapes(name):
    """{bs, A, N, R, plan_rows, pred_rows, per} of a case."""
    _, bs, A, Mp, R = SPEC[name]
    return {"bs": bs, "A": A, "N": A + Mp, "R": R, "plan_rows": bs * R * M, "pred_rows": bs * (A - 1), "per": A - 1}


def case_weights():
    """The suite's weights as they are: biases, LayerNorm affines and every matrix of the heads are non-trivial there, and every mutant
    below clears three bars under them (test_heads_cases.py)."""
    return H.weights()


def _double(d):
    return {k: _double(v) if isinstance(v, dict) else (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


_i = {}


def oracle_inputs(name):
    """(enc_out (bs, N, 128), q_final (bs, R, 12, 128), the oracle's outputs) of a case, the oracle run on double tensors (weights and
    scenes are generated BEFORE the default dtype changes: the seeded generators draw other numbers in float64)."""
    if name not in _i:
        data, sd = _double(H.clone_tree(case(name))), _double(case_weights())
        torch.set_default_dtype(torch.float64)
        try:
            out, _, taps = pluto_ref.planning_model_forward(sd, data, need_traj=True, want_taps=True)
        finally:
            torch.set_default_dtype(torch.float32)
        assert taps["q_final"].dtype == torch.float64
        _i[name] = (taps["enc_out"], taps["q_final"], out)
    return _i[name]


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 reference, operand emulation, mutants
# ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("heads_reordered", "pair_swapped", "step_column_mapping", "gather_offset_0", "gather_stride_A", "row_of_neighbour_tile",
           "ln_over_128_columns", "hidden_relu_missing", "ntiles_9_10_dropped", "ego_stride_A", "ego_row_of_neighbour_tile")


class _R:
    """The arithmetic of one run: operand rounding (fmt) and the one mutation (mut)."""

    def __init__(self, fmt, mut):
        assert mut is None or mut in MUTANTS, mut
        self.fmt, self.mut = fmt, mut

    def r(self, x):
        return x if self.fmt is None else x.float().to(FMT[self.fmt]).double()

    def lin(self, x, w, b):
        return self.r(x) @ self.r(w).t() + b


def _ln(x, g, b, cols=None):
    s = x if cols is None else x[..., :cols]
    m = s.mean(-1, keepdim=True)
    v = ((s - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + LN_EPS) * g + b


def _mlp(A, x, sd, p):
    """mlp_layer.py:8-16: Linear -> LayerNorm -> ReLU -> Linear."""
    h = A.lin(x, sd[p + "mlp.0.weight"], sd[p + "mlp.0.bias"])
    h = torch.relu(_ln(h, sd[p + "mlp.1.weight"], sd[p + "mlp.1.bias"], 128 if A.mut == "ln_over_128_columns" else None))
    y = A.lin(h, sd[p + "mlp.3.weight"], sd[p + "mlp.3.bias"])
    if A.mut == "ntiles_9_10_dropped" and y.shape[-1] == 160:      # columns 128 .. 159: the bias alone
        y = torch.cat([y[..., :128], sd[p + "mlp.3.bias"][128:].expand_as(y[..., 128:])], -1)
    return y


def _three(A, x, sd, prefixes):
    """Three MLPLayer(128, 256, 160) heads on rows x (rows, 128) -> (rows, 80, 6) = [x, y, cos, sin, vx, vy] per step."""
    rows = x.shape[0]
    if A.mut == "row_of_neighbour_tile":                            # row r of an even tile reads the row 128 further on, and back
        i = torch.arange(rows)
        j = i ^ TILE
        x = x[torch.where(j < rows, j, i)]
    ys = []
    for p in prefixes:
        y = _mlp(A, x, sd, p)
        y = y.view(rows, 2, STEPS).transpose(1, 2) if A.mut == "step_column_mapping" else y.view(rows, STEPS, 2)
        ys.append(y.flip(-1) if A.mut == "pair_swapped" else y)
    if A.mut == "heads_reordered":
        ys = [ys[0], ys[2], ys[1]]
    return torch.cat(ys, -1)


def reference64(sd, enc_out, q_final, A_slots, fmt=None, mut=None, need_traj=True):
    """{tap: fp64}.  sd: the model's state dict; enc_out (bs, N, 128); q_final (bs, R, 12, 128); A_slots: the agent slots A of a scene."""
    A = _R(fmt, mut)
    sd = {k: v.double() for k, v in sd.items() if v.is_floating_point() and k.split(".")[0] in
          ("planning_decoder", "agent_predictor", "hidden_proj", "ref_free_decoder")}
    enc_out, q_final = enc_out.double(), q_final.double()
    bs, N = enc_out.shape[:2]
    R = q_final.shape[1]
    flat = enc_out.reshape(bs * N, D)
    b = torch.arange(bs)
    ego_rows = b * (A_slots if mut == "ego_stride_A" else N)
    if mut == "ego_row_of_neighbour_tile":
        j = b ^ EGO_TILE
        ego_rows = torch.where(j < bs, j, b) * N
    ego = flat[ego_rows]
    h = A.lin(ego, sd["hidden_proj.0.weight"], sd["hidden_proj.0.bias"])
    out = {"hidden": A.lin(h if mut == "hidden_relu_missing" else torch.relu(h), sd["hidden_proj.2.weight"], sd["hidden_proj.2.bias"])}
    if not need_traj:
        return out
    out["ref_free_trajectory"] = _mlp(A, ego, sd, "ref_free_decoder.").view(bs, STEPS, 4)
    out["trajectory"] = _three(A, q_final.reshape(bs * R * M, D), sd, [f"planning_decoder.{h}_head." for h in HEADS]).view(bs, R, M, STEPS, 6)
    per = A_slots - 1
    stride, off = (A_slots if mut == "gather_stride_A" else N), (0 if mut == "gather_offset_0" else 1)
    src = (b[:, None] * stride + off + torch.arange(per)[None, :]).reshape(-1)      # heads_fused.h: (r / per) * stride + off + r % per
    out["prediction"] = _three(A, flat[src], sd, [f"agent_predictor.{h}_predictor." for h in HEADS]).view(bs, per, STEPS, 6)
    return out


def compared(out, data):
    """{tap: the part of a tap that is compared}: trajectory on the valid lines, prediction on the valid agents, the ego heads whole."""
    rv, av = masks(data)
    sel = {"trajectory": lambda v: v[rv], "prediction": lambda v: v[av]}
    return {k: sel.get(k, lambda v: v)(out[k]) for k in TAPS if k in out}


def max_shift(a, b, data):
    """{tap: max |a - b| over the compared part}; a non-finite difference counts as infinite."""
    ca, cb = compared(a, data), compared(b, data)
    return {k: float(torch.nan_to_num((ca[k].double() - cb[k].double()).abs(), nan=float("inf")).max()) for k in ca if k in cb}


def emu_error(sd, enc_out, q_final, data, ref=None):
    """E_emu of these inputs: {(tap, fmt): max |emulation - fp64| over the compared part}."""
    A_slots = data["agent"]["position"].shape[1]
    ref = reference64(sd, enc_out, q_final, A_slots) if ref is None else ref
    return {(k, fmt): d for fmt in FMT for k, d in max_shift(reference64(sd, enc_out, q_final, A_slots, fmt), ref, data).items()}


_r, _e = {}, {}


def case_reference(name):
    """The fp64 reference of a case on the oracle's enc_out / q_final."""
    if name not in _r:
        enc_out, q_final, _ = oracle_inputs(name)
        _r[name] = reference64(case_weights(), enc_out, q_final, SPEC[name][2])
    return _r[name]


def case_emu_error(name):
    if name not in _e:
        enc_out, q_final, _ = oracle_inputs(name)
        _e[name] = emu_error(case_weights(), enc_out, q_final, case(name), case_reference(name))
    return _e[name]
