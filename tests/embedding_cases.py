"""Designed batches, the fp64 reference, its 16-bit operand emulation and its mutants for the Fourier embeddings (fo_w_kernel,
fourier_fused_kernel, fourier_layerwise), the ego state token (ego_fused_kernel, ego_token_layerwise) and the token assembly (token_kernel,
static_token_kernel): what tests/test_gpu_embeddings.py compares the engine's fo_pos / fo_speed / fo_static / r_emb / x_ego / x_tokens taps
with, and what tests/test_embedding_cases.py checks on the CPU.  No GPU import.

The reference restates oracle/pluto_ref.py's `fourier_embedding`, `state_attention_encoder`, `map_encoder`'s sum, `agent_encoder`'s
assembly and `static_objects_encoder` in fp64 on the batch's fp32 inputs:
    fo_pos (bs N, 128): pos_emb of the token positions, heading wrapped | fo_speed (bs Mp, 128): speed_limit_emb of EVERY polygon's value,
    with or without a limit | fo_ref (bs R, 128): r_pos_emb | fo_static (bs S, 128): obj_encoder | x_ego (bs, 128) | x_tokens (bs, N, 128).
The reference-line side adds into the PointsEncoder's output in place (the taps r_pe and r_emb read one buffer), so it is seen where that
output is exactly zero: every line but the first of a scene carries geometry and NO valid point.  On the first lines r_emb is compared
against tests/points_cases.py's encoder reference plus fo_ref, within the sum of the two bars.
`fmt` = "bf16" / "fp16" rounds BOTH operands of every contraction to that format and nothing else (tests/history_cases.py's method): the
129-column first Linear of a Fourier dimension counts as one contraction (the layer-wise path runs it as one; the fused kernels keep its
129th column, x_d itself, in fp32 and come out below E_emu).  The phase x f is formed in fp32 in the emulation, as oracle and kernels
do, so E_emu carries the phase term of large positions.  E_emu[case, tap, fmt] = max |emulation - fp64| is the yardstick of the device bars.
`mut` names ONE wrong restatement (MUTANTS): the CPU test asserts that each moves a compared tap by at least three device bars."""
import math

import numpy as np
import torch

from rift_amd import synthetic as syn
from tests import helpers as H
from tests import points_cases as PC

FMT = {"bf16": torch.bfloat16, "fp16": torch.float16}
LN_EPS = 1e-5
EGO = "agent_encoder.ego_state_emb."
FO_TAPS = ("fo_pos", "fo_speed", "fo_ref", "fo_static")
TAPS = FO_TAPS + ("x_ego",)
# The device bar of a tap is K[fmt] * E_emu[case, tap, fmt]: one factor per format for all taps, cases and builds = twice the worst measured
# device-error / E_emu ratio, rounded up, and never more than 6 (the rule of history_cases.K).  Measured on MI355X over all taps, cases and
# builds: bf16 1.40 (fo_w_kernel / fourier_fused_kernel and the poisoned builds alike: static, fo_static; next 1.20: p258, fo_speed;
# layer-wise 1.20: t128, x_ego), fp16 1.26 (fused: r17, fo_pos; layer-wise 1.18: t65, x_ego); x_ego under state dropout 1.23 at the most
# (fp16, b15).  The hardware sine / cosine of the fused kernels and their fp32 LayerNorms are what the emulation does not round.
K = {"bf16": 3, "fp16": 3}
# The exact-fp32 path against fp64, every tap: twice the worst measured on MI355X (1.218e-6: l129, fo_ref; x_ego under state dropout
# 5.1e-7), rounded up to one digit; tests/test_gpu_embeddings.py asserts it stays under 1e-4 max(1, max |tap|).
FP32_BAR = 3e-6
# The random stream of the ego token's state dropout (engine.hip: next_stream()): behind the history encoder's.  The wave-private levels
# take 1, 6, 11 (one + four each): 16.  The layer-wise history encoder of the exact-fp32 forward takes one per DropPath site with a positive
# rate (embedding.py:30: five of the six blocks, two branches each: 1 .. 10): 11.
EGO_STREAM = {"16-bit": 16, "fp32": 11}
EGO_DROP_P = np.float32(0.75)
TRAIN_SEEDS = (4, 18)           # under both and on both streams, b33 has a scene with all of tokens 3..5 masked and one with none (test_embedding_cases.py)
SEAM_MARGIN = 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
# name: (first scene seed, scenes bs, agent slots A, polygon slots Mp, line slots R, static slots S).  Rows of the three sides of the one
# launch: token positions bs (A + Mp), speed limits bs Mp, reference lines bs R; what each case reaches is asserted from these shapes in
# tests/test_embedding_cases.py.
SPEC = {
    "r1": (9900, 1, 15, 1, 1, 0),           # 16 | 1 | 1
    "r17": (9905, 1, 5, 12, 16, 0),         # 17 | 12 | 16
    "t65": (9910, 5, 3, 10, 1, 0),          # 65 | 50 | 5
    "t128": (9920, 2, 4, 60, 1, 0),         # 128 | 120: the speed side's second pass is empty | 2
    "p129": (9930, 3, 4, 43, 1, 0),         # 141: two workgroups | 129: one workgroup, second pass one tile | 3
    "p258": (9940, 6, 4, 43, 1, 0),         # 282: three workgroups | 258: two, the second with one tile | 6: one
    "l128": (9950, 16, 2, 2, 8, 0),         # 64 | 32 | 128; bs = 16
    "l129": (9970, 43, 2, 1, 3, 0),         # 129 | 43 | 129
    "b15": (10020, 15, 3, 6, 1, 0),         # 135 | 90 | 15; bs = 15
    "b17": (10040, 17, 2, 2, 1, 0),         # 68 | 34 | 17; bs = 17
    "b33": (10060, 33, 2, 4, 1, 0),         # 198 | 132: second pass partial | 33; bs = 33
    "static": (10100, 4, 12, 8, 2, 5),      # S > 0: every embedding a launch of its own (D = 2 for the static objects), static_token_kernel
}
CASES = tuple(SPEC)
# headings of several turns of both signs, values just inside (-pi, pi), ordinary ones
HEADINGS = (7.0, -7.0, 9.5, -9.5, math.pi - 0.01, -math.pi + 0.01, 3.0, -3.0, 16.0, -22.5)
_c = {}


def _build(name):
    seed0, bs, A, Mp, R, S = SPEC[name]
    g = torch.Generator().manual_seed(seed0)
    scenes = [syn.make_scene(seed0 + i, A, Mp, R, R) for i in range(bs)]
    for b, s in enumerate(scenes):
        f = s["feature"]
        ag, mp, rl = f["agent"], f["map"], f["reference_line"]
        mp["valid_mask"][:, 0] = True
        ag["valid_mask"][:] = True
        if A > 2:
            ag["valid_mask"][1 + b % (A - 1)] = False                       # a padded agent: its token is its type embedding alone
        for i in range(1, A):                                               # every other row: a designed heading (the last step is the token's)
            if (i + b) % 2 == 0:
                ag["heading"][i, -1] = HEADINGS[(i + 3 * b) % len(HEADINGS)]
        for m in range(Mp):
            k = m + b
            if k % 2 == 1:
                mp["polygon_center"][m, 2] = HEADINGS[(k // 2 + b) % len(HEADINGS)]
            mp["polygon_type"][m] = k % 3
            mp["polygon_on_route"][m] = (k // 3) % 2 == 1
            mp["polygon_tl_status"][m] = (k // 2) % 4
            mp["polygon_has_speed_limit"][m] = k % 4 != 2                   # with and without a limit inside every 16-row tile
        mp["polygon_speed_limit"] = (torch.rand(Mp, generator=g) * 30.0).float()
        mp["polygon_speed_limit"][~mp["polygon_has_speed_limit"]] = 0.0
        # reference lines: all 120 points carry geometry; only the first line keeps valid points (the others: the PointsEncoder's output is
        # exactly zero there, and r_emb IS the position embedding)
        th = torch.randn(R, 1, generator=g) * 1.5 + torch.randn(R, 1, generator=g) * 0.01 * torch.arange(120, dtype=torch.float32)
        pos = torch.randn(R, 1, 2, generator=g) * 25.0 + torch.cumsum(torch.stack([th.cos(), th.sin()], -1), dim=1)
        rl["position"] = pos.float().contiguous()
        rl["vector"] = torch.cat([pos[:, 1:] - pos[:, :-1], pos[:, -1:] - pos[:, -2:-1]], dim=1).float().contiguous()
        rl["orientation"] = th.float().contiguous()
        rl["valid_mask"][1:] = False
        rl["valid_mask"][0, :40] = True
        # current_state: both signs, another magnitude per token
        mag = torch.tensor([0.3, 1.5, 4.0, 9.0, 0.7, 2.5])[torch.randperm(6, generator=g)]
        f["current_state"][:6] = mag * (torch.randint(0, 2, (6,), generator=g) * 2 - 1).float() * (0.5 + torch.rand(6, generator=g))
        if S > 0:
            sv = torch.rand(S, generator=g) < 0.7
            sv[b % S] = True
            f["static_objects"] = {
                "position": (torch.randn(S, 2, generator=g) * 30.0).float(), "heading": torch.tensor([HEADINGS[(s_ + b) % len(HEADINGS)] for s_ in range(S)]),
                "shape": (0.5 + 2.5 * torch.rand(S, 2, generator=g)).float(), "category": torch.randint(0, 4, (S,), generator=g).to(torch.int8),
                "valid_mask": sv}
    return syn.collate_scenes(scenes)["cur_pluto_feature_torch"]


def case(name):
    if name not in _c:
        _c[name] = _build(name)
    return _c[name]


def shapes(name):
    _, bs, A, Mp, R, S = SPEC[name]
    N = A + Mp + S
    return {"bs": bs, "A": A, "Mp": Mp, "R": R, "S": S, "N": N, "nT": bs * N, "nP": bs * Mp, "nL": bs * R, "nS": bs * S}


def fow_workgroups(name):
    """The workgroups fo_w_kernel gives the three sides (engine.hip: 8 tiles of 16 rows per pass, two passes for the one-dimensional side)."""
    s = shapes(name)
    t = lambda rows: -(-rows // 16)
    return (-(-t(s["nT"]) // 8), -(-t(s["nP"]) // 16), -(-t(s["nL"]) // 8))


def wrap(x):
    return (x + math.pi) % (2 * math.pi) - math.pi


def sides(data):
    """{side: (x (rows, D) fp32 inputs, prefix of the embedding's weights, wrapped dimension or None)} -- pluto_model.py:133-147,
    map_encoder.py:73-80, planning_decoder.py:155-158, static_objects_encoder.py:17-31."""
    ag, mp, rl, so = data["agent"], data["map"], data["reference_line"], data["static_objects"]
    pos = torch.cat([ag["position"][:, :, 20], mp["polygon_center"][..., :2], so["position"]], dim=1)
    ang = torch.cat([ag["heading"][:, :, 20], mp["polygon_center"][..., 2], so["heading"]], dim=1)
    out = {"fo_pos": (torch.cat([pos, ang[..., None]], -1).reshape(-1, 3), "pos_emb.", 2),
           "fo_speed": (mp["polygon_speed_limit"].reshape(-1, 1), "map_encoder.speed_limit_emb.", None),
           "fo_ref": (torch.cat([rl["position"][:, :, 0], rl["orientation"][:, :, 0, None]], -1).reshape(-1, 3), "planning_decoder.r_pos_emb.", None)}
    if so["position"].shape[1] > 0:
        out["fo_static"] = (so["shape"].reshape(-1, 2), "static_objects_encoder.obj_encoder.", None)
    return out


def seam_margin(data):
    """The smallest distance of a heading the token side wraps from an odd multiple of pi."""
    h = sides(data)["fo_pos"][0][:, 2].double()
    return float((wrap(h).abs() - math.pi).abs().min())


# ---------------------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------------------
B3_SCALE, POS_EMBED_SCALE, STATIC_TYPE_SCALE = 8.0, 8.0, 8.0
_w = {}


def case_weights():
    """perturbed_state_dict with: every mlps.d.3.bias of the four embeddings x 8 (N(0, 0.02) against a sum of unit size: whether the
    bias counts once or once per dimension is 0.03 of it otherwise); ego_state_emb.pos_embed x 8 (N(0, 0.02) against tokens of size
    |state| x 0.2); static_objects_encoder.type_emb x 8 (N(0, 0.02): where the position embedding is added in place, x_tokens carries that
    embedding's 16-bit bar, 0.03, and a missing type embedding stays under three of them otherwise)."""
    if "sd" not in _w:
        sd = {k: v.clone() for k, v in H.weights().items()}
        hit = 0
        for k in sd:
            if ".mlps." in k and k.endswith(".3.bias"):
                sd[k] = sd[k] * B3_SCALE
                hit += 1
        sd[EGO + "pos_embed"] = sd[EGO + "pos_embed"] * POS_EMBED_SCALE
        sd["static_objects_encoder.type_emb.weight"] = sd["static_objects_encoder.type_emb.weight"] * STATIC_TYPE_SCALE
        assert hit == 3 + 1 + 3 + 2, hit
        _w["sd"] = sd
    return _w["sd"]


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 reference, operand emulation, mutants
# ---------------------------------------------------------------------------------------------------------------------------------
FO_MUTANTS = ("wrap_missing", "wrap_other_dim", "cos_sin_swapped", "rank1_dropped", "b3_counted_once", "ref_overwrites", "rows_tile_shift",
              "rows_pass_shift", "speed_second_pass_dropped")
EGO_MUTANTS = ("ego_scale_missing", "ego_pos_embed_missing", "ego_mask_on_first_three", "ego_mask_ignored")
TOKEN_MUTANTS = ("limit_unknown_exchanged", "pos_row_stride_A", "static_type_missing")
MUTANTS = FO_MUTANTS + EGO_MUTANTS + TOKEN_MUTANTS


class _R:
    def __init__(self, fmt, mut):
        assert mut is None or mut in MUTANTS, mut
        self.fmt, self.mut = fmt, mut

    def r(self, x):
        return x if self.fmt is None else x.float().to(FMT[self.fmt]).double()

    def lin(self, x, w, b=None):
        y = self.r(x) @ self.r(w).t()
        return y if b is None else y + b


def _ln(x, g, b):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + LN_EPS) * g + b


def fourier64(A, x, sd, p, wrap_dim, side=None):
    """fourier_embedding.py:45-55 on x (rows, D) fp32 -> (rows, 128) fp64; p: the embedding's prefix in sd (fp64 tensors)."""
    rows, D = x.shape
    mut = A.mut
    x = x.double().clone()
    wd = {"wrap_missing": None, "wrap_other_dim": 0 if wrap_dim is not None else None}.get(mut, wrap_dim)
    if wd is not None:
        x[:, wd] = wrap(x[:, wd])
    for name, step in (("rows_tile_shift", 16), ("rows_pass_shift", 128)):
        if mut == name:
            i = torch.arange(rows)
            j = i ^ step
            x = x[torch.where(j < rows, j, i)]
    f = sd[p + "freqs.weight"]                                       # (D, 64)
    if A.fmt is None:
        ph = x[:, :, None] * f[None]
    else:                                                            # the phase in fp32, as oracle and kernels form it
        ph = (x.float()[:, :, None] * f.float()[None]).double()
    ph = ph * (2 * math.pi)
    c, s = ph.cos(), ph.sin()
    feat = torch.cat([s, c] if mut == "cos_sin_swapped" else [c, s], -1)      # (rows, D, 128)
    acc = 0.0
    for d in range(D):
        m = f"{p}mlps.{d}."
        w0 = sd[m + "0.weight"]
        fd = torch.cat([feat[:, d], x[:, d, None]], -1)
        if mut == "rank1_dropped":
            fd = torch.cat([feat[:, d], torch.zeros(rows, 1).double()], -1)
        h = torch.relu(_ln(A.lin(fd, w0, sd[m + "0.bias"]), sd[m + "1.weight"], sd[m + "1.bias"]))
        acc = acc + A.lin(h, sd[m + "3.weight"], None if (mut == "b3_counted_once" and d > 0) else sd[m + "3.bias"])
    y = A.lin(torch.relu(_ln(acc, sd[p + "to_out.0.weight"], sd[p + "to_out.0.bias"])), sd[p + "to_out.2.weight"], sd[p + "to_out.2.bias"])
    if mut == "speed_second_pass_dropped" and side == "fo_speed":    # rows of the odd 128-row passes: never written
        y = torch.where(((torch.arange(rows) // 128) % 2 == 1)[:, None], torch.zeros(()).double(), y)
    return y


def ego_drop_mask(seed, bs, path="16-bit"):
    """(bs, 6) bool: the keys ego_fused_kernel / ego_dropmask_kernel mask in a train forward with drops: uniform01(seed, stream, 6 b + j) <
    0.75 for the tokens j = 3..5 (agent_encoder.py:119-129); path: whose stream, EGO_STREAM."""
    from tests.test_gpu_skip_discarded import _uniform01
    u = _uniform01(seed, EGO_STREAM[path], np.arange(bs * 6)).reshape(bs, 6)
    m = u < EGO_DROP_P
    m[:, :3] = False
    return torch.from_numpy(m)


def ego64(A, cs, sd, drop_mask=None):
    """agent_encoder.py:99-140 on cs (bs, >= 6) fp32 -> (bs, 128) fp64."""
    mut = A.mut
    bs = cs.shape[0]
    x = cs[:, :6].double()
    emb = torch.stack([x[:, i, None] * sd[f"{EGO}linears.{i}.weight"][:, 0] + sd[f"{EGO}linears.{i}.bias"] for i in range(6)], 1)
    if mut != "ego_pos_embed_missing":
        emb = emb + sd[EGO + "pos_embed"].reshape(6, 128)
    w, b = sd[EGO + "attn.in_proj_weight"], sd[EGO + "attn.in_proj_bias"]
    q = A.lin(sd[EGO + "query"].reshape(1, 128), w[:128], b[:128]).view(1, 4, 1, 32)
    k = A.lin(emb, w[128:256], b[128:256]).view(bs, 6, 4, 32).transpose(1, 2)
    v = A.lin(emb, w[256:], b[256:]).view(bs, 6, 4, 32).transpose(1, 2)
    s = A.r(q * (1.0 if mut == "ego_scale_missing" else 32 ** -0.5)) @ A.r(k).transpose(-1, -2)          # (bs, 4, 1, 6)
    if drop_mask is not None and mut != "ego_mask_ignored":
        dm = drop_mask.roll(3, 1) if mut == "ego_mask_on_first_three" else drop_mask
        s = s.masked_fill(dm[:, None, None, :], float("-inf"))
    o = (A.r(torch.softmax(s, -1)) @ A.r(v)).transpose(1, 2).reshape(bs, 128)
    return A.lin(o, sd[EGO + "attn.out_proj.weight"], sd[EGO + "attn.out_proj.bias"])


def _sd64(sd):
    return {k: v.double() for k, v in sd.items() if v.is_floating_point()}


def reference(data, sd, fmt=None, mut=None, drop_seed=None):
    """{tap: fp64} of TAPS (fo_static where the batch has static objects); drop_seed: x_ego of a train forward with drops under that seed, or (seed, path)."""
    A = _R(fmt, mut)
    sd = _sd64(sd)
    out = {side: fourier64(A, x, sd, p, wd, side) for side, (x, p, wd) in sides(data).items()}
    bs = data["current_state"].shape[0]
    seed, path = drop_seed if isinstance(drop_seed, tuple) else (drop_seed, "16-bit")
    out["x_ego"] = ego64(A, data["current_state"], sd, None if seed is None else ego_drop_mask(seed, bs, path))
    return out


def line_rows(data):
    """(rows of lines with a valid point, rows of lines without one) of the bs R reference lines."""
    v = data["reference_line"]["valid_mask"].any(-1).reshape(-1)
    return v, ~v


def r_emb64(data, sd, fmt=None, mut=None):
    """(r_pe, r_emb) (bs R, 128): the PointsEncoder's output (tests/points_cases.py's reference, eval mode) and the sum with fo_ref."""
    r_pe = PC.reference(data, sd, False, fmt)["b"]["out"]
    x, p, wd = sides(data)["fo_ref"]
    fo = fourier64(_R(fmt, mut), x, _sd64(sd), p, wd, "fo_ref")
    return r_pe, (fo if mut == "ref_overwrites" else r_pe + fo)


def assemble64(data, sd, taps, mut=None):
    """x_tokens (bs, N, 128) in fp64 from what the assembly reads -- nat_out (bs A, 128) in slot order, x_ego (bs, 128), poly_pe (bs Mp, 128),
    fo_speed (bs Mp, 128), fo_pos (bs N, 128), fo_static (bs S, 128) -- and the embedding tables, and `mag`: the sum of the |terms| of every
    element, what bounds every partial sum (sum_bar).  agent_encoder.py:87-96, map_encoder.py:82-91, static_objects_encoder.py:17-31,
    pluto_model.py:149-150."""
    ag, mp, so = data["agent"], data["map"], data["static_objects"]
    bs, A = ag["position"].shape[:2]
    Mp, S = mp["polygon_center"].shape[1], so["position"].shape[1]
    N = A + Mp + S
    t = {k: v.double() for k, v in taps.items()}
    w = lambda k: sd[k].double()
    valid = ag["valid_mask"][:, :, :21].any(-1)
    nat = torch.where(valid[..., None], t["nat_out"].view(bs, A, 128), torch.zeros(()).double()).clone()
    nat[:, 0] = t["x_ego"]
    has = mp["polygon_has_speed_limit"]
    if mut == "limit_unknown_exchanged":
        has = ~has
    speed = torch.where(has[..., None], t["fo_speed"].view(bs, Mp, 128), w("map_encoder.unknown_speed_emb.weight")[0])
    terms_a = [nat, w("agent_encoder.type_emb.weight")[ag["category"].long()]]
    terms_p = [t["poly_pe"].view(bs, Mp, 128), w("map_encoder.type_emb.weight")[mp["polygon_type"].long()],
               w("map_encoder.on_route_emb.weight")[mp["polygon_on_route"].long()],
               w("map_encoder.traffic_light_emb.weight")[mp["polygon_tl_status"].long()], speed]
    parts = [(sum(terms_a), sum(x.abs() for x in terms_a)), (sum(terms_p), sum(x.abs() for x in terms_p))]
    if S > 0:
        ty = w("static_objects_encoder.type_emb.weight")[so["category"].long()]
        if mut == "static_type_missing":
            ty = ty * 0.0
        ts = [torch.where(so["valid_mask"][..., None], x, torch.zeros(()).double()) for x in (t["fo_static"].view(bs, S, 128), ty)]
        parts.append((sum(ts), sum(x.abs() for x in ts)))
    x, mag = torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
    pe = t["fo_pos"].view(bs, N, 128)
    if mut == "pos_row_stride_A":                                    # the positional embedding of row b N + a taken at b A + a
        rows = (torch.arange(bs)[:, None] * A + torch.arange(N)[None, :]).clamp(max=bs * N - 1)
        pe = t["fo_pos"].view(bs * N, 128)[rows]
    return x + pe, mag + pe.abs()


ADDS = 5            # fp32 additions of a polygon token: type, on-route, traffic light, speed, position (an agent token: 2, a static token: 2)


def sum_bar(mag):
    """What ADDS fp32 additions cost an element whose partial sums are bounded by mag: half an ulp of the running sum each, 2^-24 mag at
    the most (the style of small_kernel_cases.normalize_ref64)."""
    return ADDS * 2.0 ** -24 * float(mag.max())


def compared(taps, data):
    """{tap: the compared part}: all rows of every tap; fo_ref from r_emb on the lines without a valid point."""
    return {k: v for k, v in taps.items() if k in TAPS}


def max_shift(a, b):
    return {k: float(torch.nan_to_num((a[k].double() - b[k].double()).abs(), nan=float("inf")).max()) for k in a if k in b}


_r, _e = {}, {}


def reference64(name, drop_seed=None):
    if (name, drop_seed) not in _r:
        _r[name, drop_seed] = reference(case(name), case_weights(), drop_seed=drop_seed)
    return _r[name, drop_seed]


def emu_error(name, drop_seed=None):
    """E_emu[case]: {(tap, fmt): max |emulation - fp64| over all rows}."""
    if (name, drop_seed) not in _e:
        ref = reference64(name, drop_seed)
        _e[name, drop_seed] = {(k, fmt): d for fmt in FMT
                               for k, d in max_shift(reference(case(name), case_weights(), fmt, drop_seed=drop_seed), ref).items()}
    return _e[name, drop_seed]


_p = {}


def r_pe_emu_error(name):
    """(r_pe fp64 (bs R, 128), {fmt: E_emu of the PointsEncoder's output on the lines with a valid point})."""
    if name not in _p:
        data, sd = case(name), case_weights()
        ref = PC.reference(data, sd, False)["b"]["out"]
        v = line_rows(data)[0]
        _p[name] = (ref, {fmt: float((PC.reference(data, sd, False, fmt)["b"]["out"] - ref)[v].abs().max()) for fmt in FMT})
    return _p[name]
