"""Designed batches, the fp64 reference, its 16-bit operand emulation and its mutants for the planning decoder (q0_fused_kernel's q_proj,
dec_w_kernel in its four compiled variants or the layer-wise launches, the four producers of its cross-attention K | V^T image,
cat_x_proj in pi_forward_kernel): what tests/test_gpu_planning_decoder.py compares the engine's decoder taps with, and what
tests/test_decoder_cases.py checks on the CPU.  No GPU import.

`reference64` restates oracle/pluto_ref.py's `planning_decoder` from r_emb / enc_out on (q_proj, four `decoder_layer`s, cat_x_proj) in fp64
and returns q0, dec0..dec3 and q_final (bs, R, 12, 128) for ALL rows -- those of padded reference lines are defined: r2r computes them, the
m2m scatter zeroes them, cross attention and the FFN run on the zero rows, and the r2r mask quirk (mode m of scene b takes the line padding
of scene (12 b + m) % bs) can expose them as keys of the next layer.  Its inputs are arguments, so the GPU test feeds it the DEVICE's r_emb
and enc_out taps (device error and E_emu then measure the decoder alone) and the CPU test the oracle's.
`fmt` = "bf16" / "fp16" rounds BOTH operands of every contraction (linear, the q / K / V projections of the three attentions, Q K, P V) to
that format and nothing else: E_emu[case, tap, fmt] = max |emulation - fp64| is the yardstick of the device bars (tests/history_cases.py).
`mut` names ONE wrong restatement (MUTANTS): the CPU test asserts that each moves a compared tap by at least three device bars."""
import torch

from oracle import pluto_ref
from rift_amd import synthetic as syn
from tests import helpers as H

PD = "planning_decoder."
M, D, HEADS = 12, 128, 4
LN_EPS = 1e-5
FMT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TAPS = ("q0", "dec1", "dec3", "q_final")                    # what a 16-bit build offers (dec1: a context with RIFT_DEC_LAYERS=2)
ALL_TAPS = ("q0", "dec0", "dec1", "dec2", "dec3", "q_final")
# The device bar of a tap is K[fmt] * E_emu[case, tap, fmt]: one factor per format for all taps and cases = twice the worst measured
# device-error / E_emu ratio, rounded up, and never more than 6 (the rule of history_cases.K).  Measured on MI355X over all taps, cases and
# builds (profiles/NOTES_r17.md): bf16 1.39 (dense_r9, dec1, fused), fp16 1.16 (mid128, q_final, fused).
K = {"bf16": 3, "fp16": 3}
# The exact-fp32 layer-wise path against fp64, every tap: four times the worst measured (1.09e-5: mid128, dec3, values up to 23), rounded up
# to one digit (NOTES_r17.md).
FP32_BAR = 5e-5


# ---------------------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------------------
# Rescaled planning-decoder tensors (name suffix: factor, rows).  m_pos N(0, 0.02) -> N(0, 0.6): as large as a LayerNorm output row, so
# where it is added (q and k of m2m, never v) shows.  m2m in_proj's q | k rows x 4: the m2m scores then depend on what q and k hold (with
# xavier rows a softmax over twelve modes is nearly flat, and a dropped or rolled m_pos moves nothing).  m_emb N(0, 0.02) -> N(0, 0.6):
# the twelve modes of a line differ from q0 on, so which mode's keys r2r reads and which mode m_pos belongs to shows.  cross_attn in_proj
# x 3 (q, k and v rows): sharper cross-attention scores -- a key more or less in the sum shows -- and a larger share of the
# cross-attention block in the layer's output.  norm4.weight x 1.5: norm3 in norm4's place is another affine map, not a 5 % perturbation.
# What each factor buys, mutant by mutant: profiles/NOTES_r17.md.
SCALES = {"m_pos": (30.0, None), "m_emb": (30.0, None), "m2m_attn.in_proj_weight": (4.0, 2 * D), "cross_attn.in_proj_weight": (3.0, None),
          "norm4.weight": (1.5, None)}
_w = {}


def case_weights():
    """perturbed_state_dict with the planning-decoder tensors of SCALES rescaled."""
    if "sd" not in _w:
        sd = {k: v.clone() for k, v in H.weights().items()}
        hit = {s: 0 for s in SCALES}
        for k in sd:
            for sfx, (f, rows) in SCALES.items():
                if k.startswith(PD) and k.endswith(sfx):
                    if rows is None:
                        sd[k] = sd[k] * f
                    else:
                        sd[k][:rows] *= f
                    hit[sfx] += 1
        assert hit == {"m_pos": 1, "m_emb": 1, "m2m_attn.in_proj_weight": 4, "cross_attn.in_proj_weight": 4, "norm4.weight": 4}, hit
        _w["sd"] = sd
    return _w["sd"]


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
# name: (first scene seed, agent slots A, polygon slots Mp, line slots R, valid keys per scene (negative: the ego slot is one of the padded
# ones), valid lines per scene (a count = that prefix, a tuple = those slots))
SPEC = {
    "std80": (9500, 48, 32, 8, (80, 65, 64, 33, 17, 16, 2, 1, -40), (8, 1, 7, 3, (0, 2, 5), (4, 6), 8, 1, 5)),
    "std96": (9520, 64, 32, 8, (96, 81, 80, 17, 1), (8, 5, 8, 2, 7)),
    "mid112": (9540, 64, 48, 8, (112, 97, 96, 81, 1), (8, 3, 8, 6, 1)),
    "mid128": (9560, 64, 64, 8, (128, 113, 112, 1), (8, 4, 1, 7)),
    "dense_r9": (9580, 24, 16, 9, (40, 33, 17, 40, 25), (9, 8, 1, 5, 9)),
    "dense_192": (9600, 128, 64, 16, (192, 177, 176), (16, 9, 1)),
}
CASES = tuple(SPEC)
# the kernels a 16-bit fused forward of the case runs (prof_report labels): the scene encoder, the producer of the K | V^T image where that
# is a launch of its own (dense_r9: 40 token slots keep the standard encoder, whose tail writes the image for R <= 8 only), the decoder
KERNELS = {"std80": ("enc_fused_kernel", "dec_w_kernel"), "std96": ("enc_fused_kernel", "dec_w_kernel"),
           "mid112": ("enc_fused112_kernel", "dec_w_kernel"), "mid128": ("enc_w_kernel", "dec_w_kernel"),
           "dense_r9": ("enc_fused_kernel", "dec_kv_frag_kernel", "dec_w_kernel"), "dense_192": ("enc_w_kernel", "dec_w_kernel")}
_c = {}


def _build(name):
    seed0, A, Mp, R, keys, lines = SPEC[name]
    N = A + Mp
    g = torch.Generator().manual_seed(seed0)
    scenes = [syn.make_scene(seed0 + i, A, Mp, R, R) for i in range(len(keys))]
    for s, want, ln in zip(scenes, keys, lines):
        f = s["feature"]
        f["agent"]["valid_mask"][:] = True
        f["map"]["valid_mask"][:] = True
        ego = want > 0
        want = abs(want)
        pad = (torch.randperm(N - 1, generator=g)[: N - want - (0 if ego else 1)] + 1).tolist() + ([] if ego else [0])
        for sl in pad:                                            # scattered over the slots: a compaction is a real permutation
            if sl < A:
                f["agent"]["valid_mask"][sl] = False
            else:
                f["map"]["valid_mask"][sl - A] = False
        keep = set(range(ln)) if isinstance(ln, int) else set(ln)
        rl = f["reference_line"]
        for r in range(R):                                        # a padded line is what the collation pads with: zeros, no valid point
            if r not in keep:
                for k in ("position", "vector", "orientation", "valid_mask", "future_projection"):
                    rl[k][r] = 0
    return syn.collate_scenes(scenes)["cur_pluto_feature_torch"]


def case(name):
    if name not in _c:
        _c[name] = _build(name) if name in SPEC else H.build_batch(name)["cur_pluto_feature_torch"]
    return _c[name]


def paddings(data):
    """(encoder key padding (bs, N), line padding (bs, R)), True = padded."""
    return H.token_padding(data), ~data["reference_line"]["valid_mask"].any(-1)


def quirk_rows(r_kpm):
    """(bs * 12, R): row b * 12 + m = the line padding of scene (12 b + m) % bs (planning_decoder.py:56-60: `.repeat(M, 1)`)."""
    return r_kpm.repeat(M, 1)


_i = {}


def oracle_inputs(name, scaled=True):
    """(r_emb, enc_out, enc_kpm, r_kpm, oracle taps) of a case under case_weights() (scaled=False: the suite's weights as they are): what the
    CPU test feeds the reference, and what the GPU test's gate holds the device's r_emb / enc_out against."""
    if (name, scaled) not in _i:
        # the oracle itself, on double tensors (in fp32 its own rounding is 1.1e-5 .. 1.5e-5 at taps of magnitude 15 to 20); weights and
        # scenes are generated BEFORE the default dtype changes (the seeded generators draw other numbers in float64)
        data, sd = _double(H.clone_tree(case(name))), _double(case_weights() if scaled else H.weights())
        torch.set_default_dtype(torch.float64)
        try:
            _, _, taps = pluto_ref.planning_model_forward(sd, data, need_traj=False, want_taps=True)
        finally:
            torch.set_default_dtype(torch.float32)
        assert taps["dec3"].dtype == torch.float64
        kpm, r_kpm = paddings(data)
        _i[name, scaled] = (taps["r_emb"], taps["enc_out"], kpm, r_kpm, taps)
    return _i[name, scaled]


def _double(d):
    return {k: _double(v) if isinstance(v, dict) else (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 reference, operand emulation, mutants
# ---------------------------------------------------------------------------------------------------------------------------------
EDGES = (80, 96, 112, 128)
MUTANTS = tuple(
    ["r2r_own_row", "r2r_no_mask", "r2r_next_scene", "r2r_mode_pair_swapped", "r2r_dense_slots8"]
    + ["m2m_pos_dropped", "m2m_pos_on_v", "m2m_pos_rolled", "m2m_neighbour_line", "m2m_padded_keep_r2r", "m2m_padded_stay_zero"]
    + ["x_no_padding", "x_last_valid_masked", "x_first_padded_admitted"] + [f"x_edge_{e}" for e in EDGES]
    + ["x_k_head_pairs_swapped", "x_no_scale"]
    + ["norm3_for_norm4", "catx_ego_next_scene", "catx_halves_swapped", "qproj_halves_swapped"])

# A mutant that belongs to one path counts only in the cases that run that path: the key-tile edge of the sixth tile (std96: per scene,
# under compaction), of the seventh (mid112), of the eighth (mid128), of the dense variant's ninth (dense_192); the second round of
# line tiles (R > 8).
ONLY = {"x_edge_80": ("std96",), "x_edge_96": ("mid112",), "x_edge_112": ("mid128",), "x_edge_128": ("dense_192",),
        "r2r_dense_slots8": ("dense_r9", "dense_192")}


class _R:
    """The arithmetic of one run: operand rounding (fmt) and the one mutation (mut)."""

    def __init__(self, fmt, mut):
        assert mut is None or mut in MUTANTS, mut
        self.fmt, self.mut = fmt, mut

    def r(self, x):
        return x if self.fmt is None else x.float().to(FMT[self.fmt]).double()

    def lin(self, x, w, b=None):
        y = self.r(x) @ self.r(w).t()
        return y if b is None else y + b

    def mha(self, sd, p, q_in, k_in, v_in, mask=None, scale=True, k_heads=None, kv_rows=None):
        """torch.nn.MultiheadAttention(batch_first=True), no dropout.  mask (B, Lk) or (B, 1, Lk) bool, True = ignore.  k_heads: the K side's
        heads in that order.  kv_rows: batch row i attends to the keys / values of batch row kv_rows[i]."""
        w, b = sd[p + "in_proj_weight"], sd[p + "in_proj_bias"]
        B, Lq, Lk, hd = q_in.shape[0], q_in.shape[1], k_in.shape[1], D // HEADS
        q = self.lin(q_in, w[:D], b[:D]).view(B, Lq, HEADS, hd).transpose(1, 2)
        k = self.lin(k_in, w[D:2 * D], b[D:2 * D]).view(B, Lk, HEADS, hd).transpose(1, 2)
        v = self.lin(v_in, w[2 * D:], b[2 * D:]).view(B, Lk, HEADS, hd).transpose(1, 2)
        if k_heads is not None:
            k = k[:, k_heads]
        if kv_rows is not None:
            k, v = k[kv_rows], v[kv_rows]
        s = self.r(q * (hd ** -0.5 if scale else 1.0)) @ self.r(k).transpose(-1, -2)
        if mask is not None:
            s = s.masked_fill(mask.view(B, 1, 1, Lk), float("-inf"))
        o = (self.r(torch.softmax(s, dim=-1)) @ self.r(v)).transpose(1, 2).reshape(B, Lq, D)
        return self.lin(o, sd[p + "out_proj.weight"], sd[p + "out_proj.bias"])


def _ln(x, sd, p):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + LN_EPS) * sd[p + ".weight"] + sd[p + ".bias"]


def _layer(A, tgt, memory, sd, p, r_kpm, quirk, enc_kpm, m_pos, last):
    """planning_decoder.py:42-86 on tgt (bs, R, 12, 128)."""
    mut = A.mut
    bs, R = tgt.shape[:2]
    # ---- r2r: the R lines of one (scene, mode), key padding = the quirk row
    x = tgt.transpose(1, 2).reshape(bs * M, R, D)
    h = _ln(x, sd, p + "norm1")
    mask = quirk
    if mut == "r2r_own_row":
        mask = r_kpm.repeat_interleave(M, 0)
    if mut == "r2r_no_mask":
        mask = None
    if mut == "r2r_next_scene":
        mask = r_kpm[(torch.arange(bs * M) + 1) % bs]
    if mut == "r2r_dense_slots8":
        mask = mask | (torch.arange(R) >= 8)[None, :]
    rows = torch.arange(bs * M) ^ 1 if mut == "r2r_mode_pair_swapped" else None
    x = x + A.mha(sd, p + "r2r_attn.", h, h, h, mask, kv_rows=rows)
    # ---- m2m: the twelve modes of one line; q = k = h + m_pos, v = h; the rows of padded lines become zero
    x = x.reshape(bs, M, R, D).transpose(1, 2).reshape(bs * R, M, D)
    h = _ln(x, sd, p + "norm2")
    mp = {"m2m_pos_dropped": m_pos * 0.0, "m2m_pos_rolled": m_pos.roll(1, 0)}.get(mut, m_pos)
    rows = (torch.arange(bs * R) + 1) % (bs * R) if mut == "m2m_neighbour_line" else None
    y = x + A.mha(sd, p + "m2m_attn.", h + mp, h + mp, h + mp if mut == "m2m_pos_on_v" else h, kv_rows=rows)
    pad = r_kpm.reshape(-1, 1, 1)
    x = torch.where(pad, x if mut == "m2m_padded_keep_r2r" else torch.zeros_like(x), y).reshape(bs, R * M, D)
    # ---- cross attention against the scene's tokens
    N = memory.shape[1]
    valid = ~enc_kpm
    mask = enc_kpm
    if mut == "x_no_padding":
        mask = None
    if mut == "x_last_valid_masked":                    # (a scene with a single valid key keeps it)
        lastv = (valid * torch.arange(1, N + 1)).argmax(1)
        mask = enc_kpm.clone()
        mask[torch.arange(bs)[valid.sum(1) > 1], lastv[valid.sum(1) > 1]] = True
    if mut == "x_first_padded_admitted":
        first = (enc_kpm * torch.arange(N, 0, -1)).argmax(1)
        mask = enc_kpm.clone()
        mask[torch.arange(bs)[enc_kpm.any(1)], first[enc_kpm.any(1)]] = False
    for e in EDGES:
        if mut == f"x_edge_{e}":
            mask = enc_kpm | (torch.arange(N) >= e)[None, :]
    h = _ln(x, sd, p + "norm3")
    x = x + A.mha(sd, p + "cross_attn.", h, memory, memory, mask, scale=mut != "x_no_scale",
                  k_heads=[2, 3, 0, 1] if mut == "x_k_head_pairs_swapped" else None)
    # ---- FFN
    h = _ln(x, sd, p + ("norm3" if mut == "norm3_for_norm4" else "norm4"))
    x = x + A.lin(torch.relu(A.lin(h, sd[p + "ffn.0.weight"], sd[p + "ffn.0.bias"])), sd[p + "ffn.3.weight"], sd[p + "ffn.3.bias"])
    x = x.reshape(bs, R, M, D)
    if mut == "m2m_padded_stay_zero" and not last:
        x = torch.where(r_kpm[:, :, None, None], torch.zeros_like(x), x)
    return x


def reference64(sd, r_emb, enc_out, enc_kpm, r_kpm, quirk=None, fmt=None, mut=None):
    """{tap: fp64 (bs, R, 12, 128)} for q0, dec0..dec3, q_final.  sd: the model's state dict; r_emb (bs, R, 128); enc_out (bs, N, 128);
    enc_kpm (bs, N), r_kpm (bs, R) bool, True = padded; quirk (bs * 12, R): the padding row of every (scene, mode), default quirk_rows."""
    A = _R(fmt, mut)
    sd = {k: v.double() for k, v in sd.items() if k.startswith(PD) and v.is_floating_point()}
    r_emb, enc_out = r_emb.double(), enc_out.double()
    bs, R = r_emb.shape[:2]
    quirk = quirk_rows(r_kpm) if quirk is None else quirk
    halves = [r_emb[:, :, None, :].expand(bs, R, M, D), sd[PD + "m_emb"].reshape(1, 1, M, D).expand(bs, R, M, D)]
    q = A.lin(torch.cat(halves[::-1] if mut == "qproj_halves_swapped" else halves, -1), sd[PD + "q_proj.weight"], sd[PD + "q_proj.bias"])
    taps = {"q0": q}
    m_pos = sd[PD + "m_pos"].reshape(M, D)
    for i in range(4):
        q = _layer(A, q, enc_out, sd, f"{PD}decoder_blocks.{i}.", r_kpm, quirk, enc_kpm, m_pos, i == 3)
        taps[f"dec{i}"] = q
    ego = enc_out[(torch.arange(bs) + 1) % bs, 0] if mut == "catx_ego_next_scene" else enc_out[:, 0]
    halves = [q, ego[:, None, None, :].expand(bs, R, M, D)]
    taps["q_final"] = A.lin(torch.cat(halves[::-1] if mut == "catx_halves_swapped" else halves, -1), sd[PD + "cat_x_proj.weight"],
                            sd[PD + "cat_x_proj.bias"])
    return taps


def max_shift(a, b, rows=None, taps=ALL_TAPS):
    """{tap: max |a - b| over the rows (bs, R) bool, all rows by default}; a non-finite difference counts as infinite."""
    out = {}
    for k in taps:
        if k in a and k in b:
            d = (a[k] - b[k]).abs() if rows is None else (a[k][rows] - b[k][rows]).abs()
            out[k] = float(torch.nan_to_num(d, nan=float("inf")).max()) if d.numel() else 0.0
    return out


def emu_error(sd, r_emb, enc_out, enc_kpm, r_kpm, ref=None, quirk=None):
    """E_emu of these inputs: {(tap, fmt): max |emulation - fp64| over all rows}."""
    ref = reference64(sd, r_emb, enc_out, enc_kpm, r_kpm, quirk) if ref is None else ref
    return {(k, fmt): d for fmt in FMT for k, d in max_shift(reference64(sd, r_emb, enc_out, enc_kpm, r_kpm, quirk, fmt), ref).items()}


_r, _e = {}, {}


def case_reference(name):
    """The fp64 reference of a case on the oracle's r_emb / enc_out under case_weights()."""
    if name not in _r:
        r_emb, enc_out, kpm, r_kpm, _ = oracle_inputs(name)
        _r[name] = reference64(case_weights(), r_emb, enc_out, kpm, r_kpm)
    return _r[name]


def case_emu_error(name):
    if name not in _e:
        r_emb, enc_out, kpm, r_kpm, _ = oracle_inputs(name)
        _e[name] = emu_error(case_weights(), r_emb, enc_out, kpm, r_kpm, case_reference(name))
    return _e[name]
