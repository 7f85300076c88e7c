"""Designed inputs, the fp64 reference, its 16-bit operand emulation, its mutants and the pack-table invariants for the two PointsEncoders
(map polygons: 20 points, 10 features; reference lines: 120 points, 6 features -- pe_fused.h, pe_w.hip): what
tests/test_gpu_points_encoder.py compares the engine's pe_* taps with, and what tests/test_points_cases.py checks on the CPU.  No GPU import.

The reference restates oracle/pluto_ref.py's `points_encoder` / `batch_norm` in fp64 for both encoders ("a" polygons, "b" lines) and returns
what the passes hand to one another:
    s1, t1 (128,), s2, t2 (256,): the folded BatchNorm affines y = x s + t | gp (groups, 256) = pooled W3b^T + b3 | g (groups, n, 256): the
    second_mlp.0 pre-activation, defined on valid rows | out (groups, 128): defined for ALL groups, 0 for a group without a valid point |
    train mode: rm1, rv1, rm2, rv2 = the new running statistics (momentum 0.1, unbiased variance n / max(n - 1, 1)), nbt1, nbt2.
`fmt` = "bf16" / "fp16" rounds BOTH operands of every contraction to that format and nothing else (history_cases' method):
E_emu[case, mode, tap, fmt] = max |emulation - fp64| is the yardstick of the device bars.  `mut` names ONE wrong restatement (MUTANTS): the
CPU test asserts that each moves a compared tap by at least three device bars."""
import torch

from rift_amd import synthetic as syn
from tests import helpers as H

PE = {"a": "map_encoder.polygon_encoder.", "b": "planning_decoder.r_encoder."}
ROUND_GROUPS = {"a": 12, "b": 2}           # polylines of a 240-row round of pass B (reference lines: of the unpacked walk)
BN_EPS = 1e-5
FMT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TAPS = ("s1", "t1", "s2", "t2", "gp", "g", "out")
STAT_TAPS = ("rm1", "rv1", "rm2", "rv2")
# The device bar of a tap is K[fmt] * E_emu[case, mode, tap, fmt]: one factor per format for all taps, cases and builds = twice the worst
# measured device-error / E_emu ratio, rounded up, and never more than 6 (the rule of history_cases.K).  Measured on MI355X over all taps,
# cases, modes and builds (profiles/NOTES_r20.md): bf16 1.13, fp16 1.79.
K = {"bf16": 3, "fp16": 4}
# s*, t* (and the running statistics) come out of an fp32 finalize whatever the operand format -- var + eps, rsqrtf, * gamma, beta - mean * s:
# four roundings of half an ulp each plus rsqrtf's own ulp, on values no larger than the tap's largest: 8 ulp of fp32 cover it.  In eval
# mode no contraction stands in front of them (E_emu = 0) and this floor is their whole bar.
FP32_ULPS = 8.0


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _scenes(seed0, n, Mp, R, A=4):
    """n scenes of A agents, Mp polygon slots and R reference-line slots.  Every point of every polyline carries geometry (the generator
    zeroes a line behind its valid prefix): what stands in an invalid row is a value the encoder must not let through."""
    data = syn.collate_scenes([syn.make_scene(seed0 + i, A, Mp, R, R) for i in range(n)])["cur_pluto_feature_torch"]
    g = torch.Generator().manual_seed(seed0)
    rl = data["reference_line"]
    a0, k0 = torch.randn(n, R, generator=g) * 0.3, torch.randn(n, R, generator=g) * 0.01
    th = a0[..., None] + k0[..., None] * torch.arange(120, dtype=torch.float32)
    step = torch.stack([th.cos(), th.sin()], -1)
    pos = torch.randn(n, R, 1, 2, generator=g) * 2.0 + torch.cumsum(step, dim=2)
    rl["position"] = pos.float().contiguous()
    rl["vector"] = torch.cat([pos[:, :, 1:] - pos[:, :, :-1], pos[:, :, -1:] - pos[:, :, -2:-1]], dim=2).float().contiguous()
    rl["orientation"] = th.float().contiguous()
    rl["valid_mask"] = torch.zeros(n, R, 120, dtype=torch.bool)
    return data


def _prefix(v, length):
    v[:] = False
    v[:length] = True


ENDS_FULL_LINE, ENDS_PART_LINE, ENDS_PART_POLY = 14, 8, 4


def _ends():
    """3 scenes x 7 polygon slots x 5 line slots: nP = 21 -> 420 rows (pass B: rounds of 240 + 180; passes A and C: tiles 120, 120, 120, 60;
    polygon boundaries inside 16-row tiles), nL = 15."""
    data = _scenes(9500, 3, 7, 5)
    pv = data["map"]["valid_mask"].view(21, 20)
    pv[0] = True
    pv[1] = False
    pv[2] = False; pv[2, 0] = True
    pv[3] = False; pv[3, 19] = True
    pv[4] = False; pv[4, 4:16] = True
    pv[5] = False; pv[5, 0::2] = True
    pv[20, 19] = True                       # the batch's last row is a valid point
    lv = data["reference_line"]["valid_mask"].view(15, 120)
    lv[0] = True
    for l, last in ((1, 15), (2, 16), (3, 111), (4, 112)):      # both sides of (last + 16) >> 4
        _prefix(lv[l], last + 1)
    lv[5, 119] = True
    lv[6, 0] = True
    # lv[7]: no valid point
    _prefix(lv[8], 60); lv[8, 7] = False; lv[8, 32:48] = False
    lv[9, 104:120] = True
    lv[10, 0::2] = True
    _prefix(lv[11], 45); _prefix(lv[12], 77); _prefix(lv[13], 100)
    lv[14] = True                           # the batch's last line: rows 120..127 of its eighth tile lie past the feature buffer
    return data


def _rounds():
    """4 scenes x 10 polygon slots x 2 line slots: nP = 40 -> 800 rows = three 240-row rounds + 80.  Polygons 12..23 dead: round 1 is dead,
    the live list is {0, 2, 3}; 24..29 dead: a dead 120-row tile inside live round 2.  Line 5 dead: the unpacked round of lines 4, 5 is
    half dead.  Few valid points (66 / 78): BatchNorm's n / (n - 1) stays visible, the batch variance stays well defined."""
    data = _scenes(9600, 4, 10, 2)
    pv = data["map"]["valid_mask"].view(40, 20)
    pv[:] = False
    for i in list(range(0, 12)) + list(range(30, 40)):
        pv[i, i % 5] = True; pv[i, 7 + i % 3] = True; pv[i, 19 - i % 4] = True
    lv = data["reference_line"]["valid_mask"].view(8, 120)
    for l, n in enumerate((12, 9, 20, 7, 11, 0, 5, 14)):
        _prefix(lv[l], n)
    return data


def _segments(long):
    """11 scenes x 9 line slots: nL = 99 -> three packing segments of 33 lines (pe_fused.h: pe_pack_nseg / pe_pack_per); one polygon slot."""
    data = _scenes(9700, 11, 1, 9)
    lv = data["reference_line"]["valid_mask"].view(99, 120)
    for l in range(99):
        if long:                            # 7 or 8 tiles each: two lines fill a round, every segment ends on a one-line round -> 51 records
            _prefix(lv[l], 97 + (7 * l) % 24)
        elif l not in (32, 33, 65, 66, 98):                     # (the segment ends hold lines without a valid point)
            _prefix(lv[l], 16 * ((5 * l) % 8) + 1 + (3 * l) % 16)
    return data


CASES = {"ends": _ends, "rounds": _rounds, "segments_long": lambda: _segments(True), "segments_mixed": lambda: _segments(False)}
_c = {}


def case(name):
    if name not in _c:
        _c[name] = CASES[name]()
    return _c[name]


def features(data):
    """{encoder: (x (groups, n, C) fp64, mask (groups, n))} -- map_encoder.py:43-59, planning_decoder.py:139-153 on the fp32 inputs."""
    mp, rl = data["map"], data["reference_line"]
    pp, pv, po, c = (mp[k].double() for k in ("point_position", "point_vector", "point_orientation", "polygon_center"))
    xa = torch.cat([pp[:, :, 0] - c[..., None, :2], pv[:, :, 0], torch.stack([po[:, :, 0].cos(), po[:, :, 0].sin()], dim=-1),
                    pp[:, :, 1] - pp[:, :, 0], pp[:, :, 2] - pp[:, :, 0]], dim=-1)
    rp, rv, ro = (rl[k].double() for k in ("position", "vector", "orientation"))
    xb = torch.cat([rp - rp[..., 0:1, :2], rv, torch.stack([ro.cos(), ro.sin()], dim=-1)], dim=-1)
    return {"a": (xa.reshape(-1, 20, 10), mp["valid_mask"].reshape(-1, 20)), "b": (xb.reshape(-1, 120, 6), rl["valid_mask"].reshape(-1, 120))}


def tiles_per_line(mask_b):
    """16-row tiles of every line up to its LAST valid point, 0 .. 8 (kernels.h: refline_mask_body)."""
    idx = torch.arange(120)
    last = torch.where(mask_b, idx, torch.full_like(idx, -1)).amax(-1)
    return ((last + 16) >> 4).tolist()


def live_rounds(mask, e):
    """The 240-row rounds of the unpacked walk that hold a valid point."""
    g = ROUND_GROUPS[e]
    has = mask.any(-1)
    return [r for r in range((has.numel() + g - 1) // g) if bool(has[r * g:(r + 1) * g].any())]


# ---------------------------------------------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------------------------------------------
B2_SHIFT, B4_SHIFT = 3.0, 4.0
_w = {}


def case_weights():
    """perturbed_state_dict with, for both encoders: first_mlp.3.bias / second_mlp.3.bias shifted by -S, 0, +S on the channels c % 3 =
    0, 1, 2 (each max-pool then has channels whose valid values are all negative, of mixed sign, all positive: "a zero row takes part in
    the max" and "no zero row exists" differ); the running statistics of the four BatchNorms set from the batch statistics of `ends`
    (0.8 mean + 0.1, 1.6 var): of the right magnitude, visibly not the batch's; first_mlp.0.weight exact in bf16 and fp16 (below).  r_pos_emb.to_out.2 is zeroed: the tap `r_pe` shares its
    buffer with r_emb, which the reference-line position embedding is added into -- with a zero embedding it reads the encoder's output."""
    if "sd" not in _w:
        sd = {k: v.clone() for k, v in H.weights().items()}
        hit = 0
        for p in PE.values():
            for name, amp in (("first_mlp.3.bias", B2_SHIFT), ("second_mlp.3.bias", B4_SHIFT)):
                b = sd[p + name]
                sd[p + name] = b + (torch.arange(b.numel()) % 3 - 1).float() * amp
                hit += 1
            # first_mlp.0.weight exact in both 16-bit formats: a rounded weight is the SAME error on every row, which the BatchNorm-1
            # statistics keep whole while the rows' own rounding averages out -- without it E_emu of s1 / rv1 hides 1 / n of a variance
            w = sd[p + "first_mlp.0.weight"].bfloat16().float().half().float()
            assert torch.equal(w.bfloat16().float(), w) and torch.equal(w.half().float(), w)
            sd[p + "first_mlp.0.weight"] = w
            hit += 1
        for k in ("planning_decoder.r_pos_emb.to_out.2.weight", "planning_decoder.r_pos_emb.to_out.2.bias"):
            sd[k] = torch.zeros_like(sd[k])
            hit += 1
        ref = reference(case("ends"), sd, True, keep_stats=True)
        for e, p in PE.items():
            for i, bn in ((1, "first_mlp.1"), (2, "second_mlp.1")):
                mean, var = ref[e][f"_mean{i}"], ref[e][f"_var{i}"]
                assert sd[p + bn + ".running_mean"].shape == mean.shape
                sd[p + bn + ".running_mean"] = (0.8 * mean + 0.1).float()
                sd[p + bn + ".running_var"] = (1.6 * var).float()
                hit += 2
        assert hit == 16, hit
        _w["sd"] = sd
    return _w["sd"]


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 reference, operand emulation, mutants
# ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("max2_no_zero_row", "max1_no_zero_row", "full_line_zero_row", "tiles_last_shift", "poly_neighbour_max1", "poly_neighbour_max2",
           "gp_previous", "bn_all_rows", "bn_var_swapped", "bn_wrong_mode", "w3_swapped", "invalid_not_zeroed2")
TRAIN_ONLY = ("bn_all_rows", "bn_var_swapped")          # (mutants of the batch statistics: nothing to see in eval mode)


class _R:
    def __init__(self, fmt, mut):
        assert mut is None or mut in MUTANTS, mut
        self.fmt, self.mut = fmt, mut

    def r(self, x):
        return x if self.fmt is None else x.float().to(FMT[self.fmt]).double()

    def lin(self, x, w, b=None):
        y = self.r(x) @ self.r(w).t()
        return y if b is None else y + b


def _bn(R, x_valid, x_all, sd, p, train):
    """(s, t, stats): nn.BatchNorm1d over the valid rows folded to y = x s + t; stats = batch mean / biased variance / the new running
    statistics in train mode."""
    w, b, rm, rv = (sd[p + k].double() for k in (".weight", ".bias", ".running_mean", ".running_var"))
    xs = x_all if R.mut == "bn_all_rows" else x_valid
    n = xs.shape[0]
    mean, var = xs.mean(0), xs.var(0, unbiased=False)
    unb = var * n / max(n - 1, 1)
    if R.mut == "bn_var_swapped":
        var, unb = unb, var
    st = {"mean": mean, "var": var}
    if train:
        st.update(rm=0.9 * rm + 0.1 * mean, rv=0.9 * rv + 0.1 * unb, nbt=int(sd[p + ".num_batches_tracked"]) + 1)
    batch = train != (R.mut == "bn_wrong_mode")
    m, v = (mean, var) if batch else (rm, rv)
    s = w / torch.sqrt(v + BN_EPS)
    return s, b - m * s, st


def _pool(R, z, mask, e, which):
    """max over the points of a polyline; z (groups, n, C) holds zero rows at the invalid points (embedding.py:282-293)."""
    G, n, C = z.shape
    any_ = mask.any(-1)
    if R.mut == f"max{which}_no_zero_row":             # invalid points left out of the max (a group without a valid point stays 0)
        m = z.masked_fill(~mask[..., None], float("-inf")).amax(1)
        return torch.where(any_[:, None], m, torch.zeros(()).double())
    if R.mut == f"poly_neighbour_max{which}" and e == "a":          # points 0..20: the next polygon's first row leaks in
        flat = torch.cat([z.reshape(G * n, C), z.new_zeros(1, C)])
        return torch.stack([flat[i * n:i * n + n + 1].amax(0) for i in range(G)])
    if R.mut == "tiles_last_shift" and e == "b":       # tiles counted as last >> 4: the rows of the last partial tile are dropped (zero rows)
        idx = torch.arange(n)
        last = torch.where(mask, idx, torch.full_like(idx, -1)).amax(-1)
        keep = idx[None, :] < 16 * (last.clamp(min=0) >> 4)[:, None]
        return z.masked_fill(~keep[..., None], 0.0).amax(1)
    out = z.amax(1)
    if R.mut == "full_line_zero_row" and e == "b" and which == 2:   # rows 120..127 of the eighth tile taken for zero rows
        out = out.clamp(min=0.0)
    return out


def _encoder(R, x, mask, sd, p, e, train):
    G, n, _ = x.shape
    W1, b1, W2, b2, W3, b3, W4, b4 = (sd[p + k].double() for k in (
        "first_mlp.0.weight", "first_mlp.0.bias", "first_mlp.3.weight", "first_mlp.3.bias", "second_mlp.0.weight", "second_mlp.0.bias",
        "second_mlp.3.weight", "second_mlp.3.bias"))
    h1 = R.lin(x, W1, b1)                                          # (G, n, 128), rows of invalid points computed and never used
    s1, t1, st1 = _bn(R, h1[mask], h1.reshape(G * n, -1), sd, p + "first_mlp.1", train)
    f = R.lin(torch.relu(h1 * s1 + t1), W2, b2)
    feat = torch.where(mask[..., None], f, torch.zeros(()).double())
    pooled = _pool(R, feat, mask, e, 1)
    W3a, W3b = W3[:, :256], W3[:, 256:]                            # cat([feat, pooled]): the pooled half are the LAST 256 columns
    if R.mut == "w3_swapped":
        W3a, W3b = W3b, W3a
    gp = R.lin(pooled, W3b) + b3
    gpu = gp
    if R.mut == "gp_previous":                                     # gp of the previous polyline of the round
        i = torch.arange(G)
        gpu = gp[torch.where(i % ROUND_GROUPS[e] != 0, i - 1, i)]
    g = R.lin(feat, W3a) + gpu[:, None]
    s2, t2, st2 = _bn(R, g[mask], g.reshape(G * n, -1), sd, p + "second_mlp.1", train)
    o = R.lin(torch.relu(g * s2 + t2), W4, b4)
    res = o if R.mut == "invalid_not_zeroed2" else torch.where(mask[..., None], o, torch.zeros(()).double())
    out = _pool(R, res, mask, e, 2)
    taps = {"s1": s1, "t1": t1, "s2": s2, "t2": t2, "gp": gp, "g": g, "out": out, "_f": feat, "_o": res,
            "_mean1": st1["mean"], "_var1": st1["var"], "_mean2": st2["mean"], "_var2": st2["var"]}
    if train:
        taps.update(rm1=st1["rm"], rv1=st1["rv"], nbt1=st1["nbt"], rm2=st2["rm"], rv2=st2["rv"], nbt2=st2["nbt"])
    return taps


def reference(data, sd, train, fmt=None, mut=None, keep_stats=False):
    """{encoder: {tap: fp64 tensor}}; keep_stats: with the batch statistics and the second max's operand (`_mean1`, `_var1`, ..., `_o`)."""
    R = _R(fmt, mut)
    out = {}
    for e, (x, mask) in features(data).items():
        t = _encoder(R, x, mask, sd, PE[e], e, train)
        out[e] = t if keep_stats else {k: v for k, v in t.items() if not k.startswith("_")}
    return out


def compared(taps, data):
    """{tap_e: the part of a tap that is compared, flat}: g on the valid rows, gp on the groups with a valid point, the rest whole."""
    out = {}
    for e, (_, mask) in features(data).items():
        for k, v in taps[e].items():
            if k in TAPS + STAT_TAPS:
                out[f"{k}_{e}"] = v[mask] if k == "g" else (v[mask.any(-1)] if k == "gp" else v)
    return out


def max_shift(a, b, data):
    ca, cb = compared(a, data), compared(b, data)
    return {k: float((ca[k] - cb[k]).abs().max()) for k in ca if k in cb}


_r, _e = {}, {}


def reference64(name, train, keep_stats=False):
    key = (name, bool(train), keep_stats)
    if key not in _r:
        _r[key] = reference(case(name), case_weights(), train, keep_stats=keep_stats)
    return _r[key]


def emu_error(name, train):
    """E_emu[case, mode]: {(tap_e, fmt): max |emulation - fp64| over the compared part of the tap} (eval-mode s*, t*: 0)."""
    key = (name, bool(train))
    if key not in _e:
        data, sd = case(name), case_weights()
        ref = reference64(name, train)
        _e[key] = {(k, fmt): d for fmt in FMT for k, d in max_shift(reference(data, sd, train, fmt), ref, data).items()}
    return _e[key]


def fp32_floor(name, train, tap):
    """FP32_ULPS ulp of the tap's largest value, for the taps that an fp32 finalize writes (s*, t*, running statistics); 0 for the others."""
    if tap.split("_")[0] not in ("s1", "t1", "s2", "t2") + STAT_TAPS:
        return 0.0
    ref = compared(reference64(name, train), case(name))[tap]
    return FP32_ULPS * 2.0 ** -24 * max(1.0, float(ref.abs().max()))


def bar(name, train, tap, fmt):
    """The device bar of a tap (`s1_a`, `g_b`, ...) of a 16-bit build."""
    return K[fmt] * emu_error(name, train)[tap, fmt] + fp32_floor(name, train, tap)


# ---------------------------------------------------------------------------------------------------------------------------------
# the packed rounds of the reference lines (pe_fused.h: pe_pack_body)
# ---------------------------------------------------------------------------------------------------------------------------------
PACK_SEGS = 32


def pack_nseg(nlines):
    return min(PACK_SEGS, max(1, nlines // 32))


def pack_per(nlines):
    nseg = pack_nseg(nlines)
    return (nlines + nseg - 1) // nseg


def pack_max_rounds(nlines):
    """The table's records (pe_fused.h: pe_pack_max_rounds): every segment of n lines ends with at most ceil(n / 2) rounds."""
    return pack_nseg(nlines) * ((pack_per(nlines) + 1) // 2)


def pack_rounds(tiles):
    """The ROUND COUNT of pe_pack_body and nothing else: per segment, bounded-space first fit with three open rounds of 16 tiles /
    16 lines -- a line goes into the first open round with room, else the oldest is closed and a new one opened."""
    nl = len(tiles)
    per, total = pack_per(nl), 0
    for s in range(pack_nseg(nl)):
        open_ = []                                  # [tiles, lines] of the open rounds, oldest first
        for t in tiles[s * per:min(nl, (s + 1) * per)]:
            if t == 0:
                continue
            for o in open_:
                if o[0] + t <= 16 and o[1] < 16:
                    o[0] += t; o[1] += 1
                    break
            else:
                if len(open_) == 3:
                    open_.pop(0)
                open_.append([t, 1])
                total += 1
    return total


def check_pack_table(tiles, hdr, tab):
    """Invariants of the round table (hdr: ints, hdr[0] = records in use; tab: ints, 32 per record), not the first-fit order: every line
    with t > 0 tiles sits in exactly one record and slot, its t descriptors consecutive and in order; a line with t = 0 nowhere; at most
    16 tiles and 16 lines per record; unused entries -1 / 0; hdr[0] within the packing's bound."""
    nl = len(tiles)
    n = int(hdr[0])
    assert 0 <= n <= (nl + 1) // 2 + pack_nseg(nl), (n, nl)          # every closed round holds at least two lines (pe_fused.h)
    assert n <= pack_max_rounds(nl) and n * 32 <= len(tab), (n, pack_max_rounds(nl), len(tab))
    seen = {}
    for r in range(n):
        rec = [int(v) for v in tab[r * 32:r * 32 + 32]]
        used = [False] * 16
        nslot = 0
        for s in range(16):
            w = rec[16 + s]
            if w == 0:
                continue
            nslot += 1
            first, last, dropped, exists = w & 0xff, (w >> 8) & 0xff, (w >> 16) & 1, (w >> 17) & 1
            assert exists == 1 and w >> 18 == 0 and 0 <= first <= last < 16, (r, s, hex(w))
            d0 = rec[first]
            assert d0 >= 0 and (d0 >> 8) % 120 == 0, (r, s, d0)
            l = (d0 >> 8) // 120
            assert 0 <= l < nl and l not in seen, (r, s, l)
            seen[l] = (r, s)
            t = tiles[l]
            assert t > 0 and last - first + 1 == t and dropped == (1 if t < 8 else 0), (r, s, l, t, hex(w))
            for k in range(t):
                assert rec[first + k] == ((l * 120 + 16 * k) << 8) | (k << 4) | s, (r, s, l, k, rec[first + k])
                assert not used[first + k]
                used[first + k] = True
        assert nslot >= 1, f"record {r} holds no line"
        assert all(rec[i] == -1 for i in range(16) if not used[i]), (r, rec[:16])
    assert sorted(seen) == [l for l in range(nl) if tiles[l] > 0], "every line with a valid point sits in exactly one record"
    return n
