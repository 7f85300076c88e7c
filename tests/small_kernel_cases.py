"""Seeded inputs and plain fp64 restatements for the small kernels around the forward path (optimizer tail, gradient clip, reverse
scans, z-scores, rollout return, critic, PPO objective, other-vehicle forecast, SFT teacher label) at hyper-parameters and sizes
where every term and every edge of those kernels is numerically visible.  Shared by tests/test_small_kernel_cases.py (CPU: the
conditions the inputs must satisfy, checked on the references alone) and tests/test_gpu_small_kernels.py (the kernels against the
references).  Nothing here calls the library."""
import functools

import numpy as np
import torch

from oracle import advantage as oadv


def ulp32(x):
    """Spacing of fp32 at |x| (elementwise)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- 1. AdamW --------------------------------------------------------------------------------------------------------------------
ADAM_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 16384, 70001, 3, 129, 511, 2049)       # 16 tensors, 95 493 elements (> 65 536)
ADAM_BETAS, ADAM_EPS = (0.8, 0.95), 1e-3
ADAM_BASE_LR = (1.0e-2, 2.0e-2, 1.5e-2, 0.7e-2, 1.2e-2, 0.9e-2)                                   # one per step
ADAM_WD_CYCLE = (0.1, 0.0, 0.03)
PI_SHAPES = ((128, 128), (128,), (128,), (128,), (1, 128), (1,))                                  # W1 | b1 | ln_w | ln_b | w2 | b2 (the flat order)


def adam_lrs(step, n):
    """A different learning rate for every tensor, of the order of 1e-2, moving with the step."""
    return [ADAM_BASE_LR[step % len(ADAM_BASE_LR)] * (1.0 + 0.07 * i) for i in range(n)]


def adam_wds(n):
    return [ADAM_WD_CYCLE[i % 3] for i in range(n)]


@functools.lru_cache(maxsize=None)
def adam_case(sizes=ADAM_SIZES, steps=6, seed=9090):
    """init (fp32), grads[step][tensor] (fp32; scale 3.0 on even steps and 1e-4 on odd ones, a tenth of the entries exactly zero),
    lrs[step][tensor], wds[tensor]."""
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=g) * 0.5 for n in sizes]
    grads = []
    for k in range(steps):
        row = []
        for n in sizes:
            t = torch.randn(n, generator=g) * (3.0 if k % 2 == 0 else 1e-4)
            t[torch.rand(n, generator=g) < 0.1] = 0.0
            row.append(t)
        grads.append(row)
    return {"init": init, "grads": grads, "lrs": [adam_lrs(k, len(sizes)) for k in range(steps)], "wds": adam_wds(len(sizes))}


def adamw_step64(p, m, v, g, lr, wd, step, betas=ADAM_BETAS, eps=ADAM_EPS):
    """One step of torch.optim.AdamW (amsgrad False, maximize False, decoupled decay, torch's bias corrections) in fp64 numpy."""
    b1, b2 = betas
    p = p * (1.0 - lr * wd)
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def adamw_ref64(case, betas=ADAM_BETAS, eps=ADAM_EPS, lrs=None, wds=None):
    """The whole trajectory of `case` in fp64 from zero state: [(p, m, v)] per tensor after the last step."""
    lrs = case["lrs"] if lrs is None else lrs
    wds = case["wds"] if wds is None else wds
    out = []
    for i, p0 in enumerate(case["init"]):
        p = p0.double().numpy()
        m, v = np.zeros_like(p), np.zeros_like(p)
        for k, row in enumerate(case["grads"]):
            p, m, v = adamw_step64(p, m, v, row[i].double().numpy(), lrs[k][i], wds[i], k + 1, betas, eps)
        out.append((p, m, v))
    return out


def adamw_torch32(case, betas=ADAM_BETAS, eps=ADAM_EPS):
    """torch's own fp32 CPU AdamW (foreach=False, one parameter group per tensor) on the same inputs."""
    ps = [torch.nn.Parameter(t.clone()) for t in case["init"]]
    opt = torch.optim.AdamW([{"params": [p], "lr": case["lrs"][0][i], "weight_decay": case["wds"][i]} for i, p in enumerate(ps)],
                            lr=1e-2, betas=betas, eps=eps, foreach=False)
    for k, row in enumerate(case["grads"]):
        for i, (p, grp) in enumerate(zip(ps, opt.param_groups)):
            grp["lr"] = case["lrs"][k][i]
            p.grad = row[i].clone()
        opt.step()
    return [(p.detach().double().numpy(), opt.state[p]["exp_avg"].double().numpy(), opt.state[p]["exp_avg_sq"].double().numpy()) for p in ps]


def adam_bars(ref, t32):
    """Per quantity (parameters, exp_avg, exp_avg_sq): the distance D between torch's fp32 CPU AdamW and the fp64 restatement over all
    tensors, and the per-tensor bars max(4 D, four fp32 ulps of the tensor's largest magnitude)."""
    dist = [max(float(np.max(np.abs(r[q] - t[q]))) for r, t in zip(ref, t32)) for q in range(3)]
    bars = [[max(4.0 * dist[q], 4.0 * float(ulp32(np.max(np.abs(r[q]))))) for q in range(3)] for r in ref]
    return dist, bars


# ---- 1b. the fused tail: finalize + clip + AdamW of the six pi_head tensors ---------------------------------------------------------
PI_NPARAM = 16897
TAIL_CNT, TAIL_S, TAIL_MAX_NORM = 4242.0, -37.25, 0.5
TAIL_ORDER = (4, 0, 5, 2, 1, 3)             # position in the AdamW list -> gradient segment: a shuffled list (the header allows any order)
# (accumulate, exchange buffer, flat-sum scale per step): every configuration sees a clipped and a passed-through step
TAIL_CONFIGS = ((0, False, (40.0, 10.0, 40.0)), (1, False, (10.0, 40.0, 1.0)), (0, True, (5.0, 20.0, 5.0)), (1, True, (5.0, 20.0, 0.5)))


@functools.lru_cache(maxsize=None)
def tail_case(config, seed=4711):
    """Three consecutive steps of the update tail.  flat[k]: the fp32 gradient sums of step k; prev: the .grad tensors before step 0
    (read when accumulating); init: the parameters; per-segment lr / weight decay as in adam_case."""
    acc, use_x, scales = TAIL_CONFIGS[config]
    g = torch.Generator().manual_seed(seed + config)
    numel = [int(np.prod(s)) for s in PI_SHAPES]
    return {"accumulate": acc, "xchg": use_x, "flat": [torch.randn(PI_NPARAM, generator=g) * s for s in scales],
            "prev": [torch.randn(n, generator=g) * 1e-3 for n in numel], "init": [torch.randn(n, generator=g) * 0.5 for n in numel],
            "lrs": [adam_lrs(k, 6) for k in range(3)], "wds": adam_wds(6)}


def tail_sums(case, k):
    """(gradient sums as the kernel reads them, objective sum, count) of step k: from the f64 exchange buffer -- which holds twice the
    local sums, as after an all-reduce over two equal shards -- when the case uses one."""
    flat = case["flat"][k].double().numpy()
    if case["xchg"]:
        return (2.0 * flat).astype(np.float32).astype(np.float64), 2.0 * TAIL_S, 2.0 * TAIL_CNT
    return flat, TAIL_S, TAIL_CNT


def tail_ref(case, fp32=False):
    """finalize (grads = -sum / count, + the existing .grad when accumulating), clip_grad_norm_(0.5), AdamW -- three steps from zero
    optimizer state.  fp64 throughout, or (fp32=True) with torch's fp32 CPU operations: the yardstick for the bar.
    Returns per segment (p, m, v, clipped grad) and per step (loss, total norm)."""
    dt = torch.float32 if fp32 else torch.float64
    seg = np.cumsum([0] + [int(np.prod(s)) for s in PI_SHAPES])
    p = [t.to(dt).clone() for t in case["init"]]
    grad = [t.to(dt).clone() for t in case["prev"]]
    per_step = []
    if fp32:
        params = [torch.nn.Parameter(t) for t in p]
        opt = torch.optim.AdamW([{"params": [q], "weight_decay": case["wds"][i]} for i, q in enumerate(params)], lr=1e-2, betas=ADAM_BETAS,
                                eps=ADAM_EPS, foreach=False)
    else:
        m = [np.zeros(t.numel()) for t in p]
        v = [np.zeros(t.numel()) for t in p]
        p = [t.numpy() for t in p]
    for k in range(3):
        flat, S, cnt = tail_sums(case, k)
        sc = torch.tensor(-1.0 / cnt, dtype=dt)
        new = [torch.from_numpy(flat[seg[i]:seg[i + 1]]).to(dt) * sc for i in range(6)]
        grad = [n + g if case["accumulate"] else n for n, g in zip(new, grad)]
        total = torch.sqrt(sum((g.double() ** 2).sum() for g in grad)).to(dt)
        coef = torch.clamp(TAIL_MAX_NORM / (total + 1e-6), max=1.0)
        grad = [g * coef for g in grad]
        per_step.append((-S / cnt, float(total)))
        if fp32:
            for i, (q, grp) in enumerate(zip(params, opt.param_groups)):
                grp["lr"] = case["lrs"][k][i]
                q.grad = grad[i].clone()
            opt.step()
        else:
            for i in range(6):
                p[i], m[i], v[i] = adamw_step64(p[i], m[i], v[i], grad[i].numpy(), case["lrs"][k][i], case["wds"][i], k + 1)
    if fp32:
        out = [(q.detach().double().numpy(), opt.state[q]["exp_avg"].double().numpy(), opt.state[q]["exp_avg_sq"].double().numpy(),
                grad[i].double().numpy()) for i, q in enumerate(params)]
    else:
        out = [(p[i], m[i], v[i], grad[i].numpy()) for i in range(6)]
    return out, per_step


# ---- 2. gradient clip ---------------------------------------------------------------------------------------------------------------
CLIP_SIZES = (1, 3, 63, 65, 127, 255, 257, 999, 1001, 2047, 2049, 4097, 8191, 16385, 30001, 5)     # 16 odd sizes, several 2048-element blocks
CLIP_MAX_NORM = 0.5


@functools.lru_cache(maxsize=None)
def clip_case(rel, seed=2121):
    """16 fp32 gradient tensors whose fp64 total norm is CLIP_MAX_NORM * (1 + rel) (to fp32 rounding of the entries); rel None: all zero."""
    g = torch.Generator().manual_seed(seed)
    ts = [torch.randn(n, generator=g) for n in CLIP_SIZES]
    if rel is None:
        return [torch.zeros_like(t) for t in ts]
    norm = float(np.sqrt(sum(float((t.double() ** 2).sum()) for t in ts)))
    return [(t.double() * (CLIP_MAX_NORM * (1.0 + rel) / norm)).float() for t in ts]


def clip_ref64(grads, max_norm=CLIP_MAX_NORM):
    """torch.nn.utils.clip_grad_norm_ (norm_type 2) in fp64: (total norm, clipped gradients)."""
    g64 = [t.double().numpy() for t in grads]
    total = float(np.sqrt(sum(float((a * a).sum()) for a in g64)))
    coef = min(max_norm / (total + 1e-6), 1.0)
    return total, [a * coef for a in g64]


# ---- 3. reverse scans ---------------------------------------------------------------------------------------------------------------
SCAN_NS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 4095, 4097, 20011)
SCAN_RATES = (0.05, 0.5)
SCAN_GAMMA, SCAN_LAMBDA = 0.9, 0.6
SCAN_THREADS = 1024


def forced_ends(n):
    """Episode ends at index 0, at n - 1 and on both sides of every 97th chunk boundary of the one-workgroup scan (chunk = ceil(n / 1024))."""
    ch = -(-n // SCAN_THREADS)
    idx = {0, n - 1}
    b = 97 * ch
    while b < n:
        idx.update((b - 1, b))
        b += 97 * ch
    return sorted(idx)


@functools.lru_cache(maxsize=None)
def scan_inputs(n, rate, seed=1357):
    g = torch.Generator().manual_seed(seed + n + int(rate * 1000))
    rewards = torch.randn(n, generator=g, dtype=torch.float64)
    done = torch.rand(n, generator=g) < rate
    done[forced_ends(n)] = True
    term = done & (torch.rand(n, generator=g) < 0.4)            # a terminated step is done; a done step is terminated 40 % of the time
    return {"rewards": rewards, "dones": done.float(), "undones": 1.0 - done.float(), "unterminated": 1.0 - term.float(),
            "values": torch.randn(n, generator=g), "next_values": torch.randn(n, generator=g)}


@functools.lru_cache(maxsize=None)
def gae_ref(n, rate, gamma=SCAN_GAMMA, lambda_=SCAN_LAMBDA, exchange_masks=False):
    i = scan_inputs(n, rate)
    ud, ut = (i["unterminated"], i["undones"]) if exchange_masks else (i["undones"], i["unterminated"])
    return oadv.get_advantages_gae(i["rewards"], ud, i["values"], i["next_values"], ut, gamma, lambda_)


@functools.lru_cache(maxsize=None)
def return_ref(n, rate, gamma=SCAN_GAMMA):
    i = scan_inputs(n, rate)
    return oadv.compute_return(i["rewards"], i["dones"], gamma)


# ---- 4. z-scores --------------------------------------------------------------------------------------------------------------------
NORM_NS = (2, 3, 255, 256, 257, 1000, 4099)
GROUP_GS = (1, 2, 12, 13, 63, 64, 65, 127, 192, 193)
GROUP_NS = (1, 3, 4, 5, 9)


def normalize_input(n, shifted, seed=8642):
    g = torch.Generator().manual_seed(seed + n)
    x = torch.randn(n, generator=g)
    return (8.0 + 0.5 * x) if shifted else x


def normalize_ref64(x):
    """(x - mean) / (unbiased std + 1e-5) in fp64 on the fp32 inputs, and the bar of the fp32 kernel.
    The kernel (like torch) forms mean and variance, rounds the mean to fp32 (error <= ulp32(|mean|) / 2), subtracts in fp32 (each
    difference rounds by <= ulp32(max |x - mean|) / 2, and the rounded mean moves it by the first term; 2 ulps allow for both
    roundings landing in the next binade), divides by an fp32 denominator (fp32 sqrt, fp32 + 1e-5f: relative 2^-23 together) and rounds
    the quotient (half an ulp): the last two are the two fp32 ulps of the result."""
    a = x.double().numpy()
    mean, std = a.mean(), a.std(ddof=1)
    ref = (a - mean) / (std + 1e-5)
    bar = (ulp32(abs(mean)) / 2 + 2 * ulp32(np.max(np.abs(a - mean)))) / (std + 1e-5) + 2 * ulp32(ref)
    return ref, bar


def group_input(n_groups, G, shifted, seed=97531):
    g = torch.Generator().manual_seed(seed + 1000 * n_groups + G)
    x = torch.randn(n_groups, G, generator=g, dtype=torch.float64)
    return (-300.0 + 0.5 * x) if shifted else x


def group_ref(ret):
    return np.stack([oadv.group_zscore(row) for row in ret.numpy()])


# ---- 5. rollout return --------------------------------------------------------------------------------------------------------------
RR_TS = (1, 39, 40, 63, 64, 65, 130)
RR_GS = (1, 3, 4, 5, 9)
RR_GAMMA = 0.93
RR_MARGIN = 1e-5
# collision steps of a row, by placement (a step beyond the horizon is dropped; "last" = Ts - 1, "round2" = the last step of the second round)
RR_PLACEMENTS = ((), (0,), ("last",), (63,), (64,), (65,), (64, 70), ("round2",))


def _away(a, centre, margin=RR_MARGIN):
    """Move the entries of |a| that lie within 10 margins of `centre` to 1e-3 above it (keeps their sign)."""
    near = np.abs(np.abs(a) - centre) < 10 * margin
    a[near] = np.sign(a[near]) * np.float32(centre + 1e-3)
    return a


@functools.lru_cache(maxsize=None)
def rollout_return_case(G, Ts, shift=0, seed=60606):
    """Inputs of rift_rollout_return: six (G, Ts) fp32 arrays, collision (G, Ts + 7) and off_road (G, 2 Ts + 3) -- WIDER than the horizon, the
    columns beyond it all set, so that both row strides differ from Ts and a read past the horizon shows.  Row i takes collision
    placement (i + shift) % 8."""
    g = torch.Generator().manual_seed(seed + 1000 * G + Ts)
    f = lambda s: (torch.randn(G, Ts, generator=g) * s).numpy()  # noqa: E731
    c = {"delta_dis": f(1.5), "delta_angle": f(0.8), "speed": f(6.0) + np.float32(5.0), "acc": f(3.0), "ang_vel": f(0.5), "ang_acc": f(3.0)}
    _away(c["acc"], 4.0); _away(c["ang_acc"], 4.0); _away(c["speed"], 3.0); _away(c["speed"], 20.0)
    da = c["delta_angle"]
    near = np.abs(np.cos(np.abs(da)) - np.float32(0.5)) < 10 * RR_MARGIN
    da[near] += np.float32(1e-3)
    col = np.ones((G, Ts + 7), dtype=bool)
    col[:, :Ts] = False
    for i in range(G):
        for s in RR_PLACEMENTS[(i + shift) % len(RR_PLACEMENTS)]:
            s = Ts - 1 if s == "last" else (127 if s == "round2" else s)
            if s < Ts:
                col[i, s] = True
    off = np.ones((G, 2 * Ts + 3), dtype=bool)
    off[:, :Ts] = (torch.rand(G, Ts, generator=g) < 0.1).numpy()
    c["collision"], c["off_road"] = col, off
    return c


def rollout_return_margins(c):
    """Distance of every thresholded quantity from its threshold (all must exceed RR_MARGIN): the device's cosf may differ from numpy's
    in the last bit, and no decision may ride on that."""
    cosd = np.cos(np.abs(c["delta_angle"]))
    return {"acc": float(np.min(np.abs(np.abs(c["acc"]) - 4))), "ang_acc": float(np.min(np.abs(np.abs(c["ang_acc"]) - 4))),
            "cos": float(np.min(np.abs(cosd - 0.5))), "speed3": float(np.min(np.abs(np.abs(c["speed"]) - 3))),
            "speed20": float(np.min(np.abs(np.abs(c["speed"]) - 20)))}


def rollout_return_ref(c, collision=None):
    Ts = c["delta_angle"].shape[1]
    col = c["collision"] if collision is None else collision
    return oadv.rollout_return(c["delta_dis"], c["delta_angle"], c["speed"], c["acc"], c["ang_vel"], c["ang_acc"], col[:, :Ts],
                               c["off_road"][:, :Ts], RR_GAMMA)


# (delta_dis, delta_angle, speed, acc, ang_acc, collision, off_road): one step, inputs exactly ON the thresholds
REWARD_KAT = (
    (0.7, 0.3, 5.0, 4.0, 0.0, 0, 0), (0.7, 0.3, 5.0, -4.0, -4.0, 0, 0),          # |acc| = 4: not a comfort violation
    (0.7, 0.3, 5.0, 4.5, -4.5, 0, 0),                                            # ... and beyond it: two
    (0.2, 0.1, 3.0, 0.0, 0.0, 0, 0), (0.2, 0.1, 20.0, 0.0, 0.0, 0, 0),           # |speed| = 3 and 20: outside the velocity bonus
    (0.2, 0.1, -3.0, 0.0, 0.0, 0, 0), (0.2, 0.1, 12.0, 0.0, 0.0, 0, 0),
    (0.0, 0.0, 0.0, 0.0, 0.0, 0, 0),                                             # standing still: no time-step penalty
    (0.0, 0.0, 0.0, 0.1, 0.0, 0, 0),                                             # standing still but accelerating
    (1.5, 0.0, 8.0, 1.0, 1.0, 0, 0),                                             # delta_angle = 0
    (1.5, 2.0, 8.0, 1.0, 1.0, 0, 0),                                             # negative cosine
    (0.5, 0.4, -6.0, 1.0, 1.0, 0, 0), (0.5, 2.0, -6.0, 1.0, 1.0, 0, 0),          # negative speed
    (0.5, 0.4, 6.0, 1.0, 1.0, 1, 0), (0.5, 0.4, 6.0, 1.0, 1.0, 1, 1), (0.5, 0.4, 6.0, 1.0, 1.0, 0, 1),
)


def reward_kat_ref():
    f = np.float32
    return np.array([oadv.dense_reward(f(dd), f(da), f(sp), f(ac), f(0.0), f(aa), col, off) for dd, da, sp, ac, aa, col, off in REWARD_KAT])


# ---- 6. PPO critic ------------------------------------------------------------------------------------------------------------------
CRITIC_NS = (1, 15, 17, 50, 257, 15)          # in this order on one engine: the scratch buffer grows, then is reused larger than needed


@functools.lru_cache(maxsize=None)
def critic_case(call, seed=3434):
    """State (n, 128) and SmoothL1 targets of call number `call`: target = oracle value + e with |e| alternating between the quadratic
    (0.2 .. 0.8) and the linear (1.2 .. 2.5) branch, both signs; no |e| within 0.2 of the branch point."""
    from oracle import critic as ocr
    from tests import helpers as H
    n = CRITIC_NS[call]
    g = torch.Generator().manual_seed(seed + 10 * call)
    state = torch.randn(n, 128, generator=g)
    value = ocr.critic_forward(H.critic_weights(), state)
    u = torch.rand(n, generator=g)
    mag = torch.where(torch.arange(n) % 2 == 0, 1.2 + 1.3 * u, 0.2 + 0.6 * u)
    sign = torch.where(torch.arange(n) % 4 < 2, 1.0, -1.0)
    return {"state": state, "target": (value + mag * sign).float()}


def critic_ref(case):
    """(values, SmoothL1 loss (mean), {parameter: gradient}) from the oracle with autograd."""
    import torch.nn.functional as F
    from oracle import critic as ocr
    from tests import helpers as H
    sd = H.critic_weights()
    params = {k: sd[k].clone().requires_grad_(True) for k in ocr.CRITIC_KEYS}
    value = ocr.critic_forward(params, case["state"])
    loss = F.smooth_l1_loss(value, case["target"])
    loss.backward()
    return value.detach(), float(loss.detach()), {k: v.grad.detach() for k, v in params.items()}


# ---- 7. PPO hyper-parameters --------------------------------------------------------------------------------------------------------
PPO_RATIOS = (0.5, 0.7, 0.9, 1.1, 1.3, 2.0)
PPO_ADV = (1.0, -0.8, 0.6, -1.2, 0.9, -0.5)
PPO_CLIP, PPO_ENT = 0.4, 0.2


def ppo_case(probability, r_pad):
    """Per-scene PPO inputs for the six scenes of the `small` fixture given the policy's own logits (bs, R, M): the chosen action is a
    candidate of the first reference line, old_log_prob puts the ratio on PPO_RATIOS (0.7 and 1.3 lie inside the 0.4 clip range and
    outside the default 0.2 one; every ratio is at least 0.1 from a boundary of either), advantages of both signs."""
    bs, R, M = probability.shape
    assert bs == len(PPO_RATIOS) and not bool(r_pad[:, 0].any())
    lp = torch.log_softmax(probability.float().masked_fill(r_pad.unsqueeze(-1), -1e8).view(bs, -1), dim=1).view(bs, R, M)
    mode = torch.stack([torch.zeros(bs, dtype=torch.int64), (torch.arange(bs) * 5 + 1) % M], 1)
    cur = lp[torch.arange(bs), mode[:, 0], mode[:, 1]]
    return {"action_mode_torch": mode, "advantage_torch": torch.tensor(PPO_ADV), "old_log_prob_torch": cur - torch.log(torch.tensor(PPO_RATIOS))}


# ---- 8. other-vehicle forecast and the SFT teacher label -----------------------------------------------------------------------------
OV_NS, OV_TS = (1, 64, 65), (1, 40)


def other_vehicle_case(N, seed=5151):
    """N actors cycling through braking, coasting (no pedal), slow (below the 1 m/s extent threshold, some accelerating across it) and
    accelerating ones."""
    g = np.random.default_rng(seed + N)
    kind = (np.arange(N) + N) % 4
    brake = (kind == 0).astype(np.float64)
    throttle = np.where(kind == 0, 0.0, np.where(kind == 1, 0.0, g.uniform(0.2, 0.9, N)))
    speed = np.where(kind == 2, g.uniform(0.1, 0.95, N), g.uniform(1.5, 14.0, N))
    return {"steer": g.uniform(-0.6, 0.6, N), "throttle": throttle, "brake": brake, "speed": speed,
            "location": np.stack([g.normal(20, 15, N), g.normal(-5, 15, N), g.uniform(0, 0.3, N)], -1),
            "yaw_deg": g.uniform(-180, 180, N), "extent": np.stack([g.uniform(1.8, 2.6, N), g.uniform(0.8, 1.1, N)], -1)}


SFT_TS, SFT_R, SFT_M, SFT_FR = (7, 25, 80), 6, 12, 10
SFT_TIES = ((5, 70), (7, 71), (2, 66), (0, 64))        # per scene: the two candidates (>= 64 apart) that share the minimum; (7, 71) share a lane


def sft_case(T):
    """Candidates moving along +x on an integer grid, teacher heading 0 and an integer origin: every local coordinate and every target
    speed is an exact fp32 integer.  In scene b the candidates SFT_TIES[b] have speed 9 against the teacher's 10; every other candidate is
    at least 2 away (some above, some below)."""
    bs, G = len(SFT_TIES), SFT_R * SFT_M
    traj = torch.zeros(bs, G, T, 6)
    t = torch.arange(T)
    k = torch.clamp((t + 1) // SFT_FR, min=1) if T >= SFT_FR else torch.ones(T, dtype=torch.int64)
    for b, tie in enumerate(SFT_TIES):
        for gi in range(G):
            d = 9 if gi in tie else (12 + (gi * 7 + b) % 8 if gi % 2 else 8 - (gi + b) % 7)
            traj[b, gi, :, 0] = 100.0 + b + d * k
            traj[b, gi, :, 1] = -40.0 + b
    teacher = torch.tensor([[10.0, 100.0 + b, -40.0 + b, 0.0, 6.0] for b in range(bs)])
    return traj.view(bs, SFT_R, SFT_M, T, 6).contiguous(), teacher
