"""The operand-format-free entries (rift_amd/csrc/shared.hip: one definition per library) called through contexts of BOTH engine builds alive
in one process: a bf16-operand and an fp16-operand Engine.  The entries' code is the same whatever context they are given, so the two
answer bit for bit; what belongs to a context (last error, profiler record, destructor) stays with that context.  Tiny shapes, chosen for
the kernels' edges: a tail workgroup and an odd group size, one element and one past a 256-thread pass, one row past a 16-row tile.
The unit's call protocol (csrc/launch.h) is checked through `eng.lib` with ctypes, so that no Python-side assert answers first: every launch
of an accepted call is on the profiler's record, an accepted call leaves an empty message, a refused one a message that names its entry.
Nothing here provokes a fault: every call is a valid one or a refusal decided on the host."""
import ctypes as C

import pytest
import torch

from rift_amd import _ffi
from rift_amd import synthetic as syn
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pair():
    engs = {"bf16": _ffi.Engine(DEV, operands="bf16"), "fp16": _ffi.Engine(DEV, operands="fp16")}
    assert [e.lib.rift_ctx_operand_format(e.ctx) for e in engs.values()] == [_ffi.OPERANDS["bf16"], _ffi.OPERANDS["fp16"]]
    yield engs
    torch.cuda.synchronize()
    for e in engs.values():
        e.close()


def _bits(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32}.get(t.element_size(), torch.uint8))


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what      # (bit patterns: a NaN equals itself)


def _two_tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(DEV) for n in (1, 300)]


def test_both_contexts_answer_bit_for_bit(pair):
    g = torch.Generator().manual_seed(18)
    returns = torch.randn(3, 5, generator=g, dtype=torch.float64).to(DEV)           # 3 groups (4 per workgroup: a tail workgroup), odd G
    norm_in = {n: torch.randn(n, generator=g).to(DEV) for n in (1, 257)}            # one element; one past a 256-thread pass
    csd = {k: v.to(DEV) for k, v in H.critic_weights().items()}
    state = H.critic_inputs(17)["state"].to(DEV)                                    # one row past a 16-row tile
    got = {}
    for name, eng in pair.items():
        r = {"group_advantage": eng.group_advantage(returns).clone()}
        for n, x in norm_in.items():
            r[f"normalize_{n}"] = eng.normalize_advantage_(x.clone())
        r["critic_forward"] = eng.critic_forward(csd, state).clone()
        p, grads = _two_tensors(1), _two_tensors(2)
        m, v = ([torch.zeros_like(t) for t in p] for _ in range(2))
        steps = [torch.zeros(1, device=DEV) for _ in p]
        eng.adamw_step_raw(eng.make_adam_list(p, grads, m, v, steps), [1e-3, 2e-3], [0.01, 0.0], 1.0, 0.9, 0.999, 1e-8)
        for k, ts in (("adam_p", p), ("adam_m", m), ("adam_v", v), ("adam_step", steps)):
            for i, t in enumerate(ts):
                r[f"{k}{i}"] = t
        clipped, tn = _two_tensors(3), torch.full((1,), -1.0, device=DEV)
        eng.clip_grad_norm_raw(eng.make_clip_list(clipped), 0.5, tn)
        r["clip0"], r["clip1"], r["clip_norm"] = clipped[0], clipped[1], tn
        torch.cuda.synchronize()
        got[name] = r
    assert set(got["bf16"]) == set(got["fp16"])
    for k in got["bf16"]:
        _same_bits(got["bf16"][k], got["fp16"][k], k)
    # (the calls did something: the advantages are not the returns, the parameters moved, the norm was written, the gradients were scaled)
    assert not torch.equal(got["bf16"]["group_advantage"], returns) and float(got["bf16"]["clip_norm"]) > 0.5
    assert not torch.equal(got["bf16"]["adam_p1"], _two_tensors(1)[1]) and not torch.equal(got["bf16"]["clip1"], _two_tensors(3)[1])
    assert float(got["bf16"]["adam_step0"]) == 1.0


@pytest.mark.parametrize("refused, other", [("bf16", "fp16"), ("fp16", "bf16")])
def test_a_refusal_stays_with_its_context(pair, refused, other):
    """rift_control_tick with two CBVs on the one slot there is: refused on the host, before any launch; the message is that context's."""
    eng, quiet = pair[refused], pair[other]
    traj = torch.zeros(1, 1, 12, 20, 6, device=DEV)
    prob = torch.zeros(1, 1, 12, device=DEV)
    assert quiet.control_tick(traj, prob, None, []).shape == (0, 8)      # (an accepted tick, here an empty one, leaves an empty message)
    state = torch.zeros(1, _ffi.CONTROL_STATE, dtype=torch.float64, device=DEV)
    dec = torch.full((2, 8), -7.0, dtype=torch.float64, device=DEV)
    cbvs = (_ffi.RiftControlCBV * 2)()
    for t in cbvs:
        t.batch_index, t.slot, t.x, t.y, t.heading, t.speed = 0, 0, 0.0, 0.0, 0.0, 1.0
    rc = eng.lib.rift_control_tick(eng.ctx, traj.data_ptr(), prob.data_ptr(), None, 1, 20, cbvs, 2, 1, 10, state.data_ptr(), 1, dec.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1
    assert (eng.lib.rift_last_error(eng.ctx) or b"").decode() == "rift_control_tick: two CBVs with the same slot"
    assert (quiet.lib.rift_last_error(quiet.ctx) or b"") == b""
    assert bool((dec == -7.0).all()) and not bool(state.any())


def test_launch_bookkeeping_reaches_the_shared_unit_through_the_core(pair):
    """The profiler switch of the fp16 context records the shared unit's launch on that context; the bf16 context's record stays empty."""
    eng = pair["fp16"]
    eng.prof_enable(True)
    try:
        p, grads = _two_tensors(1), _two_tensors(2)
        m, v = ([torch.zeros_like(t) for t in p] for _ in range(2))
        steps = [torch.zeros(1, device=DEV) for _ in p]
        eng.adamw_step_raw(eng.make_adam_list(p, grads, m, v, steps), [1e-3, 2e-3], [0.01, 0.0], 1.0, 0.9, 0.999, 1e-8)
        report = eng.prof_report()
    finally:
        eng.prof_enable(False)
    assert list(report) == ["adamw_kernel"] and report["adamw_kernel"]["count"] == 1
    assert pair["bf16"].prof_report() == {}


def test_contexts_of_both_formats_are_destroyed_by_their_own_build():
    """Both formats load a model and run a forward at batch 1; the fp16 context goes first, then the bf16 one; a new context of each format
    still loads and runs.  (Each build's table entry deletes its own context type.)"""
    sd = {k: v.to(DEV) for k, v in H.weights().items()}
    feat = syn.collate_scenes([syn.make_scene(7318, r_min=1, r_max=3)])["cur_pluto_feature_torch"]

    def run(operands):
        eng = _ffi.Engine(DEV, operands=operands)
        eng.load_state_dict(sd)
        out = eng.forward(feat, no_drop=True, bn_update=False)["probability"].clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        return eng, out

    bf, out_bf = run("bf16")
    hf, out_hf = run("fp16")
    hf.close()
    bf.close()
    torch.cuda.synchronize()
    for operands, want in (("fp16", out_hf), ("bf16", out_bf)):
        eng, out = run(operands)
        assert torch.equal(out, want), operands
        eng.close()


# ---- the call protocol: one accepted call of every entry whose launches the record did not use to see, at its smallest valid shape ----------
FILL = -7.0


def _protocol_calls():
    """[(entry, arguments after the context, outputs, the labels its launches leave on the record, what the pointers point to)], on fresh
    tensors from one seed: two lists hold the same inputs.  Outputs start at FILL (7 where the type has no sign)."""
    g = torch.Generator().manual_seed(28)

    def rn(*shape, dt=torch.float32):
        return torch.randn(*shape, generator=g, dtype=dt).to(DEV)

    def out(*shape, dt=torch.float32):
        return torch.full(shape, abs(FILL) if dt == torch.uint8 else FILL, dtype=dt, device=DEV)

    def zeros(*shape, dt=torch.float32):
        return torch.zeros(*shape, dtype=dt, device=DEV)

    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    calls = []

    def add(entry, args, outs, labels, keep=()):
        calls.append((entry, list(args) + [None], outs, labels, keep))      # (the stream: NULL, torch's default here)

    # the three scans: one element; the 256-thread normalise also one past a pass
    rew, undone, val, nval, unterm, adv = rn(1, dt=torch.float64), torch.ones(1, device=DEV), rn(1), rn(1), torch.ones(1, device=DEV), out(1)
    add("rift_gae", [P(rew), P(undone), P(val), P(nval), P(unterm), 0.98, 0.95, 1, P(adv)], {"advantages": adv}, {"affine_scan_reverse_kernel": 1},
        (rew, undone, val, nval, unterm))
    rew, done, ret = rn(1, dt=torch.float64), zeros(1), out(1, dt=torch.float64)
    add("rift_discounted_return", [P(rew), P(done), 0.98, 1, P(ret)], {"returns": ret}, {"affine_scan_reverse_kernel": 1}, (rew, done))
    for n in (1, 257):
        x = rn(n)
        add("rift_normalize_advantage", [P(x), n], {"x": x}, {"normalize_unbiased_kernel": 1})
    ret, adv = rn(3, 5, dt=torch.float64), out(3, 5, dt=torch.float64)      # 3 groups, 4 per workgroup: a tail
    add("rift_group_advantage", [P(ret), 3, 5, P(adv)], {"advantage": adv}, {"group_zscore_kernel": 1}, (ret,))
    # neighbour forecast N = 1, T = 1; collision G = 1, Tc = Ts = 1, no neighbours; off-road: one point on a 1 x 1 mask
    act, sp, loc, yaw, ext = (rn(*s, dt=torch.float64) for s in ((1, 3), (1,), (1, 3), (1,), (1, 2)))
    vert = out(1, 1, 4, 2, dt=torch.float64)
    add("rift_other_vehicle_rollout", [P(act), P(sp), P(loc), P(yaw), P(ext), 1, 1, 1, 1.1, P(vert)], {"vertices": vert},
        {"other_vehicle_rollout_kernel": 1}, (act, sp, loc, yaw, ext))
    cv, col = rn(1, 1, 4, 2), out(1, 1, dt=torch.uint8)
    add("rift_collision_matrix", [P(cv), 1, 1, None, 0, 1, P(col)], {"collision": col}, {"collision_matrix_kernel": 1}, (cv,))
    pt, mask, off = zeros(1, 2), torch.ones(1, 1, dtype=torch.uint8, device=DEV), out(1, dt=torch.uint8)
    add("rift_off_road_matrix", [P(pt), 1, P(mask), 1, 1, 0.0, 0.0, 0.0, 0.5, -0.5, 0.0, 0.0, P(off)], {"off_road": off}, {"off_road_kernel": 1}, (pt, mask))
    # reference-line info: G = M = 1, Ts = 1, one two-point line
    traj, rp, ra, rl = rn(1, 1, 6), rn(1, 2, 2), rn(1, 2), torch.tensor([2], dtype=torch.int32, device=DEV)
    dd, da, ci = out(1), out(1), out(1, dt=torch.int32)
    add("rift_ref_line_info", [P(traj), 1, 1, 1, 1, P(rp), P(ra), P(rl), 2, P(dd), P(da), P(ci)], {"dd": dd, "da": da, "ci": ci},
        {"ref_line_info_kernel": 1}, (traj, rp, ra, rl))
    six, flags, ret = [rn(1) for _ in range(6)], [zeros(1, dt=torch.uint8) for _ in range(2)], out(1, dt=torch.float64)
    add("rift_rollout_return", [P(t) for t in six] + [P(flags[0]), 1, P(flags[1]), 1, 1, 1, 0.98, P(ret)], {"returns": ret},
        {"rollout_return_kernel": 1}, (six, flags))
    traj, teacher, mode = rn(1, 1, 1, 6), rn(1, 5), out(1, 2, dt=torch.int64)
    add("rift_sft_teacher_mode", [P(traj), P(teacher), 1, 1, 1, 1, 10, P(mode)], {"mode": mode}, {"sft_teacher_mode_kernel": 1}, (traj, teacher))

    def path(*lead, T):          # candidates that drive ahead along x at about 5 m/s: (x, y, cos, sin, vx, vy) per frame
        t = torch.zeros(*lead, T, 6)
        t[..., 0] = 0.5 * torch.arange(1, T + 1) + 0.05 * torch.randn(*lead, T, generator=g)
        t[..., 1] = 0.05 * torch.randn(*lead, T, generator=g)
        t[..., 2], t[..., 4] = 1.0, 5.0
        return t.to(DEV)

    def pid():                   # the two never-reset PID filters, twelve candidates
        return [zeros(12, 20), zeros(12, dt=torch.int32), zeros(12, dt=torch.int32), zeros(12, 20), zeros(12, dt=torch.int32), zeros(12, dt=torch.int32)]

    center = torch.tensor([[0.0, 0.0, 0.0, 5.0, 2.0, 4.5]], device=DEV)
    # the candidate rollout: G = 12 (one group), Tfull = 40
    traj, state = path(12, T=40), pid()
    io = _ffi.RiftRolloutIO()
    io.trajectories, io.G, io.Tfull, io.G_per_group, io.center_state = traj.data_ptr(), 12, 40, 12, center.data_ptr()
    outs = {"center": out(12, 80, 2), "vertices": out(12, 80, 4, 2), "closest_index": out(12, 79, dt=torch.int32), "aim_idx": out(12, 79, dt=torch.int32)}
    outs.update({k: out(12, 80) for k in ("angle", "speed", "acc", "ang_vel", "ang_acc")})
    for k, t in list(zip(("turn_buf", "turn_ptr", "turn_len", "speed_buf", "speed_ptr", "speed_len"), state)) + list(outs.items()):
        setattr(io, k, t.data_ptr())
    add("rift_rollout", [C.byref(io)], dict(outs, **{f"pid{i}": t for i, t in enumerate(state)}), {"rollout8_kernel": 1, "rollout_kinematics_kernel": 1},
        (io, traj, center))
    # the control tick of this file: (1, 1, 12, 20, 6), one CBV on the one slot
    traj, prob, ctl = zeros(1, 1, 12, 20, 6), zeros(1, 1, 12), zeros(1, _ffi.CONTROL_STATE, dt=torch.float64)
    dec, cbv = out(1, 8, dt=torch.float64), (_ffi.RiftControlCBV * 1)()
    cbv[0].batch_index, cbv[0].slot, cbv[0].x, cbv[0].y, cbv[0].heading, cbv[0].speed = 0, 0, 0.0, 0.0, 0.0, 1.0
    add("rift_control_tick", [P(traj), P(prob), None, 1, 20, cbv, 1, 1, 10, P(ctl), 1, P(dec)], {"decision": dec, "state": ctl},
        {"control_tick_kernel": 1}, (traj, prob, cbv))
    # the group-advantage tick: K = 1, R = 1, Tfull = 80, no actors, no mask -- K + 7 launches less the neighbour forecast
    traj, state, adv = path(1, 1, 12, T=80), pid(), out(1, 1, 12, dt=torch.float64)
    rp, ra, rl = torch.tensor([[[0.0, 0.0], [40.0, 0.0]]], device=DEV), zeros(1, 2), torch.tensor([2], dtype=torch.int32, device=DEV)
    tick = (_ffi.RiftTickCBV * 1)()
    tick[0].batch_index, tick[0].R, tick[0].Pmax, tick[0].n_actors = 0, 1, 2, 0
    tick[0].center_state, tick[0].ref_pos, tick[0].ref_angle, tick[0].ref_len = center.data_ptr(), rp.data_ptr(), ra.data_ptr(), rl.data_ptr()
    add("rift_group_advantage_tick", [P(traj), 1, 80, tick, 1] + [P(t) for t in state] + [0.98, P(adv)], dict({"advantage": adv}, **{f"pid{i}": t for i, t in enumerate(state)}),
        dict({f"tick_multi_kernel_{i}": 1 for i in (0, 2, 3, 4, 5, 6)}, rollout8_kernel=1), (traj, center, rp, ra, rl, tick))
    # collate: the second scene of a two-scene arena that stores the logits and the advantages of one line each
    logits, advs, idx = rn(2, 1, 12), rn(2, 1, 12, dt=torch.float64), torch.tensor([1], dtype=torch.int32, device=DEV)
    ar, fb = _ffi.RiftReplayArena(), _ffi.RiftFeatureBatch()
    ar.n_scenes, ar.A, ar.Mp, ar.Rcap, ar.S, ar.T, ar.cs_ld = 2, 1, 1, 1, 0, 1, 1
    ar.old_group_logits, ar.group_advantage = logits.data_ptr(), advs.data_ptr()
    fb.bs, fb.A, fb.Mp, fb.R, fb.S, fb.T = 1, 1, 1, 1, 0, 1
    o_logits, o_adv = out(1, 1, 12), out(1, 1, 12, dt=torch.float64)
    add("rift_collate", [C.byref(ar), P(idx), 1, 1, C.byref(fb), P(o_logits), None, P(o_adv), None], {"old_logits": o_logits, "advantage": o_adv},
        {"collate_kernel": 1}, (ar, fb, logits, advs, idx))
    return calls


def _call(eng, entry, args):
    rc = getattr(eng.lib, entry)(eng.ctx, *args)
    torch.cuda.synchronize()
    return rc, (eng.lib.rift_last_error(eng.ctx) or b"").decode()


def test_every_launch_of_the_unit_is_on_the_record_and_the_record_changes_nothing(pair):
    """Profiler on: each accepted call leaves exactly its kernels' labels on the record (the tick's stages by number, one label per templated
    kernel); every output is bit-equal to the same call with the profiler off."""
    eng = pair["fp16"]
    plain = _protocol_calls()
    for entry, args, _, _, _ in plain:
        assert _call(eng, entry, args) == (0, ""), entry
    whole = {}
    try:
        for (entry, args, outs, labels, _), (_, _, want, _, _) in zip(_protocol_calls(), plain):
            eng.prof_enable(True)                      # (clears the record)
            assert _call(eng, entry, args) == (0, ""), entry
            report = eng.prof_report()
            assert {k: v["count"] for k, v in report.items()} == labels, entry
            for k in labels:
                whole[k] = whole.get(k, 0) + labels[k]
            for k in outs:
                _same_bits(outs[k], want[k], f"{entry}: {k}")
            assert not any(bool((t.double().abs() == abs(FILL)).all()) for t in outs.values()), entry      # (the call wrote its outputs)
    finally:
        eng.prof_enable(False)
    assert whole == {"affine_scan_reverse_kernel": 2, "normalize_unbiased_kernel": 2, "group_zscore_kernel": 1, "other_vehicle_rollout_kernel": 1,
                     "collision_matrix_kernel": 1, "off_road_kernel": 1, "ref_line_info_kernel": 1, "rollout_return_kernel": 1,
                     "sft_teacher_mode_kernel": 1, "rollout8_kernel": 2, "rollout_kinematics_kernel": 1, "control_tick_kernel": 1,
                     "tick_multi_kernel_0": 1, "tick_multi_kernel_2": 1, "tick_multi_kernel_3": 1, "tick_multi_kernel_4": 1,
                     "tick_multi_kernel_5": 1, "tick_multi_kernel_6": 1, "collate_kernel": 1}


def _refusals():
    """[(entry, arguments, tensors that must keep their contents)]: each entry once, with an argument its own first check rejects."""
    calls = {}
    for entry, args, outs, _, keep in _protocol_calls():
        calls.setdefault(entry, (args, outs, keep))

    def bad(entry, at, value):
        args, outs, keep = calls[entry]
        return entry, args[:at] + [value] + args[at + 1:], outs, keep

    ref = [bad("rift_gae", 7, -1), bad("rift_discounted_return", 3, -1), bad("rift_normalize_advantage", 1, -1), bad("rift_group_advantage", 1, 0),
           bad("rift_rollout_return", 10, 0), bad("rift_ref_line_info", 1, 0), bad("rift_collision_matrix", 1, 0), bad("rift_off_road_matrix", 1, 0),
           bad("rift_collate", 2, 0), bad("rift_sft_teacher_mode", 2, 0), bad("rift_other_vehicle_rollout", 6, 0)]
    for field, value in (("G", 0), ("Tfull", 39)):
        entry, args, outs, keep = bad("rift_rollout", 0, None)
        io = _ffi.RiftRolloutIO.from_buffer_copy(keep[0])
        setattr(io, field, value)
        ref.append((entry, [C.byref(io)] + args[1:], outs, keep + (io,)))
    flat, loss, total = torch.full((_ffi.PI_NPARAM,), FILL, device=DEV), torch.full((1,), FILL, dtype=torch.float64, device=DEV), torch.full((1,), FILL, device=DEV)
    lo = _ffi.RiftLossOut()
    lo.loss, lo.stats, lo.flat_grad_sum = loss.data_ptr(), None, flat.data_ptr()
    ref.append(("rift_loss_finalize", [C.byref(lo), 0, None], {"flat": flat, "loss": loss}, (lo,)))
    ref.append(("rift_loss_finalize_clip", [C.byref(lo), 0, 1.0, C.c_void_p(total.data_ptr()), None], {"flat": flat, "loss": loss, "norm": total}, (lo,)))
    stats, gw = torch.full((2,), FILL, dtype=torch.float64, device=DEV), torch.full((4,), FILL, device=DEV)
    ref.append(("rift_critic_finalize", [None, C.c_void_p(stats.data_ptr())] + [C.c_void_p(gw.data_ptr())] + [None] * 10, {"stats": stats, "g_w0": gw}, ()))
    return ref


def test_no_stale_message_and_no_silent_refusal(pair):
    """After a refusal on the context, every accepted call leaves rc 0 and an empty message; then every entry, refused once by its own first
    check, answers a negative code and a message that starts with ITS name, writes nothing and launches nothing."""
    eng = pair["fp16"]
    test_a_refusal_stays_with_its_context(pair, "fp16", "bf16")      # the stale message: "rift_control_tick: two CBVs with the same slot"
    for entry, args, _, _, _ in _protocol_calls():
        assert _call(eng, entry, args) == (0, ""), entry
    p, grads = _two_tensors(1), _two_tensors(2)
    m, v = ([torch.zeros_like(t) for t in p] for _ in range(2))
    al = eng.make_adam_list(p, grads, m, v, [torch.zeros(1, device=DEV) for _ in p])
    lrs, wds = (C.c_double * 2)(1e-3, 2e-3), (C.c_double * 2)(0.01, 0.0)
    clipped, tn = _two_tensors(3), torch.full((1,), FILL, device=DEV)
    ptrs, nums, _, _ = eng.make_clip_list(clipped)
    refusals = _refusals() + [
        ("rift_adamw_step", [0, al["p"], al["g"], al["m"], al["v"], al["s"], al["numel"], lrs, wds, 1.0, 0.9, 0.999, 1e-8, None],
         {f"adam{i}": t for i, t in enumerate(p + m + v)}, ()),
        ("rift_clip_grad_norm", [ptrs, nums, 17, 0.5, C.c_void_p(tn.data_ptr()), None], {"clip0": clipped[0], "clip1": clipped[1], "norm": tn}, ())]
    assert len(refusals) == 18
    eng.prof_enable(True)
    try:
        for entry, args, outs, _ in refusals:
            before = {k: t.clone() for k, t in outs.items()}
            rc, msg = _call(eng, entry, args)
            assert rc < 0, entry
            assert msg.startswith(entry + ": ") and len(msg) > len(entry) + 2, (entry, msg)
            for k in outs:
                _same_bits(outs[k], before[k], f"{entry}: {k}")
            assert _call(eng, "rift_normalize_advantage", [None, 0, None]) == (0, "")      # (an accepted call in between: the next message is not this one)
        assert eng.prof_report() == {}
    finally:
        eng.prof_enable(False)
