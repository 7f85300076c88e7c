"""The engine context's device memory over its lifetime: scratch that grows and is reused, weight images replaced by a reload, a reload
that fails, and create / close cycles (csrc/devmem.h: DevBuf; tests/test_devmem_host.py runs the type's failure paths on the CPU).

Default-size scenes with one to three reference lines: the allocation logic does not depend on the scene size.  Forwards run with
no_drop=True, bn_update=False, so that two engines given the same input answer bit for bit; every comparison is torch.equal."""
import re

import pytest
import torch

from rift_amd import _ffi
from rift_amd import synthetic as syn
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MISSING = "planning_decoder.pi_head.mlp.3.weight"
# one tensor of each kind the forward reads: embedding tables, a raw vector, LayerNorms of every module, a Fourier frequency table, a
# BatchNorm running statistic, a head's LayerNorm, the static-object table (no scene of this batch has static objects) and a mode embedding
READ_BY_THE_FORWARD = ["map_encoder.on_route_emb.weight", "agent_encoder.ego_state_emb.pos_embed", "agent_encoder.history_encoder.norm1.bias",
                       "encoder_blocks.2.norm2.bias", "pos_emb.freqs.weight", "map_encoder.polygon_encoder.second_mlp.1.running_var",
                       "planning_decoder.decoder_blocks.3.norm4.weight", "planning_decoder.loc_head.mlp.1.weight", "ref_free_decoder.mlp.1.bias",
                       "static_objects_encoder.type_emb.weight", "planning_decoder.m_emb",
                       # and one of each kind that is packed into a GEMM image: a linear's weight, a linear's bias, an in_proj_bias that is
                       # sliced, a conv weight, and the bias of the conv that is packed from two of its taps
                       "encoder_blocks.1.mlp.fc1.weight", "planning_decoder.decoder_blocks.0.ffn.3.bias",
                       "planning_decoder.decoder_blocks.2.cross_attn.in_proj_bias", "agent_encoder.history_encoder.lateral_convs.1.weight",
                       "agent_encoder.history_encoder.fpn_conv.bias"]
OPTIONAL = "map_encoder.polygon_encoder.first_mlp.1.num_batches_tracked"
_cache = {}


def _to_dev(d):
    return {k: _to_dev(v) if isinstance(v, dict) else (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


# two scenes each: 49 agents + 60 polygons = 109 token slots (the scene encoder's 112-row layout, the decoder's dense variant on its image),
# and nine reference lines (the decoder's dense variant on dec_kv_frag_kernel's image)
SHAPES = {"wide": dict(num_agents=49, num_polygons=60, r_min=1, r_max=3), "dense": dict(r_min=9, r_max=9)}


def _batch(n):
    if n not in _cache:
        kind, count, base = (SHAPES[n], 2, 7400 + 10 * sorted(SHAPES).index(n)) if n in SHAPES else (dict(r_min=1, r_max=3), n, 7300 + 10 * n)
        _cache[n] = _to_dev(syn.collate_scenes([syn.make_scene(base + i, **kind) for i in range(count)]))
    return _cache[n]


def _sd(perturbed=False):
    """The test weights on the device (built once: an engine binds views onto them); perturbed: every floating tensor scaled by 1.05."""
    if "sd" not in _cache:
        _cache["sd"] = {k: v.to(DEV) for k, v in H.weights().items()}
        _cache["sd2"] = {k: (v * 1.05 if v.is_floating_point() else v.clone()) for k, v in _cache["sd"].items()}
    return _cache["sd2" if perturbed else "sd"]


def _forward(eng, batch):
    out = eng.forward(batch["cur_pluto_feature_torch"], no_drop=True, bn_update=False)
    return [out["probability"].clone(), out["hidden"].clone()]


def _step(eng, batch):
    """forward + loss_backward("rift") + loss_finalize: [probability, hidden, stats, flat, loss, the six gradients]"""
    res = _forward(eng, batch)
    stats, flat, _ = eng.loss_backward("rift", batch)
    grads = {k: torch.zeros_like(_sd()["planning_decoder.pi_head." + k]) for k in _ffi.PI_KEYS}
    loss = eng.loss_finalize(stats, flat, grads)
    return res + [stats.clone(), flat.clone(), loss.clone()] + [grads[k] for k in _ffi.PI_KEYS]


def _critic(eng, n):
    ci, csd = H.critic_inputs(n), _cache.setdefault("csd", {k: v.to(DEV) for k, v in H.critic_weights().items()})
    state, dv = ci["state"].to(DEV), ci["advantage"].to(DEV)
    return [eng.critic_forward(csd, state).clone(), eng.critic_backward(csd, state, dv).clone()]


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), i


def test_scratch_grows_and_is_reused_on_one_engine():
    """One bf16 engine at 2, 5, 2 scenes, then at two scenes of 109 token slots, two of nine reference lines and 2 again (forward, loss,
    finalize; head_backward behind the 5-scene forward) and its critic at 3, 40, 3
    rows: every result equals that of a fresh engine given the same input alone.  Each grow path of the arena, the loss scratch, the
    pi_head backward scratch and the critic scratch runs once, and so does the reuse below capacity.  The growth of the ranking's
    published words (rk_pub) needs a batch of more than 4096 scenes and is NOT exercised here."""
    dz = torch.randn(5, 3, 12, generator=torch.Generator().manual_seed(5)).to(DEV)
    eng = _ffi.Engine(DEV)
    eng.load_state_dict(_sd())
    got, got_head = [], None
    for n in (2, 5, 2, "wide", "dense", 2):
        got.append(_step(eng, _batch(n)))
        if n == 5:
            dz = dz[:, :got[-1][0].shape[1]].contiguous()
            got_head = eng.head_backward(dz).clone()
    got_critic = [_critic(eng, n) for n in (3, 40, 3)]
    torch.cuda.synchronize()
    eng.close()
    want = {}
    for n, nc in ((2, 3), (5, 40), ("wide", None), ("dense", None)):
        fresh = _ffi.Engine(DEV)
        fresh.load_state_dict(_sd())
        want[n] = _step(fresh, _batch(n))
        if n == 5:
            _same([got_head], [fresh.head_backward(dz).clone()])
        if nc:
            want["c%d" % nc] = _critic(fresh, nc)
        torch.cuda.synchronize()
        fresh.close()
    _same(got[0], want[2]); _same(got[1], want[5]); _same(got[2], want[2])
    _same(got[3], want["wide"]); _same(got[4], want["dense"]); _same(got[5], want[2])
    _same(got_critic[0], want["c3"]); _same(got_critic[1], want["c40"]); _same(got_critic[2], want["c3"])
    assert not torch.equal(got[0][3], torch.zeros_like(got[0][3]))            # (the gradient sums are not trivially equal)


def test_reload_replaces_the_images_and_the_weight_only_products():
    eng = _ffi.Engine(DEV)
    eng.load_state_dict(_sd())
    out1 = _forward(eng, _batch(2))
    eng.load_state_dict(_sd(perturbed=True))
    out2 = _forward(eng, _batch(2))
    assert not torch.equal(out1[0], out2[0]) and not torch.equal(out1[1], out2[1])
    eng.load_state_dict(_sd())
    _same(_forward(eng, _batch(2)), out1)
    torch.cuda.synchronize()
    eng.close()


def test_failed_reload_is_refused_not_run():
    """A load that fails leaves NO model: forward and loss_backward answer RIFT_ERR_STATE (-3) ahead of any launch instead of running on
    the images the failed load freed; the next full load works as if nothing had happened."""
    eng = _ffi.Engine(DEV)
    eng.load_state_dict(_sd())
    batch = _batch(2)
    out1 = _forward(eng, batch)
    with pytest.raises(RuntimeError, match="missing parameter"):
        eng.load_state_dict({k: v for k, v in _sd().items() if k != MISSING})
    with pytest.raises(RuntimeError, match=r"rift_forward failed \(-3\).*no model is loaded"):
        eng.forward(batch["cur_pluto_feature_torch"], no_drop=True, bn_update=False)
    with pytest.raises(RuntimeError, match=r"rift_loss_backward failed \(-3\).*no model is loaded"):
        eng.loss_backward("rift", batch)
    eng.load_state_dict(_sd())
    _same(_forward(eng, batch), out1)
    torch.cuda.synchronize()
    eng.close()


def test_a_load_without_a_tensor_the_forward_reads_is_refused_by_name():
    """Every tensor the forward reads is resolved by rift_model_load: a state dict that lacks one is refused THERE, with the tensor's name
    in the message, and leaves no model -- the forward that follows answers RIFT_ERR_STATE (-3) ahead of any launch, so no kernel ever
    sees the null pointer (forward is never called on a model that loaded with a tensor missing).  Only a BatchNorm's
    num_batches_tracked is optional: an eval forward does not read it.  The last full load answers as the first one did."""
    eng = _ffi.Engine(DEV)
    eng.load_state_dict(_sd())
    batch = _batch(2)
    out1 = _forward(eng, batch)
    for name in READ_BY_THE_FORWARD:
        assert name in _sd()
        with pytest.raises(RuntimeError, match=r"rift_model_load failed \(-1\).*missing parameter: " + re.escape(name) + r"$"):
            eng.load_state_dict({k: v for k, v in _sd().items() if k != name})
        with pytest.raises(RuntimeError, match=r"rift_forward failed \(-3\).*no model is loaded"):
            eng.forward(batch["cur_pluto_feature_torch"], no_drop=True, bn_update=False)
    assert OPTIONAL in _sd()
    eng.load_state_dict({k: v for k, v in _sd().items() if k != OPTIONAL})
    _same(_forward(eng, batch), out1)
    eng.load_state_dict(_sd())
    _same(_forward(eng, batch), out1)
    torch.cuda.synchronize()
    eng.close()


def test_op_linear_shares_no_storage_with_the_model():
    """load, forward, op_linear on a small matrix, forward: the two forwards are bit-identical -- the test entry packs into images of its
    own and leaves the model's alone.  M = 5, K = 40, N = 24: K is padded to 64 and N to 32 in the image.  The result holds the bars of
    tests/test_gpu_parity.py::test_mfma_gemm_kernel (same operand recipe): 2e-5 in fp32, 4e-2 with 16-bit operands."""
    eng = _ffi.Engine(DEV)
    eng.load_state_dict(_sd())
    batch = _batch(2)
    out1 = _forward(eng, batch)
    M, K, N = 5, 40, 24
    g = torch.Generator().manual_seed(M * 131 + K * 17 + N)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    ref = torch.nn.functional.linear(x, w, b)
    y32, y16 = eng.op_linear(x, w, b, fp32=True).cpu(), eng.op_linear(x, w, b, fp32=False).cpu()
    _same(_forward(eng, batch), out1)
    assert y32.shape == ref.shape and torch.isfinite(y32).all() and torch.isfinite(y16).all()
    assert float((y32 - ref).abs().max()) < 2e-5
    assert float((y16 - ref).abs().max()) < 4e-2
    torch.cuda.synchronize()
    eng.close()


def test_nothing_accumulates_over_reloads_and_engine_lifetimes():
    """Free device memory over six reload cycles on one engine and over six create / load / forward / loss / close cycles: after cycle 6
    it is no lower than after cycle 1 by more than ONE footprint of an engine (free memory before Engine(...) minus free memory after
    its first load and forward).  Derived, not measured: a leak of the image pool or of the arenas per cycle would lose five."""
    batch, sds = _batch(2), (_sd(), _sd(perturbed=True))
    warm = _ffi.Engine(DEV)                   # (the tensors, the library and torch's own blocks exist before the first reading)
    warm.load_state_dict(sds[0])
    _step(warm, batch)
    torch.cuda.synchronize()
    warm.close()

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    free0 = free()
    eng = _ffi.Engine(DEV)
    eng.load_state_dict(sds[0])
    _forward(eng, batch)
    footprint = free0 - free()
    assert footprint > 0
    reloads = []
    for i in range(6):
        eng.load_state_dict(sds[(i + 1) % 2])
        _forward(eng, batch)
        reloads.append(free())
    eng.close()
    lives = []
    for i in range(6):
        e = _ffi.Engine(DEV)
        e.load_state_dict(sds[0])
        _step(e, batch)
        torch.cuda.synchronize()
        e.close()
        lives.append(free())
    print(f"lifetime: footprint {footprint} B; free-memory drift cycle 1 -> 6: reloads {reloads[0] - reloads[5]} B, "
          f"create/close {lives[0] - lives[5]} B; after close vs before the first engine {free0 - lives[5]} B")
    assert reloads[0] - reloads[5] <= footprint, (reloads, footprint)
    assert lives[0] - lives[5] <= footprint, (lives, footprint)
