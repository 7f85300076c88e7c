"""Host side of the autograd bridge (rift_amd/autograd.py), without a GPU: the two Functions are driven with a stand-in engine whose
head_backward / critic_backward are PyTorch-CPU restatements, so what is checked here is the graph plumbing -- which tensor comes back,
what backward hands to the engine and in which order it returns the segments, frozen parameters, in-place edits of the output, the
stale-forward refusal -- and not the kernels (tests/test_gpu_autograd_head.py)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from rift_amd import _ffi
from rift_amd.autograd import critic_value, head_logits
from tests import helpers as H


def _pi_head(seed=3):
    from rift_amd.planning.pluto.model.pluto_model import MLPLayer
    torch.manual_seed(seed)
    m = MLPLayer(128, 128, 1)
    for p in m.parameters():
        p.data.add_(0.05 * torch.randn_like(p))
    return m


def _pi_forward(m, q):
    s = m.mlp
    return s[3](F.relu(s[1](s[0](q)))).squeeze(-1)


class FakeEngine:
    """head_backward / critic_forward / critic_backward in PyTorch CPU, with the call log the tests look at."""

    def __init__(self, pi_head=None, q=None):
        self.device, self.generation, self.calls = torch.device("cpu"), 0, []
        self.pi_head, self.q = pi_head, q

    def forward(self):
        self.generation += 1
        with torch.no_grad():
            return _pi_forward(self.pi_head, self.q).clone()

    def head_backward(self, dlogits, grads, accumulate):
        assert dlogits.dtype == torch.float32 and dlogits.is_contiguous() and grads is None and accumulate is False
        self.calls.append("head_backward")
        named = dict(self.pi_head.named_parameters())
        params = [named[k].detach().clone().requires_grad_(True) for k in _ffi.PI_KEYS]
        with torch.enable_grad():               # (a Function's backward runs with grad mode off)
            z = F.linear(F.relu(F.layer_norm(F.linear(self.q, params[0], params[1]), (128,), params[2], params[3], self.pi_head.mlp[1].eps)),
                         params[4], params[5]).squeeze(-1)
            return torch.cat([g.reshape(-1) for g in torch.autograd.grad(z, params, dlogits)])

    @staticmethod
    def _critic(sd, state):
        from oracle import critic as ocritic
        return ocritic.critic_forward(sd, state)

    def critic_forward(self, sd, state):
        with torch.no_grad():
            return self._critic(sd, state)

    def critic_backward(self, sd, state, dvalue, grads, accumulate):
        assert dvalue.dtype == torch.float32 and dvalue.is_contiguous() and grads is None and accumulate is False
        self.calls.append("critic_backward")
        params = {k: sd[k].detach().clone().requires_grad_(True) for k in _ffi.CRITIC_KEYS}
        with torch.enable_grad():
            g = torch.autograd.grad(self._critic(params, state), [params[k] for k in _ffi.CRITIC_KEYS], dvalue)
        return torch.cat([t.reshape(-1) for t in g])


def _reference_grads(m, q, loss_fn):
    ref = _pi_head()
    ref.load_state_dict(m.state_dict())
    loss_fn(_pi_forward(ref, q)).backward()
    return {k: p.grad for k, p in ref.named_parameters()}


def test_flat_layouts_cover_the_parameter_counts():
    assert sum(_ffi.PI_SIZES) == _ffi.PI_NPARAM and len(_ffi.PI_SIZES) == len(_ffi.PI_KEYS)
    assert sum(_ffi.CRITIC_SIZES) == _ffi.CRITIC_NPARAM and len(_ffi.CRITIC_SIZES) == len(_ffi.CRITIC_KEYS)
    m = _pi_head()
    assert [p.numel() for p in (dict(m.named_parameters())[k] for k in _ffi.PI_KEYS)] == list(_ffi.PI_SIZES)
    assert [v.numel() for v in (H.critic_weights()[k] for k in _ffi.CRITIC_KEYS)] == list(_ffi.CRITIC_SIZES)


def test_flags_default_off():
    from rift_amd.gym_carla.utils.net import CriticPPO
    from rift_amd.planning.pluto.model.pluto_model import PlanningModel
    assert PlanningModel(radius=120).differentiable_head is False
    assert CriticPPO([256, 256], 128, 3).differentiable is False


def test_null_context_is_refused_by_both_entries():
    from rift_amd import build
    build.build()
    lib = _ffi.load_library()
    lo = _ffi.RiftLossOut()
    assert lib.rift_head_backward(None, None, 1, 1, ctypes.byref(lo), 0, None) == -1
    assert lib.rift_critic_backward(None, None, None, None, 1, None, None) == -1


def test_head_logits_returns_the_same_tensor_and_routes_the_upstream_gradient():
    m = _pi_head()
    q = torch.randn(2 * 3 * 12, 128, generator=torch.Generator().manual_seed(1)).view(2, 3, 12, 128)
    eng = FakeEngine(m, q)
    W = torch.randn(2, 3, 12, generator=torch.Generator().manual_seed(2))
    logits = eng.forward()
    prob = head_logits(m, logits, eng)
    assert prob is logits and prob.grad_fn is not None and prob.data_ptr() == logits.data_ptr()
    # in-place edit of the output, as the reference's losses do: legal (nothing was saved), and the gradient is masked by it
    pad = torch.zeros(2, 3, dtype=torch.bool)
    pad[1, 2] = True
    prob.masked_fill_(pad.unsqueeze(-1), -1e8)
    (prob * W).sum().backward()
    want = _reference_grads(m, q, lambda z: (z.masked_fill(pad.unsqueeze(-1), -1e8) * W).sum())
    assert eng.calls == ["head_backward"]
    for k, p in m.named_parameters():
        assert p.grad.shape == p.shape and torch.allclose(p.grad, want[k], rtol=1e-5, atol=1e-6), k


def test_head_logits_semantics_frozen_parameter_retain_graph_and_f64_upstream():
    m = _pi_head()
    m.mlp[1].bias.requires_grad_(False)
    q = torch.randn(1, 2, 12, 128, generator=torch.Generator().manual_seed(5))
    eng = FakeEngine(m, q)
    prob = head_logits(m, eng.forward(), eng)
    loss = prob.double().pow(2).sum()                       # (upstream gradient arrives as fp32 through the cast's backward)
    loss.backward(retain_graph=True)
    once = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert "mlp.1.bias" not in once and len(once) == 5
    loss.backward()
    for k, p in m.named_parameters():
        if k in once:
            assert torch.equal(p.grad, 2 * once[k]), k
    assert m.mlp[1].bias.grad is None and eng.calls == ["head_backward"] * 2


def test_stale_backward_is_refused_before_anything_is_launched():
    m = _pi_head()
    q = torch.randn(1, 1, 12, 128, generator=torch.Generator().manual_seed(7))
    eng = FakeEngine(m, q)
    a = head_logits(m, eng.forward(), eng)
    eng.forward()                                           # any second forward on the engine
    with pytest.raises(RuntimeError, match="another forward ran on this engine before backward; its activations are gone"):
        a.sum().backward()
    assert eng.calls == [] and all(p.grad is None for p in m.parameters())


def test_parameter_edit_between_forward_and_backward_is_refused():
    m = _pi_head()
    eng = FakeEngine(m, torch.randn(1, 1, 12, 128, generator=torch.Generator().manual_seed(8)))
    a = head_logits(m, eng.forward(), eng)
    with torch.no_grad():
        m.mlp[3].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place between forward and backward"):
        a.sum().backward()
    assert eng.calls == []


def test_critic_value_routes_gradients_to_all_ten_tensors_and_none_to_the_state():
    from rift_amd.gym_carla.utils.net import CriticPPO
    critic = CriticPPO([256, 256], 128, 3)
    critic.load_state_dict(H.critic_weights())
    for p in critic.parameters():
        p.requires_grad_(True)
    critic.value_avg.requires_grad_(False)
    g = torch.Generator().manual_seed(11)
    state, target = torch.randn(5, 128, generator=g).requires_grad_(True), torch.randn(5, generator=g)
    eng = FakeEngine()
    value = critic_value(critic, state, eng)
    F.smooth_l1_loss(value, target).backward()
    assert eng.calls == ["critic_backward"] and state.grad is None and critic.value_avg.grad is None
    sd = {k: v.clone().requires_grad_(True) for k, v in H.critic_weights().items()}
    F.smooth_l1_loss(FakeEngine._critic(sd, state.detach()), target).backward()
    for k, p in critic.named_parameters():
        if k != "value_avg":
            assert p.grad.shape == p.shape and torch.allclose(p.grad, sd[k].grad, rtol=1e-5, atol=1e-7), k
