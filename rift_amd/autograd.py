"""torch autograd over the two trainable heads: an objective written in PyTorch trains `planning_decoder.pi_head` and `value_net` through
the HIP backward kernels (rift_head_backward / rift_critic_backward, include/rift_hip.h).

The reference's LightningModule trainers compute get_rift_loss / get_ppo_loss / ... in PyTorch and call `loss.backward()`
(rift_trainer.py:140-182, ppo_trainer.py:161-183).  The two Functions here put the library's forward outputs on the autograd graph so that
those trainers -- or any variation of their objectives -- work unchanged: autograd produces d loss / d probability (d loss / d value), the
library turns it into the parameter gradients, autograd accumulates them into `.grad`.  Opt-in: PlanningModel.differentiable_head and
CriticPPO.differentiable.  The trainable set stays pi_head + value_net; nothing flows into the frozen trunk.
"""
import torch
from torch.autograd.function import once_differentiable

from rift_amd._ffi import CRITIC_KEYS, CRITIC_SIZES, PI_KEYS, PI_SIZES


def _segments(flat, sizes, params, needs):
    """Views of the flat gradient sums shaped like the parameters; None where autograd wants no gradient."""
    return tuple(seg.view_as(p) if need else None for seg, p, need in zip(flat.split(sizes), params, needs))


class HeadLogits(torch.autograd.Function):
    """probability = pi_head(q_final) as the engine's forward computed it, with the six pi_head parameters (PI_KEYS order) as its inputs
    on the graph.  The activations stay in the engine (fp32 q_final and pre-activation of the latest forward), so nothing is saved but the
    engine's forward generation: the output may be modified in place (the reference's losses masked_fill_ it), and a backward behind
    another forward of the same engine is refused instead of being computed from that forward's activations."""

    @staticmethod
    def forward(ctx, w1, b1, ln_w, ln_b, w2, b2, logits, engine, generation):
        ctx.engine, ctx.generation = engine, generation
        ctx.params = (w1, b1, ln_w, ln_b, w2, b2)
        ctx.versions = tuple(p._version for p in ctx.params)
        ctx.mark_dirty(logits)          # the same tensor, now with history: not a view of an input, so in-place edits by the caller stay legal
        return logits

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        eng = ctx.engine
        if eng.generation != ctx.generation:
            raise RuntimeError("HeadLogits.backward: another forward ran on this engine before backward; its activations are gone "
                               f"(forward generation {ctx.generation}, the engine is at {eng.generation}) -- one backward per forward, before the next one")
        if tuple(p._version for p in ctx.params) != ctx.versions:
            raise RuntimeError("HeadLogits.backward: a pi_head parameter was modified in place between forward and backward (the backward "
                               "kernels read the live parameters)")
        flat = eng.head_backward(grad_output.to(torch.float32).contiguous(), None, False)
        return _segments(flat, PI_SIZES, ctx.params, ctx.needs_input_grad[:6]) + (None, None, None)


class CriticValue(torch.autograd.Function):
    """value = value_net(state) (CriticPPO) with the ten critic parameters (CRITIC_KEYS order) on the graph.  Stateless: the backward
    kernels recompute the forward from `state`.  No gradient flows to `state` (the trunk's `hidden`: frozen)."""

    @staticmethod
    def forward(ctx, *args):
        params, state, engine = args[:10], args[10], args[11]
        ctx.engine = engine
        state = state.detach().to(device=engine.device, dtype=torch.float32).contiguous()
        ctx.save_for_backward(state, *params)       # (inputs: autograd checks that none was modified in place before backward)
        return engine.critic_forward(dict(zip(CRITIC_KEYS, params)), state)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        state, *params = ctx.saved_tensors
        flat = ctx.engine.critic_backward(dict(zip(CRITIC_KEYS, params)), state, grad_output.to(torch.float32).contiguous(), None, False)
        return _segments(flat, CRITIC_SIZES, params, ctx.needs_input_grad[:10]) + (None, None)


def head_logits(pi_head: torch.nn.Module, logits: torch.Tensor, engine) -> torch.Tensor:
    """`logits` (the `probability` the engine's latest forward returned) attached to the graph of `pi_head`'s parameters."""
    named = dict(pi_head.named_parameters())
    return HeadLogits.apply(*[named[k] for k in PI_KEYS], logits, engine, engine.generation)


def critic_value(critic: torch.nn.Module, state: torch.Tensor, engine) -> torch.Tensor:
    named = dict(critic.named_parameters())
    return CriticValue.apply(*[named[k] for k in CRITIC_KEYS], state, engine)
