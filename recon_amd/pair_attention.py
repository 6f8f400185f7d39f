"""ContextAware's "attention over ghosts" (models/baselines.py:86-112) as one device op:

    from recon_amd import pair_context_attention
    out = pair_context_attention(states, weight)                   # [B, C, D], [D, D] -> [B, C, 2 D]
    Mem = states W^T;  S[b, i, j] = Mem[b, i] . states[b, j] for j != i;  P[b, i, :] = softmax over j != i, P[b, i, i] = 0
    out[b, i] = (states[b, i] | sum_j P[b, i, j] states[b, j])

the per-sentence self-attention over the pair states with the diagonal left out.  Every pair attends over all the others of its
sentence, padding pairs included (the reference has no mask).  C = 1 gives a zero right half and no gradient through it.  Unlike the
reference, whose `.squeeze()` at :107 drops the batch axis of a batch of one, any B works.  Non-finite inputs are outside the contract:
the kernels give NaN in a row of P whose scores hold a NaN or an infinity.

With fp32 GPU tensors and a shape `recon_pair_attention_supported` takes (C <= MAX_PAIRS, D a multiple of 4 up to 1024) the kernels of
csrc/pair_attn.hip run behind `pair_transitions(states, [weight], [None], "linear")`, which forms Mem and whose backward yields g_weight
and the part of g_states through Mem: one launch forward, two backward, fp32 on the fp32 MFMA, bitwise reproducible.  Saved: references
to states and Mem, and P [B, C, C] — nothing of size B C (C - 1) D exists.  The backward destroys nothing.  Differentiable in both
arguments.  Otherwise — CPU tensors, another dtype, a shape the library refuses — the call runs `_chain`, the batched torch form; a
backward under create_graph runs the gradient's own formulas as torch ops (`_attend_grads`), so that it can be differentiated again.
DESIGN.md section 30.
"""
import torch

from . import _lib
from .transitions import pair_transitions

MAX_PAIRS = 160                   # kPaMaxPairs of csrc/pair_attn.hip: n = 13 entities give 156 pairs


def _attend(states, memory):
    """The batched torch form behind Mem: scores with the diagonal at -inf, softmax, bmm, cat.  C = 1 apart: a row of -inf alone gives NaN;
    P is then the score times zero, the empty softmax with zero gradients (as the reference's tensors of zero rows give), not None."""
    C = states.shape[1]
    scores = torch.bmm(memory, states.transpose(1, 2))
    if C == 1:
        P = scores * 0
    else:
        P = torch.softmax(scores.masked_fill(torch.eye(C, dtype=torch.bool, device=states.device), float("-inf")), dim=2)
    return torch.cat([states, torch.bmm(P, states)], dim=2)


def _attend_grads(states, memory, g_out):
    """(g_states, g_memory) of `_attend` as differentiable torch ops, with memory held an input of its own (the part of g_states through
    Mem is `pair_transitions`' to add).  `_lib.recompute_grads` cannot serve here: the saved memory carries its history, which leads back
    to states, and a gradient taken through the recomputed graph would count that path twice."""
    C, D = states.shape[1], states.shape[2]
    scores = torch.bmm(memory, states.transpose(1, 2))
    if C == 1:
        P = scores * 0
    else:
        P = torch.softmax(scores.masked_fill(torch.eye(C, dtype=torch.bool, device=states.device), float("-inf")), dim=2)
    g_left, g_ctx = g_out[:, :, :D], g_out[:, :, D:]
    T = torch.bmm(g_ctx, states.transpose(1, 2))
    g_S = P * (T - (P * T).sum(dim=2, keepdim=True))
    return g_left + torch.bmm(P.transpose(1, 2), g_ctx) + torch.bmm(g_S.transpose(1, 2), memory), torch.bmm(g_S, states)


def _chain(states, weight):
    """models/baselines.py:86-112 as batched torch ops: the second implementation (CPU tensors, another dtype, an unsupported shape)."""
    return _attend(states, states @ weight.t())


def _rows(x, inner):
    """x [B, C, inner] as the kernels read it: B C rows at one 4-element-aligned stride from a 16-byte aligned base (a copy where the view is not)."""
    flat, ld = _lib.rows_in_place(x, inner)
    if ld % 4 or flat.data_ptr() % 16:
        flat, ld = flat.contiguous(), inner
    return flat, ld


class _PairAttention(torch.autograd.Function):
    """csrc/pair_attn.hip over (states, memory): saves references to the two and P — nothing else."""

    @staticmethod
    def forward(ctx, wants, states, memory):
        B, C, D = states.shape
        s, ld_s = _rows(states.detach(), D)
        m, ld_m = _rows(memory.detach(), D)
        dev = states.device
        out = torch.empty((B, C, 2 * D), dtype=torch.float32, device=dev)
        P = torch.empty((B, C, C), dtype=torch.float32, device=dev) if wants else None
        with _lib.on_device(dev):
            _lib.check(_lib.lib().recon_pair_attention_fwd(s.data_ptr(), ld_s, m.data_ptr(), ld_m, B, C, D, out.data_ptr(), 2 * D, _lib.ptr(P),
                                                           _lib.current_stream()), "recon_pair_attention_fwd")
        ctx.set_materialize_grads(False)
        if wants:
            ctx.save_for_backward(states, memory, P)
        return out

    @staticmethod
    def backward(ctx, g_out):
        states, memory, P = ctx.saved_tensors
        need = ctx.needs_input_grad[1:]
        if g_out is None or not any(need):
            return None, None, None
        if torch.is_grad_enabled():                                      # create_graph: the gradient itself must be differentiable
            g_states, g_memory = _attend_grads(states, memory, g_out)
            return None, g_states if need[0] else None, g_memory if need[1] else None
        B, C, D = states.shape
        lib = _lib.lib()
        s, ld_s = _rows(states.detach(), D)
        m, ld_m = _rows(memory.detach(), D)
        g, ld_g = _rows(g_out.to(torch.float32), 2 * D)
        dev = states.device
        g_states = torch.empty((B, C, D), dtype=torch.float32, device=dev) if need[0] else None
        g_memory = torch.empty((B, C, D), dtype=torch.float32, device=dev) if need[1] else None
        ws = _lib.workspace(lib.recon_pair_attention_workspace_bytes(B, C, D, 1), dev)
        with _lib.on_device(dev):
            _lib.check(lib.recon_pair_attention_bwd(s.data_ptr(), ld_s, m.data_ptr(), ld_m, P.data_ptr(), g.data_ptr(), ld_g, B, C, D,
                                                    _lib.ptr(g_states), _lib.ptr(g_memory), ws.data_ptr(), ws.numel(), _lib.current_stream()),
                       "recon_pair_attention_bwd")
        return None, g_states, g_memory


def _fused(states, weight):
    if not states.is_cuda or states.dtype != torch.float32:
        return False
    B, C, D = states.shape
    if B == 0 or not _lib.lib().recon_pair_attention_supported(B, C, D):
        return False
    return max(_rows(states, D)[1], 2 * D) < 2 ** 31


def pair_context_attention(states, weight):
    """[B, C, D], [D, D] -> [B, C, 2 D]: (states | attention over the other pairs of the sentence), differentiable in both arguments
    (models/baselines.py:86-112; weight is linear1.weight).  B = 0 gives an empty output without a launch."""
    if not torch.is_tensor(states) or states.dim() != 3 or not states.is_floating_point():
        raise ValueError("pair_context_attention: states must be a floating-point [B, C, D] tensor, got %s %s"
                         % (getattr(states, "dtype", type(states).__name__), tuple(getattr(states, "shape", ()))))
    D = states.shape[2]
    if not torch.is_tensor(weight) or tuple(weight.shape) != (D, D) or weight.dtype != states.dtype:
        raise ValueError("pair_context_attention: weight must be [D, D] = [%d, %d] of states' dtype %s, got %s %s"
                         % (D, D, states.dtype, getattr(weight, "dtype", type(weight).__name__), tuple(getattr(weight, "shape", ()))))
    if weight.device != states.device:
        raise ValueError("pair_context_attention: the tensors must be on one device, got %s and %s" % (states.device, weight.device))
    if _fused(states, weight):
        memory = pair_transitions(states, [weight], [None], "linear")[0]
        # (inside the function grad mode is off and needs_input_grad ignores no_grad: whether a backward can follow is decided here)
        wants = torch.is_grad_enabled() and (states.requires_grad or memory.requires_grad)
        return _PairAttention.apply(wants, states, memory)
    return _chain(states, weight)
