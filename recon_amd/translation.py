"""RECON's per-relation translation residuals (models/models.py:939-958) as one device op:

    from recon_amd import translation_residuals
    s = translation_residuals(head, tail, W, rel)          # [M, n_rel]
    s[m, r] = sum_d | tanh(head[m] @ W[r])[d] + rel[r, d] - tanh(tail[m] @ W[r])[d] |

head, tail [M, ent_dim] (any row stride: the two halves of one [M, 2 ent_dim] tensor are read in place), W [n_rel, ent_dim, rel_dim],
rel [n_rel, rel_dim].  With fp32 tensors of a shape `recon_rel_translation_supported` takes and a gradient wanted for `rel` at most, the
forward is one launch of csrc/rel_trans.hip (no [M, n_rel, rel_dim] tensor exists; two sign bits per element are kept for the backward)
and the backward one more; both are bitwise reproducible.  If head, tail or W requires a gradient, or the shape or dtype is outside the
kernels', the call runs the op chain `RECON.translation_scores` used to be (two products on small_mm, tanh / + / - / abs / sum in torch):
value and every gradient stay correct.  DESIGN.md section 15.
"""
import torch

from . import _lib

_MAX_LD = 1 << 22          # row stride the kernel's tile descriptors reach (include/recon_hip.h: recon_rel_translation_fwd)


def _chain(head, tail, W, rel):
    """All relations at once: one [M, ent_dim] x [ent_dim, n_rel * rel_dim] product per side on the library-free GEMM."""
    from .gat_layers import small_mm
    n_rel, ent_dim, rel_dim = W.shape
    Wf = W.permute(1, 0, 2).reshape(ent_dim, n_rel * rel_dim)
    h = torch.tanh(small_mm(head.contiguous(), Wf)).view(-1, n_rel, rel_dim)
    t = torch.tanh(small_mm(tail.contiguous(), Wf)).view(-1, n_rel, rel_dim)
    return (h + rel.unsqueeze(0) - t).abs().sum(-1)


class _TranslationResiduals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, head, tail, W, rel):
        Wc, g = W.detach().contiguous(), rel.detach().contiguous()
        M, (n_rel, ent_dim, rel_dim) = head.shape[0], Wc.shape
        (h, ld_h), (t, ld_t) = _lib.rows_in_place(head.detach(), ent_dim, _MAX_LD), _lib.rows_in_place(tail.detach(), ent_dim, _MAX_LD)
        L = _lib.lib()
        out = torch.empty(M, n_rel, dtype=torch.float32, device=h.device)
        saved = None
        if ctx.needs_input_grad[3]:
            saved = torch.empty(L.recon_rel_translation_saved_bytes(M, n_rel, rel_dim) // 4, dtype=torch.int32, device=h.device)
        with _lib.on_device(h.device):
            _lib.check(L.recon_rel_translation_fwd(h.data_ptr(), ld_h, t.data_ptr(), ld_t, Wc.data_ptr(), g.data_ptr(), M, n_rel, ent_dim,
                                                   rel_dim, out.data_ptr(), _lib.ptr(saved), _lib.current_stream()), "recon_rel_translation_fwd")
        if saved is not None:
            ctx.save_for_backward(saved)
            ctx.meta = (M, n_rel, rel_dim)
        return out

    @staticmethod
    def backward(ctx, g_out):
        saved, = ctx.saved_tensors
        M, n_rel, rel_dim = ctx.meta
        g = g_out.contiguous().to(torch.float32)
        g_rel = torch.empty(n_rel, rel_dim, dtype=torch.float32, device=g.device)
        with _lib.on_device(g.device):
            _lib.check(_lib.lib().recon_rel_translation_bwd(g.data_ptr(), saved.data_ptr(), M, n_rel, rel_dim, g_rel.data_ptr(), _lib.current_stream()),
                       "recon_rel_translation_bwd")
        return None, None, None, g_rel


def _fused(head, tail, W, rel):
    if not (head.dtype == tail.dtype == W.dtype == rel.dtype == torch.float32):
        return False
    if torch.is_grad_enabled() and (head.requires_grad or tail.requires_grad or W.requires_grad):
        return False                                                     # those three gradients are the chain's
    n_rel, ent_dim, rel_dim = W.shape
    return bool(_lib.lib().recon_rel_translation_supported(head.shape[0], n_rel, ent_dim, rel_dim))


def translation_residuals(head, tail, W, rel):
    """[M, ent_dim], [M, ent_dim], [n_rel, ent_dim, rel_dim], [n_rel, rel_dim] -> [M, n_rel] L1 translation residuals of every pair in every
    relation's space (models/models.py:939-958).  GPU tensors on one device; M == 0 gives an empty [0, n_rel] without a launch."""
    _lib.require_gpu(head, tail, W, rel)
    if not (head.dim() == 2 and tail.shape == head.shape and W.dim() == 3 and W.shape[1] == head.shape[1] and tuple(rel.shape) == (W.shape[0], W.shape[2])):
        raise ValueError("translation_residuals: head, tail [M, ent_dim], W [n_rel, ent_dim, rel_dim], rel [n_rel, rel_dim] expected, got %s, %s, %s, %s"
                         % (tuple(head.shape), tuple(tail.shape), tuple(W.shape), tuple(rel.shape)))
    if not (tail.device == W.device == rel.device == head.device):
        raise ValueError("translation_residuals: the four tensors must be on one device")
    if head.shape[0] == 0:
        return torch.empty(0, W.shape[0], dtype=rel.dtype, device=rel.device)
    if _fused(head, tail, W, rel):
        return _TranslationResiduals.apply(head, tail, W, rel)
    return _chain(head, tail, W, rel)
