"""The entity-context encoder's character CNN (models/models.py:57-61) as one device op:

    from recon_amd import char_word_features
    feat = char_word_features(chars, emb_weight, conv_weight, conv_bias, word_span)        # [S, W, Fo]
    pre[s, t, o]  = conv_bias[o] + sum_k sum_c (keep * emb_weight[chars])[s, t + k, c] * conv_weight[o, c, k]
    feat[s, w, o] = tanh(max over t in [w * word_span, (w + 1) * word_span) of pre[s, t, o])

chars [S, Lc] int64 or int32 with Lc = cfs - 1 + W * word_span, emb_weight [V, C], conv_weight [Fo, C, cfs], conv_bias [Fo].  With fp32 GPU
tensors of a shape `recon_char_features_supported` takes and no dropout factors, the forward is two launches of csrc/char_cnn.hip (the cfs
tables T[k] = E . W[:, :, k]^T, then one wave per word looking them up: no [S, Lc, .] tensor exists; tanh(max) and one position byte per
output element are kept for the backward) and the backward three; both are bitwise reproducible.  Otherwise — CPU tensors, another dtype,
a shape outside the kernels', `keep` given (the masked form has no kernel yet), or a backward under create_graph — the call runs `_chain`,
the op sequence `EntityEmbedding.forward` used to be: value and gradients stay correct.  DESIGN.md section 18.
"""
import torch
import torch.nn.functional as F

from . import _lib


def _chain(chars, emb_weight, conv_weight, conv_bias, word_span, keep=None, padding_idx=0):
    """The stock sequence (models/models.py:57-61): embedding, dropout factors, conv1d, max_pool1d, tanh."""
    char_vec = F.embedding(chars, emb_weight, padding_idx=padding_idx)
    if keep is not None:
        char_vec = char_vec * keep
    char_vec = char_vec.permute(0, 2, 1)
    return torch.tanh(F.max_pool1d(F.conv1d(char_vec, conv_weight, conv_bias), word_span, word_span)).permute(0, 2, 1)


def _geometry(chars, emb_weight, conv_weight, word_span):
    (S, Lc), (V, C), (Fo, _, cfs) = chars.shape, emb_weight.shape, conv_weight.shape
    return S, (Lc - (cfs - 1)) // word_span, word_span, cfs, V, C, Fo


def _workspace(nbytes, device):
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)


class _CharWordFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chars, emb_weight, conv_weight, conv_bias, word_span, padding_idx):
        E, Wc, b = emb_weight.detach().contiguous(), conv_weight.detach().contiguous(), conv_bias.detach().contiguous()
        ids = chars if chars.stride(1) == 1 and (chars.shape[0] == 1 or chars.stride(0) >= chars.shape[1]) else chars.contiguous()
        geo = _geometry(ids, E, Wc, word_span)
        S, W, Fo = geo[0], geo[1], geo[6]
        L = _lib.lib()
        wants = any(ctx.needs_input_grad[1:4])
        out = torch.empty(S, W, Fo, dtype=torch.float32, device=E.device)
        arg = torch.empty(S, W, Fo, dtype=torch.uint8, device=E.device) if wants else None
        ws = _workspace(L.recon_char_features_workspace_bytes(*geo, 0), E.device)
        ld = ids.stride(0) if S > 1 else ids.shape[1]                       # (a single row's stride is arbitrary)
        with _lib.on_device(E.device):
            _lib.check(L.recon_char_features_fwd(ids.data_ptr(), ids.element_size(), ld, E.data_ptr(), Wc.data_ptr(), b.data_ptr(), None, *geo,
                                                 out.data_ptr(), _lib.ptr(arg), ws.data_ptr(), ws.numel(), _lib.current_stream()),
                       "recon_char_features_fwd")
        if wants:
            ctx.save_for_backward(ids, emb_weight, conv_weight, conv_bias, out, arg)
            ctx.geo, ctx.ld, ctx.word_span, ctx.padding_idx = geo, ld, word_span, padding_idx
        return out

    @staticmethod
    def backward(ctx, g_out):
        ids, emb_weight, conv_weight, conv_bias, out, arg = ctx.saved_tensors
        need = ctx.needs_input_grad[1:4]
        if torch.is_grad_enabled():                                          # create_graph: the gradient itself must be differentiable
            with torch.enable_grad():
                y = _chain(ids, emb_weight, conv_weight, conv_bias, ctx.word_span, None, ctx.padding_idx)
                params = [p for p, n in zip((emb_weight, conv_weight, conv_bias), need) if n]
                grads = list(torch.autograd.grad(y, params, g_out, create_graph=True))
            return (None,) + tuple(grads.pop(0) if n else None for n in need) + (None, None)
        geo = ctx.geo
        cfs, V, C, Fo = geo[3], geo[4], geo[5], geo[6]
        L = _lib.lib()
        E, Wc = emb_weight.detach().contiguous(), conv_weight.detach().contiguous()
        g = g_out.contiguous().to(torch.float32)
        g_emb = torch.empty(V, C, dtype=torch.float32, device=g.device)
        g_w = torch.empty(Fo, C, cfs, dtype=torch.float32, device=g.device)
        g_b = torch.empty(Fo, dtype=torch.float32, device=g.device)
        ws = _workspace(L.recon_char_features_workspace_bytes(*geo, 1), g.device)
        pad = -1 if ctx.padding_idx is None else int(ctx.padding_idx)
        with _lib.on_device(g.device):
            _lib.check(L.recon_char_features_bwd(ids.data_ptr(), ids.element_size(), ctx.ld, E.data_ptr(), Wc.data_ptr(), None, g.data_ptr(),
                                                 out.data_ptr(), arg.data_ptr(), *geo, pad, g_emb.data_ptr(), g_w.data_ptr(), g_b.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _lib.current_stream()), "recon_char_features_bwd")
        return None, (g_emb if need[0] else None), (g_w if need[1] else None), (g_b if need[2] else None), None, None


def _fused(chars, emb_weight, conv_weight, conv_bias, word_span, keep):
    if keep is not None or not chars.is_cuda:
        return False
    if not (emb_weight.dtype == conv_weight.dtype == conv_bias.dtype == torch.float32):
        return False
    return bool(_lib.lib().recon_char_features_supported(*_geometry(chars, emb_weight, conv_weight, word_span)))


def char_word_features(chars, emb_weight, conv_weight, conv_bias, word_span, keep=None, padding_idx=0):
    """[S, Lc] ids, [V, C], [Fo, C, cfs], [Fo] -> [S, W, Fo] char-CNN features of every word (models/models.py:57-61), differentiable in the
    three parameters.  keep: None or [S, Lc, C] dropout factors (0 or 1 / (1 - p)) multiplied onto the gathered embedding, drawn by the
    caller (`CharEmbeddings.draw_keep`).  padding_idx: that row of emb_weight's gradient is zero, as with nn.Embedding.  S == 0 gives an
    empty [0, W, Fo] without a launch."""
    word_span = int(word_span)
    if chars.dim() != 2 or chars.dtype not in (torch.int64, torch.int32):
        raise ValueError("char_word_features: chars must be an int64 or int32 [S, Lc] tensor, got %s %s" % (chars.dtype, tuple(chars.shape)))
    if not (emb_weight.dim() == 2 and conv_weight.dim() == 3 and conv_weight.shape[1] == emb_weight.shape[1]
            and tuple(conv_bias.shape) == (conv_weight.shape[0],)):
        raise ValueError("char_word_features: emb_weight [V, C], conv_weight [Fo, C, cfs], conv_bias [Fo] expected, got %s, %s, %s"
                         % (tuple(emb_weight.shape), tuple(conv_weight.shape), tuple(conv_bias.shape)))
    if not (emb_weight.dtype == conv_weight.dtype == conv_bias.dtype and emb_weight.is_floating_point()):
        raise ValueError("char_word_features: emb_weight, conv_weight and conv_bias must share one floating-point dtype")
    cfs = conv_weight.shape[2]
    W = (chars.shape[1] - (cfs - 1)) // word_span if word_span >= 1 else 0
    if word_span < 1 or W < 1 or chars.shape[1] != cfs - 1 + W * word_span:
        raise ValueError("char_word_features: chars has %d columns, expected cfs - 1 + W * word_span with cfs = %d, word_span = %d"
                         % (chars.shape[1], cfs, word_span))
    if keep is not None and (tuple(keep.shape) != (chars.shape[0], chars.shape[1], emb_weight.shape[1]) or keep.dtype != emb_weight.dtype):
        raise ValueError("char_word_features: keep must be [S, Lc, C] of the parameters' dtype, got %s %s" % (keep.dtype, tuple(keep.shape)))
    if not (emb_weight.device == conv_weight.device == conv_bias.device == chars.device and (keep is None or keep.device == chars.device)):
        raise ValueError("char_word_features: the tensors must be on one device")
    if chars.shape[0] == 0:
        return torch.empty(0, W, conv_weight.shape[0], dtype=emb_weight.dtype, device=emb_weight.device)
    if _fused(chars, emb_weight, conv_weight, conv_bias, word_span, keep):
        return _CharWordFeatures.apply(chars, emb_weight, conv_weight, conv_bias, word_span, padding_idx)
    return _chain(chars, emb_weight, conv_weight, conv_bias, word_span, keep, padding_idx)
