"""The entity-context encoder's character CNN (models/models.py:57-61) as one device op:

    from recon_amd import char_word_features
    feat = char_word_features(chars, emb_weight, conv_weight, conv_bias, word_span)        # [S, W, Fo]
    pre[s, t, o]  = conv_bias[o] + sum_k sum_c (keep * emb_weight[chars])[s, t + k, c] * conv_weight[o, c, k]
    feat[s, w, o] = tanh(max over t in [w * word_span, (w + 1) * word_span) of pre[s, t, o])

chars [S, Lc] int64 or int32 with Lc = cfs - 1 + W * word_span, emb_weight [V, C], conv_weight [Fo, C, cfs], conv_bias [Fo].  With fp32 GPU
tensors there are two kernel forms, both bitwise reproducible:
  * no dropout factors, a shape `recon_char_features_supported` takes: the table form of csrc/char_cnn.hip (the cfs tables T[k] = E .
    W[:, :, k]^T, then one wave per word looking them up; two launches forward, three backward);
  * `keep` a `PackedKeep` (one bit per factor and a scalar scale: `pack_keep`, `draw_packed_keep`), a shape `recon_char_masked_supported`
    takes: the masked form of csrc/char_mask.hip, a real fp32 convolution on the fp32 MFMA over the word's masked rows staged in LDS (two
    launches forward, two backward).
Neither writes an [S, Lc, .] tensor; tanh(max) and one position byte per output element are kept for the backward.  Otherwise — CPU
tensors, another dtype, a shape outside the kernels', `keep` an fp32 [S, Lc, C] tensor, or a backward under create_graph — the call runs
`_chain`, the op sequence `EntityEmbedding.forward` used to be: value and gradients stay correct.  DESIGN.md section 18.
"""
import collections

import numpy as np
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


class PackedKeep:
    """Dropout factors of the [S, Lc, C] gathered embedding, one bit each: factor (s, j, c) = scale if bit c % 32 of bits[s, j, c // 32] is
    set, else 0.  bits int32 [S, Lc, ceil(C / 32)], contiguous.  Bits at and above C in the last word are ignored by every consumer."""

    def __init__(self, bits, scale, C):
        self.bits, self.scale, self.C = bits, float(scale), int(C)

    def factors(self, dtype=torch.float32):
        """The [S, Lc, C] tensor of factors `_chain` takes."""
        shifts = torch.arange(32, dtype=torch.int32, device=self.bits.device)
        on = ((self.bits.unsqueeze(-1) >> shifts) & 1).reshape(self.bits.shape[0], self.bits.shape[1], -1)[:, :, :self.C]
        return on.to(dtype) * self.scale


def pack_keep(keep, scale=None):
    """fp32 factors [S, Lc, C] with values in {0, scale} -> PackedKeep, to replay recorded draws.  scale=None takes keep.max(), which
    costs one read of a device value on the host (a synchronisation).  ValueError if a non-zero value differs from the scale."""
    if keep.dim() != 3:
        raise ValueError("pack_keep: keep must be [S, Lc, C], got %s" % (tuple(keep.shape),))
    S, Lc, C = keep.shape
    if scale is None:
        scale = float(keep.max()) if keep.numel() else 1.0
    on = keep != 0
    if bool((on & (keep != scale)).any()):
        raise ValueError("pack_keep: a non-zero factor differs from the scale %r" % (scale,))
    KW = (C + 31) // 32
    padded = torch.zeros(S, Lc, KW * 32, dtype=torch.int64, device=keep.device)
    padded[:, :, :C] = on
    words = (padded.view(S, Lc, KW, 32) << torch.arange(32, dtype=torch.int64, device=keep.device)).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    return PackedKeep(words.contiguous(), scale, C)


_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 on numpy arrays: counter [..., 4] and key [..., 2] (or broadcastable) of 32-bit words -> [..., 4] uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = (np.asarray(key)[..., i].astype(np.uint64) for i in range(2))
    lo = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & lo]
        k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & lo, (k1 + np.uint64(_PHILOX_W1)) & lo
    return np.stack(c, -1).astype(np.uint32)


def keep_threshold(p):
    """The 32-bit threshold of a drop probability p: a bit is set iff its Philox word >= min(2^32 - 1, floor(p 2^32))."""
    return min(2 ** 32 - 1, int(p * 2.0 ** 32))


def _draw_bits_host(S, Lc, C, threshold, seed, offset):
    """The draw definition of include/recon_hip.h (recon_char_keep_bits_draw) in numpy: int32 [S, Lc, KW]."""
    KW, Gp = (C + 31) // 32, (C + 3) // 4
    ctr = (np.arange(S * Lc * Gp, dtype=np.uint64) + np.uint64(offset % 2 ** 64)) if S * Lc else np.zeros(0, np.uint64)
    counter = np.stack([ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), np.zeros_like(ctr), np.zeros_like(ctr)], -1)
    words = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64))
    on = np.zeros((S * Lc, KW * 32), np.uint64)
    on[:, :C] = (words.reshape(S * Lc, Gp * 4) >= np.uint32(threshold))[:, :C]
    packed = (on.reshape(S * Lc, KW, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(packed.view(np.int32).reshape(S, Lc, KW).copy())


def draw_keep_bits(S, Lc, C, threshold, seed, offset, device):
    """int32 [S, Lc, ceil(C / 32)] bits of the counter-based draw for an explicit (seed, offset): one launch of the draw kernel on a GPU
    device, the same definition in numpy on the CPU, bit-identical."""
    device = torch.device(device)
    if device.type != "cuda":
        return _draw_bits_host(S, Lc, C, threshold, seed, offset).to(device)
    bits = torch.empty(S, Lc, (C + 31) // 32, dtype=torch.int32, device=device)
    with _lib.on_device(device):
        _lib.check(_lib.lib().recon_char_keep_bits_draw(bits.data_ptr(), S * Lc, C, threshold, seed % 2 ** 64, offset % 2 ** 64,
                                                        _lib.current_stream()), "recon_char_keep_bits_draw")
    return bits


def draw_packed_keep(S, Lc, C, p, device, generator=None):
    """PackedKeep of Bernoulli(1 - p) bits with scale 1 / (1 - p), counter-based (Philox4x32-10; the definition is at
    recon_char_keep_bits_draw in include/recon_hip.h): one launch on a GPU device, numpy on the CPU, bit-identical for one (seed, offset).
    (seed, offset) are `generator`'s (default: the device's default generator) initial_seed() and get_offset(); the offset is then advanced
    by the Philox counters consumed, rounded up to a multiple of 4, so torch.manual_seed governs the draw and consecutive draws differ.  A
    CPU generator keeps no offset: one is drawn from it (torch.randint), which advances it likewise.  The distribution is dropout's, the
    stream is not torch's.  Reads and sets generator state on the host: not usable under graph capture."""
    device = torch.device(device)
    if not 0.0 <= p < 1.0:
        raise ValueError("draw_packed_keep: p must be in [0, 1), got %r" % (p,))
    if generator is None:
        generator = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()] \
            if device.type == "cuda" else torch.default_generator
    seed = generator.initial_seed()
    n_counters = S * Lc * ((C + 3) // 4)
    if generator.device.type == "cuda":
        offset = generator.get_offset()
        generator.set_offset(offset + (n_counters + 3) // 4 * 4)
    else:
        offset = int(torch.randint(0, 2 ** 60, (), generator=generator)) * 4
    return PackedKeep(draw_keep_bits(S, Lc, C, keep_threshold(p), seed, offset, device), 1.0 / (1.0 - p), C)


# A kernel form of the op: the stem of its C entries (_supported, _workspace_bytes, _fwd, _bwd); how many of the arguments its Function takes
# behind padding_idx are tensors to save (they come first); what goes where the entries take the mask; the factors `_chain` takes for it.
_Form = collections.namedtuple("_Form", "stem n_saved call_extra keep")
_TABLE = _Form("recon_char_features", 0, lambda: (None,), lambda C, dtype: None)                         # csrc/char_cnn.hip
_MASKED = _Form("recon_char_masked", 1, lambda bits, scale: (bits.data_ptr(), scale),                     # csrc/char_mask.hip
                lambda C, dtype, bits, scale: PackedKeep(bits, scale, C).factors(dtype))


def _forward(form, ctx, chars, emb_weight, conv_weight, conv_bias, word_span, padding_idx, *extra):
    """Saves ids, parameters, out, the position bytes and the form's tensors (the masked form's bits) — nothing of size S Lc C."""
    E, Wc, b = emb_weight.detach().contiguous(), conv_weight.detach().contiguous(), conv_bias.detach().contiguous()
    ids, ld = _lib.rows_in_place(chars, chars.shape[1])
    geo = _geometry(ids, E, Wc, word_span)
    S, W, Fo = geo[0], geo[1], geo[6]
    L = _lib.lib()
    wants = any(ctx.needs_input_grad[1:4])
    out = torch.empty(S, W, Fo, dtype=torch.float32, device=E.device)
    arg = torch.empty(S, W, Fo, dtype=torch.uint8, device=E.device) if wants else None
    ws = _lib.workspace(getattr(L, form.stem + "_workspace_bytes")(*geo, 0), E.device)
    with _lib.on_device(E.device):
        _lib.check(getattr(L, form.stem + "_fwd")(ids.data_ptr(), ids.element_size(), ld, E.data_ptr(), Wc.data_ptr(), b.data_ptr(),
                                                  *form.call_extra(*extra), *geo, out.data_ptr(), _lib.ptr(arg), ws.data_ptr(), ws.numel(),
                                                  _lib.current_stream()), form.stem + "_fwd")
    if wants:
        ctx.save_for_backward(ids, emb_weight, conv_weight, conv_bias, out, arg, *extra[:form.n_saved])
        ctx.geo, ctx.ld, ctx.word_span, ctx.padding_idx, ctx.plain = geo, ld, word_span, padding_idx, extra[form.n_saved:]
    return out


def _backward(form, ctx, g_out):
    ids, emb_weight, conv_weight, conv_bias, out, arg, *extra = ctx.saved_tensors
    extra = tuple(extra) + ctx.plain
    need = ctx.needs_input_grad[1:4]
    geo = ctx.geo
    cfs, V, C, Fo = geo[3], geo[4], geo[5], geo[6]
    if torch.is_grad_enabled():                                              # create_graph: the gradient itself must be differentiable
        grads = _lib.recompute_grads(lambda: _chain(ids, emb_weight, conv_weight, conv_bias, ctx.word_span,
                                                    form.keep(C, emb_weight.dtype, *extra), ctx.padding_idx),
                                     (emb_weight, conv_weight, conv_bias), need, g_out, True)
        return (None,) + grads + (None,) * (2 + len(extra))
    L = _lib.lib()
    E, Wc = emb_weight.detach().contiguous(), conv_weight.detach().contiguous()
    g = g_out.contiguous().to(torch.float32)
    g_emb = torch.empty(V, C, dtype=torch.float32, device=g.device)
    g_w = torch.empty(Fo, C, cfs, dtype=torch.float32, device=g.device)
    g_b = torch.empty(Fo, dtype=torch.float32, device=g.device)
    ws = _lib.workspace(getattr(L, form.stem + "_workspace_bytes")(*geo, 1), g.device)
    pad = -1 if ctx.padding_idx is None else int(ctx.padding_idx)
    with _lib.on_device(g.device):
        _lib.check(getattr(L, form.stem + "_bwd")(ids.data_ptr(), ids.element_size(), ctx.ld, E.data_ptr(), Wc.data_ptr(), *form.call_extra(*extra),
                                                  g.data_ptr(), out.data_ptr(), arg.data_ptr(), *geo, pad, g_emb.data_ptr(), g_w.data_ptr(),
                                                  g_b.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream()), form.stem + "_bwd")
    return (None, (g_emb if need[0] else None), (g_w if need[1] else None), (g_b if need[2] else None)) + (None,) * (2 + len(extra))


class _CharWordFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chars, emb_weight, conv_weight, conv_bias, word_span, padding_idx):
        return _forward(_TABLE, ctx, chars, emb_weight, conv_weight, conv_bias, word_span, padding_idx)

    @staticmethod
    def backward(ctx, g_out):
        return _backward(_TABLE, ctx, g_out)


class _CharWordFeaturesMasked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, chars, emb_weight, conv_weight, conv_bias, word_span, padding_idx, bits, scale):
        return _forward(_MASKED, ctx, chars, emb_weight, conv_weight, conv_bias, word_span, padding_idx, bits, scale)

    @staticmethod
    def backward(ctx, g_out):
        return _backward(_MASKED, ctx, g_out)


def _runs(form, chars, emb_weight, conv_weight, conv_bias, word_span):
    if not chars.is_cuda or not (emb_weight.dtype == conv_weight.dtype == conv_bias.dtype == torch.float32):
        return False
    return bool(getattr(_lib.lib(), form.stem + "_supported")(*_geometry(chars, emb_weight, conv_weight, word_span)))


def char_word_features(chars, emb_weight, conv_weight, conv_bias, word_span, keep=None, padding_idx=0):
    """[S, Lc] ids, [V, C], [Fo, C, cfs], [Fo] -> [S, W, Fo] char-CNN features of every word (models/models.py:57-61), differentiable in the
    three parameters.  keep: None, [S, Lc, C] dropout factors (0 or 1 / (1 - p)) multiplied onto the gathered embedding, drawn by the
    caller (`CharEmbeddings.draw_keep`; runs the op chain), or the same factors as a `PackedKeep` (`CharEmbeddings.draw_packed_keep`,
    `pack_keep`; runs the masked kernels).  padding_idx: that row of emb_weight's gradient is zero, as with nn.Embedding.  S == 0 gives
    an empty [0, W, Fo] without a launch."""
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
    packed = isinstance(keep, PackedKeep)
    if packed:
        C = emb_weight.shape[1]
        if (keep.C != C or not torch.is_tensor(keep.bits) or keep.bits.dtype != torch.int32 or not keep.bits.is_contiguous()
                or tuple(keep.bits.shape) != (chars.shape[0], chars.shape[1], (C + 31) // 32)):
            raise ValueError("char_word_features: a PackedKeep needs C = %d and contiguous int32 bits [S, Lc, ceil(C / 32)], got C = %d, %s %s"
                             % (C, keep.C, getattr(keep.bits, "dtype", None), tuple(getattr(keep.bits, "shape", ()))))
    elif keep is not None and (tuple(keep.shape) != (chars.shape[0], chars.shape[1], emb_weight.shape[1]) or keep.dtype != emb_weight.dtype):
        raise ValueError("char_word_features: keep must be [S, Lc, C] of the parameters' dtype, got %s %s" % (keep.dtype, tuple(keep.shape)))
    keep_device = None if keep is None else (keep.bits.device if packed else keep.device)
    if not (emb_weight.device == conv_weight.device == conv_bias.device == chars.device and (keep is None or keep_device == chars.device)):
        raise ValueError("char_word_features: the tensors must be on one device")
    if chars.shape[0] == 0:
        return torch.empty(0, W, conv_weight.shape[0], dtype=emb_weight.dtype, device=emb_weight.device)
    if packed:
        if _runs(_MASKED, chars, emb_weight, conv_weight, conv_bias, word_span):
            return _CharWordFeaturesMasked.apply(chars, emb_weight, conv_weight, conv_bias, word_span, padding_idx, keep.bits, keep.scale)
        keep = keep.factors(emb_weight.dtype)
    if keep is None and _runs(_TABLE, chars, emb_weight, conv_weight, conv_bias, word_span):
        return _CharWordFeatures.apply(chars, emb_weight, conv_weight, conv_bias, word_span, padding_idx)
    return _chain(chars, emb_weight, conv_weight, conv_bias, word_span, keep, padding_idx)
