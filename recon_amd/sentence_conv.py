"""The sentence convolution and pool of the per-pair baselines CNN and PCNN (models/baselines.py:237-247 and :297-308) as one device op:

    from recon_amd import sentence_conv_pool
    out = sentence_conv_pool(sentence, positions, word_table, pos_table_0, pos_table_1, weights, biases,
                             segments=None, keep=None, pool_keep=None, activation="none", pos_padding_idx=0)      # [B, n E]
    x[b, t]          = (keep * word_table[sentence[b, t]] | pos_table_0[positions[b, 0, t]] | pos_table_1[positions[b, 1, t]])
    conv_i[b, e, t]  = bias_i[e] + sum_j sum_c w_i[e, c, j] x[b, t + j - pad_i, c]                    (x zero outside 0..T-1)
    segments None:      pad_i = 0, T_out = T - k_i + 1, pooled[b, i E + e] = max_t conv_i[b, e, t]                      (CNN)
    segments [B, 3, T]: one weight, k odd, pad = k // 2, pooled[b, s E + e] = max_t conv[b, e, t] segments[b, s, t]      (PCNN)
    out = act(pool_keep * pooled)

sentence [B, T] int32/int64, positions [B, 2, T] int8/int32/int64, word_table [V, Dw], pos_table_0/1 [P, Dp], weights a list of 1..4
[E, Cin, k_i] tensors in nn.Conv1d's layout with Cin = Dw + 2 Dp, biases a list of [E]; keep None, a `PackedKeep` over [B, T, Dw] or
fp32 [B, T, Dw] factors; pool_keep None or [B, n E] factors; activation "none", "tanh" or "relu".  The segment factors multiply, as the
reference has it: a position whose factor is 0 contributes exactly 0 and takes no gradient.  An exact tie takes the lowest position.
Row pos_padding_idx of both position tables is read as it is and gets a zero gradient; row 0 of word_table is an ordinary row.

With fp32 GPU tensors, a word_table that requires no gradient and a shape `recon_sent_conv_supported` takes (T <= 128, Cin <= 320,
E <= 1024, k <= 9, four weights, and 2 P Dp <= 4096 and 2 T Dp <= 4096 for the position tables' backward: at T = 128 and P = 257 that is
Dp <= 7) the kernels of csrc/sent_conv.hip run: two launches forward (the weights K-major; gather, product on the
fp32 MFMA and pool), at most three backward, no atomics, bitwise reproducible.  Neither x, its transpose, a convolution output nor a
masked copy is written: the op saves references to its inputs, out and one position byte per output (255: the maximum was the 0 of a
zero-factor position).  Differentiable in both position tables, every weight and every bias; an input that does not require a
gradient gets none and costs nothing.  The backward destroys nothing.  An id outside its table raises ValueError (one host read of a
status word per forward, a synchronisation of the calling stream; the word is the stream's own; inside `ids_prechecked()` one read where
the context ends instead).  Otherwise — CPU tensors, another dtype, a word_table that requires a gradient, a shape the library refuses,
a backward under create_graph — the call runs `_chain`, the reference's lines as torch ops.  DESIGN.md sections 31 and 32.
"""
import contextlib
import ctypes
import threading

import torch
import torch.nn.functional as F

from . import _lib
from .char_features import PackedKeep

MAX_T, MAX_CIN, MAX_E, MAX_K, MAX_WEIGHTS = 128, 320, 1024, 9, 4          # kScMax* of csrc/sent_conv.hip
NO_POSITION = 255                                                         # kScNone
ACTIVATIONS = {"none": 0, "tanh": 1, "relu": 2}


def _act(x, activation):
    return torch.tanh(x) if activation == "tanh" else (torch.relu(x) if activation == "relu" else x)


def _chain(sentence, positions, word_table, pos_table_0, pos_table_1, weights, biases, segments=None, keep=None, pool_keep=None,
           activation="none", pos_padding_idx=0):
    """The stock lines (models/baselines.py:237-247 / :297-308): the gathers, the factors, cat, transpose, the Conv1d's, max, the pooled
    factors, the activation."""
    word = F.embedding(sentence.long(), word_table)
    if keep is not None:
        word = word * keep
    pos0 = F.embedding(positions[:, 0, :].long(), pos_table_0, padding_idx=pos_padding_idx)
    pos1 = F.embedding(positions[:, 1, :].long(), pos_table_1, padding_idx=pos_padding_idx)
    merged = torch.cat([word, pos0, pos1], dim=2).transpose(1, 2)
    if segments is None:
        pooled = torch.cat([torch.max(F.conv1d(merged, w, b), dim=2)[0] for w, b in zip(weights, biases)], dim=1)
    else:
        conv = F.conv1d(merged, weights[0], biases[0], padding=weights[0].shape[2] // 2)
        pooled = torch.cat([torch.max(conv * segments[:, s].unsqueeze(1), dim=2)[0] for s in range(3)], dim=1)
    if pool_keep is not None:
        pooled = pooled * pool_keep
    return _act(pooled, activation)


_STATUS = {}


def _status(dev, stream):
    """One zeroed int32 per device and stream: the kernels set it to 1 at an id outside its table; reset here after it was seen.  A
    forward on another stream has a word of its own, so neither reads nor clears this one's."""
    s = _STATUS.get((dev, stream))
    if s is None:
        with torch.cuda.device(dev):
            s = _STATUS[(dev, stream)] = torch.zeros(1, dtype=torch.int32, device=dev)
    return s


def _outside(V, P):
    return ValueError("sentence_conv_pool: a word id outside [0, %d) or a position id outside [0, %d)" % (V, P))


_PRECHECKED = threading.local()


@contextlib.contextmanager
def ids_prechecked():
    """For a loop whose ids were checked on the host beforehand (`PairData.check_model`; `run_epoch` over a `PairData` enters it): inside,
    `sentence_conv_pool` launches exactly as outside — an id outside its table still reads row 0 and still sets the stream's status word —
    but the forward does not read the word, so it does not stall the host.  On leaving, the word of every (device, stream) the
    context's forwards used is read once; a set word is cleared and raises the ValueError the forward would have raised.  Thread-local;
    a context inside another leaves the reading to the outer one.  When an exception leaves the context, set words are cleared and the
    exception goes on."""
    if getattr(_PRECHECKED, "used", None) is not None:
        yield
        return
    used = _PRECHECKED.used = {}
    try:
        yield
    except BaseException:
        _PRECHECKED.used = None
        _read_words(used)
        raise
    _PRECHECKED.used = None
    bad = _read_words(used)
    if bad:
        raise _outside(*bad[0])


def _read_words(used):
    """One read per word; clears the set ones and returns their (V, P)."""
    bad = []
    for status, stream, V, P in used.values():
        with torch.cuda.stream(stream):                               # the read and the clear in the forwards' own order
            if int(status):
                status.zero_()
                bad.append((V, P))
    return bad


def _ks(weights):
    return (ctypes.c_int32 * len(weights))(*[w.shape[2] for w in weights])


class _SentenceConvPool(torch.autograd.Function):
    """csrc/sent_conv.hip: saves references to its inputs, out and the position bytes — nothing else."""

    @staticmethod
    def forward(ctx, meta, sentence, positions, word_table, pos_table_0, pos_table_1, segments, keep_bits, keep_f, pool_keep, *params):
        wants, activation, pad_idx, scale = meta
        lib = _lib.lib()
        n = len(params) // 2
        weights, biases = params[:n], params[n:]
        B, T = sentence.shape
        (V, Dw), (P, Dp), E = word_table.shape, pos_table_0.shape, weights[0].shape[0]
        dev = word_table.device
        n_out = 3 if segments is not None else n
        out = torch.empty(B, n_out * E, dtype=torch.float32, device=dev)
        at = torch.empty(B, n_out * E, dtype=torch.uint8, device=dev) if wants else None
        ks = _ks(weights)
        ws = _lib.workspace(lib.recon_sent_conv_workspace_bytes(B, T, Dw, Dp, P, E, ks, n, int(segments is not None), 0), dev)
        with _lib.on_device(dev):
            status = _status(dev, _lib.current_stream())
            _lib.check(lib.recon_sent_conv_fwd(sentence.data_ptr(), sentence.element_size(), positions.data_ptr(), positions.element_size(),
                                               word_table.data_ptr(), V, pos_table_0.data_ptr(), pos_table_1.data_ptr(), P, _lib.ptr(keep_bits),
                                               scale, _lib.ptr(keep_f), _lib.ptr(segments), _lib.ptr_array([w.detach() for w in weights]),
                                               _lib.ptr_array([b.detach() for b in biases]), ks, n, _lib.ptr(pool_keep), ACTIVATIONS[activation],
                                               B, T, Dw, Dp, E, out.data_ptr(), _lib.ptr(at), status.data_ptr(), ws.data_ptr(), ws.numel(),
                                               _lib.current_stream()), "recon_sent_conv_fwd")
        used = getattr(_PRECHECKED, "used", None)
        if used is not None:                                              # ids_prechecked(): the word is read where the context ends
            key = (dev, _lib.current_stream())
            if key not in used:
                used[key] = (status, torch.cuda.current_stream(dev), V, P)
        elif B and int(status):
            status.zero_()
            raise _outside(V, P)
        ctx.set_materialize_grads(False)
        if wants:
            ctx.save_for_backward(sentence, positions, word_table, pos_table_0, pos_table_1, segments, keep_bits, keep_f, pool_keep, out, at, *params)
            ctx.meta = meta
        return out

    @staticmethod
    def backward(ctx, g_out):
        sentence, positions, word_table, pos_table_0, pos_table_1, segments, keep_bits, keep_f, pool_keep, out, at, *params = ctx.saved_tensors
        _, activation, pad_idx, scale = ctx.meta
        n = len(params) // 2
        weights, biases = params[:n], params[n:]
        need = [ctx.needs_input_grad[4], ctx.needs_input_grad[5]] + list(ctx.needs_input_grad[10:])
        if g_out is None or not any(need):
            return (None,) * (10 + 2 * n)
        B, T = sentence.shape
        (V, Dw), (P, Dp), E = word_table.shape, pos_table_0.shape, weights[0].shape[0]
        if torch.is_grad_enabled():                                      # create_graph: the gradient itself must be differentiable
            keep = PackedKeep(keep_bits, scale, Dw).factors(word_table.dtype) if keep_bits is not None else keep_f
            rerun = lambda: _chain(sentence, positions, word_table, pos_table_0, pos_table_1, weights, biases, segments, keep, pool_keep,
                                   activation, pad_idx)
            grads = _lib.recompute_grads(rerun, [pos_table_0, pos_table_1] + list(params), need, g_out, True)
            return (None,) * 4 + grads[:2] + (None,) * 4 + grads[2:]
        lib = _lib.lib()
        dev = word_table.device
        g = g_out.to(torch.float32).contiguous()
        g_p0 = torch.empty_like(pos_table_0) if need[0] else None
        g_p1 = torch.empty_like(pos_table_1) if need[1] else None
        g_par = [torch.empty_like(p) if nd else None for p, nd in zip(params, need[2:])]
        ks = _ks(weights)
        ws = _lib.workspace(lib.recon_sent_conv_workspace_bytes(B, T, Dw, Dp, P, E, ks, n, int(segments is not None), 1), dev)
        with _lib.on_device(dev):
            _lib.check(lib.recon_sent_conv_bwd(sentence.data_ptr(), sentence.element_size(), positions.data_ptr(), positions.element_size(),
                                               word_table.data_ptr(), V, pos_table_0.data_ptr(), pos_table_1.data_ptr(), P, _lib.ptr(keep_bits),
                                               scale, _lib.ptr(keep_f), _lib.ptr(segments), _lib.ptr_array([w.detach() for w in weights]), ks, n,
                                               _lib.ptr(pool_keep), ACTIVATIONS[activation], B, T, Dw, Dp, E, out.data_ptr(), at.data_ptr(),
                                               g.data_ptr(), -1 if pad_idx is None else int(pad_idx), _lib.ptr(g_p0), _lib.ptr(g_p1),
                                               _lib.ptr_array(g_par[:n]), _lib.ptr_array(g_par[n:]), ws.data_ptr(), ws.numel(),
                                               _lib.current_stream()), "recon_sent_conv_bwd")
        return (None,) * 4 + (g_p0, g_p1) + (None,) * 4 + tuple(g_par)


def _fused(sentence, word_table, pos_table_0, pos_table_1, weights, biases, segments, keep, pool_keep):
    floats = [word_table, pos_table_0, pos_table_1] + list(weights) + list(biases)
    floats += [t for t in (segments, pool_keep) if t is not None] + ([keep] if torch.is_tensor(keep) else [])
    if not word_table.is_cuda or any(t.dtype != torch.float32 for t in floats) or word_table.requires_grad:
        return False
    B, T = sentence.shape
    return bool(_lib.lib().recon_sent_conv_supported(B, T, word_table.shape[1], pos_table_0.shape[1], pos_table_0.shape[0], weights[0].shape[0],
                                                     _ks(weights), len(weights), int(segments is not None)))


def _shape(t):
    return tuple(getattr(t, "shape", ())) if torch.is_tensor(t) else type(t).__name__


def sentence_conv_pool(sentence, positions, word_table, pos_table_0, pos_table_1, weights, biases, segments=None, keep=None, pool_keep=None,
                       activation="none", pos_padding_idx=0):
    """[B, T] ids, [B, 2, T] ids, [V, Dw], [P, Dp], [P, Dp], n x [E, Dw + 2 Dp, k_i], n x [E] -> [B, n E] (segments [B, 3, T]: one weight,
    [B, 3 E]): the pooled sentence convolutions of the CNN and PCNN baselines (models/baselines.py:237-247, :297-308), differentiable in
    the position tables, the weights and the biases.  B = 0 gives an empty result without a launch."""
    name = "sentence_conv_pool: "
    if not (torch.is_tensor(sentence) and sentence.dim() == 2 and sentence.dtype in (torch.int32, torch.int64)):
        raise ValueError(name + "sentence must be an int32 or int64 [B, T] tensor, got %s %s" % (getattr(sentence, "dtype", None), _shape(sentence)))
    B, T = sentence.shape
    if not (torch.is_tensor(positions) and positions.dtype in (torch.int8, torch.int32, torch.int64) and tuple(positions.shape) == (B, 2, T)):
        raise ValueError(name + "positions must be an int8, int32 or int64 [B, 2, T] = [%d, 2, %d] tensor, got %s %s"
                         % (B, T, getattr(positions, "dtype", None), _shape(positions)))
    tables = (word_table, pos_table_0, pos_table_1)
    if not all(torch.is_tensor(t) and t.dim() == 2 and t.is_floating_point() and t.dtype == word_table.dtype and t.shape[0] >= 1
               and t.shape[1] >= 1 for t in tables) or pos_table_0.shape != pos_table_1.shape:
        raise ValueError(name + "word_table [V, Dw] and pos_table_0, pos_table_1 [P, Dp] must share one floating-point dtype, got %s"
                         % [(getattr(t, "dtype", None), _shape(t)) for t in tables])
    Dw, Dp = word_table.shape[1], pos_table_0.shape[1]
    Cin = Dw + 2 * Dp
    if not isinstance(weights, (list, tuple)) or not isinstance(biases, (list, tuple)) or not 1 <= len(weights) <= MAX_WEIGHTS \
            or len(biases) != len(weights):
        raise ValueError(name + "weights and biases must be lists of 1..%d tensors of one length" % MAX_WEIGHTS)
    E = weights[0].shape[0] if torch.is_tensor(weights[0]) and weights[0].dim() == 3 else 0
    for w, b in zip(weights, biases):
        if not (torch.is_tensor(w) and w.dim() == 3 and w.dtype == word_table.dtype and w.shape[0] == E >= 1 and w.shape[1] == Cin and w.shape[2] >= 1):
            raise ValueError(name + "a weight must be [E, Cin, k] = [%d, %d, k] of the tables' dtype, got %s %s"
                             % (E, Cin, getattr(w, "dtype", None), _shape(w)))
        if not (torch.is_tensor(b) and tuple(b.shape) == (E,) and b.dtype == word_table.dtype):
            raise ValueError(name + "a bias must be [E] = [%d] of the tables' dtype, got %s %s" % (E, getattr(b, "dtype", None), _shape(b)))
    if activation not in ACTIVATIONS:
        raise ValueError(name + "activation must be one of %s, got %r" % (sorted(ACTIVATIONS), activation))
    if segments is None:
        for w in weights:
            if w.shape[2] > T:
                raise ValueError(name + "a window of k = %d does not fit T = %d positions" % (w.shape[2], T))
        n_out = len(weights)
    else:
        if not (torch.is_tensor(segments) and tuple(segments.shape) == (B, 3, T) and segments.dtype == word_table.dtype):
            raise ValueError(name + "segments must be [B, 3, T] = [%d, 3, %d] of the tables' dtype, got %s %s"
                             % (B, T, getattr(segments, "dtype", None), _shape(segments)))
        if len(weights) != 1 or weights[0].shape[2] % 2 == 0:
            raise ValueError(name + "with segments there is exactly one weight, of an odd k, got %s" % [_shape(w) for w in weights])
        n_out = 3
    packed = isinstance(keep, PackedKeep)
    if packed:
        if (keep.C != Dw or not torch.is_tensor(keep.bits) or keep.bits.dtype != torch.int32 or not keep.bits.is_contiguous()
                or tuple(keep.bits.shape) != (B, T, (Dw + 31) // 32)):
            raise ValueError(name + "a PackedKeep needs C = %d and contiguous int32 bits [B, T, ceil(Dw / 32)], got C = %d, %s %s"
                             % (Dw, keep.C, getattr(keep.bits, "dtype", None), _shape(keep.bits)))
    elif keep is not None and not (torch.is_tensor(keep) and tuple(keep.shape) == (B, T, Dw) and keep.dtype == word_table.dtype):
        raise ValueError(name + "keep must be [B, T, Dw] = [%d, %d, %d] of the tables' dtype, got %s %s"
                         % (B, T, Dw, getattr(keep, "dtype", None), _shape(keep)))
    if pool_keep is not None and not (torch.is_tensor(pool_keep) and tuple(pool_keep.shape) == (B, n_out * E) and pool_keep.dtype == word_table.dtype):
        raise ValueError(name + "pool_keep must be [B, n E] = [%d, %d] of the tables' dtype, got %s %s"
                         % (B, n_out * E, getattr(pool_keep, "dtype", None), _shape(pool_keep)))
    others = [positions, pos_table_0, pos_table_1, segments, keep.bits if packed else keep, pool_keep] + list(weights) + list(biases)
    if any(t is not None and t.device != word_table.device for t in others) or sentence.device != word_table.device:
        raise ValueError(name + "the tensors must be on one device")
    if B == 0:
        return word_table.new_zeros((0, n_out * E))
    if _fused(sentence, word_table, pos_table_0, pos_table_1, weights, biases, segments, keep, pool_keep):
        params = list(weights) + list(biases)
        # (inside the function grad mode is off and needs_input_grad ignores no_grad: whether a backward can follow is decided here)
        wants = torch.is_grad_enabled() and any(t.requires_grad for t in [pos_table_0, pos_table_1] + params)
        c = lambda t: None if t is None else t.detach().contiguous()
        meta = (wants, activation, pos_padding_idx, keep.scale if packed else 1.0)
        return _SentenceConvPool.apply(meta, sentence.contiguous(), positions.contiguous(), word_table.detach().contiguous(),
                                       pos_table_0 if pos_table_0.is_contiguous() else pos_table_0.contiguous(),
                                       pos_table_1 if pos_table_1.is_contiguous() else pos_table_1.contiguous(), c(segments),
                                       keep.bits if packed else None, None if packed else c(keep), c(pool_keep),
                                       *[p if p.is_contiguous() else p.contiguous() for p in params])
    if packed:
        keep = keep.factors(word_table.dtype)
    return _chain(sentence, positions, word_table, pos_table_0, pos_table_1, weights, biases, segments, keep, pool_keep, activation,
                  pos_padding_idx)
