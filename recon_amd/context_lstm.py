"""The entity-context encoder's line LSTM (models/models.py:56-70) as one device op:

    from recon_amd import context_line_states
    states = context_line_states(lstm, feat, words, word_table)                     # [S, 2H]
    x[s, t]   = (word_table[words[s, t]] | feat[s, t])                              # never written
    states[s] = (h of the forward direction after t = T - 1 | h of the reverse direction after t = 0)

lstm an nn.LSTM, feat [S, T, Fc] (a strided view with unit last stride is read in place), words [S, T] int64 or int32 and word_table
[Vw, Dw] (both or neither).  With fp32 GPU tensors, a one-layer bidirectional batch_first nn.LSTM with bias, without projection and with
dropout 0, and a shape `recon_ctx_lstm_supported` takes, the kernels of csrc/ctx_lstm.hip run: two launches forward, four backward, all
fp32 on the fp32 MFMA, bitwise reproducible.  Neither the gathered word vectors, nor the concatenation, nor the [S, T, 2H] outputs are
written; for the backward the forward keeps gates and cell state (5 H floats per direction, sequence and step), which the backward
consumes.  Otherwise — CPU tensors, another dtype, another kind of LSTM, a shape outside the kernels', a backward under create_graph or a
second backward over a retained graph — the call runs `_chain`, the op sequence `EntityEmbedding.forward` used to be.  DESIGN.md
section 20.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, _lstm
from ._lstm import _PARAMS, _kernel_lstm           # (importable from here under these names)

BWD_MAX_WORKGROUPS = 128          # kClMaxWg of csrc/ctx_lstm.hip: the weight-gradient pass gives each of them ceil(S / 128) sequences


def _chain(lstm, feat, words=None, word_table=None, padding_idx=None):
    """The stock sequence (models/models.py:56-70): embedding, cat, lstm, the reshape of h_n of the last layer."""
    x = feat if words is None else torch.cat((F.embedding(words, word_table, padding_idx=padding_idx), feat), -1)
    _, (h_n, _) = lstm(x)
    dirs = 2 if lstm.bidirectional else 1
    h_n = h_n.view(lstm.num_layers, dirs, x.shape[0], -1)[-1]
    return h_n.permute(1, 0, 2).reshape(x.shape[0], -1)


class _ContextLineStates(torch.autograd.Function):
    """csrc/ctx_lstm.hip: saves the ids, references to the inputs, out and the saved-state buffer — nothing of size S T I."""

    @staticmethod
    def forward(ctx, lstm, padding_idx, wants, feat, words, word_table, *params):
        L = _lib.lib()
        x, ld_feat = _lib.rows_in_place(feat.detach(), feat.shape[2])
        S, T, Fc = x.shape
        H = params[1].shape[1]
        Dw = 0 if words is None else word_table.shape[1]
        ids, ld_words, table = None, 0, None
        if words is not None:
            ids, ld_words = _lib.rows_in_place(words, T)
            table = word_table.detach().contiguous()
        p = [q.detach().contiguous() for q in params]
        geo = (S, T, Dw, Fc, H)
        out = torch.empty(S, 2 * H, dtype=torch.float32, device=x.device)
        saved = torch.empty(L.recon_ctx_lstm_saved_bytes(*geo), dtype=torch.uint8, device=x.device) if wants else None
        ws = _lib.workspace(L.recon_ctx_lstm_workspace_bytes(*geo, 0), x.device)
        with _lib.on_device(x.device):
            _lib.check(L.recon_ctx_lstm_fwd(_lib.ptr(ids), ids.element_size() if ids is not None else 8, ld_words, _lib.ptr(table),
                                            table.shape[0] if table is not None else 0, x.data_ptr(), ld_feat, *[q.data_ptr() for q in p],
                                            *geo, out.data_ptr(), _lib.ptr(saved), ws.data_ptr(), ws.numel(), _lib.current_stream()),
                       "recon_ctx_lstm_fwd")
        if wants:
            ctx.save_for_backward(feat, ids, word_table, out, saved, *params)
            ctx.lstm, ctx.padding_idx, ctx.geo, ctx.consumed = lstm, padding_idx, geo, False
        return out

    @staticmethod
    def backward(ctx, g_out):
        feat, ids, word_table, out, saved, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        S, T, Dw, Fc, H = ctx.geo
        def stock():
            safe = None if ids is None else ids.clamp(0, word_table.shape[0] - 1)               # as the kernels clamp them
            return _chain(ctx.lstm, feat, safe, word_table, ctx.padding_idx)
        grads = _lstm._recompute(ctx, stock, (feat, None, word_table) + tuple(params), need[3:], g_out)
        if grads is not None:
            return (None, None, None) + grads
        L = _lib.lib()
        x, ld_feat = _lib.rows_in_place(feat.detach(), Fc)
        ld_words = 0
        table = None
        if ids is not None:
            ids, ld_words = _lib.rows_in_place(ids, T)
            table = word_table.detach().contiguous()
        p = [q.detach().contiguous() for q in params]
        g = g_out.contiguous().to(torch.float32)
        dev = g.device
        d_feat = torch.empty(S, T, Fc, dtype=torch.float32, device=dev) if need[3] else None
        d_wv = torch.empty(S, T, Dw, dtype=torch.float32, device=dev) if (ids is not None and need[5]) else None
        gp = [torch.empty_like(q) for q in p]
        ws = _lib.workspace(L.recon_ctx_lstm_workspace_bytes(*ctx.geo, 1), dev)
        with _lib.on_device(dev):
            _lib.check(L.recon_ctx_lstm_bwd(_lib.ptr(ids), ids.element_size() if ids is not None else 8, ld_words, _lib.ptr(table),
                                            table.shape[0] if table is not None else 0, x.data_ptr(), ld_feat, p[0].data_ptr(), p[1].data_ptr(),
                                            p[4].data_ptr(), p[5].data_ptr(), g.data_ptr(), saved.data_ptr(), *ctx.geo, _lib.ptr(d_feat),
                                            _lib.ptr(d_wv), *[q.data_ptr() for q in gp], ws.data_ptr(), ws.numel(), _lib.current_stream()),
                       "recon_ctx_lstm_bwd")
        g_table = None
        if d_wv is not None:                                                # the embedding's own backward (ids clamped as the kernels clamp them)
            Vw = word_table.shape[0]
            pad = -1 if ctx.padding_idx is None else int(ctx.padding_idx)
            g_table = torch.ops.aten.embedding_dense_backward(d_wv, ids.long().clamp(0, Vw - 1), Vw, pad, False)
        return (None, None, None, d_feat, None, g_table) + tuple(q if n else None for q, n in zip(gp, need[6:]))


def _fused(lstm, feat, words, word_table):
    if not feat.is_cuda or feat.dtype != torch.float32 or not _kernel_lstm(lstm):
        return False
    if any(getattr(lstm, n).dtype != torch.float32 for n in _PARAMS):
        return False
    Dw = 0 if words is None else word_table.shape[1]
    return bool(_lib.lib().recon_ctx_lstm_supported(feat.shape[0], feat.shape[1], Dw, feat.shape[2], lstm.hidden_size))


def context_line_states(lstm, feat, words=None, word_table=None, padding_idx=None):
    """nn.LSTM, [S, T, Fc] (, [S, T] ids, [Vw, Dw]) -> [S, 2H] final hidden states of both directions of every line (models/models.py:56-70;
    [S, dirs * H] of the last layer for the LSTMs only the stock ops take), differentiable in feat, word_table and the LSTM's parameters.
    padding_idx: that row of word_table's gradient is zero, as with nn.Embedding.  S == 0 gives an empty [0, 2H] without a launch."""
    if not isinstance(lstm, nn.LSTM):
        raise ValueError("context_line_states: lstm must be an nn.LSTM, got %s" % type(lstm).__name__)
    if feat.dim() != 3 or not feat.is_floating_point():
        raise ValueError("context_line_states: feat must be a floating-point [S, T, Fc] tensor, got %s %s" % (feat.dtype, tuple(feat.shape)))
    if (words is None) != (word_table is None):
        raise ValueError("context_line_states: pass words and word_table together or neither")
    Dw = 0
    if words is not None:
        if words.dtype not in (torch.int64, torch.int32) or tuple(words.shape) != tuple(feat.shape[:2]):
            raise ValueError("context_line_states: words must be an int64 or int32 [S, T] = %s tensor, got %s %s"
                             % (tuple(feat.shape[:2]), words.dtype, tuple(words.shape)))
        if word_table.dim() != 2 or word_table.dtype != feat.dtype:
            raise ValueError("context_line_states: word_table must be [Vw, Dw] of feat's dtype %s, got %s %s"
                             % (feat.dtype, word_table.dtype, tuple(word_table.shape)))
        Dw = word_table.shape[1]
        if not (words.device == word_table.device == feat.device):
            raise ValueError("context_line_states: the tensors must be on one device")
    if feat.shape[1] < 1 or feat.shape[2] < 1 or Dw + feat.shape[2] != lstm.input_size:
        raise ValueError("context_line_states: the LSTM takes %d inputs, got Dw + Fc = %d + %d over T = %d steps"
                         % (lstm.input_size, Dw, feat.shape[2], feat.shape[1]))
    if feat.shape[0] == 0:
        return _lstm._empty_states(lstm, (0,), feat)
    if _fused(lstm, feat, words, word_table):
        params = [getattr(lstm, n) for n in _PARAMS]
        # (inside the function grad mode is off and needs_input_grad ignores no_grad: whether a backward can follow is decided here)
        wants = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [feat, word_table] + params)
        return _ContextLineStates.apply(lstm, padding_idx, wants, feat, words, word_table, *params)
    return _chain(lstm, feat, words, word_table, padding_idx)
