"""The sentence encoder's pair LSTM (`GPGNN.encode`, models/models.py:160-184) as one device op:

    from recon_amd import pair_sentence_states
    states = pair_sentence_states(rnn, sentence, markers, word_table, pos_table, keep=None, pos_padding_idx=0, groups=None)   # [B, C, 2H]
    x[b, c, t]   = (word_table[sentence[b, t]] * keep[b C + c, t] | pos_table[markers[b, c, t]])                # never written
    states[b, c] = (h of the forward direction after t = T - 1 | h of the reverse direction after t = 0)

rnn an nn.LSTM, sentence [B, T] and markers [B, C, T] int64 or int32 (strided views with unit last stride are read in place), word_table
[Vw, Dw], pos_table [Vp, P]; keep None, a `PackedKeep` over [B C, T, Dw] (`char_features.draw_packed_keep` / `pack_keep`) or an fp32
[B, C, T, Dw] tensor of factors; groups None or a `PairGroups` (pair_groups.py: only the batch's distinct sequences run, at B' = S_d and
C' = 1, and `groups.expand` gives every pair its sequence's state).  With fp32 GPU tensors, a one-layer
bidirectional batch_first nn.LSTM with bias, without projection and with dropout 0, a word_table that requires no gradient, keep None or packed, at most MAX_POS_ROWS rows in pos_table and a shape
`recon_sent_lstm_supported` takes (H up to 256), the kernels of csrc/sent_lstm.hip run: two launches forward, five backward, all fp32 on the
fp32 MFMA, bitwise reproducible.  Neither the C copies of the sentence, nor the gathered rows, their product with keep, the concatenation
or the [B C, T, 2H] outputs are written; for the backward the forward keeps gates and cell state (5 H floats per direction, sequence and
step), which the backward consumes.  Differentiable in pos_table and the eight LSTM parameters; word_table is a constant of the kernels.
Otherwise — CPU tensors, another dtype, another kind of LSTM, fp32 keep, a table that requires a gradient, an unsupported shape, a
backward under create_graph or a second backward over a retained graph — the call runs `_chain`, the op sequence `GPGNN.encode` is without
it.  DESIGN.md section 21.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, _lstm
from ._lstm import _PARAMS, _kernel_lstm
from .char_features import PackedKeep

MAX_POS_ROWS = 16                 # kSlMaxVp of csrc/sent_lstm.hip: one-hot columns of the weight-gradient pass
BWD_MAX_ROW_GROUPS = 32           # kSlMaxGroups: the weight-gradient pass gives each row group ceil(B C / 32) sequences
WIDE_TILE_FROM = 2048             # kSlWideFrom: above this many sequences a workgroup's tile is 32 rows, else 16


def _chain(rnn, sentence, markers, word_table, pos_table, keep=None, pos_padding_idx=0):
    """The stock sequence (models/models.py:160-184): the sentence copied per pair, both embeddings, the factors, cat, rnn, the two rows."""
    B, T = sentence.shape
    C = markers.shape[1]
    expanded = torch.transpose(sentence.expand(C, B, T), 0, 1)
    word = F.embedding(expanded.contiguous().view(-1, T), word_table).view(B, C, T, -1)
    if keep is not None:
        word = word * keep
    pos = F.embedding(markers.contiguous().view(-1, T), pos_table, padding_idx=pos_padding_idx).view(B, C, T, -1)
    merged = torch.cat([word, pos], dim=3)
    merged = merged.view(-1, T, merged.size(-1))
    rnn_output, _ = rnn(merged)
    u = rnn.hidden_size
    return torch.cat([rnn_output[:, -1, :u], rnn_output[:, 0, u:]], dim=1).view(B, C, -1)


def _ids(sentence, markers):
    """Both id arrays as the kernels read them (one element size; rows in place where the strides allow) and their row strides."""
    if sentence.dtype != markers.dtype:
        sentence, markers = sentence.long(), markers.long()
    s, ld_s = _lib.rows_in_place(sentence, sentence.shape[1])
    m, ld_m = _lib.rows_in_place(markers, markers.shape[2])
    return s, ld_s, m, ld_m


class _PairSentenceStates(torch.autograd.Function):
    """csrc/sent_lstm.hip: saves the ids, references to the inputs, the keep bits, out and the saved-state buffer — nothing of size S T I."""

    @staticmethod
    def forward(ctx, rnn, pos_padding_idx, wants, scale, sentence, markers, word_table, bits, pos_table, *params):
        L = _lib.lib()
        B, C, T = markers.shape
        Dw, P, H = word_table.shape[1], pos_table.shape[1], params[1].shape[1]
        s, ld_s, m, ld_m = _ids(sentence, markers)
        table, pos = word_table.detach().contiguous(), pos_table.detach().contiguous()
        p = [q.detach().contiguous() for q in params]
        geo = (B, C, T, Dw, P, H)
        dev = table.device
        out = torch.empty(B * C, 2 * H, dtype=torch.float32, device=dev)
        saved = torch.empty(L.recon_sent_lstm_saved_bytes(*geo), dtype=torch.uint8, device=dev) if wants else None
        ws = _lib.workspace(L.recon_sent_lstm_workspace_bytes(*geo, pos.shape[0], 0), dev)
        with _lib.on_device(dev):
            _lib.check(L.recon_sent_lstm_fwd(s.data_ptr(), m.data_ptr(), s.element_size(), ld_s, ld_m, table.data_ptr(), table.shape[0],
                                             pos.data_ptr(), pos.shape[0], _lib.ptr(bits), scale, *[q.data_ptr() for q in p], *geo,
                                             out.data_ptr(), _lib.ptr(saved), ws.data_ptr(), ws.numel(), _lib.current_stream()),
                       "recon_sent_lstm_fwd")
        if wants:
            ctx.save_for_backward(s, m, word_table, bits, pos_table, out, saved, *params)
            ctx.rnn, ctx.pos_padding_idx, ctx.geo, ctx.scale, ctx.consumed = rnn, pos_padding_idx, geo, scale, False
        return out.view(B, C, 2 * H)

    @staticmethod
    def backward(ctx, g_out):
        s, m, word_table, bits, pos_table, out, saved, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        B, C, T, Dw, P, H = ctx.geo
        Vw, Vp = word_table.shape[0], pos_table.shape[0]
        def stock():
            keep = None if bits is None else PackedKeep(bits, ctx.scale, Dw).factors(word_table.dtype).view(B, C, T, Dw)
            ss, mm = s.clamp(0, Vw - 1), m.clamp(0, Vp - 1)                                      # as the kernels clamp them
            return _chain(ctx.rnn, ss, mm, word_table, pos_table, keep, ctx.pos_padding_idx)
        grads = _lstm._recompute(ctx, stock, (pos_table,) + tuple(params), need[8:], g_out)
        if grads is not None:
            return (None,) * 8 + grads
        L = _lib.lib()
        s, ld_s, m, ld_m = _ids(s, m)
        table, pos = word_table.detach().contiguous(), pos_table.detach().contiguous()
        p = [q.detach().contiguous() for q in params]
        g = g_out.reshape(B * C, 2 * H).contiguous().to(torch.float32)
        dev = g.device
        g_pos = torch.empty_like(pos)
        gp = [torch.empty_like(q) for q in p]
        ws = _lib.workspace(L.recon_sent_lstm_workspace_bytes(*ctx.geo, Vp, 1), dev)
        pad = -1 if ctx.pos_padding_idx is None else int(ctx.pos_padding_idx)
        with _lib.on_device(dev):
            _lib.check(L.recon_sent_lstm_bwd(s.data_ptr(), m.data_ptr(), s.element_size(), ld_s, ld_m, table.data_ptr(), Vw, pos.data_ptr(), Vp,
                                             _lib.ptr(bits), ctx.scale, p[0].data_ptr(), p[1].data_ptr(), p[4].data_ptr(), p[5].data_ptr(),
                                             g.data_ptr(), saved.data_ptr(), *ctx.geo, pad, g_pos.data_ptr(), *[q.data_ptr() for q in gp],
                                             ws.data_ptr(), ws.numel(), _lib.current_stream()), "recon_sent_lstm_bwd")
        return (None,) * 8 + ((g_pos if need[8] else None),) + tuple(q if n else None for q, n in zip(gp, need[9:]))


def _fused(rnn, sentence, markers, word_table, pos_table, keep):
    if not word_table.is_cuda or word_table.dtype != torch.float32 or pos_table.dtype != torch.float32 or not _kernel_lstm(rnn):
        return False
    if word_table.requires_grad or not (keep is None or isinstance(keep, PackedKeep)):
        return False
    if any(getattr(rnn, n).dtype != torch.float32 or not getattr(rnn, n).is_cuda for n in _PARAMS) or pos_table.shape[0] > MAX_POS_ROWS:
        return False
    B, C, T = markers.shape
    return bool(_lib.lib().recon_sent_lstm_supported(B, C, T, word_table.shape[1], pos_table.shape[1], rnn.hidden_size))


def _grouped(rnn, sentence, markers, word_table, pos_table, keep, pos_padding_idx, groups):
    """The call over the distinct sequences of `groups`: the op itself at B' = S_d, C' = 1 over the compact copies —
    the kernels or `_chain`, by the same rules — and `groups.expand` behind it."""
    from .pair_groups import PairGroups
    if not isinstance(groups, PairGroups):
        raise ValueError("pair_sentence_states: groups must be a PairGroups or None, got %s" % type(groups).__name__)
    sentence_d, markers_d = groups.compact(sentence, markers)
    S_d, T, Dw = groups.total, sentence.shape[1], word_table.shape[1]
    if keep is not None and not isinstance(keep, PackedKeep):
        if not torch.is_tensor(keep) or tuple(keep.shape) != (S_d, 1, T, Dw):
            raise ValueError("pair_sentence_states: with groups, keep must be [S_d, 1, T, Dw] = [%d, 1, %d, %d] (sequence j has one draw), got %s"
                             % (S_d, T, Dw, tuple(getattr(keep, "shape", ()))))
    rows = pair_sentence_states(rnn, sentence_d, markers_d, word_table, pos_table, keep, pos_padding_idx)
    return groups.expand(rows.reshape(S_d, rows.shape[-1]))


def pair_sentence_states(rnn, sentence, markers, word_table, pos_table, keep=None, pos_padding_idx=0, groups=None):
    """nn.LSTM, [B, T] ids, [B, C, T] ids, [Vw, Dw], [Vp, P] -> [B, C, 2H]: the final hidden states of both directions of every (sentence,
    entity pair) sequence (models/models.py:160-184; for the LSTMs only the stock ops take, whatever those lines give), differentiable in
    pos_table and the LSTM's parameters (and, through the stock ops, in a word_table that requires a gradient: a plain table, no padding
    row).  keep: None, a `PackedKeep` over [B C, T, Dw] or fp32 [B, C, T, Dw] factors multiplied onto the gathered word rows.
    pos_padding_idx: that row of pos_table's gradient is zero, as with nn.Embedding; its values are read as they are.  B C == 0 gives an
    empty [B, C, 2H] without a launch.  groups: a `PairGroups` over the [B, C] pairs: the S_d distinct sequences alone are encoded (the same
    op over the compact copies at B' = S_d, C' = 1) and `groups.expand` gives every pair its sequence's state; keep then has S_d rows (a
    `PackedKeep` over [S_d, T, Dw], or fp32 [S_d, 1, T, Dw]): sequence j has one draw."""
    if groups is not None and sentence.dim() == 2 and markers.dim() == 3 and sentence.shape[0] * markers.shape[1] > 0:
        return _grouped(rnn, sentence, markers, word_table, pos_table, keep, pos_padding_idx, groups)
    if not isinstance(rnn, nn.LSTM):
        raise ValueError("pair_sentence_states: rnn must be an nn.LSTM, got %s" % type(rnn).__name__)
    if sentence.dim() != 2 or sentence.dtype not in (torch.int64, torch.int32):
        raise ValueError("pair_sentence_states: sentence must be an int64 or int32 [B, T] tensor, got %s %s" % (sentence.dtype, tuple(sentence.shape)))
    B, T = sentence.shape
    if markers.dim() != 3 or markers.dtype not in (torch.int64, torch.int32) or markers.shape[0] != B or markers.shape[2] != T:
        raise ValueError("pair_sentence_states: markers must be an int64 or int32 [B, C, T] = [%d, C, %d] tensor, got %s %s"
                         % (B, T, markers.dtype, tuple(markers.shape)))
    C = markers.shape[1]
    if word_table.dim() != 2 or pos_table.dim() != 2 or not word_table.is_floating_point() or word_table.dtype != pos_table.dtype:
        raise ValueError("pair_sentence_states: word_table [Vw, Dw] and pos_table [Vp, P] must share one floating-point dtype, got %s %s, %s %s"
                         % (word_table.dtype, tuple(word_table.shape), pos_table.dtype, tuple(pos_table.shape)))
    Dw, P = word_table.shape[1], pos_table.shape[1]
    if T < 1 or Dw < 1 or P < 1 or word_table.shape[0] < 1 or pos_table.shape[0] < 1 or Dw + P != rnn.input_size:
        raise ValueError("pair_sentence_states: the LSTM takes %d inputs, got Dw + P = %d + %d over T = %d steps" % (rnn.input_size, Dw, P, T))
    packed = isinstance(keep, PackedKeep)
    if packed:
        if (keep.C != Dw or not torch.is_tensor(keep.bits) or keep.bits.dtype != torch.int32 or not keep.bits.is_contiguous()
                or tuple(keep.bits.shape) != (B * C, T, (Dw + 31) // 32)):
            raise ValueError("pair_sentence_states: a PackedKeep needs C = %d and contiguous int32 bits [B C, T, ceil(Dw / 32)], got C = %d, %s %s"
                             % (Dw, keep.C, getattr(keep.bits, "dtype", None), tuple(getattr(keep.bits, "shape", ()))))
    elif keep is not None and (not torch.is_tensor(keep) or tuple(keep.shape) != (B, C, T, Dw) or keep.dtype != word_table.dtype):
        raise ValueError("pair_sentence_states: keep must be [B, C, T, Dw] of the tables' dtype, got %s %s"
                         % (getattr(keep, "dtype", None), tuple(getattr(keep, "shape", ()))))
    keep_device = None if keep is None else (keep.bits.device if packed else keep.device)
    if not (sentence.device == markers.device == word_table.device == pos_table.device and (keep is None or keep_device == sentence.device)):
        raise ValueError("pair_sentence_states: the tensors must be on one device")
    if B * C == 0:
        return _lstm._empty_states(rnn, (B, C), word_table)
    if _fused(rnn, sentence, markers, word_table, pos_table, keep):
        params = [getattr(rnn, n) for n in _PARAMS]
        # (inside the function grad mode is off and needs_input_grad ignores no_grad: whether a backward can follow is decided here)
        wants = torch.is_grad_enabled() and any(t.requires_grad for t in [pos_table] + params)
        bits, scale = (keep.bits, keep.scale) if packed else (None, 1.0)
        return _PairSentenceStates.apply(rnn, pos_padding_idx, wants, scale, sentence, markers, word_table, bits, pos_table, *params)
    if packed:
        keep = keep.factors(word_table.dtype).view(B, C, T, Dw)
    return _chain(rnn, sentence, markers, word_table, pos_table, keep, pos_padding_idx)
