"""recon_amd.pair_sentence_states without a GPU: the ABI entries, the stock lines of GPGNN.encode on CPU tensors (bit for bit, with every kind
of keep), the conditions that reach `_chain`, argument errors, the empty batch, and GPGNN.encode with the op switched on."""
import os

import pytest
import torch
from torch import nn

from conftest import ROOT
from op_checks import calls_of, entries_declared_and_bound

VW, VP = 11, 4                                                                  # rows of the tables `inputs` draws
ENTRIES = ("recon_sent_lstm_supported", "recon_sent_lstm_workspace_bytes", "recon_sent_lstm_saved_bytes", "recon_sent_lstm_fwd",
           "recon_sent_lstm_bwd")


def stock(rnn, sentence, markers, word_table, pos_table, keep=None):
    """models/models.py:160-184 as GPGNN.encode writes it, with the dropout factors given."""
    B, T = sentence.shape
    C = markers.shape[1]
    expanded = torch.transpose(sentence.expand(C, B, T), 0, 1)
    word = nn.functional.embedding(expanded.contiguous().view(-1, T), word_table, padding_idx=0).view(B, C, T, -1)
    if keep is not None:
        word = word * keep
    pos = nn.functional.embedding(markers.contiguous().view(-1, T), pos_table, padding_idx=0).view(B, C, T, -1)
    merged = torch.cat([word, pos], dim=3)
    merged = merged.view(-1, T, merged.size(-1))
    rnn_output, _ = rnn(merged)
    u = rnn.hidden_size
    return torch.cat([rnn_output[:, -1, :u], rnn_output[:, 0, u:]], dim=1).view(B, C, -1)


def inputs(B, C, T, Dw, P, H, seed=0):
    """The GPU file's cases: the seeds are mixed with the shape, weights uniform in +-1 / sqrt(H) (nn.LSTM's own init), tables N(0, 1) with
    a non-zero padding row, markers over all VP values, g_out and packed dropout bits (p = 0.5) drawn too."""
    from recon_amd.char_features import pack_keep
    g = torch.Generator().manual_seed(1000 * seed + B + C + T + Dw + P + H)
    torch.manual_seed(1000 * seed + B + 7 * T + C + Dw + P + H)
    rnn = nn.LSTM(Dw + P, H, 1, batch_first=True, bidirectional=True)          # uniform in +-1 / sqrt(H)
    sentence = torch.randint(0, VW, (B, T), generator=g)
    markers = torch.randint(0, VP, (B, C, T), generator=g)
    word_table = torch.randn(VW, Dw, generator=g)
    pos_table = torch.randn(VP, P, generator=g)
    g_out = torch.randn(B, C, 2 * H, generator=g)
    keep = pack_keep((torch.rand(B * C, T, Dw, generator=g) >= 0.5).float() * 2.0, 2.0)        # p = 0.5
    return rnn, sentence, markers, word_table, pos_table, g_out, keep


def make(B=2, C=3, T=4, Dw=5, P=3, H=3, dtype=torch.float32, seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    kw.setdefault("bidirectional", True)
    rnn = nn.LSTM(Dw + P, H, kw.pop("num_layers", 1), batch_first=True, **kw).to(dtype)
    sentence = torch.randint(0, 7, (B, T), generator=g)
    markers = torch.randint(0, 4, (B, C, T), generator=g)
    word_table = torch.randn(7, Dw, generator=g).to(dtype)
    pos_table = torch.randn(4, P, generator=g).to(dtype)
    return rnn, sentence, markers, word_table, pos_table


def test_header_declares_and_lib_binds_the_entries():
    entries_declared_and_bound(ENTRIES, "models/models.py:160-184")
    assert "sent_lstm.hip" in open(os.path.join(ROOT, "recon_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("keep_kind", ["none", "fp32", "packed"])
def test_cpu_tensors_are_the_stock_lines_bit_for_bit(keep_kind):
    from recon_amd import pair_sentence_states
    from recon_amd.char_features import pack_keep
    rnn, sentence, markers, word_table, pos_table = make()
    B, C, T, Dw = 2, 3, 4, 5
    g_out = torch.randn(B, C, 6)
    keep = None
    if keep_kind != "none":
        keep = (torch.rand(B, C, T, Dw, generator=torch.Generator().manual_seed(3)) < 0.5).float() * 2.0
    given = pack_keep(keep.view(B * C, T, Dw), 2.0) if keep_kind == "packed" else keep
    if keep_kind == "packed":
        assert torch.equal(given.factors().view(B, C, T, Dw), keep)
    res = []
    for fn, k in ((pair_sentence_states, given), (stock, keep)):
        rnn.zero_grad()
        pt = pos_table.clone().requires_grad_(True)
        out = fn(rnn, sentence, markers, word_table, pt, k)
        out.backward(g_out)
        res.append([out.detach(), pt.grad] + [p.grad.clone() for p in rnn.parameters()])
    assert len(res[0]) == 10 and res[0][0].shape == (B, C, 6)
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert torch.count_nonzero(res[0][1][0]) == 0 and torch.count_nonzero(res[0][1][1:]) > 0       # the padding row's gradient


@pytest.mark.parametrize("how", ["fp64", "two_layers", "unidirectional", "proj_size", "cpu_fp32", "fp32_keep", "trainable_table"])
def test_fallback_conditions_reach_the_chain(how, monkeypatch):
    from recon_amd import pair_sentence_states, sentence_lstm
    kw = {"fp64": dict(dtype=torch.float64), "two_layers": dict(num_layers=2), "unidirectional": dict(bidirectional=False),
          "proj_size": dict(proj_size=2)}.get(how, {})
    rnn, sentence, markers, word_table, pos_table = make(**kw)
    keep = torch.full((2, 3, 4, 5), 2.0) if how == "fp32_keep" else None
    if how == "trainable_table":
        word_table.requires_grad_(True)
    calls = calls_of(monkeypatch, sentence_lstm, "_chain")
    monkeypatch.setattr(sentence_lstm._PairSentenceStates, "apply", staticmethod(lambda *a: pytest.fail("the kernels' function was entered")))
    out = pair_sentence_states(rnn, sentence, markers, word_table, pos_table, keep)
    assert calls == [1]
    assert out.dtype == word_table.dtype and out.shape[:2] == (2, 3)
    assert torch.equal(out, stock(rnn, sentence, markers, word_table, pos_table, keep))


def test_the_gate_refuses_what_the_kernels_do_not_take():
    """`_fused` on CPU tensors and on the conditions that need no device: each one alone sends the call to the chain."""
    from recon_amd.sentence_lstm import _fused, MAX_POS_ROWS
    rnn, sentence, markers, word_table, pos_table = make()
    assert not _fused(rnn, sentence, markers, word_table, pos_table, None)                      # CPU tensors
    assert MAX_POS_ROWS == 16


def test_argument_errors():
    from recon_amd import pair_sentence_states
    from recon_amd.char_features import pack_keep
    rnn, sentence, markers, word_table, pos_table = make()
    keep = torch.ones(2, 3, 4, 5)
    bad = [lambda: pair_sentence_states(nn.GRU(8, 3, batch_first=True), sentence, markers, word_table, pos_table),
           lambda: pair_sentence_states(rnn, sentence[0], markers, word_table, pos_table),
           lambda: pair_sentence_states(rnn, sentence.float(), markers, word_table, pos_table),
           lambda: pair_sentence_states(rnn, sentence, markers[:, 0], word_table, pos_table),          # markers not [B, C, T]
           lambda: pair_sentence_states(rnn, sentence, markers[:1], word_table, pos_table),
           lambda: pair_sentence_states(rnn, sentence, markers[:, :, :3], word_table, pos_table),
           lambda: pair_sentence_states(rnn, sentence, markers.float(), word_table, pos_table),
           lambda: pair_sentence_states(rnn, sentence, markers, word_table[0], pos_table),
           lambda: pair_sentence_states(rnn, sentence, markers, word_table.double(), pos_table),
           lambda: pair_sentence_states(rnn, sentence, markers, word_table.long(), pos_table.long()),
           lambda: pair_sentence_states(rnn, sentence, markers, word_table[:, :4], pos_table),          # Dw + P is not the LSTM's input size
           lambda: pair_sentence_states(rnn, sentence, markers, word_table, pos_table, keep[:, :2]),
           lambda: pair_sentence_states(rnn, sentence, markers, word_table, pos_table, keep.double()),
           lambda: pair_sentence_states(rnn, sentence, markers, word_table, pos_table, pack_keep(keep.view(6, 4, 5)[:5], 1.0)),
           lambda: pair_sentence_states(rnn, sentence, markers, word_table, pos_table, pack_keep(torch.ones(6, 4, 4), 1.0))]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError, match="pair_sentence_states"):
            call()
            pytest.fail("case %d raised nothing" % i)


def test_empty_batch():
    from recon_amd import pair_sentence_states
    rnn, sentence, markers, word_table, pos_table = make()
    out = pair_sentence_states(rnn, sentence[:0], markers[:0], word_table, pos_table)
    assert out.shape == (0, 3, 6) and out.dtype == torch.float32
    out = pair_sentence_states(rnn, sentence, markers[:, :0], word_table, pos_table)
    assert out.shape == (2, 0, 6)


def test_exported():
    import recon_amd
    from recon_amd.sentence_lstm import pair_sentence_states
    assert recon_amd.pair_sentence_states is pair_sentence_states


def _gpgnn(dropout=0.0):
    import numpy as np
    from recon_amd.gpgnn import GPGNN
    torch.manual_seed(5)
    p = {"max_num_nodes": 3, "embedding_dim": 2, "layer_number": 2, "projection_style": "untie", "non-linear1": "relu", "non-linear": "tanh",
         "dropout1": dropout, "position_emb": 3, "units1": 4, "rnn1_layers": 1, "bidirectional": 1, "batch_size": 2}
    emb = np.random.RandomState(0).randn(9, 5).astype("float32")
    return GPGNN(p, emb, max_sent_len=4, n_out=3)


def test_gpgnn_attributes_and_their_defaults():
    from recon_amd.gpgnn import GPGNN, RECON_EAC
    assert GPGNN.packed_word_dropout is False and isinstance(GPGNN.fused_sentence_encoder, bool)
    assert RECON_EAC.fused_sentence_encoder is GPGNN.fused_sentence_encoder


@pytest.mark.parametrize("mode", ["eval_with_dropout", "train_p0"])
def test_gpgnn_encode_with_the_op_switched_on_equals_todays_encode(mode, monkeypatch):
    from recon_amd import gpgnn
    m = _gpgnn(0.5 if mode == "eval_with_dropout" else 0.0)
    m.train(mode == "train_p0")
    g = torch.Generator().manual_seed(1)
    sent, mark = torch.randint(0, 9, (2, 4), generator=g), torch.randint(0, 4, (2, 6, 4), generator=g)
    g_out = torch.randn(2, 6, 8, generator=g)
    res = []
    for fused in (False, True):
        calls = calls_of(monkeypatch, gpgnn, "pair_sentence_states")
        monkeypatch.setattr(m, "fused_sentence_encoder", fused, raising=False)
        monkeypatch.setattr(m, "packed_word_dropout", fused, raising=False)
        m.zero_grad()
        out = m.encode(sent, mark)
        out.backward(g_out)
        assert bool(calls) == fused
        res.append([out.detach()] + [p.grad.clone() for n, p in m.named_parameters() if n.startswith(("rnn1", "pos_embedding"))])
        monkeypatch.undo()
    assert len(res[0]) == 10
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_gpgnn_encode_keeps_the_stock_calls_where_the_op_does_not_apply(monkeypatch):
    """Active dropout without packed_word_dropout, or a trainable word table: the calls of today, never the op."""
    from recon_amd import gpgnn
    g = torch.Generator().manual_seed(1)
    sent, mark = torch.randint(0, 9, (2, 4), generator=g), torch.randint(0, 4, (2, 6, 4), generator=g)
    monkeypatch.setattr(gpgnn, "pair_sentence_states", lambda *a, **k: pytest.fail("the op was called"))
    m = _gpgnn(0.5).train()
    m.fused_sentence_encoder = True
    assert m.encode(sent, mark).shape == (2, 6, 8)
    m = _gpgnn(0.0).train()
    m.fused_sentence_encoder = True
    m.word_embedding.weight.requires_grad_(True)
    assert m.encode(sent, mark).shape == (2, 6, 8)


def test_gpgnn_packed_word_dropout_draws_packed_bits_on_the_cpu_too():
    m = _gpgnn(0.5).train()
    m.fused_sentence_encoder, m.packed_word_dropout = True, True
    g = torch.Generator().manual_seed(1)
    sent, mark = torch.randint(1, 9, (2, 4), generator=g), torch.randint(0, 4, (2, 6, 4), generator=g)
    torch.manual_seed(3)
    a = m.encode(sent, mark)
    torch.manual_seed(3)
    b = m.encode(sent, mark)
    c = m.encode(sent, mark)
    assert torch.equal(a, b) and not torch.equal(a, c)
