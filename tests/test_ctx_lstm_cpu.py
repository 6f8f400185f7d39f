"""recon_amd.context_line_states without a GPU: the ABI entries, the stock sequence on CPU tensors, the conditions that reach `_chain`,
argument errors, the empty batch, and the fixture tests/golden/ctx_lstm1.npz under the stock lines in fp64 (which pins the fixture to the
reference before any kernel is involved)."""
import os

import numpy as np
import pytest
import torch
from torch import nn

from conftest import ROOT, load_golden
from op_checks import calls_of, entries_declared_and_bound
from test_char_features_cpu import fixture_model

VW = 11                                                                      # rows of the word table `inputs` draws
ENTRIES = ("recon_ctx_lstm_supported", "recon_ctx_lstm_workspace_bytes", "recon_ctx_lstm_saved_bytes", "recon_ctx_lstm_fwd",
           "recon_ctx_lstm_bwd")


def stock(lstm, feat, words=None, table=None):
    """models/models.py:56-70 written out: embedding, cat, lstm, h_n of the last layer with the directions side by side."""
    x = feat if words is None else torch.cat((nn.functional.embedding(words, table), feat), -1)
    _, (h_n, _) = lstm(x)
    h_n = h_n.view(lstm.num_layers, 2, x.shape[0], lstm.hidden_size)[-1]
    return h_n.permute(1, 0, 2).contiguous().view(x.shape[0], 2 * lstm.hidden_size)


def inputs(S, T, Dw, Fc, H, seed=0):
    """The GPU file's cases: the seeds are mixed with the shape, weights uniform in +-1 / sqrt(H) (nn.LSTM's own init), g_out is drawn too."""
    g = torch.Generator().manual_seed(1000 * seed + S + T + Dw + Fc + H)
    torch.manual_seed(1000 * seed + S + 7 * T + Dw + Fc + H)
    lstm = nn.LSTM(Dw + Fc, H, 1, batch_first=True, bidirectional=True)       # uniform in +-1 / sqrt(H)
    feat = torch.randn(S, T, Fc, generator=g)
    words = torch.randint(0, VW, (S, T), generator=g) if Dw else None
    table = torch.randn(VW, Dw, generator=g) if Dw else None
    g_out = torch.randn(S, 2 * H, generator=g)
    return lstm, feat, words, table, g_out


def make(S=5, T=4, Dw=3, Fc=2, H=3, dtype=torch.float32, seed=0, **kw):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    kw.setdefault("bidirectional", True)
    lstm = nn.LSTM(Dw + Fc, H, kw.pop("num_layers", 1), batch_first=True, **kw).to(dtype)
    feat = torch.randn(S, T, Fc, generator=g).to(dtype)
    words = torch.randint(0, 6, (S, T), generator=g) if Dw else None
    table = torch.randn(6, Dw, generator=g).to(dtype) if Dw else None
    return lstm, feat, words, table


def test_header_declares_and_lib_binds_the_entries():
    entries_declared_and_bound(ENTRIES, "models/models.py:56-70")


@pytest.mark.parametrize("gather", [True, False])
def test_cpu_tensors_are_the_stock_lines_bit_for_bit(gather):
    from recon_amd import context_line_states
    lstm, feat, words, table = make(Dw=3 if gather else 0)
    g_out = torch.randn(5, 6)
    res = []
    for fn in (context_line_states, stock):
        lstm.zero_grad()
        f = feat.clone().requires_grad_(True)
        tb = table.clone().requires_grad_(True) if gather else None
        out = fn(lstm, f, words, tb)
        out.backward(g_out)
        res.append([out.detach(), f.grad] + ([tb.grad] if gather else []) + [p.grad.clone() for p in lstm.parameters()])
    assert len(res[0]) == (3 if gather else 2) + 8
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("how", ["fp64", "two_layers", "unidirectional", "proj_size", "cpu_fp32"])
def test_fallback_conditions_reach_the_chain(how, monkeypatch):
    from recon_amd import context_line_states, context_lstm
    kw = {"fp64": dict(dtype=torch.float64), "two_layers": dict(num_layers=2), "unidirectional": dict(bidirectional=False),
          "proj_size": dict(proj_size=2), "cpu_fp32": {}}[how]
    lstm, feat, words, table = make(**kw)
    calls = calls_of(monkeypatch, context_lstm, "_chain")
    monkeypatch.setattr(context_lstm._ContextLineStates, "apply", staticmethod(lambda *a: pytest.fail("the kernels' function was entered")))
    out = context_line_states(lstm, feat, words, table)
    assert calls == [1]
    width = (2 if lstm.bidirectional else 1) * (lstm.proj_size or lstm.hidden_size)
    assert out.shape == (5, width) and out.dtype == feat.dtype
    _, (h_n, _) = lstm(torch.cat((nn.functional.embedding(words, table), feat), -1))
    assert torch.equal(out[:, :width // (2 if lstm.bidirectional else 1)], h_n[-(2 if lstm.bidirectional else 1)])


def test_kernel_lstm_predicate():
    from recon_amd.context_lstm import _kernel_lstm
    assert _kernel_lstm(nn.LSTM(4, 3, 1, batch_first=True, bidirectional=True))
    assert not _kernel_lstm(nn.LSTM(4, 3, 1, batch_first=False, bidirectional=True))
    assert not _kernel_lstm(nn.LSTM(4, 3, 1, batch_first=True, bidirectional=True, bias=False))
    assert not _kernel_lstm(nn.LSTM(4, 3, 2, batch_first=True, bidirectional=True, dropout=0.5))
    assert not _kernel_lstm(nn.LSTM(4, 3, 1, batch_first=True, bidirectional=True, proj_size=2))
    assert not _kernel_lstm(nn.LSTM(4, 3, 1, batch_first=True))
    assert not _kernel_lstm(nn.GRU(4, 3, 1, batch_first=True, bidirectional=True))


def test_argument_errors():
    from recon_amd import context_line_states
    lstm, feat, words, table = make()
    bad = [lambda: context_line_states(nn.GRU(5, 3, batch_first=True), feat, words, table),
           lambda: context_line_states(lstm, feat[0], words, table),
           lambda: context_line_states(lstm, feat.long(), words, table),
           lambda: context_line_states(lstm, feat, words, None),
           lambda: context_line_states(lstm, feat, None, table),
           lambda: context_line_states(lstm, feat, words.float(), table),
           lambda: context_line_states(lstm, feat, words[:, :3], table),
           lambda: context_line_states(lstm, feat, words, table[0]),
           lambda: context_line_states(lstm, feat, words, table.double()),
           lambda: context_line_states(lstm, feat, words, table[:, :2]),          # Dw + Fc is not the LSTM's input size
           lambda: context_line_states(lstm, feat)]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError, match="context_line_states"):
            call()
            pytest.fail("case %d raised nothing" % i)


def test_empty_batch():
    from recon_amd import context_line_states
    lstm, feat, words, table = make()
    out = context_line_states(lstm, feat[:0], words[:0], table)
    assert out.shape == (0, 6) and out.dtype == torch.float32


def test_exported():
    import recon_amd
    from recon_amd.context_lstm import context_line_states
    assert recon_amd.context_line_states is context_line_states


def fixture_gradients(g, m):
    t = lambda k: torch.from_numpy(np.asarray(g[k]))
    out = m(t("words"), t("chars"), t("mask"))
    (out * t("G").to(out.dtype)).sum().backward()
    return out.detach(), {k: p.grad for k, p in m.named_parameters()}


def test_fixture_reproduces_under_the_stock_lines_in_fp64(monkeypatch):
    """EntityEmbedding in fp64 on the CPU (its op runs `_chain` there) against the reference module's recorded output and the gradient of
    every parameter."""
    from recon_amd import context_lstm
    g = load_golden("ctx_lstm1")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ctx_lstm1.npz")) < 32 * 1024
    m = fixture_model(g).double()
    calls = calls_of(monkeypatch, context_lstm, "_chain")
    out, grads = fixture_gradients(g, m)
    assert calls == [1]
    np.testing.assert_allclose(out.numpy(), g["out"], rtol=0, atol=1e-12)
    names = {k[2:] for k in g if k.startswith("g.")}
    assert names == set(grads) and {"lstm.weight_hh_l0_reverse", "word_embeddings.weight"} <= names
    for k in sorted(names):
        np.testing.assert_allclose(grads[k].numpy(), g["g." + k], rtol=0, atol=1e-12 * max(1.0, np.abs(g["g." + k]).max()), err_msg=k)
    assert np.count_nonzero(g["g.word_embeddings.weight"][0]) == 0 and np.count_nonzero(g["g.word_embeddings.weight"][1:]) > 0
