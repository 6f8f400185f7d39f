"""recon_amd.char_word_features (csrc/char_cnn.hip) against the stock sequence of models/models.py:57-61 in fp64 on the CPU, and against
the fixtures written from the reference's EntityEmbedding.

Tolerance of value and gradients: `op_checks.bound` of the stock chain's own error on the GPU against fp64 on the same inputs, measured in
the test.  The figures measured on an MI355X are in DESIGN.md section 18.

Gradient cells near a tie: a window whose two best positions differ by less than fp32 rounding can pick another position than fp64 does,
and the gradient then differs discretely, which is not an error.  g_out is zeroed at every (s, w, o) where, in fp64, the maximum and the
best position with a different id tuple are closer than 1e-5 (about 10x the fp32 error); positions with identical ids tie harmlessly.  At
most 1 % of the cells may be zeroed.

Only the table form (no dropout factors) has kernels; with `keep` the op runs the stock chain, which one test asserts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from op_checks import band_failures, bound, calls_of, close, dev, peak_bytes, rel_err, rounded, same
from test_char_features_cpu import fixture_model, inputs, stock

pytestmark = pytest.mark.gpu

#        S    W  max_char cfs C   Fo  V
CASES = [(1, 1, 1, 1, 1, 1, 2), (3, 3, 4, 3, 5, 6, 9), (24, 5, 4, 2, 3, 3, 8), (7, 2, 10, 3, 50, 50, 90), (65, 4, 6, 5, 33, 65, 40),
         (19, 3, 10, 3, 50, 50, 300), (130, 32, 10, 3, 50, 50, 90)]
REF_GEOMETRY = (130, 32, 10, 3, 50, 50, 90)
PARAMS = ("emb_weight", "conv_weight", "conv_bias")


def near_ties(chars, E, Wc, b, span, margin=1e-5):
    """bool [S, W, Fo]: in fp64 the window's maximum and its best position with a different id tuple are closer than `margin`."""
    cfs, S = Wc.shape[2], chars.shape[0]
    W = (chars.shape[1] - cfs + 1) // span
    pre = F.conv1d(F.embedding(chars, E.double()).permute(0, 2, 1), Wc.double(), b.double())          # [S, Fo, W span]
    pre = pre.view(S, -1, W, span)
    top, at = pre.max(-1, keepdim=True)
    tuples = chars.unfold(1, cfs, 1).reshape(S, 1, W, span, cfs).expand(-1, pre.shape[1], -1, -1, -1)   # ids under every position
    best = torch.gather(tuples, 3, at.unsqueeze(-1).expand(-1, -1, -1, -1, cfs))
    other = (tuples != best).any(-1)
    close = other & (top - pre < margin)
    return close.any(-1).permute(0, 2, 1)


_CASES = {}


def case(shape):
    """Inputs, tie-masked g_out and the fp64 oracle (value and the three gradients) of a shape, computed once."""
    if shape not in _CASES:
        chars, E, Wc, b, span, g_out = inputs(*shape)
        ties = near_ties(chars, E, Wc, b, span)
        assert ties.float().mean().item() <= 0.01, ties.float().mean().item()
        g_out = g_out.masked_fill(ties, 0.0)
        p = [t.double().requires_grad_(True) for t in (E, Wc, b)]
        ref = stock(chars, *p, span)
        ref.backward(g_out.double())
        _CASES[shape] = (chars, E, Wc, b, span, g_out, [ref.detach()] + [t.grad for t in p], int(ties.sum()))
    return _CASES[shape]


def run(fn, chars, E, Wc, b, span, g_out, **kw):
    p = [t.to(dev()).requires_grad_(True) for t in (E, Wc, b)]
    out = fn(chars.to(dev()), *p, span, **kw)
    out.backward(g_out.to(dev()))
    return [out.detach()] + [t.grad for t in p]


def fused_ran(monkeypatch):
    from recon_amd import char_features
    return calls_of(monkeypatch, char_features._CharWordFeatures, "apply")


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradients(shape, monkeypatch):
    from recon_amd import _lib, char_word_features
    from recon_amd.char_features import _chain
    chars, E, Wc, b, span, g_out, ref, n_ties = case(shape)
    calls = fused_ran(monkeypatch)
    fused = run(char_word_features, chars, E, Wc, b, span, g_out)
    S, W, max_char, cfs, C, Fo, V = shape
    if _lib.lib().recon_char_features_supported(S, W, span, cfs, V, C, Fo):
        assert calls, "the kernels take this shape: the op must not run the chain"
    else:
        assert not calls
    chain = run(_chain, chars, E, Wc, b, span, g_out)
    assert fused[0].shape == (S, W, Fo) and fused[1].shape == E.shape and fused[2].shape == Wc.shape and fused[3].shape == b.shape
    print("char_features %s: %d of %d cells near a tie" % (shape, n_ties, S * W * Fo))
    failures = band_failures(("out",) + PARAMS, fused, chain, ref, "char_features %s" % (shape,))
    assert not failures, failures
    assert torch.count_nonzero(fused[1][0]) == 0                                    # the padding row's gradient


def test_int32_ids():
    from recon_amd import char_word_features
    chars, E, Wc, b, span, g_out, ref, _ = case((7, 2, 10, 3, 50, 50, 90))
    a = run(char_word_features, chars, E, Wc, b, span, g_out)
    c = run(char_word_features, chars.to(torch.int32), E, Wc, b, span, g_out)
    same(a, c)
    assert rel_err(c[0], ref[0]) <= 2e-5


def test_strided_ids_are_read_in_place():
    from recon_amd import char_word_features
    chars, E, Wc, b, span, g_out, ref, _ = case((24, 5, 4, 2, 3, 3, 8))
    wide = torch.full((24, chars.shape[1] + 3), 5, dtype=torch.int64)
    wide[:, :chars.shape[1]] = chars
    a = run(char_word_features, chars, E, Wc, b, span, g_out)
    c = run(lambda ch, *r: char_word_features(ch[:, :chars.shape[1]], *r), wide, E, Wc, b, span, g_out)
    same(a, c)


def test_all_padding_gives_tanh_of_the_bias_exactly():
    from recon_amd import char_word_features
    chars, E, Wc, b, span, g_out = inputs(9, 3, 10, 3, 50, 50, 90, seed=3)
    chars.zero_()
    out, g_e, g_w, g_b = run(char_word_features, chars, E, Wc, b, span, g_out)
    assert torch.equal(out, torch.tanh(b.to(dev())).expand(9, 3, 50))
    assert torch.count_nonzero(g_e) == 0 and torch.count_nonzero(g_w) == 0
    want = (g_out.double() * (1 - torch.tanh(b.double()) ** 2)).sum((0, 1))
    assert rel_err(g_b, want) <= 2e-5


def test_nonzero_padding_row_gets_no_gradient():
    from recon_amd import char_word_features
    chars, E, Wc, b, span, g_out = inputs(24, 5, 4, 2, 3, 3, 8, seed=4)
    E = E.clone()
    E[0] = torch.tensor([0.5, -1.0, 0.25])
    ties = near_ties(chars, E, Wc, b, span)
    assert ties.float().mean().item() <= 0.01
    g_out = g_out.masked_fill(ties, 0.0)
    p = [t.double().requires_grad_(True) for t in (E, Wc, b)]
    ref = stock(chars, *p, span)
    ref.backward(g_out.double())
    got = run(char_word_features, chars, E, Wc, b, span, g_out)
    assert torch.count_nonzero(got[1][0]) == 0 and torch.count_nonzero(p[0].grad[0]) == 0
    assert torch.count_nonzero(got[1][1:]) > 0
    for f, r in zip(got, [ref.detach()] + [t.grad for t in p]):
        assert rel_err(f, r) <= 2e-5


def test_backward_is_bitwise_reproducible():
    from recon_amd import char_word_features
    for shape in ((65, 4, 6, 5, 33, 65, 40), (19, 3, 10, 3, 50, 50, 300), REF_GEOMETRY):
        chars, E, Wc, b, span, g_out, _, _ = case(shape)
        a = run(char_word_features, chars, E, Wc, b, span, g_out)
        c = run(char_word_features, chars, E, Wc, b, span, g_out)
        for x, y in zip(a, c):
            assert torch.equal(x, y), shape


def test_dropout_factors_run_the_stock_chain(monkeypatch):
    """`keep` has no kernel: value and gradients are the chain's, bit for bit, and the fused function is not entered."""
    from recon_amd import char_word_features
    chars, E, Wc, b, span, g_out, _, _ = case((3, 3, 4, 3, 5, 6, 9))
    keep = F.dropout(torch.ones(3, chars.shape[1], 5), 0.5, True).to(dev())
    calls = fused_ran(monkeypatch)
    a = run(char_word_features, chars, E, Wc, b, span, g_out, keep=keep)
    c = run(stock, chars, E, Wc, b, span, g_out, keep=keep)
    assert not calls
    same(a, c)


def test_create_graph_stays_differentiable():
    from recon_amd import char_word_features
    chars, E, Wc, b, span, g_out, ref, _ = case((3, 3, 4, 3, 5, 6, 9))
    p = [t.to(dev()).requires_grad_(True) for t in (E, Wc, b)]
    out = char_word_features(chars.to(dev()), *p, span)
    grads = torch.autograd.grad(out, p, g_out.to(dev()), create_graph=True)
    for g, r in zip(grads, ref[1:]):
        assert g.requires_grad and rel_err(g, r) <= 2e-5
    grads[1].square().sum().backward()
    assert p[0].grad is not None and torch.isfinite(p[0].grad).all()


def test_empty_batch():
    from recon_amd import char_word_features
    chars, E, Wc, b, span, _ = inputs(2, 3, 4, 3, 5, 6, 9)
    out = char_word_features(chars[:0].to(dev()), E.to(dev()), Wc.to(dev()), b.to(dev()).requires_grad_(True), span)
    assert out.shape == (0, 3, 6) and out.is_cuda


@pytest.mark.parametrize("name", ["char_features1_eval", "char_features2_train"])
def test_fixture_pool_output(name):
    """The op against the reference module's hooked max_pool output (tanh of it), within the tolerance above."""
    from recon_amd import char_word_features
    from recon_amd.char_features import _chain
    g = load_golden(name)
    t = lambda k: torch.from_numpy(np.asarray(g[k]))
    chars = t("chars").reshape(-1, g["chars"].shape[-1]).to(dev())
    keep = t("keep").float().to(dev()) if "keep" in g else None
    E, Wc, b = (t(k).float().to(dev()) for k in ("sd.char_embeddings.embeddings.weight", "sd.conv1d.weight", "sd.conv1d.bias"))
    ref = torch.tanh(t("pool")).permute(0, 2, 1)
    e_f = rel_err(char_word_features(chars, E, Wc, b, int(g["word_span"]), keep=keep), ref)
    e_c = rel_err(_chain(chars, E, Wc, b, int(g["word_span"]), keep), ref)
    print("char_features fixture %s: fused %.3e chain %.3e" % (name, e_f, e_c))
    assert e_f <= bound(e_c)


@pytest.mark.parametrize("name", ["char_features1_eval", "char_features2_train"])
def test_fixture_entity_embedding(name, monkeypatch):
    """EntityEmbedding with the fixture's parameters (strict load) against the reference module's output and the three gradients; the
    training fixture replays its recorded factors through draw_keep.  The bound is the whole-model LSTM fixtures' (test_prop_gpu.py)."""
    g = load_golden(name)
    m = fixture_model(g)
    calls = fused_ran(monkeypatch)
    m.train().to(dev())                     # MIOpen's LSTM backward needs training mode; the eval fixture has p = 0: no factors drawn
    t = lambda k: torch.from_numpy(g[k]).to(dev())
    out = m(t("words"), t("chars"), t("mask"))
    assert bool(calls) == (float(g["p"]) == 0.0)
    close(out, g["out"], atol=1e-4, what=name + " out")
    (out * t("G").float()).sum().backward()
    for k in ("char_embeddings.embeddings.weight", "conv1d.weight", "conv1d.bias"):
        close(dict(m.named_parameters())[k].grad, g["g." + k], atol=1e-4, rel_to_max=1e-4, what=name + " grad " + k)


@pytest.mark.parametrize("wants_grad", [False, True])
def test_forward_materialises_nothing_of_size_S_Lc(wants_grad):
    """A forward at the reference's word and width geometry raises the allocated bytes by the output, the workspace and (with a gradient
    wanted) one position byte per output element, each a block of the allocator; the stock chain's gathered embedding alone is S Lc C 4
    bytes, more than ten times that."""
    from recon_amd import _lib, char_word_features
    S, W, max_char, cfs, C, Fo, V = REF_GEOMETRY
    chars, E, Wc, b, span, _ = inputs(*REF_GEOMETRY)
    chars, E, Wc, b = (x.to(dev()) for x in (chars, E, Wc, b))
    ws = _lib.lib().recon_char_features_workspace_bytes(S, W, span, cfs, V, C, Fo, 0)
    allowed = rounded(S * W * Fo * 4) + rounded(ws)
    assert 10 * allowed < S * chars.shape[1] * C * 4
    if wants_grad:
        allowed += rounded(S * W * Fo)
    E.requires_grad_(wants_grad)

    def forward():
        if wants_grad:
            return char_word_features(chars, E, Wc, b, span)
        with torch.no_grad():
            return char_word_features(chars, E, Wc, b, span)
    peak, out = peak_bytes(forward)
    print("char_features memory (grad %s): peak %d bytes, allowed %d, gathered embedding %d" % (wants_grad, peak, allowed, S * chars.shape[1] * C * 4))
    assert peak <= allowed, (peak, allowed)
    assert out.shape == (S, W, Fo)
