"""recon_amd.translation_residuals (csrc/rel_trans.hip) against an fp64 restatement of models/models.py:939-958, and against the op chain
it replaced in RECON.translation_scores.

Tolerance of value and gradient: the chain's own error against fp64 on the same inputs is measured in the test; the fused op has to stay
within 4x that (another summation order over up to 200 terms) and never above 2e-5 of the largest magnitude (the figure README.md gives
for the split-precision products).  The figures measured on an MI355X are in DESIGN.md section 15."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from op_checks import dev, peak_bytes, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 7, 5), (17, 3, 50, 200), (65, 5, 200, 50), (33, 353, 200, 200), (130, 9, 33, 47)]


def reference(head, tail, W, rel, g_out=None):
    """fp64 on the CPU: (out, and with g_out the gradients of head, tail, W, rel)."""
    h, t, w, g = (x.detach().double().cpu().requires_grad_(True) for x in (head, tail, W, rel))
    diff = torch.tanh(torch.einsum("me,red->mrd", h, w)) + g.unsqueeze(0) - torch.tanh(torch.einsum("me,red->mrd", t, w))
    out = diff.abs().sum(-1)
    if g_out is None:
        return out.detach()
    out.backward(g_out.double().cpu())
    return out.detach(), h.grad, t.grad, w.grad, g.grad


def inputs(M, n_rel, ent_dim, rel_dim, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + M + n_rel + ent_dim + rel_dim)
    emb = torch.randn(M, 2 * ent_dim, generator=g) * 0.5
    W = torch.randn(n_rel, ent_dim, rel_dim, generator=g) / ent_dim ** 0.5
    rel = torch.randn(n_rel, rel_dim, generator=g) * 0.5
    g_out = torch.randn(M, n_rel, generator=g)
    return emb.to(dev()), W.to(dev()), rel.to(dev()), g_out.to(dev())


_CASES = {}


def case(shape):
    """Inputs and fp64 reference of a shape, computed once (the GEMM-family parametrisation of conftest.py runs every test three times)."""
    if shape not in _CASES:
        emb, W, rel, g_out = inputs(*shape)
        ent_dim = shape[2]
        _CASES[shape] = (emb, W, rel, g_out, reference(emb[:, :ent_dim], emb[:, ent_dim:], W, rel, g_out))
    return _CASES[shape]


def run(fn, emb, W, rel, g_out, contiguous=False):
    half = emb.shape[1] // 2
    head, tail = emb[:, :half], emb[:, half:]
    if contiguous:
        head, tail = head.contiguous(), tail.contiguous()
    r = rel.detach().clone().requires_grad_(True)
    out = fn(head, tail, W, r)
    out.backward(g_out)
    return out.detach(), r.grad


@pytest.mark.parametrize("M,n_rel,ent_dim,rel_dim", SHAPES)
def test_translation_value_and_gradient(M, n_rel, ent_dim, rel_dim):
    from recon_amd import translation_residuals
    from recon_amd.translation import _chain
    emb, W, rel, g_out, (ref_out, _, _, _, ref_g) = case((M, n_rel, ent_dim, rel_dim))
    c_out, c_g = run(_chain, emb, W, rel, g_out)
    f_out, f_g = run(translation_residuals, emb, W, rel, g_out)
    assert f_out.shape == (M, n_rel) and f_g.shape == (n_rel, rel_dim)
    for what, fused, chain, ref in (("out", f_out, c_out, ref_out), ("rel.grad", f_g, c_g, ref_g)):
        e_f, e_c = rel_err(fused, ref), rel_err(chain, ref)
        print("translation %s %s: fused %.3e chain %.3e (of max |ref|)" % ((M, n_rel, ent_dim, rel_dim), what, e_f, e_c))
        assert e_f <= min(4 * e_c, 2e-5), (what, e_f, e_c)


def test_translation_empty_batch():
    from recon_amd import translation_residuals
    emb, W, rel, _ = inputs(0, 3, 8, 8)
    out = translation_residuals(emb[:, :8], emb[:, 8:], W, rel.requires_grad_(True))
    assert out.shape == (0, 3) and out.is_cuda


def test_translation_zero_rows():
    """A property without a KB-GAT relation has W_r = 0 and g_r = 0 (models/models.py:779-793): its residual and its gradient are exactly 0.
    g_r = 0 alone (row 4) is an ordinary row."""
    from recon_amd import translation_residuals
    emb, W, rel, g_out = inputs(33, 6, 16, 16)
    W[2] = 0
    rel[2] = 0
    rel[4] = 0
    ref_out, _, _, _, ref_g = reference(emb[:, :16], emb[:, 16:], W, rel, g_out)
    out, g = run(translation_residuals, emb, W, rel, g_out)
    assert (out[:, 2] == 0).all() and (g[2] == 0).all()
    from recon_amd.translation import _chain
    c_out, c_g = run(_chain, emb, W, rel, g_out)
    assert rel_err(out, ref_out) <= min(4 * rel_err(c_out, ref_out), 2e-5)
    assert rel_err(g[4], ref_g[4]) <= min(4 * rel_err(c_g[4], ref_g[4]), 2e-5)
    assert rel_err(g, ref_g) <= min(4 * rel_err(c_g, ref_g), 2e-5)


def test_translation_strided_halves_and_determinism():
    from recon_amd import translation_residuals
    emb, W, rel, g_out = inputs(65, 5, 200, 50, seed=1)
    a_out, a_g = run(translation_residuals, emb, W, rel, g_out)
    b_out, b_g = run(translation_residuals, emb, W, rel, g_out, contiguous=True)
    assert torch.equal(a_out, b_out) and torch.equal(a_g, b_g)
    c_out, c_g = run(translation_residuals, emb, W, rel, g_out)
    assert torch.equal(a_out, c_out) and torch.equal(a_g, c_g)


def test_translation_memory():
    """Forward + backward keep less than a quarter of ONE [M, n_rel, rel_dim] fp32 tensor above the inputs (two sign bits per element are
    1/16 of it); the op chain holds at least four such tensors."""
    from recon_amd import translation_residuals
    M, n_rel, ent_dim, rel_dim = 256, 64, 64, 64
    emb, W, rel, g_out = inputs(M, n_rel, ent_dim, rel_dim)
    rel.requires_grad_(True)
    head, tail = emb[:, :ent_dim], emb[:, ent_dim:]

    def forward_backward():
        translation_residuals(head, tail, W, rel).backward(g_out)
        rel.grad = None                                                   # the gradient counts in the peak and not in the next call's base
    peak, _ = peak_bytes(forward_backward)
    print("translation memory: peak above the inputs %d bytes, one intermediate %d" % (peak, M * n_rel * rel_dim * 4))
    assert peak < M * n_rel * rel_dim * 4 // 4, peak


@pytest.mark.parametrize("which", ["head", "W"])
def test_translation_fallback_gradients(which):
    """head / tail / W gradients are the op chain's: value and all four gradients against fp64."""
    from recon_amd import translation_residuals
    M, n_rel, ent_dim, rel_dim = 17, 3, 50, 200
    emb, W, rel, g_out, ref = case((M, n_rel, ent_dim, rel_dim))
    head, tail, W, rel = emb[:, :ent_dim].clone(), emb[:, ent_dim:].clone(), W.clone(), rel.clone()
    rel.requires_grad_(True)
    if which == "head":
        head.requires_grad_(True)
        tail.requires_grad_(True)
    if which == "W":
        W.requires_grad_(True)
    out = translation_residuals(head, tail, W, rel)
    out.backward(g_out)
    assert rel_err(out, ref[0]) <= 2e-5
    got = {"head": head.grad, "tail": tail.grad, "W": W.grad, "rel": rel.grad}
    for i, k in enumerate(("head", "tail", "W", "rel")):
        if got[k] is None:
            assert k != "rel" and (which == "W") == (k != "W")           # only the tensors that did not ask have none
            continue
        assert rel_err(got[k], ref[1 + i]) <= 2e-5, k
    # with all four asked for, all four are there
    head2, tail2, W2, rel2 = (x.detach().clone().requires_grad_(True) for x in (head, tail, W, rel))
    translation_residuals(head2, tail2, W2, rel2).backward(g_out)
    for i, x in enumerate((head2, tail2, W2, rel2)):
        assert rel_err(x.grad, ref[1 + i]) <= 2e-5, i


def test_translation_model_matches_op():
    """RECON.translation_scores is the op on the two halves of its argument: bit-identical."""
    from recon_amd import translation_residuals
    from recon_amd.gpgnn import RECON
    from tests.test_host_cpu import KGGAT_P, recon_constructor_tables
    g = load_golden("recon1_untied")
    m = RECON(dict(KGGAT_P), g["emb"], 4, 3, list(range(int(g["n_chars"]))), *recon_constructor_tables(g)).to(dev())
    nz = torch.from_numpy(g["nz"]).to(dev())
    half = nz.shape[1] // 2
    a = m.translation_scores(nz)
    b = translation_residuals(nz[:, :half].float(), nz[:, half:].float(), m.W_ent2rel, m.gat_relation_embeddings)
    assert a.shape == (nz.shape[0], 3) and torch.equal(a.detach(), b.detach())
    np.testing.assert_allclose(a.detach().cpu().numpy(), reference(nz[:, :half], nz[:, half:], m.W_ent2rel, m.gat_relation_embeddings).numpy(), atol=1e-4)
