"""recon_amd.relation_logits (csrc/rel_head.hip) against the stock lines of models/models.py:213 / :693-697 / :954-966 in fp64 on the CPU,
and against the fixtures written from the reference's RECON_EAC_KGGAT and RECON.

Shapes, inputs, the fp64 oracle and the comparison are those of tests/test_relation_head_cpu.py, which also guards them; the band is
`op_checks.bound` of the stock fp32 chain's own error on the GPU, for the value and every gradient.  The figures measured on an MI355X
are in DESIGN.md section 23."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import load_golden
from op_checks import calls_of, close, dev, eac_fixture, gpgnn_fixture, kggat_fixture, peak_bytes, pinned, rel_err, rounded, same, state_dict_of
from test_relation_head_cpu import (SHAPES, FIXTURE, REF_WIDTHS, FOUR_BLOCKS, REF_BATCH, EMPTY_SCATTER, case, chain_fn, failures, inputs, run,
                                    shape_id, width)

pytestmark = pytest.mark.gpu


def kernels_ran(monkeypatch):
    from recon_amd import relation_head
    return calls_of(monkeypatch, relation_head._RelationLogits, "apply")


def on_gpu(c, needs=None):
    """The case's tensors on the GPU as leaves: blocks, W, b, scattered, positions, g_out."""
    nb = len(c["blocks"])
    needs = [True] * nb if needs is None else needs
    blocks = [t.to(dev()).requires_grad_(n) for t, n in zip(c["blocks"], needs)]
    W, b = c["W"].to(dev()).requires_grad_(True), c["b"].to(dev()).requires_grad_(True)
    scattered = None if c["scattered"] is None else c["scattered"].to(dev()).requires_grad_(True)
    pos = None if c["pos"] is None else c["pos"].to(dev())
    return blocks, W, b, scattered, pos, c["g_out"].to(dev())


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_value_and_gradients(shape, monkeypatch):
    from recon_amd import _lib, relation_logits
    assert _lib.lib().recon_relation_logits_supported(shape[0], len(shape[1]), width(shape), shape[3])
    c = case(shape)
    calls = kernels_ran(monkeypatch)
    fused = run(relation_logits, c, dev())
    assert len(calls) == 1, "the kernels take this shape: the op must not run the chain"
    chain = run(chain_fn, c, dev())
    bad = failures(fused, chain, c["ref"], shape, shape_id(shape))
    assert not bad, bad


def test_a_block_without_gradient_gets_none(monkeypatch):
    from recon_amd import relation_logits
    c = case(REF_WIDTHS)
    calls = kernels_ran(monkeypatch)
    needs = [True, False]                                                # the KB-GAT columns
    fused = run(relation_logits, c, dev(), needs=needs)
    chain = run(chain_fn, c, dev(), needs=needs)
    assert len(calls) == 1 and fused[2] is None and chain[2] is None and fused[1] is not None
    ref = list(c["ref"])
    ref[2] = None
    bad = failures(fused, chain, ref, REF_WIDTHS, "no gradient for block 1")
    assert not bad, bad
    # scattered under no_grad semantics: a scattered block that does not require a gradient gets none either
    blocks, W, b, scattered, pos, g = on_gpu(c, needs)
    scattered = scattered.detach()
    relation_logits(blocks, W, b, scattered, pos).backward(g)
    assert scattered.grad is None and blocks[1].grad is None
    same([blocks[0].grad, W.grad, b.grad], [fused[1], fused[4], fused[5]])


def test_strided_views_give_the_contiguous_copies_bits(monkeypatch):
    from recon_amd import relation_logits
    calls = kernels_ran(monkeypatch)

    def view_of(left, right):
        def strided(x):
            wide = torch.full((x.shape[0], x.shape[1] + left + right), 99.0, device=x.device)
            wide[:, left:left + x.shape[1]] = x
            v = wide[:, left:left + x.shape[1]]
            assert not v.is_contiguous() or x.shape[0] <= 1
            return v.detach()
        return strided
    for shape, left, right in ((REF_WIDTHS, 3, 4), (FOUR_BLOCKS, 4, 4), (FIXTURE, 1, 0)):      # (3, 4): the float4 blocks become scalar ones
        c = case(shape)
        same(run(relation_logits, c, dev()), run(relation_logits, c, dev(), block_of=view_of(left, right), scattered_of=view_of(left, right)))
    assert len(calls) == 6


def test_forward_and_backward_are_bitwise_reproducible():
    from recon_amd import relation_logits
    for shape in (FIXTURE, REF_WIDTHS, FOUR_BLOCKS):
        c = case(shape)
        same(run(relation_logits, c, dev()), run(relation_logits, c, dev()))


def test_second_backward_over_a_retained_graph_gives_the_same_bits(monkeypatch):
    from recon_amd import relation_logits
    c = case(REF_WIDTHS)
    blocks, W, b, scattered, pos, g = on_gpu(c)
    lin = calls_of(monkeypatch, F, "linear")
    out = relation_logits(blocks, W, b, scattered, pos)
    kept = out.clone()
    leaves = blocks + [scattered, W, b]
    first = torch.autograd.grad(out, leaves, g, retain_graph=True)
    second = torch.autograd.grad(out, leaves, g, retain_graph=True)
    same(first, second)
    same([kept], [out])                                                 # the backward destroys nothing
    assert not lin
    for a, r in zip(first, c["ref"][1:]):
        assert rel_err(a, r) <= 2e-5


def test_no_grad_gives_the_training_forwards_bits_and_allocates_the_output_alone():
    from recon_amd import _lib, relation_logits
    shape = REF_BATCH
    c = case(shape)
    blocks, W, b, scattered, pos, _ = on_gpu(c)
    trained = relation_logits(blocks, W, b, scattered, pos)
    with torch.no_grad():
        plain = relation_logits(blocks, W, b, scattered, pos)
    assert trained.grad_fn is not None and plain.grad_fn is None
    same([trained.detach()], [plain])
    del trained, plain

    def forward():
        with torch.no_grad():
            return relation_logits(blocks, W, b, scattered, pos)
    peak, out = peak_bytes(forward)
    ws = _lib.lib().recon_relation_logits_workspace_bytes(shape[0], len(shape[1]), width(shape), shape[3], 0)
    assert peak <= rounded(out.numel() * 4) + rounded(ws), (peak, out.numel() * 4, ws)      # neither the zeros, nor the cat


def test_a_tile_without_present_rows_and_one_with_its_first_and_last(monkeypatch):
    from recon_amd import relation_logits
    rows = list(range(0, 64, 3)) + [128, 191] + [192, 199]             # tile 1 (rows 64..127): none; tile 2 (128..191): its first and last row
    shape = (200, (12, 6), (3, len(rows)), 3)
    c = case(shape, positions=rows)
    assert not any(64 <= r < 128 for r in rows) and [r for r in rows if 128 <= r < 192] == [128, 191]
    calls = kernels_ran(monkeypatch)
    fused, chain = run(relation_logits, c, dev()), run(chain_fn, c, dev())
    assert len(calls) == 1
    bad = failures(fused, chain, c["ref"], shape, "sparse tiles")
    assert not bad, bad
    wide = (200, (48, 400), (353, len(rows)), 353)                     # the same rows at the reference's widths
    c = case(wide, positions=rows)
    bad = failures(run(relation_logits, c, dev()), run(chain_fn, c, dev()), c["ref"], wide, "sparse tiles, reference widths")
    assert not bad, bad


def test_create_graph_unsupported_shape_and_bf16_run_the_chain(monkeypatch):
    from recon_amd import _lib, relation_logits
    kernel_calls, lin = kernels_ran(monkeypatch), calls_of(monkeypatch, F, "linear")
    c = case(FIXTURE)
    blocks, W, b, scattered, pos, g = on_gpu(c)
    out = relation_logits(blocks, W, b, scattered, pos)
    assert len(kernel_calls) == 1 and not lin
    leaves = blocks + [scattered, W, b]
    grads = torch.autograd.grad(out, leaves, g, create_graph=True)
    assert len(lin) == 1                                                # the backward recomputed through the stock lines
    for i, (a, r) in enumerate(zip(grads, c["ref"][1:])):
        assert rel_err(a, r) <= 2e-5 and (a.requires_grad or i == len(grads) - 1)      # (d_b = the column sums of g_out: a constant)
    grads[0].square().sum().backward()
    assert W.grad is not None and torch.isfinite(W.grad).all()
    # N = 1025: above what the kernels take
    del lin[:]
    wide = (3, (8,), None, 1025)
    assert not _lib.lib().recon_relation_logits_supported(3, 1, 8, 1025)
    blocks, W, b, scattered, pos, g_out = inputs(wide)
    cw = dict(blocks=blocks, W=W, b=b, scattered=scattered, pos=pos, g_out=g_out)
    a = run(relation_logits, cw, dev())
    assert len(kernel_calls) == 1 and len(lin) == 1
    same(a, run(chain_fn, cw, dev()))
    # bf16
    del lin[:]
    h = lambda t: t.to(dev()).bfloat16()
    out = relation_logits([h(t) for t in c["blocks"]], h(c["W"]), h(c["b"]), h(c["scattered"]), c["pos"].to(dev()))
    assert len(kernel_calls) == 1 and len(lin) == 1 and out.dtype == torch.bfloat16


def test_the_fused_path_needs_neither_f_linear_nor_cat(monkeypatch):
    from recon_amd import relation_logits
    c = case(REF_WIDTHS)
    monkeypatch.setattr(F, "linear", lambda *a, **k: pytest.fail("F.linear ran"))
    monkeypatch.setattr(torch, "cat", lambda *a, **k: pytest.fail("torch.cat ran"))
    got = run(relation_logits, c, dev())
    for a, r in zip(got, c["ref"]):
        assert rel_err(a, r) <= 2e-5


def test_empty_batch_and_empty_scattered_block(monkeypatch):
    from recon_amd import relation_logits
    calls = kernels_ran(monkeypatch)
    blocks, W, b, scattered, pos, _ = inputs(FIXTURE)
    W, b = W.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)
    empty = [t[:0].to(dev()).view(0, 1, t.shape[1]).requires_grad_(True) for t in blocks]
    s0, p0 = scattered[:0].to(dev()).requires_grad_(True), pos[:0].to(dev())
    out = relation_logits(empty, W, b, s0, p0)
    assert out.shape == (0, 1, 3) and out.is_cuda and len(calls) == 1
    out.sum().backward()
    assert empty[0].grad.shape == (0, 1, 12)
    for t in (W, b):
        assert t.grad is not None and torch.count_nonzero(t.grad) == 0
    # Mnz = 0 passed as empty tensors: an all-zero block
    W.grad = b.grad = None
    full = [t.to(dev()).requires_grad_(True) for t in blocks]
    out = relation_logits(full, W, b, s0, p0)
    assert len(calls) == 2
    out.backward(torch.ones_like(out))
    x64 = torch.cat([t.double() for t in blocks], dim=1)
    assert rel_err(out, x64 @ W.detach().double().cpu()[:, :18].t() + b.detach().double().cpu()) <= 2e-5
    assert torch.count_nonzero(W.grad[:, 18:]) == 0 and rel_err(W.grad[:, :18], torch.ones(24, 3).double().t() @ x64) <= 2e-5
    assert rel_err(b.grad, torch.full((3,), 24.0).double()) <= 2e-5 and s0.grad is None


# ------------------------------------------------------------------------------------------------------------- the models
def _classifier(m):
    assert type(m.linear3) is nn.Linear
    return [m.linear3], "linear3.forward ran"


def recon_fixture():
    """(model, fixture, model -> logits, name) of the fixture written from the reference's RECON, built as tests/test_prop_gpu.py builds it."""
    from recon_amd.gpgnn import RECON
    from tests.test_host_cpu import KGGAT_P, recon_constructor_tables
    g = load_golden("recon1_untied")
    m = RECON(dict(KGGAT_P), g["emb"], 4, 3, list(range(int(g["n_chars"]))), *recon_constructor_tables(g))
    m.load_state_dict(state_dict_of(g), strict=False)
    t = lambda k: torch.from_numpy(g[k]).to(dev())
    args = lambda: (t("sent"), t("mark"), None, None, None, t("ctx_words"), t("ctx_chars"), t("ctx_mask"), t("pos"), int(g["max_occ"]))
    return m, g, lambda m: m(*args(), t("nz"), t("nz_pos"), t("gat")), "recon1_untied"


def test_recon_eac_kggat_fixture_through_the_op(monkeypatch):
    pinned(*kggat_fixture(), monkeypatch, "fused_classifier", kernels_ran(monkeypatch), _classifier, ["g.linear3."])


def test_recon_fixture_through_the_op(monkeypatch):
    pinned(*recon_fixture(), monkeypatch, "fused_classifier", kernels_ran(monkeypatch), _classifier, ["g.linear3."])


def test_recon_without_known_embeddings_gives_finite_logits_through_the_op(monkeypatch):
    m, g, _, _ = recon_fixture()
    m.fused_classifier = True
    m.train().to(dev())
    calls = kernels_ran(monkeypatch)
    monkeypatch.setattr(m.linear3, "forward", lambda *a, **k: pytest.fail("linear3.forward ran"))
    t = lambda k: torch.from_numpy(g[k]).to(dev())
    out0 = m(t("sent"), t("mark"), None, None, None, t("ctx_words"), t("ctx_chars"), t("ctx_mask"), t("pos"), int(g["max_occ"]), t("nz")[:0],
             t("nz_pos")[:0], t("gat"))
    assert len(calls) == 1 and out0.shape == (4 * 6, 3) and torch.isfinite(out0).all()
    out0.sum().backward()
    assert torch.isfinite(m.linear3.weight.grad).all() and torch.count_nonzero(m.linear3.weight.grad[:, -3:]) == 0


@pytest.mark.parametrize("fixture", [lambda: gpgnn_fixture("gpgnn1_untied"), eac_fixture], ids=["gpgnn", "recon_eac"])
def test_one_block_has_nothing_to_fuse(fixture, monkeypatch):
    m, g, out_of, name = fixture()
    m.fused_classifier = True
    m.train().to(dev())
    op, lin = kernels_ran(monkeypatch), calls_of(monkeypatch, m.linear3, "forward")
    out = out_of(m)
    assert not op and len(lin) == 1
    close(out, g["out"], atol=1e-4, what=name + " logits")
