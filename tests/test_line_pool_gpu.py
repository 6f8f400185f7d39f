"""recon_amd.entity_line_pool (csrc/line_pool.hip) against the stock lines of models/models.py:73-81 in fp64 on the CPU, and against the
fixtures written from the reference's EntityEmbedding and RECON_EAC.

Shapes, inputs, the near-tie rule, the fp64 oracle and the comparison are those of tests/test_line_pool_cpu.py, which also guards them;
the band is `op_checks.bound` of the stock fp32 chain's own error on the GPU, for the value and every gradient.  The figures measured on
an MI355X are in DESIGN.md section 24."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import load_golden
from op_checks import calls_of, dev, eac_fixture, entries_declared_and_bound, peak_bytes, pinned, rel_err, rounded, same
from test_char_features_cpu import fixture_model
from test_line_pool_cpu import (CITES, ENTRIES, FIXTURE, LONG_THIN, REF_WIDTHS, SHAPES, SMALL_ODD, UNALIGNED, case, failures, inputs,
                                reference, run, shape_id, stock, tie_case)

pytestmark = pytest.mark.gpu


def kernels_ran(monkeypatch):
    from recon_amd import line_pool
    return calls_of(monkeypatch, line_pool._LinePool, "apply")


def chain_fn(*a):
    from recon_amd.line_pool import _chain
    return _chain(*a)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_value_and_gradients(shape, monkeypatch):
    from recon_amd import _lib, entity_line_pool
    assert _lib.lib().recon_line_pool_supported(*shape)
    c = case(shape)
    calls = kernels_ran(monkeypatch)
    fused = run(entity_line_pool, c, dev())
    assert len(calls) == 1, "the kernels take this shape: the op must not run the chain"
    chain = run(chain_fn, c, dev())
    print("entity_line_pool %s: %d of %d cells near a tie" % (shape_id(shape), int(c["ties"].sum()), c["ties"].numel()))
    bad = failures(fused, chain, c["ref"], shape_id(shape))
    assert not bad, bad


def test_a_scattered_mask(monkeypatch):
    from recon_amd import entity_line_pool
    calls = kernels_ran(monkeypatch)
    for shape in (SMALL_ODD, UNALIGNED, REF_WIDTHS):
        c = dict(case(shape))
        P = c["mask"].shape[1]
        g = torch.Generator().manual_seed(5 + P)
        mask = torch.rand(shape[0], P, generator=g) < 0.5
        mask[torch.arange(shape[0]), torch.randint(0, P, (shape[0],), generator=g)] = False      # one valid position at least
        mask[0, 0], mask[0, P - 1] = True, False                          # not a suffix: the first masked, the last valid
        c["ref"] = reference(stock, c["states"], c["weight"], c["bias"], mask, c["g_out"])
        bad = failures(run(entity_line_pool, c, dev(), mask=mask), run(chain_fn, c, dev(), mask=mask), c["ref"], "%s scattered mask" % shape_id(shape))
        assert not bad, bad
    assert len(calls) == 3


def test_a_fully_masked_entity_among_valid_ones(monkeypatch):
    from recon_amd import entity_line_pool
    c = dict(case(REF_WIDTHS))
    mask = c["mask"].clone()
    mask[3] = True
    ref = reference(stock, c["states"], c["weight"], c["bias"], mask, c["g_out"])
    calls = kernels_ran(monkeypatch)
    fused, chain = run(entity_line_pool, c, dev(), mask=mask), run(chain_fn, c, dev(), mask=mask)
    assert len(calls) == 1
    assert (fused[0][3] == -float('inf')).all() and torch.count_nonzero(fused[1][3]) == 0 and torch.count_nonzero(ref[1][3]) == 0
    others = [i for i in range(REF_WIDTHS[0]) if i != 3]
    cut = lambda r: [r[0][others], r[1], r[2], r[3]]                      # (-inf has no relative error: the other entities' values)
    bad = failures(cut(fused), cut(chain), cut(ref), "one fully masked entity")
    assert not bad, bad


def test_an_exact_tie_takes_the_lowest_position(monkeypatch):
    from recon_amd import entity_line_pool
    c = tie_case()                                                       # small integers: every sum exact in fp32, in any order
    calls = kernels_ran(monkeypatch)
    got = run(entity_line_pool, c, dev())
    assert len(calls) == 1
    for a, r in zip(got, c["ref"]):
        assert torch.equal(a.cpu().double(), r)


def test_a_nan_at_an_unmasked_position_gives_nan_and_a_masked_one_does_not():
    from recon_amd import entity_line_pool
    states, weight, bias, mask, _ = inputs(*SMALL_ODD)
    mask = torch.zeros_like(mask)
    mask[1, -1] = True
    states[0, 2, 1] = float('nan')                                       # entity 0: under the unmasked positions 0..2
    states[1, -1, 0] = float('nan')                                      # entity 1: under its masked last position alone
    out = entity_line_pool(*[t.to(dev()) for t in (states, weight, bias, mask)]).cpu()
    want = stock(states, weight, bias, mask)
    assert torch.isnan(out[0]).all() and torch.isnan(want[0]).all() and torch.isfinite(out[1:]).all() and torch.isfinite(want[1:]).all()


def test_forward_and_backward_are_bitwise_reproducible():
    from recon_amd import entity_line_pool
    for shape in (FIXTURE, UNALIGNED, REF_WIDTHS, LONG_THIN):
        c = case(shape)
        same(run(entity_line_pool, c, dev()), run(entity_line_pool, c, dev()))


def test_second_backward_over_a_retained_graph_gives_the_same_bits(monkeypatch):
    from recon_amd import entity_line_pool
    c = case(REF_WIDTHS)
    leaves = [c[k].to(dev()).requires_grad_(True) for k in ("states", "weight", "bias")]
    conv = calls_of(monkeypatch, F, "conv1d")
    out = entity_line_pool(*leaves, c["mask"].to(dev()))
    kept = out.clone()
    g = c["g_out"].to(dev())
    first = torch.autograd.grad(out, leaves, g, retain_graph=True)
    second = torch.autograd.grad(out, leaves, g, retain_graph=True)
    same(first, second)
    same([kept], [out])                                                 # the backward destroys nothing
    assert not conv
    for a, r in zip(first, c["ref"][1:]):
        assert rel_err(a, r) <= 2e-5


def test_a_strided_view_gives_the_contiguous_copys_bits(monkeypatch):
    from recon_amd import _lib, entity_line_pool
    calls = kernels_ran(monkeypatch)
    strides, real = [], _lib.rows_in_place
    monkeypatch.setattr(_lib, "rows_in_place", lambda *a, **k: (lambda r: strides.append(r[1]) or r)(real(*a, **k)))
    for shape in (FIXTURE, UNALIGNED, REF_WIDTHS):
        c = case(shape)
        U, Ln, C = c["states"].shape
        wide = torch.full((U, Ln, C + 7), 99.0, device=dev())
        wide[:, :, 3:3 + C] = c["states"].to(dev())
        wide.requires_grad_(True)
        view = wide[:, :, 3:3 + C]
        assert not view.is_contiguous()
        weight, bias = c["weight"].to(dev()).requires_grad_(True), c["bias"].to(dev()).requires_grad_(True)
        del strides[:]
        out = entity_line_pool(view, weight, bias, c["mask"].to(dev()))
        out.backward(c["g_out"].to(dev()))
        assert strides == [C + 7, C + 7]                                 # read in place, forward and backward
        plain = run(entity_line_pool, c, dev())
        same([out.detach(), wide.grad[:, :, 3:3 + C].contiguous(), weight.grad, bias.grad], plain)
        assert torch.count_nonzero(wide.grad[:, :, :3]) == 0 and torch.count_nonzero(wide.grad[:, :, 3 + C:]) == 0      # the view's columns only
    assert len(calls) == 6


@pytest.mark.parametrize("needs", [(True, False, False), (False, True, True), (False, True, False), (False, False, True)],
                         ids=["states", "parameters", "weight", "bias"])
def test_only_the_wanted_gradients_are_computed(needs, monkeypatch):
    from recon_amd import entity_line_pool
    calls = kernels_ran(monkeypatch)
    for shape in (UNALIGNED, REF_WIDTHS):
        c = case(shape)
        full = run(entity_line_pool, c, dev())
        part = run(entity_line_pool, c, dev(), needs=needs)
        same(part, [full[0]] + [f if n else None for f, n in zip(full[1:], needs)])
    assert len(calls) == 4


def test_no_grad_gives_the_training_forwards_bits_and_memory_is_the_output_alone():
    from recon_amd import entity_line_pool
    U, Ln, C, E, k = REF_WIDTHS
    c = case(REF_WIDTHS)
    states, weight, bias, mask = (c[n].to(dev()) for n in ("states", "weight", "bias", "mask"))
    weight.requires_grad_(True)
    trained = entity_line_pool(states, weight, bias, mask)
    with torch.no_grad():
        plain = entity_line_pool(states, weight, bias, mask)
    assert trained.grad_fn is not None and plain.grad_fn is None
    same([trained.detach()], [plain])
    del trained, plain

    def forward():
        with torch.no_grad():
            return entity_line_pool(states, weight, bias, mask)
    unwritten = U * E * (Ln - k + 1) * 4                                 # the convolution output the stock lines write (and its masked copy)
    peak, out = peak_bytes(forward)
    print("entity_line_pool memory: no_grad peak %d bytes, the [U, E, P] tensor %d" % (peak, unwritten))
    assert peak == rounded(U * E * 4) and peak < unwritten, (peak, U * E * 4)
    del out
    peak, out = peak_bytes(lambda: entity_line_pool(states, weight, bias, mask))
    print("entity_line_pool memory: training forward peak %d bytes" % peak)
    assert out.grad_fn is not None and peak == rounded(U * E * 4) + rounded(U * E) and peak < unwritten, (peak, U * E * 4, U * E)
    peak_chain, _ = peak_bytes(lambda: chain_fn(states, weight, bias, mask))
    assert peak_chain >= unwritten > peak


def test_create_graph_unsupported_shape_and_bf16_run_the_chain(monkeypatch):
    from recon_amd import _lib, entity_line_pool
    kernel_calls, conv = kernels_ran(monkeypatch), calls_of(monkeypatch, F, "conv1d")
    c = case(FIXTURE)
    leaves = [c[k].to(dev()).requires_grad_(True) for k in ("states", "weight", "bias")]
    mask = c["mask"].to(dev())
    out = entity_line_pool(*leaves, mask)
    assert len(kernel_calls) == 1 and not conv
    grads = torch.autograd.grad(out, leaves, c["g_out"].to(dev()), create_graph=True)
    assert len(conv) == 1                                               # the backward recomputed through the stock lines
    for a, r in zip(grads, c["ref"][1:]):
        assert rel_err(a, r) <= 2e-5
    assert grads[0].requires_grad and grads[1].requires_grad
    grads[0].square().sum().backward()
    assert leaves[1].grad is not None and torch.isfinite(leaves[1].grad).all()
    # P = 256: one position past the position byte
    del conv[:]
    wide = (3, 256, 4, 2, 1)
    assert not _lib.lib().recon_line_pool_supported(*wide)
    states, weight, bias, m, g_out = inputs(*wide)
    cw = dict(states=states, weight=weight, bias=bias, mask=m, g_out=g_out)
    a = run(entity_line_pool, cw, dev())
    assert len(kernel_calls) == 1 and len(conv) == 1
    for x, y in zip(a, run(chain_fn, cw, dev())):                        # (the vendor convolution's backward is not bitwise reproducible)
        assert rel_err(x, y.double().cpu()) <= 2e-5
    # bf16
    del conv[:]
    out = entity_line_pool(*[c[k].to(dev()).bfloat16() for k in ("states", "weight", "bias")], mask)
    assert len(kernel_calls) == 1 and len(conv) == 1 and out.dtype == torch.bfloat16


def test_the_fused_path_needs_neither_the_convolution_nor_the_mask_copy(monkeypatch):
    from recon_amd import entity_line_pool
    c = case(REF_WIDTHS)
    monkeypatch.setattr(F, "conv1d", lambda *a, **k: pytest.fail("F.conv1d ran"))
    monkeypatch.setattr(torch.Tensor, "masked_fill", lambda *a, **k: pytest.fail("masked_fill ran"))
    got = run(entity_line_pool, c, dev())
    for a, r in zip(got, c["ref"]):
        assert rel_err(a, r) <= 2e-5


def test_empty_batch(monkeypatch):
    from recon_amd import entity_line_pool
    calls = kernels_ran(monkeypatch)
    states, weight, bias, mask, _ = inputs(*FIXTURE)
    weight, bias = weight.to(dev()).requires_grad_(True), bias.to(dev()).requires_grad_(True)
    empty = states[:0].to(dev()).requires_grad_(True)
    out = entity_line_pool(empty, weight, bias, mask[:0].to(dev()))
    assert out.shape == (0, 2) and out.is_cuda and len(calls) == 1
    out.sum().backward()
    assert empty.grad.shape == (0, 4, 6)
    for t in (weight, bias):
        assert t.grad is not None and torch.count_nonzero(t.grad) == 0


# ------------------------------------------------------------------------------------------------------------- the models
def _entity_conv(module):
    def forbidden(m):
        conv = module(m).conv1d_entity
        assert type(conv) is nn.Conv1d
        return [conv], "conv1d_entity.forward ran"
    return forbidden


def test_ctx_lstm_fixture_through_the_op(monkeypatch):
    g = load_golden("ctx_lstm1")
    m = fixture_model(g)
    t = lambda k: torch.from_numpy(g[k]).to(dev())
    required = ["g.conv1d_entity.weight", "g.conv1d_entity.bias"]
    pinned(m, g, lambda m: m(t("words"), t("chars"), t("mask")), "ctx_lstm1", monkeypatch, "fused_line_pool", kernels_ran(monkeypatch),
           _entity_conv(lambda m: m), required)


def test_recon_eac_fixture_through_the_op(monkeypatch):
    m, g, out_of, name = eac_fixture()
    required = ["g.entity_embedding_module.conv1d_entity.weight", "g.entity_embedding_module.conv1d_entity.bias"]
    m.entity_embedding_module.fused_line_pool = True                    # the switch is the encoder's; `pinned` sets the model's attribute of that name
    pinned(m, g, out_of, name, monkeypatch, "fused_line_pool", kernels_ran(monkeypatch), _entity_conv(lambda m: m.entity_embedding_module), required)


def test_the_four_entries_are_declared_bound_and_cite_the_reference():
    entries_declared_and_bound(ENTRIES, CITES)
