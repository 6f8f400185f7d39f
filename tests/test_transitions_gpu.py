"""recon_amd.pair_transitions (csrc/pair_trans.hip) against the stock lines of models/models.py:185-192 / :240-249 in fp64 on the CPU, and
against the fixtures written from the reference's GPGNN, RECON_EAC and RECON_EAC_KGGAT.

Inputs, the g_out mask at relu's kink and the fp64 oracle are those of tests/test_transitions_cpu.py, which also guards them; the band is
`op_checks.bound` of the stock fp32 chain's own error on the GPU, for every T_l, d_x, every d_W_l and every d_b_l.  The figures measured on
an MI355X are in DESIGN.md section 22."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from op_checks import calls_of, dev, eac_fixture, gpgnn_fixture, kggat_fixture, pinned, rel_err, same
from test_transitions_cpu import SHAPES, ACTS, LONG_THIN, REF_ONE, case, run, failures, inputs

pytestmark = pytest.mark.gpu


def chain_fn(x, Ws, bs, act):
    from recon_amd.transitions import _chain
    return _chain(x, Ws, bs, act)


def kernels_ran(monkeypatch):
    from recon_amd import transitions
    return calls_of(monkeypatch, transitions._PairTransitions, "apply")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradients(shape, act, monkeypatch):
    from recon_amd import _lib, pair_transitions
    assert _lib.lib().recon_pair_transitions_supported(*shape)
    c = case(shape, act)
    assert c["share"] <= 0.01 and (shape[0] * shape[2] * shape[3] >= 100 or c["share"] == 0.0)
    calls = kernels_ran(monkeypatch)
    fused = run(pair_transitions, c, act, dev())
    assert len(calls) == 1, "the kernels take this shape: the op must not run the chain"
    chain = run(chain_fn, c, act, dev())
    bad = failures(fused, chain, c["ref"], "%s %s" % (shape, act))
    assert not bad, bad


def test_an_output_without_gradient_and_a_missing_bias():
    from recon_amd import pair_transitions
    shape, act = (17, 20, 24, 3), "tanh"
    c = case(shape, act)
    x = c["x"].to(dev()).requires_grad_(True)
    Ws = [W.to(dev()).requires_grad_(True) for W in c["Ws"]]
    bs = [c["bs"][0].to(dev()).requires_grad_(True), None, c["bs"][2].to(dev()).requires_grad_(True)]
    Ts = pair_transitions(x, Ws, bs, act)
    leaves = [x] + Ws + [bs[0], bs[2]]
    got = torch.autograd.grad([Ts[0], Ts[1]], leaves, [c["g_out"][0].to(dev()), c["g_out"][1].to(dev())], allow_unused=True)   # Ts[2]: none
    x64 = c["x"].double().requires_grad_(True)
    W64 = [W.double().requires_grad_(True) for W in c["Ws"]]
    b64 = [c["bs"][0].double().requires_grad_(True), None, c["bs"][2].double().requires_grad_(True)]
    R = [torch.tanh(F.linear(x64, W, b)) for W, b in zip(W64, b64)]
    ref = torch.autograd.grad([R[0], R[1]], [x64] + W64 + [b64[0], b64[2]], [c["g_out"][0].double(), c["g_out"][1].double()], allow_unused=True)
    for t, r in zip(Ts, R):
        assert rel_err(t, r.detach()) <= 2e-5
    assert rel_err(Ts[1], torch.tanh(c["x"].double() @ c["Ws"][1].double().t())) <= 2e-5                  # no bias in layer 1
    for i, (a, r) in enumerate(zip(got, ref)):
        if r is None:                                                   # W_2 and b_2: their output received no gradient
            assert i in (3, 5) and a is not None and a.shape == leaves[i].shape and torch.count_nonzero(a) == 0
        else:
            assert rel_err(a, r) <= 2e-5, i


def test_row_strided_x_gives_the_contiguous_copys_bits(monkeypatch):
    from recon_amd import pair_transitions
    calls = kernels_ran(monkeypatch)

    def strided(x):
        wide = torch.full((x.shape[0], x.shape[1] + 8), 99.0, device=x.device)
        wide[:, 4:4 + x.shape[1]] = x
        v = wide[:, 4:4 + x.shape[1]]
        assert not v.is_contiguous()
        return v.detach()
    for shape, act in ((LONG_THIN, "relu"), ((531, 36, 100, 2), "tanh")):
        c = case(shape, act)
        same(run(pair_transitions, c, act, dev()), run(pair_transitions, c, act, dev(), x_of=strided))
    assert len(calls) == 4


def test_forward_and_backward_are_bitwise_reproducible():
    from recon_amd import pair_transitions
    for shape, act in ((LONG_THIN, "relu"), (REF_ONE, "tanh"), ((17, 20, 24, 3), "linear")):
        c = case(shape, act)
        same(run(pair_transitions, c, act, dev()), run(pair_transitions, c, act, dev()))


def test_second_backward_over_a_retained_graph_gives_the_same_bits(monkeypatch):
    from recon_amd import pair_transitions
    shape, act = (531, 36, 100, 2), "relu"
    c = case(shape, act)
    x = c["x"].to(dev()).requires_grad_(True)
    Ws = [W.to(dev()).requires_grad_(True) for W in c["Ws"]]
    bs = [b.to(dev()).requires_grad_(True) for b in c["bs"]]
    lin = calls_of(monkeypatch, F, "linear")
    Ts = pair_transitions(x, Ws, bs, act)
    kept = [t.clone() for t in Ts]
    gs = [g.to(dev()) for g in c["g_out"]]
    first = torch.autograd.grad(Ts, [x] + Ws + bs, gs, retain_graph=True)
    second = torch.autograd.grad(Ts, [x] + Ws + bs, gs, retain_graph=True)
    same(first, second)
    same(kept, list(Ts))                                                # the backward destroys nothing
    assert not lin
    for a, r in zip(first, c["ref"][2:]):
        assert rel_err(a, r) <= 2e-5


def test_no_grad_gives_the_training_forwards_bits():
    from recon_amd import pair_transitions
    c = case((531, 36, 100, 2), "tanh")
    x = c["x"].to(dev()).requires_grad_(True)
    Ws = [W.to(dev()).requires_grad_(True) for W in c["Ws"]]
    bs = [b.to(dev()) for b in c["bs"]]
    trained = pair_transitions(x, Ws, bs, "tanh")
    with torch.no_grad():
        plain = pair_transitions(x, Ws, bs, "tanh")
    assert all(t.grad_fn is not None for t in trained) and all(t.grad_fn is None for t in plain)
    same([t.detach() for t in trained], list(plain))


def test_create_graph_unsupported_shape_and_bf16_run_the_chain(monkeypatch):
    from recon_amd import _lib, pair_transitions
    kernel_calls, lin = kernels_ran(monkeypatch), calls_of(monkeypatch, F, "linear")
    c = case((17, 20, 24, 3), "tanh")
    x = c["x"].to(dev()).requires_grad_(True)
    Ws = [W.to(dev()).requires_grad_(True) for W in c["Ws"]]
    bs = [b.to(dev()).requires_grad_(True) for b in c["bs"]]
    gs = [g.to(dev()) for g in c["g_out"]]
    Ts = pair_transitions(x, Ws, bs, "tanh")
    assert len(kernel_calls) == 1 and not lin
    grads = torch.autograd.grad(Ts, [x] + Ws + bs, gs, create_graph=True)
    assert len(lin) == 3                                                # the backward recomputed through the stock lines
    for a, r in zip(grads, c["ref"][3:]):
        assert rel_err(a, r) <= 2e-5 and a.requires_grad
    grads[0].square().sum().backward()
    assert Ws[0].grad is not None and torch.isfinite(Ws[0].grad).all()
    # K = 6: no multiple of 4
    del lin[:]
    assert not _lib.lib().recon_pair_transitions_supported(5, 6, 8, 2)
    x6, W6, b6, raw = inputs(5, 6, 8, 2)
    c6 = dict(x=x6, Ws=W6, bs=b6, g_out=raw)
    a = run(pair_transitions, c6, "relu", dev())
    assert len(kernel_calls) == 1 and len(lin) == 2
    same(a, run(chain_fn, c6, "relu", dev()))
    # bf16
    del lin[:]
    out = pair_transitions(c["x"].to(dev()).bfloat16(), [W.to(dev()).bfloat16() for W in c["Ws"]], [b.to(dev()).bfloat16() for b in c["bs"]], "relu")
    assert len(kernel_calls) == 1 and len(lin) == 3 and out[0].dtype == torch.bfloat16
    # a name outside _lib.ACT
    del lin[:]
    pair_transitions(c["x"].to(dev()), [W.to(dev()) for W in c["Ws"]], [b.to(dev()) for b in c["bs"]], "sigmoid")
    assert len(kernel_calls) == 1 and len(lin) == 3


def test_the_fused_path_needs_no_f_linear(monkeypatch):
    from recon_amd import pair_transitions
    c = case((17, 20, 24, 3), "relu")
    monkeypatch.setattr(F, "linear", lambda *a, **k: pytest.fail("F.linear ran"))
    got = run(pair_transitions, c, "relu", dev())
    for a, r in zip(got, c["ref"]):
        assert rel_err(a, r) <= 2e-5


def test_empty_batch():
    from recon_amd import pair_transitions
    x, Ws, bs, _ = inputs(4, 8, 6, 2)
    xe = x[:0].to(dev()).requires_grad_(True)
    Ws = [W.to(dev()).requires_grad_(True) for W in Ws]
    bs = [b.to(dev()).requires_grad_(True) for b in bs]
    Ts = pair_transitions(xe.view(0, 1, 8), Ws, bs, "relu")
    assert len(Ts) == 2 and all(t.shape == (0, 1, 6) and t.is_cuda for t in Ts)
    (Ts[0].sum() + Ts[1].sum()).backward()
    assert xe.grad.shape == (0, 8)
    for t in Ws + bs:
        assert t.grad is not None and torch.count_nonzero(t.grad) == 0


# ------------------------------------------------------------------------------------------------------------- the models
def _through_the_op(fixture, monkeypatch):
    def projections(m):
        lins = [m.representation_to_adj] if m.tied else list(m.representation_to_adj)
        assert lins and all(type(lin) is nn.Linear for lin in lins)
        return lins, "a projection's nn.Linear.forward ran"
    pinned(*fixture, monkeypatch, "fused_transitions", kernels_ran(monkeypatch), projections, ["g.representation_to_adj."])


@pytest.mark.parametrize("name", ["gpgnn1_untied", "gpgnn2_tied_n9"])
def test_gpgnn_fixture_through_the_op(name, monkeypatch):
    _through_the_op(gpgnn_fixture(name), monkeypatch)


def test_recon_eac_fixture_through_the_op(monkeypatch):
    _through_the_op(eac_fixture(), monkeypatch)


def test_recon_eac_kggat_fixture_through_the_op(monkeypatch):
    _through_the_op(kggat_fixture(), monkeypatch)
