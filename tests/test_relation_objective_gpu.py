"""recon_amd.relation_objective (csrc/objective.hip) against the stock lines of train.py:232, :309-324 and test.py:274-291 in fp64 on the
CPU, against the CPU chain for the discrete outputs, and against the fixture written from torch's CrossEntropyLoss and the reference's
evaluate_instance_based.

The grid, the inputs, the fp64 reference and the comparison are those of tests/test_relation_objective_cpu.py, which also guards them: loss,
d_logits and confidence inside `op_checks.bound` of the stock fp32 lines' own error on the GPU; predicted, counts and f1 exactly equal.  The
figures measured on an MI355X are in DESIGN.md section 25."""
import copy

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from op_checks import bound, calls_of, close, dev, entries_declared_and_bound, gpgnn_fixture, peak_bytes, rel_err, rounded, same
from test_relation_objective_cpu import (ABOVE, CASES, CITES, EMPTY, ENTRIES, G_LOSS, IGNORE, REG_WIDTH, case, case_id, check_fixture_batch,
                                         expected, failures, inputs, run, run_stock, stock, stock_grad, tie_case)

pytestmark = pytest.mark.gpu


def counters(monkeypatch):
    from recon_amd import objective
    return calls_of(monkeypatch, objective._Objective, "apply"), calls_of(monkeypatch, objective, "_chain")


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_value_gradient_and_discrete_outputs(c, monkeypatch):
    from recon_amd import _lib, relation_objective
    from recon_amd.objective import _chain
    k = case(*c)
    kernel_calls, chain_calls = counters(monkeypatch)
    fused = run(relation_objective, k, dev())
    if c[0] == ABOVE:
        assert not _lib.lib().recon_relation_objective_supported(*c[0])
        assert (len(kernel_calls), len(chain_calls)) == (0, 1), "a width the library refuses: the chain"
    else:
        assert _lib.lib().recon_relation_objective_supported(*c[0])
        assert (len(kernel_calls), len(chain_calls)) == (1, 0), "the kernels take this shape: the op must not run the chain"
    bad = failures(fused, run_stock(k, dev()), k, case_id(c))
    assert not bad, bad
    cpu_chain = run(_chain, k)                                           # the discrete outputs of the CPU chain on the same inputs
    for a, b in zip(fused[3:], cpu_chain[3:]):
        assert torch.equal(a.cpu(), b)


def test_the_fixtures_epoch_with_one_accumulator(monkeypatch):
    from recon_amd import RelationMetrics, relation_objective
    from recon_amd.objective import micro_prf
    g = load_golden("relation_objective1")
    kernel_calls, chain_calls = counters(monkeypatch)
    metrics = RelationMetrics(dev())
    total = torch.zeros(4, dtype=torch.int64)
    for i in range(int(g["n_batches"])):
        x = torch.from_numpy(g["logits_%d" % i]).to(dev()).requires_grad_(True)
        res = relation_objective(x, torch.from_numpy(g["labels_%d" % i]).to(dev()), metrics=metrics)
        res.loss.backward()
        check_fixture_batch(g, i, res, x.grad, stock_grad(g, i, dev()), micro_prf)
        assert metrics.f1_sum.item() == float(g["f1_sum_%d" % i])        # the bits of the reference's `f1 += add_f1`
        total += torch.from_numpy(g["counts_%d" % i])
    assert (len(kernel_calls), len(chain_calls)) == (6, 0)
    r = metrics.result()
    assert [r.kept, r.n_pred, r.n_gold, r.n_ok] == total.tolist() and r.batches == 6 and r.f1_sum == float(g["f1_sum_5"])
    metrics.reset()
    assert metrics.result() == (0, 0, 0, 0, 0.0, 0)


# ------------------------------------------------------------------------------------------------------------- pinned semantics
def test_every_label_ignored(monkeypatch):
    from recon_amd import relation_objective
    kernel_calls, _ = counters(monkeypatch)
    x, _ = inputs(9, 63)
    x = x.to(dev()).requires_grad_(True)
    res = relation_objective(x, torch.full((9,), IGNORE, dtype=torch.int64, device=dev()))
    res.loss.backward()
    assert len(kernel_calls) == 1
    assert torch.isnan(res.loss).item() and torch.count_nonzero(x.grad) == 0 and res.counts.tolist() == [0, 0, 0, 0] and res.f1.item() == 0.0
    assert torch.equal(res.predicted.cpu(), torch.max(x.detach().cpu(), dim=1)[1])      # ignored rows are predicted too


@pytest.mark.parametrize("shape", [(9, 6), (9, 353), (5, REG_WIDTH + 1)], ids=lambda s: "%dx%d" % s)
def test_an_exact_tie_takes_the_lowest_index(shape, monkeypatch):
    from recon_amd import relation_objective
    kernel_calls, _ = counters(monkeypatch)
    k = tie_case(shape)
    assert torch.equal(k["logits"][:, 2], k["logits"][:, 3]) and (k["exact"][0] == 2).all()
    got = run(relation_objective, k, dev())
    assert len(kernel_calls) == 1
    bad = failures(got, run_stock(k, dev()), k, "tie %dx%d" % shape)
    assert not bad, bad
    zeros = dict(k, logits=torch.zeros(shape))                           # -0 and +0 tie as well
    zeros["logits"][:, 1::2] = -0.0
    assert (run(relation_objective, zeros, dev())[3] == 0).all()


@pytest.mark.parametrize("shape", [(9, 63), (9, 353), (5, REG_WIDTH + 1)], ids=lambda s: "%dx%d" % s)
def test_a_nan_logit_in_a_kept_row(shape, monkeypatch):
    from recon_amd import relation_objective
    kernel_calls, _ = counters(monkeypatch)
    x, lab = inputs(*shape)
    kept = int((lab != IGNORE).nonzero()[0])
    at = shape[1] - 2
    x[kept, at] = float('nan')
    x[kept, 1] = float('nan') if shape[1] > 100 else x[kept, 1]          # two NaNs: the lowest
    first = 1 if shape[1] > 100 else at
    want = stock(x, lab)
    assert torch.isnan(want[0]).item() and want[1][kept] == first
    xd = x.to(dev()).requires_grad_(True)
    res = relation_objective(xd, lab.to(dev()))
    res.loss.backward()
    assert len(kernel_calls) == 1
    assert torch.isnan(res.loss).item() and res.predicted[kept].item() == first and torch.isnan(res.confidence[kept]).item()
    assert torch.equal(res.predicted.cpu(), want[1])
    others = [m for m in range(shape[0]) if m != kept]
    assert torch.isfinite(res.confidence[others]).all() and torch.isfinite(xd.grad[others]).all()
    assert torch.isnan(xd.grad[kept]).all()                              # log_softmax's: the row's gradient is NaN


@pytest.mark.parametrize("label", ["n_out", "far above", "negative"])
def test_a_label_outside_the_classes(label, monkeypatch):
    from recon_amd import relation_objective
    kernel_calls, _ = counters(monkeypatch)
    k = case((72, 353))
    M, n = k["shape"]
    lab = k["labels"].clone()
    row = 5                                                              # not the last row
    lab[row] = {"n_out": n, "far above": 2 ** 40 + 3, "negative": -7}[label]
    x = k["logits"].to(dev()).requires_grad_(True)
    res = relation_objective(x, lab.to(dev()))
    res.loss.backward(torch.tensor(G_LOSS, device=dev()))
    torch.cuda.synchronize()                                             # the process carries on
    assert len(kernel_calls) == 1
    assert torch.isnan(res.loss).item() and torch.count_nonzero(x.grad[row]) == 0
    # the other rows: as if the row were ignored, but counted in kept
    as_ignored = lab.clone()
    as_ignored[row] = IGNORE
    ref = expected(k["logits"], as_ignored)
    kept = int((lab != IGNORE).sum())
    want = ref["ref"][1] * (kept - 1) / kept
    chain = run_stock(dict(k, labels=as_ignored), dev())[1] * (kept - 1) / kept
    e_op, e_chain = rel_err(x.grad, want), rel_err(chain, want)
    print("relation_objective label %s: d_logits op %.3e chain %.3e bound %.3e" % (label, e_op, e_chain, bound(e_chain)))
    assert e_op <= bound(e_chain)
    counts = ref["exact"][1].clone()
    counts[0] += 1
    counts[1] += int(k["exact"][0][row] != EMPTY)                        # its prediction counts like any kept row's
    counts[2] += 1                                                       # it counts as gold and matches nothing
    assert res.counts.tolist() == counts.tolist()
    assert torch.equal(res.predicted.cpu(), k["exact"][0])
    again = relation_objective(x.detach(), k["labels"].to(dev()))         # the next call is unharmed
    assert torch.isfinite(again.loss).item() and again.counts.tolist() == k["exact"][1].tolist()


# ------------------------------------------------------------------------------------------------------------- the frame
FRAME = [((9, 63), "x4"), ((72, 353), "x4"), ((6, REG_WIDTH + 1), "x4"), ((72, 353), "-inf")]


def test_forward_and_backward_are_bitwise_reproducible():
    from recon_amd import relation_objective
    for c in FRAME + [((3600, 353), "x4")]:
        same(run(relation_objective, case(*c), dev()), run(relation_objective, case(*c), dev()))


def test_second_backward_over_a_retained_graph_gives_the_same_bits(monkeypatch):
    from recon_amd import relation_objective
    k = case((72, 353))
    x = k["logits"].to(dev()).requires_grad_(True)
    ce = calls_of(monkeypatch, F, "cross_entropy")
    res = relation_objective(x, k["labels"].to(dev()))
    kept_loss, kept_counts = res.loss.clone(), res.counts.clone()
    g = torch.tensor(G_LOSS, device=dev())
    first = torch.autograd.grad(res.loss, [x], g, retain_graph=True)
    second = torch.autograd.grad(res.loss, [x], g, retain_graph=True)
    same(first, second)
    same([kept_loss, kept_counts], [res.loss, res.counts])               # the backward destroys nothing
    assert not ce
    assert rel_err(first[0], k["ref"][1]) <= 2e-5


def test_a_strided_view_gives_the_contiguous_copys_bits(monkeypatch):
    from recon_amd import _lib, relation_objective
    kernel_calls, _ = counters(monkeypatch)
    strides, real = [], _lib.rows_in_place
    monkeypatch.setattr(_lib, "rows_in_place", lambda *a, **k: (lambda r: strides.append(r[1]) or r)(real(*a, **k)))
    for c in FRAME:
        k = case(*c)
        M, n = k["shape"]
        wide = torch.full((M, n + 7), 99.0, device=dev())
        wide[:, 3:3 + n] = k["logits"].to(dev())
        wide.requires_grad_(True)
        view = wide[:, 3:3 + n]
        assert not view.is_contiguous()
        del strides[:]
        res = relation_objective(view, k["labels"].to(dev()))
        res.loss.backward(torch.tensor(G_LOSS, device=dev()))
        assert strides == [n + 7, n + 7]                                 # read in place, forward and backward
        plain = run(relation_objective, k, dev())
        same([res.loss.detach(), wide.grad[:, 3:3 + n].contiguous(), res.confidence, res.predicted, res.counts, res.f1], plain)
        assert torch.count_nonzero(wide.grad[:, :3]) == 0 and torch.count_nonzero(wide.grad[:, 3 + n:]) == 0
    assert len(kernel_calls) == 2 * len(FRAME)


def test_no_grad_gives_the_training_forwards_bits_and_memory_is_outputs_and_workspace(monkeypatch):
    from recon_amd import _lib, relation_objective
    M, n = 3600, 353
    k = case((M, n))
    x, lab = k["logits"].to(dev()).requires_grad_(True), k["labels"].to(dev())
    asked, real = [], _lib.workspace
    monkeypatch.setattr(_lib, "workspace", lambda nbytes, device: asked.append(nbytes) or real(nbytes, device))
    trained = relation_objective(x, lab)
    with torch.no_grad():
        plain = relation_objective(x, lab)
    ws = _lib.lib().recon_relation_objective_workspace_bytes(M, n)
    assert asked == [ws, ws] and ws == M * 4                             # the M row terms
    assert trained.loss.grad_fn is not None and plain.loss.grad_fn is None
    same([t.detach() for t in trained], list(plain))
    del trained, plain

    def forward():
        with torch.no_grad():
            return relation_objective(x, lab)
    outputs = rounded(4) + rounded(M * 8) + rounded(M * 4) + rounded(32) + rounded(8)      # loss, predicted, confidence, counts, f1
    unwritten = M * n * 4                                                # the log-softmax the stock lines write
    peak, out = peak_bytes(forward)
    print("relation_objective memory: no_grad peak %d bytes, outputs %d, workspace %d, the [M, n_out] tensor %d" % (peak, outputs, ws, unwritten))
    assert peak == outputs + rounded(ws) and peak < unwritten
    del out
    peak, out = peak_bytes(lambda: relation_objective(x, lab))
    print("relation_objective memory: training forward peak %d bytes" % peak)
    assert out.loss.grad_fn is not None and peak == outputs + rounded(ws) + rounded(M * 4)           # and the rows' log-sum-exp
    peak_stock, _ = peak_bytes(lambda: stock(x, lab))
    assert peak_stock >= unwritten > peak


def test_the_test_time_form(monkeypatch):
    from recon_amd import _lib, relation_objective
    kernel_calls, chain_calls = counters(monkeypatch)
    asked, real = [], _lib.workspace
    monkeypatch.setattr(_lib, "workspace", lambda nbytes, device: asked.append(nbytes) or real(nbytes, device))
    for c in FRAME:
        k = case(*c)
        x = k["logits"].to(dev()).requires_grad_(True)
        res = relation_objective(x)
        assert res.loss is None and res.counts is None and res.f1 is None and not res.predicted.requires_grad and not res.confidence.requires_grad
        full = relation_objective(x, k["labels"].to(dev()))
        same([res.predicted, res.confidence], [full.predicted, full.confidence.detach()])
        assert torch.equal(res.predicted.cpu(), k["exact"][0]) and rel_err(res.confidence, k["ref"][2]) <= 2e-5
    assert len(kernel_calls) == 2 * len(FRAME) and not chain_calls and len(asked) == len(FRAME)       # no workspace without labels


def test_create_graph_bf16_and_cpu_inputs_run_the_chain(monkeypatch):
    from recon_amd import relation_objective
    kernel_calls, chain_calls = counters(monkeypatch)
    ce = calls_of(monkeypatch, F, "cross_entropy")
    k = case((9, 63))
    x, lab = k["logits"].to(dev()).requires_grad_(True), k["labels"].to(dev())
    res = relation_objective(x, lab)
    assert (len(kernel_calls), len(chain_calls), len(ce)) == (1, 0, 0)
    grad, = torch.autograd.grad(res.loss, [x], torch.tensor(G_LOSS, device=dev()), create_graph=True)
    assert len(ce) == 1                                                  # the backward recomputed through the stock line
    assert rel_err(grad, k["ref"][1]) <= 2e-5 and grad.requires_grad
    grad.square().sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    res = relation_objective(x.detach().bfloat16(), lab)
    assert (len(kernel_calls), len(chain_calls)) == (1, 1) and res.loss.dtype == torch.float32 and res.confidence.dtype == torch.float32
    assert res.counts.is_cuda and res.f1.dtype == torch.float64
    res = relation_objective(k["logits"], k["labels"])
    assert (len(kernel_calls), len(chain_calls)) == (1, 2) and not res.loss.is_cuda


def test_empty_batch(monkeypatch):
    from recon_amd import RelationMetrics, relation_objective
    kernel_calls, chain_calls = counters(monkeypatch)
    metrics = RelationMetrics(dev())
    x = torch.zeros(0, 353, device=dev(), requires_grad=True)
    res = relation_objective(x, torch.zeros(0, dtype=torch.int64, device=dev()), metrics=metrics)
    assert not kernel_calls and not chain_calls                          # no launch of the kernels
    assert torch.isnan(res.loss).item() and res.loss.is_cuda and res.predicted.shape == (0,) and res.confidence.shape == (0,)
    assert res.counts.tolist() == [0, 0, 0, 0] and res.f1.item() == 0.0 and metrics.result() == (0, 0, 0, 0, 0.0, 1)
    res.loss.backward()
    assert x.grad.shape == (0, 353)


def test_workspace_bytes_are_the_librarys(monkeypatch):
    from recon_amd import _lib, relation_objective
    asked, real = [], _lib.workspace
    monkeypatch.setattr(_lib, "workspace", lambda nbytes, device: asked.append(nbytes) or real(nbytes, device))
    for shape in ((1, 2), (5, 65), (257, 353)):
        k = case(shape)
        del asked[:]
        run(relation_objective, k, dev())
        assert asked == [_lib.lib().recon_relation_objective_workspace_bytes(*shape)] and asked[0] == -(-shape[0] * 4 // 16) * 16


# ------------------------------------------------------------------------------------------------------------- end to end
def test_a_gpgnn_training_step_matches_the_stock_objective(monkeypatch):
    from recon_amd import relation_objective
    from recon_amd.optim import Adam
    kernel_calls, chain_calls = counters(monkeypatch)
    m, g, out_of, name = gpgnn_fixture("gpgnn1_untied")
    m.train().to(dev())
    twin = copy.deepcopy(m)
    rows = out_of(m).shape[0]
    gen = torch.Generator().manual_seed(3)
    lab = torch.randint(0, 3, (rows,), generator=gen).to(dev())
    assert (lab == IGNORE).any() and (lab != IGNORE).any()
    steps = []
    for model, objective in ((m, lambda o: relation_objective(o, lab).loss), (twin, lambda o: F.cross_entropy(o, lab, ignore_index=IGNORE))):
        opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3, max_grad_norm=0.25)
        opt.zero_grad()
        loss = objective(out_of(model))
        loss.backward()
        opt.step()
        steps.append(loss.detach())
    assert (len(kernel_calls), len(chain_calls)) == (1, 0)
    close(steps[0], steps[1], what=name + " loss")
    moved = 0
    before = dict(gpgnn_fixture("gpgnn1_untied")[0].named_parameters())
    for (k, a), (_, b) in zip(m.named_parameters(), twin.named_parameters()):
        close(a, b, what="%s parameter %s after the step" % (name, k))
        moved += not torch.equal(a.detach().cpu(), before[k].detach())
    assert moved > 0


def test_the_four_entries_are_declared_bound_and_cite_the_reference():
    for cite in CITES:
        entries_declared_and_bound(ENTRIES, cite)
