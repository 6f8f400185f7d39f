"""recon_amd.relation_objective without a GPU: the import, CPU tensors through the public function against the fixture written from torch's
CrossEntropyLoss and the reference's evaluate_instance_based (tests/golden/gen_golden_relation_objective.py), the counters' closed form
against a plain loop, every argument error, the empty batch, the test-time form, the queries and status codes of the C ABI, the header /
`_lib.SYMBOLS` check of the four entries, and the guard of the checks tests/test_relation_objective_gpu.py holds the kernels to.

The grid, the input generator, the fp64 reference and the comparison live here and are imported by the GPU file.  A shape is (M, n_out).
Inputs: logits ~ 4 N(0, 1) from a torch.Generator whose seed is mixed with the shape; one cell of every row, the label's in half of the
rows and the largest in the others, is set 0.5 above the row's maximum, so that some predictions are right and no row has a near-tie
(asserted: the gap between the two largest cells of every row is above 1e-3 of the row's range; no row is left out); the kind "1e4" scales them by 1e4 / 4 (overflow without the maximum's subtraction), the kind "-inf" puts -inf into three cells of
every fourth row, away from the row's label and its maximum.  Labels: about 70 % ignore_index = 0, about 20 % empty_label = 1, the rest
uniform over the other classes (n_out = 2 has none: empty_label).  The incoming gradient of the loss is 0.75.

Comparison (`failures`): loss, d_logits and confidence inside `op_checks.bound` of the stock fp32 lines' own error against fp64
(`op_checks.band_failures`); predicted, counts and f1 exactly equal to the expected ones.

Guard: a float32 restatement of the op's definition, written without the stock lines, passes at every shape and kind, and five wrong
restatements fail: no subtraction of the maximum (at the kind "1e4"); the mean over all rows; the gradient of ignored rows not zeroed;
the highest index at an exact tie (on a copied column); recall's denominator counted over the predictions."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from op_checks import band_failures, bound, entries_declared_and_bound, rel_err

IGNORE, EMPTY = 0, 1
G_LOSS = 0.75
REG_WIDTH, MAX_WIDTH = 512, 8192                # csrc/objective.hip: a row up to 512 wide sits in registers, up to 8192 is walked twice
ISSUE_GRID = [(1, 2), (3, 3), (4, 64), (5, 65), (9, 63), (72, 353), (257, 353), (3600, 353)]
# where the kernels take another path: 1, 2, 4, 6, 8 registers per lane (64, 128, 256, 384, 512 columns), the two walks above, the limit
PATHS = [(5, 128), (5, 129), (6, 256), (5, 257), (5, 384), (7, 385), (6, REG_WIDTH), (6, REG_WIDTH + 1), (3, MAX_WIDTH)]
GRID = ISSUE_GRID + PATHS
ABOVE = (3, MAX_WIDTH + 1)                      # the library refuses it: the chain
KINDS = {"1e4": [(72, 353), (5, 65), (6, REG_WIDTH + 1)], "-inf": [(72, 353), (9, 63), (6, REG_WIDTH + 1)]}
CASES = [(s, "x4") for s in GRID + [ABOVE]] + [(s, k) for k, ss in KINDS.items() for s in ss]
BAND_NAMES = ("loss", "d_logits", "confidence")
EXACT_NAMES = ("predicted", "counts", "f1")
CITES = ("train.py:232", "train.py:309-324", "test.py:274-291", "utils/evaluation_utils.py:17-59")
ENTRIES = ["recon_relation_objective_supported", "recon_relation_objective_workspace_bytes", "recon_relation_objective_fwd",
           "recon_relation_objective_bwd"]
MIN_GAP = 1e-3


def case_id(c):
    return "%dx%d-%s" % (c[0][0], c[0][1], c[1])


def labels_for(g, M, n):
    u = torch.rand(M, generator=g)
    other = torch.randint(2, n, (M,), generator=g) if n > 2 else torch.full((M,), EMPTY)
    lab = torch.where(u < 0.7, torch.full((M,), IGNORE), torch.where(u < 0.9, torch.full((M,), EMPTY), other)).to(torch.int64)
    if M >= 3:                                                           # every class of label occurs
        lab[0], lab[1], lab[2] = n - 1, EMPTY, IGNORE
    else:
        lab[0] = n - 1
    return lab


def inputs(M, n, kind="x4", seed=0):
    """logits fp32 [M, n] and labels int64 [M] on the CPU."""
    g = torch.Generator().manual_seed(100003 * seed + 7919 * M + 131 * n)
    x = torch.randn(M, n, generator=g) * 4
    lab = labels_for(g, M, n)
    top = torch.where(torch.rand(M, generator=g) < 0.5, lab, x.argmax(1))      # half of the rows predict their label
    x[torch.arange(M), top] = x.max(1).values + 0.5
    if kind == "1e4":
        x = x * 2500.0
    if kind == "-inf":
        for m in range(0, M, 4):
            free = [c for c in range(n) if c != top[m] and c != lab[m]]
            for c in free[m % 3::max(1, len(free) // 3)][:3]:
                x[m, c] = -float('inf')
    return x, lab


def stock(logits, labels, ignore_index=IGNORE, empty_label=EMPTY):
    """train.py:232, :309-324 and test.py:285 as a caller writes them with stock ops; any floating dtype.  [loss, predicted, confidence]."""
    loss = F.cross_entropy(logits, labels, ignore_index=ignore_index)
    predicted = torch.max(logits, dim=1)[1]
    confidence = F.softmax(logits, dim=-1).gather(1, predicted.unsqueeze(1)).squeeze(1)
    return loss, predicted, confidence


def plain_counts(predicted, labels, ignore_index=IGNORE, empty_label=EMPTY):
    """(counts, prec, rec, f1) by a loop over the rows, from the description: among the rows whose label is not ignore_index, a precision
    counts the rows whose first list is not empty and, of those, the ones where both lists agree; recall is the same with the lists
    swapped; F1 is 0 unless their sum is positive."""
    kept = [(p, l) for p, l in zip(predicted, labels) if l != ignore_index]

    def share(first, second):
        count = hits = 0
        for a, b in zip(first, second):
            if a != empty_label:
                count += 1
                hits += a == b
        return (float(hits) / count if count > 0 else 0), count, hits
    prec, n_pred, ok_p = share([p for p, _ in kept], [l for _, l in kept])
    rec, n_gold, ok_r = share([l for _, l in kept], [p for p, _ in kept])
    assert ok_p == ok_r
    f1 = 2.0 * prec * rec / (prec + rec) if prec + rec > 0 else 0
    return [len(kept), n_pred, n_gold, ok_p], prec, rec, f1


_CASES = {}


def case(shape, kind="x4"):
    """Inputs and what they must give: the fp64 loss, d_logits and confidence of `stock`, and predicted, counts, f1 of the fp32 logits
    (torch.max and the plain loop).  Computed once and left unchanged."""
    key = (shape, kind)
    if key not in _CASES:
        x, lab = inputs(*shape, kind)
        _CASES[key] = dict(shape=shape, kind=kind, logits=x, labels=lab, **expected(x, lab))
    return _CASES[key]


def expected(x, lab, ignore_index=IGNORE, empty_label=EMPTY):
    xd = x.double().requires_grad_(True)
    loss, _, conf = stock(xd, lab, ignore_index, empty_label)
    loss.backward(torch.tensor(G_LOSS, dtype=torch.float64))
    predicted = torch.max(x, dim=1)[1]
    counts, _, _, f1 = plain_counts(predicted.tolist(), lab.tolist(), ignore_index, empty_label)
    return dict(ref=[loss.detach(), xd.grad, conf.detach()], exact=[predicted, torch.tensor(counts), torch.tensor(float(f1), dtype=torch.float64)])


def run(fn, c, device="cpu", logits_of=None, **kw):
    """[loss, d_logits, confidence, predicted, counts, f1] of fn(logits, labels) on `device` with the incoming gradient G_LOSS."""
    x = c["logits"].clone().to(device)
    x = (x if logits_of is None else logits_of(x)).requires_grad_(True)
    res = fn(x, c["labels"].to(device), **kw)
    res.loss.backward(torch.tensor(G_LOSS, device=device))
    return [res.loss.detach(), x.grad, res.confidence, res.predicted, res.counts, res.f1]


def run_stock(c, device="cpu"):
    """The band's yardstick: [loss, d_logits, confidence] of the stock fp32 lines."""
    x = c["logits"].clone().to(device).requires_grad_(True)
    loss, _, conf = stock(x, c["labels"].to(device))
    loss.backward(torch.tensor(G_LOSS, device=device))
    return [loss.detach(), x.grad, conf.detach()]


def failures(got, chain, c, label=""):
    """What of `got` misses: loss, d_logits, confidence outside the band of `chain`'s own error; predicted, counts, f1 not exactly equal."""
    bad = band_failures(BAND_NAMES, got[:3], chain[:3], c["ref"], "relation_objective " + label)
    for what, a, b in zip(EXACT_NAMES, got[3:], c["exact"]):
        a = a.detach().cpu()
        if a.dtype != b.dtype or a.shape != b.shape or not torch.equal(a, b):
            bad.append((what, a, b))
    return bad


def definition(x, lab, wrong=None, ignore_index=IGNORE, empty_label=EMPTY):
    """[loss, d_logits, confidence, predicted, counts, f1] by the op's definition in the logits' dtype, independent of `stock`."""
    M, n = x.shape
    mx = x.max(1).values
    shift = torch.zeros_like(mx) if wrong == "no subtraction of the maximum" else mx
    e = torch.exp(x - shift.unsqueeze(1))
    s = e.sum(1)
    lse = shift + torch.log(s)
    kept = lab != ignore_index
    inside = (lab >= 0) & (lab < n)
    onehot = (torch.arange(n).unsqueeze(0) == lab.unsqueeze(1)).to(x.dtype)
    term = torch.where(inside, lse - x.gather(1, lab.clamp(0, n - 1).unsqueeze(1)).squeeze(1), torch.full_like(lse, float('nan')))
    denom = torch.tensor(float(M if wrong == "the mean over all rows" else kept.sum().item()), dtype=x.dtype)
    loss = torch.where(kept, term, torch.zeros_like(term)).sum() / denom
    d = G_LOSS * (torch.exp(x - lse.unsqueeze(1)) - onehot) / denom
    if wrong != "the gradient of ignored rows not zeroed":
        d = torch.where((kept & inside).unsqueeze(1), d, torch.zeros_like(d))
    if kept.sum() == 0:
        d = torch.zeros_like(d)
    at = torch.arange(n).unsqueeze(0).expand(M, n)
    is_max = x == mx.unsqueeze(1)
    if wrong == "the highest index at a tie":
        predicted = torch.where(is_max, at, torch.full_like(at, -1)).max(1).values
    else:
        predicted = torch.where(is_max, at, torch.full_like(at, n)).min(1).values
    pred, gold = kept & (predicted != empty_label), kept & (lab != empty_label)
    counts = torch.stack([kept.sum(), pred.sum(), gold.sum(), (gold & (predicted == lab)).sum()])
    k, n_pred, n_gold, n_ok = (float(v) for v in counts.tolist())
    if wrong == "recall over the predictions":
        n_gold = n_pred
    prec, rec = (n_ok / n_pred if n_pred > 0 else 0.0), (n_ok / n_gold if n_gold > 0 else 0.0)
    f1 = 2.0 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    return [loss, d, e.gather(1, predicted.unsqueeze(1)).squeeze(1) / s, predicted, counts, torch.tensor(f1, dtype=torch.float64)]


def tie_case(shape=(9, 6)):
    """A copied column that wins every row: an exact tie between columns 2 and 3, with gold labels on either."""
    x, lab = inputs(*shape)
    x[:, 2] = x.max(1).values + 1
    x[:, 3] = x[:, 2]
    lab[:4] = torch.tensor([2, 3, 3, 2])
    return dict(shape=shape, kind="tie", logits=x, labels=lab, **expected(x, lab))


# ------------------------------------------------------------------------------------------------------------- the inputs
def test_import():
    from recon_amd import RelationMetrics, relation_objective
    from recon_amd.objective import RelationMetrics as same_class, relation_objective as same
    assert relation_objective is same and RelationMetrics is same_class


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_no_row_has_a_near_tie_and_every_kind_of_label_occurs(c):
    shape, kind = c
    k = case(shape, kind)
    x, lab = k["logits"], k["labels"]
    finite = torch.where(torch.isfinite(x), x, torch.full_like(x, float('nan')))
    lo = torch.where(torch.isnan(finite), torch.full_like(x, float('inf')), finite).min(1).values
    top = x.topk(2, dim=1).values
    gap, span = top[:, 0] - top[:, 1], top[:, 0] - lo
    assert (gap > MIN_GAP * span).all(), (gap / span).min()               # every row: none is left out
    assert torch.isfinite(top[:, 0]).all()
    M, n = shape
    assert (lab == IGNORE).any() or M < 3
    assert (lab == EMPTY).any() or M < 3
    assert (lab == n - 1).any() and lab.min() >= 0 and lab.max() < n
    if M >= 72:
        share = [(lab == IGNORE).float().mean().item(), (lab == EMPTY).float().mean().item()]
        assert 0.6 < share[0] < 0.8 and 0.12 < share[1] < 0.28, share
    if kind == "-inf":
        assert torch.isinf(x).any() and torch.isfinite(k["ref"][0]) and torch.isfinite(k["ref"][1]).all()
        assert not torch.isinf(x[torch.arange(M), lab]).any()
    if kind == "1e4":
        assert x.abs().max() > 1e4 and torch.isfinite(k["ref"][0])


def test_the_seed_is_mixed_with_the_shape():
    assert not torch.equal(inputs(5, 65)[0][:, :64], inputs(5, 64)[0])
    assert torch.equal(inputs(5, 65)[0], inputs(5, 65)[0])


# ------------------------------------------------------------------------------------------------------------- the op on the CPU
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_cpu_tensors_run_the_chain(c, monkeypatch):
    from recon_amd import objective, relation_objective
    from op_checks import calls_of
    k = case(*c)
    chain_calls, kernel_calls = calls_of(monkeypatch, objective, "_chain"), calls_of(monkeypatch, objective._Objective, "apply")
    got = run(relation_objective, k)
    assert len(chain_calls) == 1 and not kernel_calls
    assert got[0].dtype == torch.float32 and got[3].dtype == torch.int64 and got[4].dtype == torch.int64 and got[5].dtype == torch.float64
    assert got[0].dim() == 0 and got[5].dim() == 0 and got[4].shape == (4,) and got[2].dtype == torch.float32
    bad = failures(got, run_stock(k), k, case_id(c))
    assert not bad, bad


def test_the_fixtures_epoch_on_the_cpu():
    from recon_amd import RelationMetrics, relation_objective
    from recon_amd.objective import micro_prf
    g = load_golden("relation_objective1")
    assert int(g["ignore_index"]) == IGNORE and int(g["empty_label"]) == EMPTY
    metrics = RelationMetrics(torch.device("cpu"))
    total = np.zeros(4, dtype=np.int64)
    for i in range(int(g["n_batches"])):
        x = torch.from_numpy(g["logits_%d" % i]).requires_grad_(True)
        lab = torch.from_numpy(g["labels_%d" % i])
        res = relation_objective(x, lab, ignore_index=IGNORE, empty_label=EMPTY, metrics=metrics)
        res.loss.backward()
        check_fixture_batch(g, i, res, x.grad, stock_grad(g, i, "cpu"), micro_prf)
        assert metrics.f1_sum.item() == float(g["f1_sum_%d" % i])        # the bits of the reference's `f1 += add_f1`
        total += g["counts_%d" % i]
    r = metrics.result()
    assert [r.kept, r.n_pred, r.n_gold, r.n_ok] == total.tolist() and r.batches == 6 and r.f1_sum == float(g["f1_sum_5"])
    assert float(g["f1_4"]) == 0.39999999999999997                       # a batch whose F1 depends on the order of the arithmetic
    metrics.reset()
    assert metrics.result() == (0, 0, 0, 0, 0.0, 0)


def stock_grad(g, i, device):
    """[loss, d_logits] of the stock fp32 line on batch i of the fixture: the band's yardstick."""
    x = torch.from_numpy(g["logits_%d" % i]).to(device).requires_grad_(True)
    loss = F.cross_entropy(x, torch.from_numpy(g["labels_%d" % i]).to(device), ignore_index=IGNORE)
    loss.backward()
    return [loss.detach(), x.grad]


def check_fixture_batch(g, i, res, grad, chain, micro_prf):
    """Batch i of the fixture: every recorded double exactly, predicted and counts exactly, loss, gradient and confidence in the band."""
    assert torch.equal(res.predicted.cpu(), torch.from_numpy(g["predicted_%d" % i]))
    assert res.counts.cpu().tolist() == g["counts_%d" % i].tolist()
    prec, rec, f1 = (v.item() for v in micro_prf(res.counts))
    assert (prec, rec, f1) == (float(g["prec_%d" % i]), float(g["rec_%d" % i]), float(g["f1_%d" % i]))
    assert res.f1.dtype == torch.float64 and res.f1.item() == float(g["f1_%d" % i])
    ref_grad = torch.from_numpy(g["d_logits_%d" % i])
    if g["counts_%d" % i][0] == 0:                                        # every label ignored: NaN, a zero gradient
        assert math.isnan(float(g["loss_%d" % i])) and torch.isnan(res.loss).item() and torch.count_nonzero(grad) == 0
        assert torch.count_nonzero(ref_grad) == 0 and res.f1.item() == 0.0
        assert rel_err(res.confidence, torch.from_numpy(g["confidence_%d" % i])) <= bound(2.0 ** -24)
        return
    ref = [torch.tensor(float(g["loss_%d" % i]), dtype=torch.float64), ref_grad]
    bad = band_failures(BAND_NAMES[:2], [res.loss, grad], chain, ref, "relation_objective fixture batch %d" % i)
    assert not bad, bad
    assert rel_err(res.confidence, torch.from_numpy(g["confidence_%d" % i])) <= bound(2.0 ** -24)


def random_batch(seed):
    g = torch.Generator().manual_seed(seed)
    n = int(torch.randint(2, 7, (1,), generator=g))
    M = int(torch.randint(1, 41, (1,), generator=g))
    lab = torch.randint(0, n, (M,), generator=g)
    if M >= 2:                                                           # both special labels occur (one row cannot hold both)
        where = torch.randperm(M, generator=g)[:2]
        lab[where[0]], lab[where[1]] = IGNORE, EMPTY
    x = torch.randn(M, n, generator=g)
    if seed % 10 == 3:                                                   # nothing predicted non-empty
        x[:, EMPTY] += 9
    return x, lab


def test_the_counters_closed_form_against_a_plain_loop():
    from recon_amd import relation_objective
    from recon_amd.objective import micro_prf
    seen = set()
    for seed in range(200):
        x, lab = random_batch(seed)
        res = relation_objective(x, lab)
        counts, prec, rec, f1 = plain_counts(res.predicted.tolist(), lab.tolist())
        assert res.counts.tolist() == counts, seed
        assert tuple(v.item() for v in micro_prf(res.counts)) == (prec, rec, f1) and res.f1.item() == f1, seed
        seen.add((counts[1] > 0, counts[2] > 0, counts[3] > 0))
    assert {(True, True, True), (True, True, False), (False, True, False), (True, False, False)} <= seen, seen


def test_other_ignore_and_empty_labels():
    from recon_amd import relation_objective
    x, lab = random_batch(7)
    res = relation_objective(x, lab, ignore_index=-100, empty_label=2)
    counts, _, _, f1 = plain_counts(res.predicted.tolist(), lab.tolist(), -100, 2)
    assert res.counts.tolist() == counts and counts[0] == len(lab) and res.f1.item() == f1
    assert torch.equal(res.loss, F.cross_entropy(x, lab))


def test_labels_of_any_shape_and_the_test_time_form():
    from recon_amd import relation_objective
    x, lab = inputs(72, 5)
    a, b = relation_objective(x, lab), relation_objective(x, lab.view(8, 9))
    assert torch.equal(a.loss, b.loss) and torch.equal(a.counts, b.counts)
    res = relation_objective(x)
    assert res.loss is None and res.counts is None and res.f1 is None
    assert torch.equal(res.predicted, a.predicted) and torch.equal(res.confidence, a.confidence)
    want = F.softmax(x, dim=-1).max(1).values
    assert torch.allclose(res.confidence, want, rtol=1e-6, atol=0)


def test_empty_batch():
    from recon_amd import RelationMetrics, relation_objective
    metrics = RelationMetrics(torch.device("cpu"))
    x = torch.zeros(0, 5, requires_grad=True)
    res = relation_objective(x, torch.zeros(0, dtype=torch.int64), metrics=metrics)
    assert torch.isnan(res.loss) and res.loss.dtype == torch.float32 and res.predicted.shape == (0,) and res.confidence.shape == (0,)
    assert res.counts.tolist() == [0, 0, 0, 0] and res.f1.item() == 0.0 and metrics.result() == (0, 0, 0, 0, 0.0, 1)
    res.loss.backward()
    assert x.grad.shape == (0, 5)
    res = relation_objective(x)
    assert res.loss is None and res.predicted.shape == (0,)


def test_argument_errors():
    from recon_amd import RelationMetrics, relation_objective
    x, lab = inputs(9, 5)
    m = RelationMetrics(torch.device("cpu"))
    bad = [lambda: relation_objective(x[0], lab),                          # not [M, n_out]
           lambda: relation_objective(x.view(3, 3, 5), lab),
           lambda: relation_objective(x.long(), lab),
           lambda: relation_objective(x[:, :0], lab),
           lambda: relation_objective(x, lab[:8]),                         # not M labels
           lambda: relation_objective(x, lab.int()),
           lambda: relation_objective(x, lab.float()),
           lambda: relation_objective(x.numpy(), lab),
           lambda: relation_objective(x, lab.tolist()),
           lambda: relation_objective(x, lab, ignore_index=0.5),
           lambda: relation_objective(x, lab, empty_label=None),
           lambda: relation_objective(x, lab, metrics=[0, 0]),
           lambda: relation_objective(x, None, metrics=m)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError, match="relation_objective"):
            f()
            pytest.fail("case %d raised nothing" % i)
    with pytest.raises(ValueError, match=r"M = 9.*\(9, 5\).*\(8,\)"):      # the shapes are in the text
        relation_objective(x, lab[:8])
    with pytest.raises(ValueError, match=r"\[M, n_out\].*\(3, 3, 5\).*\(9,\)"):
        relation_objective(x.view(3, 3, 5), lab)


# ------------------------------------------------------------------------------------------------------------- the library's queries
def test_shape_and_workspace_queries():
    from recon_amd import _lib
    L = _lib.lib()
    ok, ws = L.recon_relation_objective_supported, L.recon_relation_objective_workspace_bytes
    assert all(ok(*s) for s in GRID) and not ok(*ABOVE)
    assert ok(0, 353) and ok(3600, 353) and ok(2 ** 30, 1) and ok(1, MAX_WIDTH)
    assert not ok(-1, 353) and not ok(5, 0) and not ok(2 ** 30 + 1, 353) and not ok(5, MAX_WIDTH + 1)
    for M in (1, 3, 4, 5, 360, 3600, 3601):
        assert ws(M, 353) == -(-M * 4 // 16) * 16
    assert ws(0, 353) == 0 and ws(*ABOVE) == 0


def test_status_codes_before_any_launch():
    from recon_amd import _lib
    L = _lib.lib()
    fake = 16                                                            # never dereferenced: every call returns before a launch
    fwd = lambda M, n, ld, nbytes=1 << 20, loss=fake, lse=None, labels=fake, acc=(None, None, None): L.recon_relation_objective_fwd(
        fake, ld, labels, M, n, 0, 1, loss, fake, fake, lse, loss, loss, acc[0], acc[1], acc[2], fake, nbytes, None)
    assert fwd(0, 5, 5) == 0 and fwd(-1, 5, 5) == -1 and fwd(3, 0, 5) == -1 and fwd(3, MAX_WIDTH + 1, MAX_WIDTH + 1) == -2
    assert fwd(3, 5, 4) == -1                                             # a row stride below n_out
    assert fwd(3, 5, 5, nbytes=8) == -4
    assert fwd(3, 5, 5, loss=None) == -1                                  # labels without the outputs they imply
    assert fwd(3, 5, 5, acc=(fake, None, None)) == -1                     # a part of the accumulator
    assert fwd(3, 5, 5, labels=None) == -1 and fwd(3, 5, 5, labels=None, loss=None, lse=fake) == -1      # outputs without labels
    bwd = lambda M, n, ld, g=fake: L.recon_relation_objective_bwd(fake, ld, fake, fake, g, fake, M, n, 0, fake, None)
    assert bwd(0, 5, 5) == 0 and bwd(-1, 5, 5) == -1 and bwd(3, MAX_WIDTH + 1, MAX_WIDTH + 1) == -2 and bwd(3, 5, 4) == -1
    assert bwd(3, 5, 5, g=None) == -1


def test_the_four_entries_are_declared_bound_and_cite_the_reference():
    for cite in CITES:
        entries_declared_and_bound(ENTRIES, cite)


# ------------------------------------------------------------------------------------------------------------- the guard
WRONG = {"no subtraction of the maximum": lambda c: c["kind"] == "1e4",
         "the mean over all rows": lambda c: c["kind"] != "tie" and (c["labels"] == IGNORE).any(),
         "the gradient of ignored rows not zeroed": lambda c: c["kind"] != "tie" and (c["labels"] == IGNORE).any(),
         "the highest index at a tie": lambda c: c["kind"] == "tie",
         "recall over the predictions": lambda c: c["exact"][1][1] != c["exact"][1][2] and c["exact"][1][3] > 0}
MISSES = {"no subtraction of the maximum": {"loss", "d_logits", "confidence"}, "the mean over all rows": {"loss", "d_logits"},
          "the gradient of ignored rows not zeroed": {"d_logits"}, "the highest index at a tie": {"predicted"},
          "recall over the predictions": {"f1"}}
GUARD_CASES = CASES


def _guard(c, label):
    good = definition(c["logits"], c["labels"])
    yard = run_stock(c)
    assert not failures(good, yard, c, label + " stand-in")
    applied = []
    for wrong, applies in WRONG.items():
        if applies(c):
            bad = failures(definition(c["logits"], c["labels"], wrong), yard, c, "%s %s" % (label, wrong))
            assert MISSES[wrong] & {b[0] for b in bad}, "%s passes at %s" % (wrong, label)
            applied.append(wrong)
    return applied


@pytest.mark.parametrize("c", GUARD_CASES, ids=case_id)
def test_fp32_restatement_passes_and_wrong_ones_fail(c):
    _guard(case(*c), case_id(c))


def test_every_wrong_restatement_applies_somewhere():
    applied = [w for c in GUARD_CASES for w, applies in WRONG.items() if applies(case(*c))]
    applied += _guard(tie_case(), "9x6-tie")
    for wrong in WRONG:
        assert applied.count(wrong) >= (1 if wrong == "the highest index at a tie" else 3), wrong
