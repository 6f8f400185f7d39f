"""Training of the ConvKB scorer on the device (csrc/kg_train.hip through recon_amd.kg_train): the filtered corruption against the
reference's batches, at FB15k-237 size, in distribution and at saturation; the forward / loss / backward against the reference's training
step, fp64 bands, torch autograd and a short training run; determinism and argument rejection."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = 2.0 ** -24


def _model(n_ent, n_rel, D, seed):
    from recon_amd.models import SpKBGATConvOnly
    torch.manual_seed(seed)
    m = SpKBGATConvOnly(torch.randn(n_ent, 4), torch.randn(n_rel, 4), [D, D], [D, D], 0.0, 0.0, 0.2, 0.2, [1, 1], 50).to(DEV)
    m.final_entity_embeddings.requires_grad_(False)
    m.final_relation_embeddings.requires_grad_(False)
    return m


def _synthetic_kg(n_ent, n_rel, n_known, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = n_known + n_known // 50 + 10
    tri = torch.stack([torch.randint(0, n_ent, (n,), generator=g), torch.randint(0, n_rel, (n,), generator=g),
                       torch.randint(0, n_ent, (n,), generator=g)], 1)
    tri = torch.unique(tri, dim=0)
    return tri[torch.randperm(tri.shape[0], generator=g)[:n_known]].to(DEV)


def _signature(idx, B):
    base = torch.arange(idx.shape[0], device=idx.device)
    base = torch.where(base < B, base, (base - B) % B)
    diff = idx != idx[:B][base]
    col = torch.where(diff.any(1), diff.int().argmax(1), torch.full_like(base, -1))
    return base, col, diff.sum(1)


@pytest.mark.parametrize("case", ["r4", "r3", "short"])
def test_corruption_layout_matches_reference(case):
    from recon_amd import kg_train
    g = load_golden("convkb_train1")
    known = torch.from_numpy(np.concatenate([g["train"], g["valid"], g["test"]])).to(DEV)
    filt = kg_train.TripleFilter(known, int(g["n_ent"]), int(g["n_rel"]))
    train = torch.from_numpy(g["train"][:int(g[case + "_n_train"])]).to(DEV).int()
    ones = torch.ones(train.shape[0], 1, device=DEV)
    for seed in range(3):
        idx, val = kg_train.iteration_batch(train, ones, int(g[case + "_iter"]), int(g["batch_size"]), filt, int(g[case + "_ratio"]),
                                            generator=torch.Generator().manual_seed(seed))
        B = g[case + "_positives"].shape[0]
        assert torch.equal(idx[:B].cpu(), torch.from_numpy(g[case + "_positives"]))
        base, col, ndiff = _signature(idx, B)
        assert (ndiff <= 1).all()
        assert torch.equal(base.cpu(), torch.from_numpy(g[case + "_base"]))
        assert torch.equal(col.cpu(), torch.from_numpy(g[case + "_col"]))
        assert torch.equal(val.cpu(), torch.from_numpy(g[case + "_values"]))
    assert filt.capped_rows() == 0


def test_corruption_at_fb15k237_size():
    from recon_amd import kg_train
    n_ent, n_rel, B, r = 14541, 237, 64, 40
    known = _synthetic_kg(n_ent, n_rel, 310116, 0)
    filt = kg_train.TripleFilter(known, n_ent, n_rel)
    pos = known[:B].int()
    vals = torch.ones(B, device=DEV)
    gen = lambda s: torch.Generator().manual_seed(s)
    idx, val = kg_train.corrupt_batch(pos, vals, filt, r, generator=gen(1))
    assert idx.shape == (B * (2 * r + 1), 3) and idx.dtype == torch.int64 and val.shape == (B * (2 * r + 1),)
    assert known.shape[0] == 310116
    neg = val == -1
    assert (val[B:B + 2 * B * (r // 2)] == -1).all()                         # entity rows: always replaced here (no saturated pair)
    rel_rows = slice(B + B * r, B + 2 * B * r)
    assert ((val[rel_rows] == -1) | (idx[rel_rows] == idx[:B].repeat(r, 1)).all(1)).all()
    assert not filt.contains(idx[neg]).any()
    base, col, ndiff = _signature(idx, B)
    c = torch.arange(idx.shape[0], device=DEV) - B
    own = torch.where(c < B * (r // 2), 0, torch.where(c < 2 * B * (r // 2), 2, torch.where(c >= B * r, 1, -1)))
    assert (col[neg] == own[neg]).all() and (ndiff[neg] == 1).all()
    assert (ndiff[~neg] == 0).all()
    idx2, val2 = kg_train.corrupt_batch(pos, vals, filt, r, generator=gen(1))
    assert torch.equal(idx, idx2) and torch.equal(val, val2)
    idx3, _ = kg_train.corrupt_batch(pos, vals, filt, r, generator=gen(2))
    assert not torch.equal(idx, idx3)
    torch.manual_seed(7)
    a, _ = kg_train.corrupt_batch(pos, vals, filt, r)
    torch.manual_seed(7)
    b, _ = kg_train.corrupt_batch(pos.long(), vals, filt, r)
    assert torch.equal(a, b)
    assert filt.capped_rows() == 0


def test_corruption_head_draws_are_uniform_over_allowed_ids():
    from recon_amd import kg_train
    n_ent, n_rel = 60, 4
    r0, t0 = 1, 5
    rs = np.random.RandomState(0)
    taken = rs.choice(n_ent, 15, replace=False)
    known = np.concatenate([[[h, r0, t0] for h in taken], rs.randint(0, [n_ent, n_rel, n_ent], size=(200, 3))])
    known = known[~((known[:, 1] == r0) & (known[:, 2] == t0) & ~np.isin(known[:, 0], taken))]
    filt = kg_train.TripleFilter(torch.from_numpy(known).to(DEV), n_ent, n_rel)
    B, r = 256, 40
    pos = torch.tensor([[int(taken[0]), r0, t0]] * B, device=DEV)
    idx, val = kg_train.corrupt_batch(pos, torch.ones(B, device=DEV), filt, r, generator=torch.Generator().manual_seed(123))
    heads = idx[B:B + B * (r // 2), 0].cpu().numpy()
    allowed = np.setdiff1d(np.arange(n_ent), taken)
    assert np.isin(heads, allowed).all()
    counts = np.bincount(heads, minlength=n_ent)[allowed]
    expect = len(heads) / len(allowed)
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    df = len(allowed) - 1
    crit = df * (1 - 2 / (9 * df) + 3.09 * (2 / (9 * df)) ** 0.5) ** 3      # Wilson-Hilferty, p = 0.001
    assert chi2 < crit, (chi2, crit)


def test_corruption_saturated_heads_hit_the_cap():
    from recon_amd import kg_train
    n_ent, n_rel = 20, 3
    known = torch.tensor([[h, 0, 0] for h in range(n_ent)] + [[2, 1, 3], [4, 2, 5]], device=DEV)
    filt = kg_train.TripleFilter(known, n_ent, n_rel)
    pos = torch.tensor([[1, 0, 0], [2, 1, 3]], device=DEV)
    B, r = 2, 2
    idx, val = kg_train.corrupt_batch(pos, torch.ones(B, device=DEV), filt, r, generator=torch.Generator().manual_seed(0))
    assert filt.capped_rows() == 1                                          # head row c = 0 (positive 0): every head of (0, 0) is known
    assert torch.equal(idx[B], pos[0]) and val[B] == 1
    assert val[B + 1] == -1 and (val[B + B:B + 2 * B] == -1).all()           # the other entity rows are replaced
    assert not filt.contains(idx[val == -1]).any()


def _fixture_model(g):
    from recon_amd.models import SpKBGATConvOnly
    D = g["sd__final_entity_embeddings"].shape[1]
    m = SpKBGATConvOnly(torch.randn(int(g["n_ent"]), 8), torch.randn(int(g["n_rel"]), 8), [D // 2, D], [D // 2, D], 0.0, 0.0, 0.2, 0.2, [2, 2], 50)
    m.load_state_dict({k: torch.from_numpy(g["sd__" + k]) for k in m.state_dict()}, strict=True)
    m = m.to(DEV)
    m.final_entity_embeddings.requires_grad_(False)
    m.final_relation_embeddings.requires_grad_(False)
    return m


def test_training_step_matches_reference():
    from recon_amd import kg_train
    g = load_golden("convkb_train1")
    m = _fixture_model(g)
    idx = torch.from_numpy(g["step_indices"]).to(DEV)
    val = torch.from_numpy(g["step_values"]).to(DEV)
    ratio = int(g["step_ratio"])
    preds = kg_train.convkb_scores(m, idx)
    torch.testing.assert_close(preds.detach().view(-1).cpu(), torch.from_numpy(g["preds"]), rtol=1e-5, atol=1e-5)
    opt = torch.optim.Adam(m.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
    opt.zero_grad()
    loss = kg_train.convkb_bce_loss(m, idx, val, ratio)
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    loss.backward()
    named = dict(m.named_parameters())
    for k in ("convKB.fc1.weight", "convKB.fc1.bias", "convKB.fc2.weight", "convKB.fc2.bias"):
        ref = torch.from_numpy(g["grad__" + k])
        torch.testing.assert_close(named[k].grad.cpu(), ref, rtol=1e-4, atol=1e-6 * float(ref.abs().max()) + 1e-9)
    for k in ("convKB.conv_layer.weight", "convKB.fc_layer.weight", "final_entity_embeddings"):
        assert named[k].grad is None
    opt.step()
    for k in ("convKB.fc1.weight", "convKB.fc1.bias", "convKB.fc2.weight", "convKB.fc2.bias"):
        torch.testing.assert_close(named[k].detach().cpu(), torch.from_numpy(g["after__" + k]), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("D,M", [(1, 17), (37, 333), (200, 1001), (257, 95)])
def test_forward_backward_within_fp64_band(D, M):
    from recon_amd import kg_train
    n_ent, n_rel = 300, 11
    m = _model(n_ent, n_rel, D, D + M)
    gen = torch.Generator().manual_seed(M)
    tri = torch.stack([torch.randint(0, n_ent, (M,), generator=gen), torch.randint(0, n_rel, (M,), generator=gen),
                       torch.randint(0, n_ent, (M,), generator=gen)], 1).to(DEV)
    val = (torch.randint(0, 2, (M,), generator=gen) * 2 - 1).float().to(DEV)
    E, R, W1, b1, w2, b2, slope = kg_train._params(m)
    z, s, gs, loss = kg_train._forward(tri, E, R, W1, b1, w2, b2, slope, val, 3)
    X = torch.cat([E[tri[:, 0]], R[tri[:, 1]], E[tri[:, 2]]], 1).double()
    W, bb1, ww2, bb2 = W1.detach().double(), b1.detach().double(), w2.detach().double().view(-1), b2.detach().double()
    K = 3 * D
    z64 = X @ W.T + bb1
    zb = 2 * (K + 2) * EPS32 * (X.abs() @ W.abs().T + bb1.abs())
    assert ((z.double() - z64).abs() <= zb).all()
    h64 = torch.where(z64 > 0, z64, slope * z64)
    s64 = h64 @ ww2 + bb2
    sb = 2 * (D + 2) * EPS32 * (h64.abs() @ ww2.abs() + bb2.abs()) + zb @ ww2.abs()
    assert ((s.double() - s64).abs() <= sb).all()
    # backward: g_s from the kernel, delta with the kernel's own z signs (the fp64 recomputation's may differ within zb of zero)
    g = gs.double()
    d64 = (g[:, None] * ww2[None, :]) * torch.where(z > 0, 1.0, slope).double()
    dW1, db1, dw2, db2 = kg_train._backward(tri, E, R, w2, slope, z, gs, None, W1, b1, b2)
    ref = d64.T @ X
    bound = 2 * (M + 4) * EPS32 * (d64.abs().T @ X.abs()) + 1e-30
    assert ((dW1.double() - ref).abs() <= bound).all()
    assert ((db1.double() - d64.sum(0)).abs() <= 2 * (M + 4) * EPS32 * d64.abs().sum(0) + 1e-30).all()
    h32 = torch.where(z > 0, z, z * slope).double()
    assert ((dw2.view(-1).double() - g @ h32).abs() <= 2 * (M + 4) * EPS32 * (g.abs() @ h32.abs()) + 1e-30).all()
    assert abs(db2.item() - g.sum().item()) <= 2 * (M + 4) * EPS32 * g.abs().sum().item() + 1e-30


def test_gradients_bitwise_identical_across_runs():
    from recon_amd import kg_train
    n_ent, n_rel, D, B, r = 2000, 50, 200, 64, 40
    m = _model(n_ent, n_rel, D, 1)
    filt = kg_train.TripleFilter(_synthetic_kg(n_ent, n_rel, 20000, 1), n_ent, n_rel)
    idx, val = kg_train.corrupt_batch(filt_pos(filt, B), torch.ones(B, device=DEV), filt, r, generator=torch.Generator().manual_seed(3))
    out = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        loss = kg_train.convkb_bce_loss(m, idx, val, r)
        loss.backward()
        out.append([loss.detach().clone()] + [p.grad.clone() for p in m.convKB.parameters() if p.grad is not None])
    assert len(out[0]) == 5
    for a, b in zip(*out):
        assert torch.equal(a, b)


def filt_pos(filt, B):
    """B known triples of a filter back as ids (head, relation, tail)."""
    k = filt.keys[:B]
    return torch.stack([(k // filt.n_ent) % filt.n_ent, k // (filt.n_ent * filt.n_ent), k % filt.n_ent], 1)


def _torch_loss(m, idx, val, ratio):
    preds = m(None, None, idx).view(-1)
    y = (val.view(-1) + 1) / 2
    w = y + (1 - y) * 1 / (ratio * 2)
    return preds, torch.nn.functional.binary_cross_entropy_with_logits(preds, y, weight=w)


def test_autograd_matches_torch_formulation():
    from recon_amd import kg_train
    n_ent, n_rel, D, B, r = 500, 20, 64, 16, 6
    m = _model(n_ent, n_rel, D, 2)
    filt = kg_train.TripleFilter(_synthetic_kg(n_ent, n_rel, 3000, 2), n_ent, n_rel)
    idx, val = kg_train.corrupt_batch(filt_pos(filt, B), torch.ones(B, device=DEV), filt, r, generator=torch.Generator().manual_seed(4))
    preds_t, loss_t = _torch_loss(m, idx, val, r)
    gt_loss = torch.autograd.grad(loss_t, [m.convKB.fc1.weight, m.convKB.fc1.bias, m.convKB.fc2.weight, m.convKB.fc2.bias], retain_graph=True)
    gs = torch.randn(idx.shape[0], 1, device=DEV)
    gt_sc = torch.autograd.grad(preds_t.view(-1, 1), [m.convKB.fc1.weight, m.convKB.fc1.bias, m.convKB.fc2.weight, m.convKB.fc2.bias], gs)
    loss = kg_train.convkb_bce_loss(m, idx, val, r) * 3.0                    # a non-unit upstream gradient goes through g_scale
    g_loss = torch.autograd.grad(loss, [m.convKB.fc1.weight, m.convKB.fc1.bias, m.convKB.fc2.weight, m.convKB.fc2.bias])
    preds = kg_train.convkb_scores(m, idx)
    torch.testing.assert_close(preds.detach(), preds_t.detach().view(-1, 1), rtol=1e-5, atol=1e-5)
    g_sc = torch.autograd.grad(preds, [m.convKB.fc1.weight, m.convKB.fc1.bias, m.convKB.fc2.weight, m.convKB.fc2.bias], gs)
    torch.testing.assert_close(loss.detach() / 3.0, loss_t.detach(), rtol=1e-5, atol=1e-6)
    for a, b in zip(g_loss, gt_loss):
        torch.testing.assert_close(a / 3.0, b, rtol=1e-4, atol=1e-6 * float(b.abs().max()))
    for a, b in zip(g_sc, gt_sc):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * float(b.abs().max()))


def test_short_training_run_tracks_torch():
    from recon_amd import kg_train
    n_ent, n_rel, D, B, r, lr = 800, 30, 48, 32, 10, 1e-3
    filt = kg_train.TripleFilter(_synthetic_kg(n_ent, n_rel, 6000, 3), n_ent, n_rel)
    m_dev, m_ref = _model(n_ent, n_rel, D, 5), _model(n_ent, n_rel, D, 5)
    opt_dev = torch.optim.Adam(m_dev.parameters(), lr=lr, weight_decay=1e-5)
    opt_ref = torch.optim.Adam(m_ref.parameters(), lr=lr, weight_decay=1e-5)
    train = filt_pos(filt, 400)
    ones = torch.ones(400, 1, device=DEV)
    gen = torch.Generator().manual_seed(9)
    for it in range(20):
        idx, val = kg_train.iteration_batch(train, ones, it % 13, B, filt, r, generator=gen)
        opt_dev.zero_grad()
        kg_train.convkb_bce_loss(m_dev, idx, val, r).backward()
        opt_dev.step()
        opt_ref.zero_grad()
        _torch_loss(m_ref, idx, val, r)[1].backward()
        opt_ref.step()
    init = _model(n_ent, n_rel, D, 5).convKB.state_dict()
    with torch.no_grad():
        for (k, a), b in zip(m_dev.convKB.named_parameters(), m_ref.convKB.parameters()):
            if a.grad is None:
                assert b.grad is None and torch.equal(a, b), k
                continue
            # Adam turns each gradient into a step of about lr per element, so an element whose gradient is mostly rounding noise may take a
            # different path: the band is on the whole tensor — the runs differ by at most 1 % of how far training moved it
            moved = float((b - init[k]).norm())
            assert moved > 0 and float((a - b).norm()) <= 1e-2 * moved, (k, float((a - b).norm()), moved)


def test_kg_train_rejections():
    from recon_amd import kg_train
    n_ent, n_rel = 50, 5
    m = _model(n_ent, n_rel, 16, 0)
    known = torch.tensor([[0, 0, 1], [1, 1, 2]], device=DEV)
    filt = kg_train.TripleFilter(known, n_ent, n_rel)
    with pytest.raises(ValueError):
        kg_train.TripleFilter(torch.tensor([[0, 5, 1]], device=DEV), n_ent, n_rel)
    with pytest.raises(ValueError):
        kg_train.corrupt_batch(torch.tensor([[50, 0, 1]], device=DEV), torch.ones(1, device=DEV), filt, 2)
    for bad in ([[0, 0, 50]], [[-1, 0, 1]], [[0, 5, 1]]):
        with pytest.raises(ValueError):
            kg_train.convkb_scores(m, torch.tensor(bad, device=DEV))
        with pytest.raises(ValueError):
            kg_train.convkb_bce_loss(m, torch.tensor(bad, device=DEV), torch.ones(1, device=DEV), 2)
    with pytest.raises(ValueError):
        kg_train.convkb_bce_loss(m, known, torch.ones(2, device=DEV), 0)
    m.final_relation_embeddings.requires_grad_(True)
    with pytest.raises(RuntimeError, match="741-742"):
        kg_train.convkb_bce_loss(m, known, torch.ones(2, device=DEV), 2)
    big = _model(4, 2, 513, 0)
    with pytest.raises(RuntimeError, match="unsupported"):
        kg_train.convkb_scores(big, torch.tensor([[0, 0, 1]], device=DEV))
    # without the range check an id outside its table scores NaN, and nothing is read outside a table
    s = kg_train.convkb_scores(m.requires_grad_(False), torch.tensor([[0, 0, 1], [0, 0, 50]], device=DEV), check_ids=False)
    assert torch.isfinite(s[0]).all() and torch.isnan(s[1]).all()
