"""Training of the GAT_sep_space ConvKB scorer on the device (k_kgs_ent2rel of csrc/kg_sep.hip and the fused ConvKB kernels of
csrc/kg_train.hip through recon_amd.kg_sep_train): the reference's training step and batch layout, the entity rows T and the whole step
against fp64 bands, determinism, torch autograd through the sep shell, a short training run and argument rejection."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = 2.0 ** -24
FC = ("convKB.fc1.weight", "convKB.fc1.bias", "convKB.fc2.weight", "convKB.fc2.bias")


def _model(n_ent, n_rel, D, seed):
    """A sep shell with frozen tables on the device and a frozen model_gat stand-in: (model_conv, model_gat)."""
    from recon_amd.sep_space import SpKBGATConvOnly
    torch.manual_seed(seed)
    m = SpKBGATConvOnly(torch.randn(n_ent, 8), torch.randn(n_rel, 8), [1, D], [1, D], 0.0, 0.0, 0.2, 0.2, [D, 1], 50).to(DEV)
    with torch.no_grad():
        m.convKB.fc1.weight.normal_(0, D ** -0.5)
        m.convKB.fc1.bias.normal_(0, 0.5)
        m.convKB.fc2.weight.normal_(0, D ** -0.5)
    m.final_entity_embeddings.requires_grad_(False)
    m.final_relation_embeddings.requires_grad_(False)
    gat = types.SimpleNamespace(W_ent2rel=(torch.randn(n_rel, D, D) / D ** 0.5).to(DEV), nonlinearity_ent2rel=torch.tanh)
    return m, gat


def _fixture_model(g):
    from recon_amd.sep_space import SpKBGATConvOnly
    D = g["sd__final_entity_embeddings"].shape[1]
    m = SpKBGATConvOnly(torch.randn(int(g["n_ent"]), 8), torch.randn(int(g["n_rel"]), 8), [D // 2, D], [D // 2, D], 0.0, 0.0, 0.2, 0.2, [2, 2], 50)
    m.load_state_dict({k: torch.from_numpy(g["sd__" + k]) for k in m.state_dict()}, strict=True)
    m = m.to(DEV)
    m.final_entity_embeddings.requires_grad_(False)
    m.final_relation_embeddings.requires_grad_(False)
    return m, types.SimpleNamespace(W_ent2rel=torch.from_numpy(g["gat__W_ent2rel"]).to(DEV), nonlinearity_ent2rel=torch.tanh)


def test_training_step_matches_reference():
    from recon_amd import kg_sep_train
    g = load_golden("convkb_sep_train1")
    m, gat = _fixture_model(g)
    idx = torch.from_numpy(g["indices"]).to(DEV)
    val = torch.from_numpy(g["values"]).to(DEV)
    ratio = int(g["ratio"])
    preds = kg_sep_train.sep_convkb_scores(m, gat, idx)
    torch.testing.assert_close(preds.detach().view(-1).cpu(), torch.from_numpy(g["preds"]), rtol=1e-5, atol=1e-5)
    opt = torch.optim.Adam(m.parameters(), lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
    opt.zero_grad()
    loss = kg_sep_train.sep_convkb_bce_loss(m, gat, idx, val, ratio)
    assert abs(loss.item() - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    loss.backward()
    named = dict(m.named_parameters())
    for k in FC:
        ref = torch.from_numpy(g["grad__" + k])
        torch.testing.assert_close(named[k].grad.cpu(), ref, rtol=1e-4, atol=1e-6 * float(ref.abs().max()) + 1e-9)
    for k in ("convKB.conv_layer.weight", "convKB.fc_layer.weight", "final_entity_embeddings"):
        assert named[k].grad is None
    opt.step()
    for k in FC:
        torch.testing.assert_close(named[k].detach().cpu(), torch.from_numpy(g["after__" + k]), rtol=1e-5, atol=1e-6)


def test_sampler_reproduces_the_sep_batch_layout():
    from recon_amd import kg_train
    g = load_golden("convkb_sep_train1")
    known = torch.from_numpy(np.concatenate([g["train"], g["valid"], g["test"]])).to(DEV)
    filt = kg_train.TripleFilter(known, int(g["n_ent"]), int(g["n_rel"]))
    train = torch.from_numpy(g["train"]).to(DEV).int()
    B = int(g["batch_size"])
    for seed in range(3):
        idx, val = kg_train.iteration_batch(train, torch.ones(train.shape[0], 1, device=DEV), int(g["iter"]), B, filt, int(g["ratio"]),
                                            generator=torch.Generator().manual_seed(seed))
        assert torch.equal(idx[:B].cpu(), torch.from_numpy(g["positives"]))
        base = torch.arange(idx.shape[0], device=DEV)
        base = torch.where(base < B, base, (base - B) % B)
        diff = idx != idx[:B][base]
        col = torch.where(diff.any(1), diff.int().argmax(1), torch.full_like(base, -1))
        assert (diff.sum(1) <= 1).all()
        assert torch.equal(base.cpu(), torch.from_numpy(g["base"])) and torch.equal(col.cpu(), torch.from_numpy(g["col"]))
        assert torch.equal(val.cpu(), torch.from_numpy(g["values"]))
        assert not filt.contains(idx[val == -1]).any()


# triples per relation: 0, 1 and 16 RB, 16 RB + 1 for RB = 1, 2, 4 (items, two per triple: 2, 32 / 34, 64 / 66, 128 / 130), so that
# tiles of 32 and 64 rows end exactly at and just before a relation's end
PER_REL = [0, 1, 16, 17, 32, 33, 64, 65, 3]


def _case(D, seed, n_ent=150):
    m, gat = _model(n_ent, len(PER_REL), D, seed)
    rs = np.random.RandomState(seed)
    tri = np.concatenate([np.stack([rs.randint(0, n_ent, k), np.full(k, r), rs.randint(0, n_ent, k)], 1) for r, k in enumerate(PER_REL) if k])
    tri = tri[rs.permutation(len(tri))]
    tri[3, 0] = tri[10, 2] = tri[40, 0] = 7                                  # duplicate entity ids, heads and tails
    assert len(tri) % 2 == 1                                                 # odd M
    val = np.where(rs.rand(len(tri)) < 0.3, 1.0, -1.0).astype(np.float32)
    return m, gat, torch.from_numpy(tri).to(DEV), torch.from_numpy(val).to(DEV)


def _t64(m, gat, tri):
    """fp64 T and its fp32 band: an fma chain over D terms (|dX| <= D eps sum |e w|), tanh 1-Lipschitz plus a few ulp; doubled."""
    E, W = m.final_entity_embeddings.double(), gat.W_ent2rel.double()
    t = tri.long()
    rows = torch.cat([t[:, 0], t[:, 2]])
    rel = torch.cat([t[:, 1], t[:, 1]])
    X = torch.bmm(E[rows].unsqueeze(1), W[rel]).squeeze(1)
    Xa = torch.bmm(E[rows].abs().unsqueeze(1), W[rel].abs()).squeeze(1)
    return torch.tanh(X), 2 * ((E.shape[1] + 2) * EPS32 * Xa + 8 * EPS32)


@pytest.mark.parametrize("D", [1, 37, 144, 145, 200, 257, 304, 305, 512])       # 304 | 305: the row-block switch of k_kgs_ent2rel; 144 | 145: that of the tables
def test_ent2rel_rows_within_fp64_band(D):
    from recon_amd import kg_sep_train
    m, gat, tri, _ = _case(D, D)
    M = tri.shape[0]
    for t in (tri, tri.int()):
        T, rem = kg_sep_train.ent2rel_rows(m.final_entity_embeddings, gat.W_ent2rel, t)
        assert T.shape == (2 * M, D) and rem.dtype == torch.int64
        ar = torch.arange(M, device=DEV)
        assert torch.equal(rem, torch.stack([ar, tri[:, 1].long(), ar + M], 1))
        T64, tau = _t64(m, gat, tri)
        err = (T.double() - T64).abs()
        assert bool((err <= tau).all()), (D, float((err / tau).max()))
    # rows of one (entity, relation) pair are the same bits wherever they sit
    key = torch.cat([tri[:, 0], tri[:, 2]]) * len(PER_REL) + torch.cat([tri[:, 1], tri[:, 1]])
    first = {}
    for i, k in enumerate(key.tolist()):
        if k in first:
            assert torch.equal(T[i].view(torch.int32), T[first[k]].view(torch.int32))
        first.setdefault(k, i)


@pytest.mark.parametrize("D", [1, 37, 200, 257, 512])
def test_whole_step_within_fp64_band(D):
    from recon_amd import kg_train, kg_sep_train
    m, gat, tri, val = _case(D, D + 1)
    M, ratio = tri.shape[0], 3
    T, rem = kg_sep_train.ent2rel_rows(m.final_entity_embeddings, gat.W_ent2rel, tri)
    E, R, W1, b1, w2, b2, slope = kg_train._params(m)
    z, s, gs, loss = kg_train._forward(rem, T, R, W1, b1, w2, b2, slope, val, ratio)
    T64, tau = _t64(m, gat, tri)
    X = torch.cat([T[:M], R[tri[:, 1]], T[M:]], 1).double()                  # the kernel's rows (their own band is checked above)
    Wd, bb1, ww2, bb2 = W1.detach().double(), b1.detach().double(), w2.detach().double().view(-1), b2.detach().double()
    z64 = X @ Wd.T + bb1
    zb = 2 * (3 * D + 2) * EPS32 * (X.abs() @ Wd.abs().T + bb1.abs())
    assert ((z.double() - z64).abs() <= zb).all()
    # and against the fp64 rows: the T band carried through fc1
    X64 = torch.cat([T64[:M], R[tri[:, 1]].double(), T64[M:]], 1)
    tau_x = torch.cat([tau[:M], torch.zeros(M, D, dtype=torch.float64, device=DEV), tau[M:]], 1)
    assert ((z.double() - (X64 @ Wd.T + bb1)).abs() <= zb + tau_x @ Wd.abs().T).all()
    h64 = torch.where(z64 > 0, z64, slope * z64)
    s64 = h64 @ ww2 + bb2
    sb = 2 * (D + 2) * EPS32 * (h64.abs() @ ww2.abs() + bb2.abs()) + zb @ ww2.abs()
    assert ((s.double() - s64).abs() <= sb).all()
    y = (val.double() + 1) / 2
    w = y + (1 - y) / (2 * ratio)
    sd = s.double()
    mx = torch.clamp(-sd, min=0)
    terms = w * ((1 - y) * sd + mx + torch.log(torch.exp(-mx) + torch.exp(-sd - mx)))
    assert abs(loss.item() - terms.mean().item()) <= 4 * (M + 16) * EPS32 * terms.abs().mean().item() + 1e-30
    g64 = w * (torch.sigmoid(sd) - y) / M
    assert ((gs.double() - g64).abs() <= 32 * EPS32 * g64.abs() + 1e-30).all()
    g = gs.double()
    d64 = (g[:, None] * ww2[None, :]) * torch.where(z > 0, 1.0, slope).double()
    dW1, db1, dw2, db2 = kg_train._backward(rem, T, R, w2, slope, z, gs, None, W1, b1, b2)
    assert ((dW1.double() - d64.T @ X).abs() <= 2 * (M + 4) * EPS32 * (d64.abs().T @ X.abs()) + 1e-30).all()
    assert ((db1.double() - d64.sum(0)).abs() <= 2 * (M + 4) * EPS32 * d64.abs().sum(0) + 1e-30).all()
    h32 = torch.where(z > 0, z, z * slope).double()
    assert ((dw2.view(-1).double() - g @ h32).abs() <= 2 * (M + 4) * EPS32 * (g.abs() @ h32.abs()) + 1e-30).all()
    assert abs(db2.item() - g.sum().item()) <= 2 * (M + 4) * EPS32 * g.abs().sum().item() + 1e-30


def test_step_bitwise_identical_across_runs():
    from recon_amd import kg_sep_train
    m, gat, tri, val = _case(200, 3, n_ent=2000)
    out = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        T, _ = kg_sep_train.ent2rel_rows(m.final_entity_embeddings, gat.W_ent2rel, tri)
        loss = kg_sep_train.sep_convkb_bce_loss(m, gat, tri, val, 40)
        loss.backward()
        out.append([T, loss.detach().clone()] + [p.grad.clone() for p in m.convKB.parameters() if p.grad is not None])
    assert len(out[0]) == 6
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _torch_loss(m, gat, idx, val, ratio):
    preds = m(None, None, idx, gat).view(-1)
    y = (val.view(-1) + 1) / 2
    return preds, torch.nn.functional.binary_cross_entropy_with_logits(preds, y, weight=y + (1 - y) / (2 * ratio))


def test_autograd_matches_the_sep_shell():
    from recon_amd import kg_sep_train
    m, gat, tri, val = _case(64, 4)
    r = 6
    params = [m.convKB.fc1.weight, m.convKB.fc1.bias, m.convKB.fc2.weight, m.convKB.fc2.bias]
    preds_t, loss_t = _torch_loss(m, gat, tri, val, r)
    gt_loss = torch.autograd.grad(loss_t, params, retain_graph=True)
    gs = torch.randn(tri.shape[0], 1, device=DEV)
    gt_sc = torch.autograd.grad(preds_t.view(-1, 1), params, gs)
    loss = kg_sep_train.sep_convkb_bce_loss(m, gat, tri, val, r) * 3.0       # a non-unit upstream gradient
    g_loss = torch.autograd.grad(loss, params)
    preds = kg_sep_train.sep_convkb_scores(m, gat, tri)
    torch.testing.assert_close(preds.detach(), preds_t.detach().view(-1, 1), rtol=1e-5, atol=1e-5)
    g_sc = torch.autograd.grad(preds, params, gs)
    torch.testing.assert_close(loss.detach() / 3.0, loss_t.detach(), rtol=1e-5, atol=1e-6)
    for a, b in zip(g_loss, gt_loss):
        torch.testing.assert_close(a / 3.0, b, rtol=1e-4, atol=1e-6 * float(b.abs().max()))
    for a, b in zip(g_sc, gt_sc):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * float(b.abs().max()))


def test_short_training_run_tracks_the_shell():
    from recon_amd import kg_train, kg_sep_train
    n_ent, n_rel, D, B, r, lr = 800, 30, 48, 32, 10, 1e-3
    g = torch.Generator().manual_seed(3)
    known = torch.unique(torch.stack([torch.randint(0, n_ent, (6200,), generator=g), torch.randint(0, n_rel, (6200,), generator=g),
                                      torch.randint(0, n_ent, (6200,), generator=g)], 1), dim=0)[:6000].to(DEV)
    filt = kg_train.TripleFilter(known, n_ent, n_rel)
    (m_dev, gat), (m_ref, _) = _model(n_ent, n_rel, D, 5), _model(n_ent, n_rel, D, 5)
    init = {k: v.clone() for k, v in m_dev.convKB.state_dict().items()}
    opt_dev = torch.optim.Adam(m_dev.parameters(), lr=lr, weight_decay=1e-5)
    opt_ref = torch.optim.Adam(m_ref.parameters(), lr=lr, weight_decay=1e-5)
    train, ones = known[:400], torch.ones(400, 1, device=DEV)
    gen = torch.Generator().manual_seed(9)
    for it in range(20):
        idx, val = kg_train.iteration_batch(train, ones, it % 13, B, filt, r, generator=gen)
        opt_dev.zero_grad()
        kg_sep_train.sep_convkb_bce_loss(m_dev, gat, idx, val, r).backward()
        opt_dev.step()
        opt_ref.zero_grad()
        _torch_loss(m_ref, gat, idx, val, r)[1].backward()
        opt_ref.step()
    with torch.no_grad():
        for (k, a), b in zip(m_dev.convKB.named_parameters(), m_ref.convKB.parameters()):
            if a.grad is None:
                assert b.grad is None and torch.equal(a, b), k
                continue
            moved = float((b - init[k]).norm())                              # the same 1 % drift rule as test_short_training_run_tracks_torch
            assert moved > 0 and float((a - b).norm()) <= 1e-2 * moved, (k, float((a - b).norm()), moved)


def test_kg_sep_train_rejections():
    from recon_amd import kg_sep_train as K
    m, gat = _model(50, 5, 16, 0)
    known = torch.tensor([[0, 0, 1], [1, 1, 2]], device=DEV)
    ones = torch.ones(2, device=DEV)
    for bad in ([[0, 0, 50]], [[-1, 0, 1]], [[0, 5, 1]]):
        with pytest.raises(ValueError):
            K.sep_convkb_scores(m, gat, torch.tensor(bad, device=DEV))
        with pytest.raises(ValueError):
            K.sep_convkb_bce_loss(m, gat, torch.tensor(bad, device=DEV), torch.ones(1, device=DEV), 2)
        with pytest.raises(ValueError):
            K.ent2rel_rows(m.final_entity_embeddings, gat.W_ent2rel, torch.tensor(bad, device=DEV))
    with pytest.raises(ValueError, match="ratio"):
        K.sep_convkb_bce_loss(m, gat, known, ones, 0)
    with pytest.raises(ValueError, match="empty"):
        K.sep_convkb_bce_loss(m, gat, known[:0], ones[:0], 2)
    with pytest.raises(ValueError, match="tanh"):
        K.sep_convkb_scores(m, types.SimpleNamespace(W_ent2rel=gat.W_ent2rel, nonlinearity_ent2rel=torch.relu), known)
    with pytest.raises(RuntimeError, match="808-809"):
        K.sep_convkb_bce_loss(m, types.SimpleNamespace(W_ent2rel=torch.nn.Parameter(gat.W_ent2rel), nonlinearity_ent2rel=torch.tanh), known, ones, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        K.sep_convkb_bce_loss(m, gat, known.cpu(), ones.cpu(), 2)
    big, gbig = _model(4, 2, 513, 0)
    with pytest.raises(ValueError, match="512"):
        K.sep_convkb_scores(big, gbig, torch.tensor([[0, 0, 1]], device=DEV))
    m.final_relation_embeddings.requires_grad_(True)
    with pytest.raises(RuntimeError, match="741-742"):
        K.sep_convkb_bce_loss(m, gat, known, ones, 2)
    m.final_relation_embeddings.requires_grad_(False)
    # without the range check an id outside its table scores NaN (entity or relation), and nothing is read outside a table
    s = K.sep_convkb_scores(m, gat, torch.tensor([[0, 0, 1], [0, 0, 50], [-3, 1, 2], [0, 5, 1], [2, 4, 3]], device=DEV), check_ids=False)
    assert torch.isfinite(s[0]).all() and torch.isfinite(s[4]).all() and torch.isnan(s[1:4]).all()
    torch.cuda.synchronize()
