"""The stage-A loss of the GAT_sep_space tree on the device (recon_amd.sep_space.batch_gat_loss, csrc/kg_sep.hip k_kgsl_*): the reference's
fixtures, fp64 bands for the continuous outputs, the two-step check of the gradients (every device decision against fp64 where fp64 is
decided, then the fp64 linear backward under the device's decisions), bitwise reproducibility, torch autograd through the composition the
package offered before (`ent2rel` plus torch ops), requires_grad combinations, a short SGD run, rejections and NaN."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = 2.0 ** -24
NAMES = ["sep_gat_loss1_d8", "sep_gat_loss2_d50"]


def _gat(W, nl=torch.tanh):
    return types.SimpleNamespace(W_ent2rel=W, nonlinearity_ent2rel=nl)


def _composition(fn, tri, E, Rel, gat, ratio, dedup=False):
    """What the package offered before this loss: the reference's op sequence on SpKBGATModified.ent2rel's kernel (rel_rows_mm) and torch ops."""
    from recon_amd.sep_space import rel_rows_mm
    reps = 2 * ratio
    n_pos = tri.shape[0] // (reps + 1)

    def norm(t):
        h = gat.nonlinearity_ent2rel(rel_rows_mm(E[t[:, 0]], t[:, 1].contiguous(), gat.W_ent2rel))
        tl = gat.nonlinearity_ent2rel(rel_rows_mm(E[t[:, 2]], t[:, 1].contiguous(), gat.W_ent2rel))
        return torch.norm(h + Rel[t[:, 1]] - tl, p=1, dim=1)
    pos = norm(tri[:n_pos]).repeat(reps) if dedup else norm(tri[:n_pos].repeat(reps, 1))
    return fn(pos, norm(tri[n_pos:]), -torch.ones(reps * n_pos, device=E.device))


@pytest.mark.parametrize("name", NAMES)
def test_sep_batch_gat_loss_golden(name):
    """Loss, terms and the three gradients against the reference's own function, with test_batch_gat_loss_golden's tolerances; the fused path
    and the fallback (any other loss function)."""
    from recon_amd.sep_space import batch_gat_loss, gat_loss_parts
    g = load_golden(name)
    tri = torch.from_numpy(g["train_indices"]).to(DEV)
    margin, ratio = float(g["margin"]), int(g["ratio"])
    D = g["entity"].shape[1]
    for loss_fn in (torch.nn.MarginRankingLoss(margin=margin), lambda a, b, y: torch.nn.functional.margin_ranking_loss(a, b, y, margin=margin)):
        ent, rel, W = (torch.from_numpy(g[k]).to(DEV).requires_grad_(True) for k in ("entity", "relation", "W_ent2rel"))
        loss = batch_gat_loss(loss_fn, tri, ent, rel, _gat(W), valid_invalid_ratio_gat=ratio)
        (loss * 1.5).backward()
        np.testing.assert_allclose(loss.detach().cpu().numpy(), g["loss"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(ent.grad.cpu().numpy(), 1.5 * g["g_entity"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(rel.grad.cpu().numpy(), 1.5 * g["g_relation"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(W.grad.cpu().numpy(), 1.5 * g["g_W_ent2rel"], rtol=1e-5, atol=1e-7)
    T, norms, terms, loss2 = gat_loss_parts(tri, ent.detach(), rel.detach(), W.detach(), margin, ratio)
    n_pos = tri.shape[0] // (2 * ratio + 1)
    # a term is the difference of two fp32 sums of D magnitudes, in the reference as here: twice the band of tests/test_sep_gat_loss_cpu.py
    band = 2 * (D + 4) * EPS32 * (norms[:n_pos].repeat(2 * ratio) + norms[n_pos:] + margin).double().cpu()
    assert bool(((terms.double().cpu() - torch.from_numpy(g["terms"]).double()).abs() <= band).all())
    np.testing.assert_allclose(loss2.cpu().numpy(), g["loss"], rtol=1e-5, atol=1e-6)


# triples per relation: 0, 1, 16, 17, 64, 65 (items, two per triple: tiles of 32 / 64 items and the 64-item steps of the weight-gradient
# walk end exactly at and just before a relation's end), 3, a relation that takes the rest, and an empty last relation
PER_REL = [0, 1, 16, 17, 64, 65, 3]


def _case(D, seed, ratio, n_ent=150, n_pos=None, rel_sizes=None, margin=0.7, w_scale=1.0):
    reps = 2 * ratio
    rs = np.random.RandomState(seed)
    if rel_sizes is None:
        n_pos = {2: 57, 4: 35, 6: 25}[reps]
        M = n_pos * (reps + 1)
        sizes = PER_REL + [M - sum(PER_REL), 0]
    else:
        M = n_pos * (reps + 1)
        sizes = list(rel_sizes)
    assert n_pos % 2 == 1 or rel_sizes is not None
    assert sum(sizes) == M and min(sizes) >= 0
    n_rel = len(sizes)
    tri = np.stack([rs.randint(0, n_ent, M), np.repeat(np.arange(n_rel), sizes)[rs.permutation(M)], rs.randint(0, n_ent, M)], 1)
    tri[3, 0] = tri[10, 2] = tri[40, 0] = tri[M - 1, 2] = 7                 # duplicate entity ids, heads and tails
    gen = torch.Generator().manual_seed(seed)
    E = torch.randn(n_ent, D, generator=gen)
    Rel = 0.5 * torch.randn(n_rel, D, generator=gen)
    W = w_scale * torch.randn(n_rel, D, D, generator=gen) / D ** 0.5
    return E.to(DEV), Rel.to(DEV), W.to(DEV), torch.from_numpy(tri).to(DEV), n_pos, reps, margin


def _by_relation(tri, n_rel):
    rel = tri[:, 1]
    return [(r, torch.nonzero(rel == r).view(-1)) for r in range(n_rel) if bool((rel == r).any())]


def _fp64(E, Rel, W, tri, n_pos, reps, margin):
    """fp64 T, x, norms, v (terms before the clamp) and their fp32 bands.  T: the `_t64` rule of tests/test_kg_sep_train_gpu.py (an fma chain
    over D terms, tanh 1-Lipschitz plus a few ulp; doubled).  x: T's bands plus two fp32 operations.  norm: x's bands plus a sum of D terms."""
    M, D = tri.shape[0], E.shape[1]
    E64, W64, R64 = E.double(), W.double(), Rel.double()
    T = torch.zeros(2 * M, D, dtype=torch.float64, device=DEV)
    tau = torch.zeros_like(T)
    for r, idx in _by_relation(tri, W.shape[0]):
        for rows, col in ((idx, 0), (idx + M, 2)):
            e = E64[tri[idx, col]]
            T[rows] = torch.tanh(e @ W64[r])
            tau[rows] = 2 * ((D + 2) * EPS32 * (e.abs() @ W64[r].abs()) + 8 * EPS32)
    rr = R64[tri[:, 1]]
    x = T[:M] + rr - T[M:]
    tau_x = tau[:M] + tau[M:] + 4 * EPS32 * (T[:M].abs() + rr.abs() + T[M:].abs())
    norm = x.abs().sum(1)
    tau_n = tau_x.sum(1) + 2 * (D + 2) * EPS32 * norm
    v = norm[:n_pos].repeat(reps) - norm[n_pos:] + margin
    tau_v = tau_n[:n_pos].repeat(reps) + tau_n[n_pos:] + 4 * EPS32 * (norm[:n_pos].repeat(reps) + norm[n_pos:] + margin)
    return T, tau, x, tau_x, norm, tau_n, v, tau_v


def _two_step(E, Rel, W, tri, n_pos, reps, margin, g_up=1.0, runs=1, keep_w=False):
    """The whole check of one case; returns the gradients of the last run.  keep_w: the leaf of W's gradient is W's own memory (a detached
    alias) instead of a clone, which would sit at the allocator's alignment whatever W's is."""
    from recon_amd.sep_space import batch_gat_loss, gat_loss_parts
    M, D, P = tri.shape[0], E.shape[1], n_pos * reps
    T64, tau, x64, tau_x, n64, tau_n, v64, tau_v = _fp64(E, Rel, W, tri, n_pos, reps, margin)
    # the share of undecided elements is a condition on the case, asserted on the fp64 side before the device is looked at
    x_dec, v_dec = x64.abs() > tau_x, v64.abs() > tau_v
    assert float((~x_dec).double().mean()) <= 1e-3 and float((~v_dec).double().mean()) <= 2e-2, (
        float((~x_dec).double().mean()), float((~v_dec).double().mean()))
    out = None
    for _ in range(runs):
        T, norms, terms, loss = gat_loss_parts(tri, E, Rel, W, margin, reps // 2)
        assert bool(((T.double() - T64).abs() <= tau).all())
        assert bool(((norms.double() - n64).abs() <= tau_n).all())
        assert bool(((terms.double() - v64.clamp_min(0)).abs() <= tau_v).all())
        t64 = v64.clamp_min(0)
        assert abs(loss.item() - t64.mean().item()) <= tau_v.mean().item() + 4 * (P + 16) * EPS32 * t64.mean().item() + 1e-30
        # step 1: the device's decisions.  Its x, bit for bit: the same two fp32 operations on the T it returned
        xd = (T[:M] + Rel[tri[:, 1]]) - T[M:]
        S = torch.sign(xd).double()
        assert bool((S[x_dec] == torch.sign(x64)[x_dec]).all())
        A = terms > 0
        assert bool((A[v_dec] == (v64 > 0)[v_dec]).all())
        # step 2: the fp64 linear backward under these decisions, with fp32 bands
        Ed, Rd, Wd = (t.clone().requires_grad_(True) for t in (E, Rel, W))
        if keep_w:
            Wd = W.detach().requires_grad_(True)
            assert Wd.data_ptr() == W.data_ptr() and Wd.is_contiguous()
        l = batch_gat_loss(torch.nn.MarginRankingLoss(margin=margin), tri, Ed, Rd, _gat(Wd), valid_invalid_ratio_gat=reps // 2)
        assert torch.equal(l.detach().view(torch.int32), loss.view(torch.int32))
        (l * g_up).backward()
        w = g_up / P
        c = torch.cat([w * A.view(reps, n_pos).sum(0).double(), -w * A.double()])
        gx = c[:, None] * S
        gpre = torch.cat([gx * (1 - T64[:M] ** 2), -gx * (1 - T64[M:] ** 2)])
        gpre_b = torch.cat([gx.abs(), gx.abs()]) * (2 * tau * T64.abs() + tau ** 2 + 8 * EPS32)
        ids = torch.cat([tri[:, 0], tri[:, 2]])
        E64, W64 = E.double(), W.double()
        gW, gW_b = torch.zeros_like(W64), torch.zeros_like(W64)
        rows, rows_b = torch.zeros_like(gpre), torch.zeros_like(gpre)
        gR, gR_b = torch.zeros_like(Rel, dtype=torch.float64), torch.zeros_like(Rel, dtype=torch.float64)
        for r, idx in _by_relation(tri, W.shape[0]):
            it = torch.cat([idx, idx + M])
            e, gp = E64[ids[it]], gpre[it]
            gW[r] = e.T @ gp
            gW_b[r] = e.abs().T @ gpre_b[it] + 2 * (it.numel() + 4) * EPS32 * (e.abs().T @ gp.abs())
            rows[it] = gp @ W64[r].T
            rows_b[it] = gpre_b[it] @ W64[r].abs().T + 2 * (D + 4) * EPS32 * (gp.abs() @ W64[r].abs().T)
            gR[r] = gx[idx].sum(0)
            gR_b[r] = 2 * (idx.numel() + 8) * EPS32 * gx[idx].abs().sum(0)
        cnt = torch.bincount(ids, minlength=E.shape[0]).double()[:, None]
        gE = torch.zeros_like(E64).index_add_(0, ids, rows)
        gE_b = torch.zeros_like(E64).index_add_(0, ids, rows_b) + 2 * (cnt + 4) * EPS32 * torch.zeros_like(E64).index_add_(0, ids, rows.abs())
        for name, got, ref, band in (("g_W", Wd.grad, gW, gW_b), ("g_Rel", Rd.grad, gR, gR_b), ("g_E", Ed.grad, gE, gE_b)):
            err = (got.double() - ref).abs()
            assert bool((err <= band + 1e-30).all()), (name, D, float((err / (band + 1e-30)).max()))
        new = (loss, Ed.grad, Rd.grad, Wd.grad)
        if out is not None:                                              # bitwise equality of the loss and all three gradients across runs
            for a, b in zip(out, new):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        out = new
    return out


@pytest.mark.parametrize("D,ratio,w_scale", [(1, 1, 1.0), (37, 2, 1.0), (200, 3, 1.0), (257, 1, 1.0), (331, 3, 0.5), (512, 2, 0.2)],
                         ids=["1-1", "37-2", "200-3", "257-1", "331-3", "512-2"])
def test_sep_loss_two_step_check_within_fp64_bands(D, ratio, w_scale):
    # the worst-case band grows with D times the size of the products.  At D = 512 pre-activations of unit standard deviation leave 1.4e-3 of the
    # elements and 6 % of the 140 pairs undecided in fp64, more than the check admits, 0.5 still 2.1 % of the pairs; 0.2 leaves 5.5e-4 and 0.7 %
    # (measured on the fp64 side alone, before any device run).  D = 331 (304 < D <= 512, D % 4 != 0: k_kgsl_rows<2, false>) at 0.5 leaves
    # 4.3e-4 and 0.67 %
    E, Rel, W, tri, n_pos, reps, margin = _case(D, 100 + D, ratio, w_scale=w_scale)
    _two_step(E, Rel, W, tri, n_pos, reps, margin, g_up=1.5, runs=2)


@pytest.mark.parametrize("D,ratio,w_scale", [(200, 3, 1.0), (308, 2, 0.2)])
def test_sep_loss_w_ent2rel_one_float_into_a_larger_buffer(D, ratio, w_scale):
    """W_ent2rel as a contiguous view 4 bytes into a buffer: D % 4 == 0 but no 16-byte alignment, so the row-gradient kernel takes its scalar
    loads (k_kgsl_rows<4, false> at D = 200, <2, false> at D = 308; 0.2 leaves 2.0e-4 of the elements and no pair undecided in fp64 there).
    The two-step check holds, and the float4 and the scalar loads feed the same MFMA chain: the loss and all three gradients equal the run
    on the aligned copy bit for bit."""
    E, Rel, W, tri, n_pos, reps, margin = _case(D, 100 + D, ratio, w_scale=w_scale)
    buf = torch.full((W.numel() + 8,), float("nan"), device=DEV)
    Wo = buf[1:1 + W.numel()].view(W.shape)
    Wo.copy_(W)
    assert Wo.is_contiguous() and Wo.data_ptr() % 16 == 4 and W.data_ptr() % 16 == 0
    off = _two_step(E, Rel, Wo, tri, n_pos, reps, margin, g_up=1.5, keep_w=True)
    ali = _two_step(E, Rel, W, tri, n_pos, reps, margin, g_up=1.5)
    for name, a, b in zip(("loss", "g_E", "g_Rel", "g_W"), off, ali):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[1 + W.numel():]).all())


def test_sep_loss_stage_a_size_twice():
    """14 541 entities, 237 relations with 1 / k sizes, D = 200, 2 000 positives, ratio 2: the two-step check, twice, bitwise equal.  The
    kernels keep no arrival counters (every output element is one chain written by one lane), so there is none to find non-zero; the
    workspace they get is handed over uninitialised on purpose (torch.empty in recon_amd.sep_loss)."""
    n_ent, n_rel, D, n_pos, ratio = 14541, 237, 200, 2000, 2
    M = n_pos * (2 * ratio + 1)
    wgt = 1.0 / np.arange(1, n_rel + 1)
    sizes = np.floor(M * wgt / wgt.sum()).astype(np.int64)
    sizes[0] += M - sizes.sum()
    E, Rel, W, tri, n_pos, reps, margin = _case(D, 3, ratio, n_ent=n_ent, n_pos=n_pos, rel_sizes=sizes, margin=1.0)
    _two_step(E, Rel, W, tri, n_pos, reps, margin, runs=2)


def test_sep_loss_autograd_matches_the_composition():
    """torch autograd through `rel_rows_mm` + torch ops on a decisive small case (the D = 50 fixture: smallest |x| and |term| at least 32 times
    the fp32 deviations), a non-unit upstream gradient."""
    from recon_amd.sep_space import batch_gat_loss
    g = load_golden("sep_gat_loss2_d50")
    tri, ratio, fn = torch.from_numpy(g["train_indices"]).to(DEV), int(g["ratio"]), torch.nn.MarginRankingLoss(margin=float(g["margin"]))
    grads = []
    for f in (batch_gat_loss, lambda fn_, t, e, r, gat, valid_invalid_ratio_gat: _composition(fn_, t, e, r, gat, valid_invalid_ratio_gat)):
        ent, rel, W = (torch.from_numpy(g[k]).to(DEV).requires_grad_(True) for k in ("entity", "relation", "W_ent2rel"))
        loss = f(fn, tri, ent, rel, _gat(W), valid_invalid_ratio_gat=ratio)
        (loss * 3.0).backward()
        grads.append((loss.detach(), ent.grad, rel.grad, W.grad))
    torch.testing.assert_close(grads[0][0], grads[1][0], rtol=1e-5, atol=1e-6)
    for a, b in zip(grads[0][1:], grads[1][1:]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6 * float(b.abs().max()))


def test_sep_loss_requires_grad_combinations():
    """Each gradient is computed only if it is required, and is the same bits whichever others are."""
    from recon_amd.sep_space import batch_gat_loss
    E, Rel, W, tri, n_pos, reps, margin = _case(40, 9, 2)
    fn = torch.nn.MarginRankingLoss(margin=margin)
    full = None
    for need in ((True, True, True), (True, True, False), (False, False, True), (True, False, False), (False, True, False), (False, True, True)):
        ts = [t.clone().requires_grad_(n) for t, n in zip((E, Rel, W), need)]
        loss = batch_gat_loss(fn, tri, ts[0], ts[1], _gat(ts[2]), valid_invalid_ratio_gat=reps // 2)
        loss.backward()
        grads = [t.grad for t in ts]
        if full is None:
            full = grads
        for gr, ref, n in zip(grads, full, need):
            assert (gr is not None) == n
            if n:
                assert torch.equal(gr.view(torch.int32), ref.view(torch.int32))
    frozen = batch_gat_loss(fn, tri, E, Rel, _gat(W), valid_invalid_ratio_gat=reps // 2)
    assert not frozen.requires_grad
    # a relation table with more rows than W_ent2rel: its extra rows get zero gradients; one with fewer bounds the ids
    Rel2 = torch.cat([Rel, Rel[:2]]).requires_grad_(True)
    batch_gat_loss(fn, tri, E, Rel2, _gat(W), valid_invalid_ratio_gat=reps // 2).backward()
    assert torch.equal(Rel2.grad[:Rel.shape[0]].view(torch.int32), full[1].view(torch.int32)) and not Rel2.grad[Rel.shape[0]:].any()


def test_sep_loss_short_sgd_run_tracks_the_composition():
    """20 SGD steps of a small SpKBGATModified's W_ent2rel and tables through the new loss against the composition: the 1 % drift rule of
    test_short_training_run_tracks_the_shell."""
    from recon_amd.sep_space import SpKBGATModified, batch_gat_loss
    n_ent, n_rel, D, n_pos, ratio = 120, 6, 16, 31, 2
    fn = torch.nn.MarginRankingLoss(margin=0.5)
    models, tables = [], []
    for _ in range(2):
        torch.manual_seed(4)
        m = SpKBGATModified(torch.randn(n_ent, D), torch.randn(n_rel, D), [D // 2, D], [D, D], 0.0, 0.2, [2, 2], None).to(DEV)
        with torch.no_grad():
            m.W_ent2rel.normal_(0, D ** -0.5)
        gen = torch.Generator().manual_seed(8)
        tables.append([torch.randn(n_ent, D, generator=gen).to(DEV).requires_grad_(True), (0.5 * torch.randn(n_rel, D, generator=gen)).to(DEV).requires_grad_(True)])
        models.append(m)
    init = [t.detach().clone() for t in (tables[0][0], tables[0][1], models[0].W_ent2rel)]
    opts = [torch.optim.SGD([tables[i][0], tables[i][1], models[i].W_ent2rel], lr=0.5) for i in range(2)]
    rs = np.random.RandomState(2)
    for it in range(20):
        M = n_pos * (2 * ratio + 1)
        tri = torch.from_numpy(np.stack([rs.randint(0, n_ent, M), rs.randint(0, n_rel, M), rs.randint(0, n_ent, M)], 1)).to(DEV)
        for i, f in enumerate((lambda *a: batch_gat_loss(*a, valid_invalid_ratio_gat=ratio), lambda *a: _composition(*a, ratio))):
            opts[i].zero_grad()
            f(fn, tri, tables[i][0], tables[i][1], models[i]).backward()
            opts[i].step()
    for a, b, i0 in zip((tables[0][0], tables[0][1], models[0].W_ent2rel), (tables[1][0], tables[1][1], models[1].W_ent2rel), init):
        moved, drift = float((b.detach() - i0).norm()), float((a.detach() - b.detach()).norm())
        assert moved > 0 and drift <= 1e-2 * moved, (drift, moved)


def test_sep_loss_rejections_fallbacks_and_nan():
    from recon_amd import sep_loss
    from recon_amd.sep_space import batch_gat_loss
    from recon_amd.graph import trust
    from recon_amd.gat_layers import nan_raised, enable_nan_flag
    enable_nan_flag(DEV)
    E, Rel, W, tri, n_pos, reps, margin = _case(16, 5, 2, n_ent=40)
    fn = torch.nn.MarginRankingLoss(margin=margin)
    nan_raised(DEV)                                                        # whatever an earlier test left
    clean = batch_gat_loss(fn, tri, E, Rel, _gat(W), valid_invalid_ratio_gat=reps // 2)
    assert torch.isfinite(clean) and not nan_raised(DEV)
    assert torch.equal(batch_gat_loss(fn, tri.cpu(), E, Rel, _gat(W), valid_invalid_ratio_gat=reps // 2), clean)       # CPU indices, GPU tables
    for row, col, val in ((3, 0, 40), (5, 2, -1), (7, 1, Rel.shape[0])):
        bad = tri.clone()
        bad[row, col] = val
        with pytest.raises(IndexError):
            batch_gat_loss(fn, bad, E, Rel, _gat(W), valid_invalid_ratio_gat=reps // 2)
    with pytest.raises(IndexError):                                        # a relation id must index W_ent2rel too
        batch_gat_loss(fn, tri, E, Rel, _gat(W[:-2].contiguous()), valid_invalid_ratio_gat=reps // 2)
    ok = trust(tri.clone(), bound=40, rel_bound=Rel.shape[0])              # a vouched-for tensor skips the check
    assert torch.equal(batch_gat_loss(fn, ok, E, Rel, _gat(W), valid_invalid_ratio_gat=reps // 2), clean)
    # the fallback: another loss function, another nonlinearity, another dtype, D = 513; none may reach the fused kernels
    calls = []
    orig = sep_loss._SepTransEMarginLoss.apply
    sep_loss._SepTransEMarginLoss.apply = lambda *a: calls.append(1) or orig(*a)
    try:
        other = batch_gat_loss(lambda a, b, y: torch.nn.functional.margin_ranking_loss(a, b, y, margin=margin), tri, E, Rel, _gat(W), valid_invalid_ratio_gat=reps // 2)
        torch.testing.assert_close(other, clean, rtol=1e-5, atol=1e-6)
        relu = batch_gat_loss(fn, tri, E, Rel, _gat(W, torch.relu), valid_invalid_ratio_gat=reps // 2)
        assert torch.isfinite(relu) and abs(relu.item() - clean.item()) > 1e-3
        dbl = batch_gat_loss(fn, tri, E.double(), Rel.double(), _gat(W.double()), valid_invalid_ratio_gat=reps // 2)
        assert dbl.dtype == torch.float64 and abs(dbl.item() - clean.item()) <= 1e-4 * abs(clean.item())
        gen = torch.Generator().manual_seed(1)
        Eb, Rb, Wb = torch.randn(9, 513, generator=gen).to(DEV), torch.randn(2, 513, generator=gen).to(DEV), (torch.randn(2, 513, 513, generator=gen) / 23).to(DEV).requires_grad_(True)
        tb = torch.tensor([[0, 0, 1], [2, 1, 3], [4, 1, 5]] + [[6, 0, 1], [2, 1, 7], [8, 0, 1], [2, 1, 0]] * 3, device=DEV)[:15]
        big = batch_gat_loss(fn, tb, Eb, Rb, _gat(Wb), valid_invalid_ratio_gat=2)
        big.backward()
        assert torch.isfinite(big) and Wb.grad is not None
        assert not calls
        batch_gat_loss(fn, tri, E, Rel, _gat(W), valid_invalid_ratio_gat=reps // 2)
        assert calls == [1]
    finally:
        sep_loss._SepTransEMarginLoss.apply = orig
    # a NaN row reaches the loss, fused and fallback, and raises the device word; backward, the NaN pattern of the three gradients is torch
    # autograd's of the reference expression (the fallback): c = 0 for a NaN term, sign(NaN) = 0, and 0 * (1 - NaN^2) = NaN goes through both products
    bad = E.clone()
    bad[int(tri[3, 0])] = float("nan")
    masks = []
    for f in (fn, lambda a, b, y: torch.nn.functional.margin_ranking_loss(a, b, y, margin=margin)):
        e, r, w = (t.clone().requires_grad_(True) for t in (bad, Rel, W))
        loss = batch_gat_loss(f, tri, e, r, _gat(w), valid_invalid_ratio_gat=reps // 2)
        assert torch.isnan(loss), "a NaN row must reach the loss"
        loss.backward()
        masks.append([torch.isnan(t.grad) for t in (e, r, w)])
    assert nan_raised(DEV), "the fused loss raises the device word"
    for name, a, b in zip(("g_E", "g_Rel", "g_W"), *masks):
        assert torch.equal(a, b), (name, int(a.sum()), int(b.sum()))
    assert bool(masks[0][0].any()) and bool(masks[0][2].any()) and not bool(masks[0][0].all())
