"""The fixtures of the GAT_sep_space stage-A loss (tests/golden/sep_gat_loss*.npz, written by tests/golden/gen_golden_sep_gat_loss.py from the
reference's own batch_gat_loss, GAT_sep_space/main.py:347-391) against an fp64 restatement of that loss written here, and the decisiveness
margins the generator stored: a fixture whose signs or hinges fp32 rounding could flip would test nothing."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

NAMES = ["sep_gat_loss1_d8", "sep_gat_loss2_d50"]


def restated(E, Rel, W, tri, ratio, margin):
    """x [M, D], the terms before the clamp [P] and the loss of GAT_sep_space/main.py:347-391 with every triple carried into its relation's
    space once: the positives' rows are the same whichever tiled copy reads them."""
    reps = 2 * ratio
    n_pos = tri.shape[0] // (reps + 1)
    Wt = W[tri[:, 1]]
    h = torch.tanh(torch.einsum("md,mde->me", E[tri[:, 0]], Wt))
    t = torch.tanh(torch.einsum("md,mde->me", E[tri[:, 2]], Wt))
    x = h + Rel[tri[:, 1]] - t
    norm = x.abs().sum(1)
    v = norm[:n_pos].repeat(reps) - norm[n_pos:] + margin
    return x, v, v.clamp_min(0).mean()


@pytest.mark.parametrize("name", NAMES)
def test_fixture_matches_fp64_restatement(name):
    g = load_golden(name)
    E, Rel, W = (torch.from_numpy(g[k]).double().requires_grad_(True) for k in ("entity", "relation", "W_ent2rel"))
    tri = torch.from_numpy(g["train_indices"])
    x, v, loss = restated(E, Rel, W, tri, int(g["ratio"]), float(g["margin"]))
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss_fp64"])) <= 1e-12 * abs(float(g["loss_fp64"]))
    np.testing.assert_allclose(float(g["loss"]), float(loss.detach()), rtol=1e-5, atol=1e-6)
    # a term is the difference of two fp32 sums of D magnitudes: band (D + 4) eps (norm_p + norm_n + margin), not a fixed tolerance
    norm = x.detach().abs().sum(1)
    n_pos = tri.shape[0] // (2 * int(g["ratio"]) + 1)
    band = (E.shape[1] + 4) * 2.0 ** -24 * (norm[:n_pos].repeat(2 * int(g["ratio"])) + norm[n_pos:] + float(g["margin"]))
    assert bool(((torch.from_numpy(g["terms"]).double() - v.detach().clamp_min(0)).abs() <= band).all())
    np.testing.assert_allclose(g["g_entity"], E.grad.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(g["g_relation"], Rel.grad.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(g["g_W_ent2rel"], W.grad.numpy(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_decisive(name):
    g = load_golden(name)
    E, Rel, W = (torch.from_numpy(g[k]).double() for k in ("entity", "relation", "W_ent2rel"))
    x, v, _ = restated(E, Rel, W, torch.from_numpy(g["train_indices"]), int(g["ratio"]), float(g["margin"]))
    active = float((v > 0).double().mean())
    assert 0.2 <= active <= 0.8 and abs(active - float(g["active_share"])) < 1e-12
    assert float(x.abs().min()) >= 32 * float(g["x_dev_max"]) and float(g["x_abs_min"]) >= 32 * float(g["x_dev_max"])
    assert float(v.abs().min()) >= 32 * float(g["term_dev_max"]) and float(g["term_abs_min"]) >= 32 * float(g["term_dev_max"])
    assert float(g["grad_tolerance_used"]) <= 0.25                      # the reference's own fp32 gradients against fp64, share of rtol 1e-5 / atol 1e-7
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20
