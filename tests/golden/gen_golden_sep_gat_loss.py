"""Fixtures of the GAT_sep_space stage-A loss (tests/golden/sep_gat_loss*.npz), written where the reference tree is available.

The reference's own batch_gat_loss (GAT_sep_space/main.py:347-391) is cut out of the file where it lies with ast at generation time —
main.py trains at import time — and run against a stub `args` / CUDA = False with the reference's GAT_sep_space SpKBGATModified as
model_gat; nothing of the reference's text is stored.  Recorded: the inputs, the loss, the per-pair terms and the three gradients.

The same expression is evaluated in fp64 and the fixture is ASSERTED decisive before it is written: the hinge is active for 20 % .. 80 %
of the pairs, the smallest |x| is at least 32 times the largest |x_fp32 - x_fp64| observed, the smallest |term| (before the clamp) at
least 32 times the largest term deviation observed; and the reference's own fp32 gradients deviate from the fp64 ones by at most a quarter
of the tolerance the tests apply (rtol 1e-5, atol 1e-7: a fixture whose reference spends the tolerance itself leaves none to test with).
The observed margins go into the file; tests/test_sep_gat_loss_cpu.py re-checks them.

Two cases.  A D = 200 case was tried and is not kept: with few triples the reference's own fp32 gradient of W_ent2rel spends 0.5 - 0.6 of
the tolerance (sums of ~50 products next to cancellation), with many the smallest of the 75 000 |x| falls below 32 deviations; the device
tests cover D = 200 against fp64 bands instead.

Inputs give pre-activations of order one (E ~ N(0, 1), W ~ N(0, 1) / sqrt(D), Rel ~ 0.5 N(0, 1)): with L2-normalised entity rows and a
Xavier W_ent2rel x is about Rel and every pair is active, which tests nothing.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
SEP = os.path.join(REF, "GAT_sep_space")

#        name                  n_ent n_rel  D  heads n_pos ratio margin seed
CASES = [("sep_gat_loss1_d8", 40, 5, 8, 2, 33, 2, 0.5, 11),
         ("sep_gat_loss2_d50", 60, 4, 50, 2, 41, 3, 1.0, 12)]


def _ref_batch_gat_loss(ratio):
    path = os.path.join(SEP, "main.py")
    src = open(path).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "batch_gat_loss")
    code = "\n".join(src.split("\n")[fn.lineno - 1:fn.end_lineno])
    ns = {"torch": torch, "args": types.SimpleNamespace(valid_invalid_ratio_gat=ratio), "CUDA": False}
    exec(compile(code, path, "exec"), ns)
    return ns["batch_gat_loss"]


def _expr(E, Rel, W, tri, n_pos, reps, margin):
    """x [M, D] per triple, the terms before the clamp [P] and the loss, in the dtype of the inputs."""
    h = torch.tanh(torch.bmm(E[tri[:, 0]].unsqueeze(1), W[tri[:, 1]]).squeeze(1))
    t = torch.tanh(torch.bmm(E[tri[:, 2]].unsqueeze(1), W[tri[:, 1]]).squeeze(1))
    x = h + Rel[tri[:, 1]] - t
    norm = x.abs().sum(1)
    v = norm[:n_pos].repeat(reps) - norm[n_pos:] + margin
    return x, v, v.clamp_min(0).mean()


def main():
    for k in ("layers", "models"):
        sys.modules.pop(k, None)
    sys.path.insert(0, SEP)
    import models as sep_models
    assert sep_models.__file__.startswith(SEP)
    for name, n_ent, n_rel, D, heads, n_pos, ratio, margin, seed in CASES:
        g = torch.Generator().manual_seed(seed)
        reps = 2 * ratio
        E = torch.randn(n_ent, D, generator=g)
        Rel = 0.5 * torch.randn(n_rel, D, generator=g)
        W = torch.randn(n_rel, D, D, generator=g) / D ** 0.5
        pos = torch.stack([torch.randint(0, n_ent, (n_pos,), generator=g), torch.randint(0, n_rel, (n_pos,), generator=g),
                           torch.randint(0, n_ent, (n_pos,), generator=g)], 1)
        pos[1, 0] = pos[0, 0]                                            # duplicate entity ids, heads and tails
        pos[2, 2] = pos[0, 0]
        neg = pos.repeat(reps, 1)
        half = neg.shape[0] // 2
        neg[:half, 0] = torch.randint(0, n_ent, (half,), generator=g)
        neg[half:, 2] = torch.randint(0, n_ent, (neg.shape[0] - half,), generator=g)
        tri = torch.cat([pos, neg])
        torch.manual_seed(seed)
        m = sep_models.SpKBGATModified(torch.randn(n_ent, D), torch.randn(n_rel, D), [D // heads, D], [D, D], 0.0, 0.2, [heads, heads], None)
        assert tuple(m.W_ent2rel.shape) == (n_rel, D, D) and m.nonlinearity_ent2rel is torch.tanh
        with torch.no_grad():
            m.W_ent2rel.copy_(W)
        Eg, Rg = E.clone().requires_grad_(True), Rel.clone().requires_grad_(True)
        loss = _ref_batch_gat_loss(ratio)(torch.nn.MarginRankingLoss(margin=margin), tri, Eg, Rg, m)
        loss.backward()
        x32, v32, l32 = _expr(E, Rel, W, tri, n_pos, reps, margin)
        x64, v64, l64 = _expr(E.double(), Rel.double(), W.double(), tri, n_pos, reps, margin)
        assert abs(float(l32) - float(loss.detach())) <= 1e-6 * abs(float(loss.detach())), (float(l32), float(loss.detach()))
        active = float((v64 > 0).double().mean())
        x_dev, x_min = float((x32.double() - x64).abs().max()), float(x64.abs().min())
        v_dev, v_min = float((v32.double() - v64).abs().max()), float(v64.abs().min())
        assert 0.2 <= active <= 0.8, (name, active)
        assert x_min >= 32 * x_dev, (name, x_min, x_dev)
        assert v_min >= 32 * v_dev, (name, v_min, v_dev)
        E64, R64, W64 = (t.double().requires_grad_(True) for t in (E, Rel, W))
        _expr(E64, R64, W64, tri, n_pos, reps, margin)[2].backward()
        used = max(float(((a - b.grad).abs() / (1e-7 + 1e-5 * b.grad.abs())).max()) for a, b in ((Eg.grad, E64), (Rg.grad, R64), (m.W_ent2rel.grad, W64)))
        assert used <= 0.25, (name, used)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, entity=E.numpy(), relation=Rel.numpy(), W_ent2rel=W.numpy(), train_indices=tri.numpy(), ratio=np.int32(ratio),
                            margin=np.float64(margin), loss=loss.detach().numpy(), terms=v32.clamp_min(0).numpy(), g_entity=Eg.grad.numpy(),
                            g_relation=Rg.grad.numpy(), g_W_ent2rel=m.W_ent2rel.grad.numpy(), loss_fp64=np.float64(float(l64)),
                            active_share=np.float64(active), x_abs_min=np.float64(x_min), x_dev_max=np.float64(x_dev),
                            term_abs_min=np.float64(v_min), term_dev_max=np.float64(v_dev), grad_tolerance_used=np.float64(used))
        print("wrote %-24s %7.1f KB  active %.2f  |x| min %.2e / dev %.2e  |term| min %.2e / dev %.2e"
              % (name + ".npz", os.path.getsize(path) / 1024, active, x_min, x_dev, v_min, v_dev))


if __name__ == "__main__":
    main()
