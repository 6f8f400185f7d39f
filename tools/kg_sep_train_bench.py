#!/usr/bin/env python3
"""Training step of the GAT_sep_space ConvKB scorer at FB15k-237 size (14 541 entities, 237 relations, 310 116 known triples, D = 200,
batch_size_conv 64, valid_invalid_ratio_conv 40: 5 184 rows per iteration; synthetic tables and W_ent2rel), three legs alternated in one
process on the same device-built batch:

  (a) shell, W_ent2rel trainable: SpKBGATConvOnly.forward(..., model_gat) + the weighted BCE of GAT_sep_space/main.py:893-901 + backward
      + Adam over model_conv's parameters, as the reference runs it (the W_ent2rel gradient is computed and never used)
  (b) the same with W_ent2rel frozen
  (c) device: kg_sep_train.sep_convkb_bce_loss + backward + Adam

Each sample times --iters back-to-back iterations between two device events; the median over --repeats samples is reported per iteration.
The losses and gradients of (b) and (c) on one seeded batch are compared as well.  Prints one JSON line.

    python tools/kg_sep_train_bench.py [--repeats 7] [--iters 20] [--legs abc]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/kg_sep_train_bench.py --repeats 1 --iters 20 --legs c      (kernel times)
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recon_amd import kg_train, kg_sep_train                     # noqa: E402
from recon_amd.sep_space import SpKBGATConvOnly                   # noqa: E402

N_ENT, N_REL, N_KNOWN, N_TRAIN, D, B, RATIO = 14541, 237, 310116, 272115, 200, 64, 40


def sample(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_loss(m, gat, idx, val):
    preds = m(None, None, idx, gat).view(-1)
    y = (val.view(-1) + 1) / 2
    return torch.nn.functional.binary_cross_entropy_with_logits(preds, y, weight=y + (1 - y) / (2 * RATIO))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--legs", default="abc")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n = N_KNOWN + N_KNOWN // 50
    known = torch.stack([torch.randint(0, N_ENT, (n,), generator=g), torch.randint(0, N_REL, (n,), generator=g),
                         torch.randint(0, N_ENT, (n,), generator=g)], 1)
    known = torch.unique(known, dim=0)
    known = known[torch.randperm(known.shape[0], generator=g)[:N_KNOWN]].to(dev)
    filt = kg_train.TripleFilter(known, N_ENT, N_REL)
    train = known[:N_TRAIN].int()
    ones = torch.ones(N_TRAIN, 1, device=dev)
    idx, val = kg_train.iteration_batch(train, ones, 1, B, filt, RATIO, generator=torch.Generator().manual_seed(1))

    torch.manual_seed(0)
    W = (torch.randn(N_REL, D, D) * (2.0 / D) ** 0.5).to(dev)
    gat_train = types.SimpleNamespace(W_ent2rel=torch.nn.Parameter(W.clone()), nonlinearity_ent2rel=torch.tanh)
    gat_frozen = types.SimpleNamespace(W_ent2rel=W.clone(), nonlinearity_ent2rel=torch.tanh)
    models, opts = {}, {}
    for leg in "abc":
        torch.manual_seed(0)
        m = SpKBGATConvOnly(torch.randn(N_ENT, 8), torch.randn(N_REL, 8), [D // 2, D], [D // 2, D], 0.0, 0.0, 0.2, 0.2, [2, 2], 50).to(dev)
        m.final_entity_embeddings.requires_grad_(False)
        m.final_relation_embeddings.requires_grad_(False)
        models[leg], opts[leg] = m, torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)

    # losses and gradients of (b) and (c) on the same batch, before any step
    fc = lambda m: [m.convKB.fc1.weight, m.convKB.fc1.bias, m.convKB.fc2.weight, m.convKB.fc2.bias]
    lb = torch_loss(models["b"], gat_frozen, idx, val)
    gb = torch.autograd.grad(lb, fc(models["b"]))
    lc = kg_sep_train.sep_convkb_bce_loss(models["c"], gat_frozen, idx, val, RATIO)
    gc = torch.autograd.grad(lc, fc(models["c"]))
    compare = {"loss_b": lb.item(), "loss_c": lc.item(), "loss_rel_diff": abs(lb.item() - lc.item()) / abs(lb.item()),
               "grad_rel_diff_max": max(float((x - y).norm() / y.norm()) for x, y in zip(gc, gb))}

    def step(leg, gat):
        m, opt = models[leg], opts[leg]
        opt.zero_grad()
        if leg == "c":
            loss = kg_sep_train.sep_convkb_bce_loss(m, gat, idx, val, RATIO, check_ids=False)
        else:
            loss = torch_loss(m, gat, idx, val)
        loss.backward()
        opt.step()
        if gat.W_ent2rel.grad is not None:
            gat.W_ent2rel.grad = None                                    # train_conv never steps model_gat; its gradient only accumulates

    legs = {"a": lambda: step("a", gat_train), "b": lambda: step("b", gat_frozen), "c": lambda: step("c", gat_frozen)}
    for k in a.legs:
        for _ in range(3):
            legs[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in a.legs}
    for _ in range(a.repeats):
        for k in a.legs:
            times[k].append(sample(legs[k], a.iters))
    res = {"rows": idx.shape[0], "D": D, "n_rel": N_REL, "iters": a.iters, "repeats": a.repeats}
    res.update({"ms_per_iter_" + k: round(statistics.median(v), 4) for k, v in times.items()})
    res.update({k: (round(v, 8) if isinstance(v, float) else v) for k, v in compare.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
