#!/usr/bin/env python3
"""Training of the ConvKB scorer at FB15k-237 size (14 541 entities, 237 relations, 310 116 known triples, D = 200, batch_size_conv 64,
valid_invalid_ratio_conv 40: 5 184 rows per iteration; synthetic tables), four legs alternated in one process:

  (a) host sampler: get_iteration_batch's corruption restated in numpy + a dict of the known triples (GAT/create_batch.py:103-180), then
      the copy of the batch to the device (main.py:807-809)
  (b) device sampler: recon_amd.kg_train.corrupt_batch
  (c) torch: SpKBGATConvOnly.forward + the weighted BCE of main.py:833-840 + backward + Adam, on a device-built batch
  (d) device: kg_train.convkb_bce_loss + backward + Adam, on the same batch

Each sample times --iters back-to-back iterations between two device events (no sync inside, as in a training loop without .item());
the median over --repeats samples is reported per iteration, and an epoch (4 252 iterations) is extrapolated.  Prints one JSON line.

    python tools/kg_train_bench.py [--repeats 7] [--iters 20] [--optimizer {torch,recon}]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recon_amd import kg_train                                   # noqa: E402
from recon_amd.models import SpKBGATConvOnly                      # noqa: E402

N_ENT, N_REL, N_KNOWN, N_TRAIN, D, B, RATIO = 14541, 237, 310116, 272115, 200, 64, 40
ITERS_PER_EPOCH = (N_TRAIN + B - 1) // B


def sample(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def host_batch(train_indices, known, rs, dev):
    """The corruption half of get_iteration_batch(0) in numpy with the reference's loops and dict lookups."""
    r, n = RATIO, B
    bi = np.empty((n * (2 * r + 1), 3), np.int32)
    bv = np.empty((n * (2 * r + 1), 1), np.float32)
    bi[:n] = train_indices[:n]
    bv[:n] = 1
    ent = rs.randint(0, N_ENT, n * r)
    rel = rs.randint(0, N_REL, n * r)
    bi[n:] = np.tile(bi[:n], (2 * r, 1))
    bv[n:] = np.tile(bv[:n], (2 * r, 1))
    for i in range(n):
        for j in range(r // 2):
            c = i * (r // 2) + j
            while (ent[c], bi[n + c, 1], bi[n + c, 2]) in known:
                ent[c] = rs.randint(0, N_ENT)
            bi[n + c, 0] = ent[c]
            bv[n + c] = -1
        for j in range(r // 2):
            c = n * (r // 2) + i * (r // 2) + j
            while (bi[n + c, 0], bi[n + c, 1], ent[c]) in known:
                ent[c] = rs.randint(0, N_ENT)
            bi[n + c, 2] = ent[c]
            bv[n + c] = -1
        for j in range(r):
            c = n * r + i * r + j
            k = i * r + j
            cnt = 0
            while (bi[n + c, 0], rel[k], bi[n + c, 2]) in known:
                rel[k] = rs.randint(0, N_REL)
                cnt += 1
                if cnt >= N_REL:
                    break
            if cnt < N_REL:
                bi[n + c, 1] = rel[k]
                bv[n + c] = -1
    return torch.LongTensor(bi).to(dev), torch.FloatTensor(bv).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--optimizer", choices=["torch", "recon"], default="torch", help="leg (d)'s Adam: torch.optim.Adam or recon_amd.optim.Adam (one launch)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    n = N_KNOWN + N_KNOWN // 50
    known = torch.stack([torch.randint(0, N_ENT, (n,), generator=g), torch.randint(0, N_REL, (n,), generator=g),
                         torch.randint(0, N_ENT, (n,), generator=g)], 1)
    known = torch.unique(known, dim=0)
    known = known[torch.randperm(known.shape[0], generator=g)[:N_KNOWN]]
    train = known[:N_TRAIN]
    known_dict = {tuple(x): i for i, x in enumerate(known.tolist())}
    train_np = train.numpy().astype(np.int32)
    rs = np.random.RandomState(0)
    known_d, train_d = known.to(dev), train.to(dev).int()
    ones = torch.ones(N_TRAIN, 1, device=dev)
    filt = kg_train.TripleFilter(known_d, N_ENT, N_REL)

    models, opts = [], []
    for _ in range(2):
        torch.manual_seed(0)
        m = SpKBGATConvOnly(torch.randn(N_ENT, 8), torch.randn(N_REL, 8), [D // 2, D], [D // 2, D], 0.0, 0.0, 0.2, 0.2, [2, 2], 50).to(dev)
        m.final_entity_embeddings.requires_grad_(False)
        m.final_relation_embeddings.requires_grad_(False)
        models.append(m)
        if a.optimizer == "recon" and len(opts) == 1:                       # models[1] / opts[1] are leg (d)'s
            from recon_amd.optim import Adam
            opts.append(Adam(m.parameters(), lr=1e-3, weight_decay=1e-5))
        else:
            opts.append(torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5))
    batch = kg_train.iteration_batch(train_d, ones, 0, B, filt, RATIO)
    idx, val = batch

    def leg_a():
        host_batch(train_np, known_dict, rs, dev)

    def leg_b():
        kg_train.iteration_batch(train_d, ones, 0, B, filt, RATIO, check_ids=False)

    def leg_c():
        m, opt = models[0], opts[0]
        preds = m(None, None, idx).view(-1)
        opt.zero_grad()
        y = (val.view(-1) + 1) / 2
        w = y + (1 - y) * 1 / (RATIO * 2)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(preds, y, weight=w)
        loss.backward()
        opt.step()

    def leg_d():
        m, opt = models[1], opts[1]
        loss = kg_train.convkb_bce_loss(m, idx, val, RATIO, check_ids=False)
        opt.zero_grad()
        loss.backward()
        opt.step()

    legs = {"a": (leg_a, a.host_iters), "b": (leg_b, a.iters), "c": (leg_c, a.iters), "d": (leg_d, a.iters)}
    for fn, it in legs.values():                                         # warm-up: allocator, kernels, Adam state
        sample(fn, min(it, 3))
    times = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, (fn, it) in legs.items():
            times[k].append(sample(fn, it))
    med = {k: statistics.median(v) for k, v in times.items()}
    drift = max(float((p - q).abs().max()) for p, q in zip(models[0].convKB.parameters(), models[1].convKB.parameters()))
    print(json.dumps({
        "workload": "ConvKB training FB15k-237-sized: %d entities, %d relations, %d known, D=%d, B=%d, ratio=%d (%d rows)" % (
            N_ENT, N_REL, N_KNOWN, D, B, RATIO, B * (2 * RATIO + 1)),
        "a_host_sampler_ms": round(med["a"], 4), "b_device_sampler_ms": round(med["b"], 4),
        "c_torch_step_ms": round(med["c"], 4), "d_device_step_ms": round(med["d"], 4),
        "sampler_speedup": round(med["a"] / med["b"], 1), "step_speedup": round(med["c"] / med["d"], 2),
        "epoch_iters": ITERS_PER_EPOCH,
        "epoch_s_reference_path": round((med["a"] + med["c"]) * ITERS_PER_EPOCH / 1e3, 2),
        "epoch_s_device_path": round((med["b"] + med["d"]) * ITERS_PER_EPOCH / 1e3, 2),
        "samples_ms": {k: [round(x, 4) for x in v] for k, v in times.items()},
        "param_max_abs_diff_c_vs_d": drift, "optimizer_leg_d": a.optimizer,
    }))


if __name__ == "__main__":
    main()
