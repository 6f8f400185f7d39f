#!/usr/bin/env python3
"""The optimizer step alone: torch.optim (what the training loops use by default) against recon_amd.optim (csrc/optim.hip), in one process,
over the parameter sets of the three training programs:

  stage_a   SpKBGATModified as tools/stage_a_iter_bench.py builds it (GAT/main.py:445-449: SGD)
  convkb    the ConvKB scorer's fc1 / fc2 as tools/kg_train_bench.py builds it (GAT/main.py:747-751: Adam, weight decay)
  stage_b   gpgnn.GPGNN with the reference's model_params.json sizes (train.py:234: Adam; :314-315: clip_grad_norm)

Per set and per variant (plain; with gradient-norm clipping: clip_grad_norm_ + step against max_grad_norm=): gradients filled once,
20 warm-up steps, 200 timed steps ending in a device synchronise, five repeats alternating which optimizer goes first.  Reported: the
per-step wall median of the five repeats, their spread (max - min), and the device launches per step.  One JSON line per set and variant,
appended to profiles/optim_bench.jsonl.

    python tools/optim_bench.py [--out profiles/optim_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from stage_a_iter_bench import count_launches  # noqa: E402

WARMUP, STEPS, REPEATS, CLIP = 20, 200, 5, 1.0
# the reference's model_params.json (the keys GPGNN reads)
STAGE_B_PARAMS = {"max_num_nodes": 9, "embedding_dim": 8, "layer_number": 3, "projection_style": "untie", "non-linear1": "relu", "non-linear": "tanh",
                  "dropout1": 0.5, "position_emb": 3, "units1": 256, "rnn1_layers": 1, "bidirectional": 1, "batch_size": 5}


def stage_a_params(dev):
    from recon_amd.models import SpKBGATModified
    torch.manual_seed(0)
    m = SpKBGATModified(torch.randn(14541, 50), torch.randn(237, 50), [100, 200], [100, 200], 0.3, 0.2, [2, 2]).to(dev)
    return m, [p for p in m.parameters() if p.requires_grad]


def convkb_params(dev):
    from recon_amd.models import SpKBGATConvOnly
    torch.manual_seed(0)
    D = 200
    m = SpKBGATConvOnly(torch.randn(14541, 8), torch.randn(237, 8), [D // 2, D], [D // 2, D], 0.0, 0.0, 0.2, 0.2, [2, 2], 50).to(dev)
    named = dict(m.named_parameters())
    return m, [named[k] for k in ("convKB.fc1.weight", "convKB.fc1.bias", "convKB.fc2.weight", "convKB.fc2.bias")]


def stage_b_params(dev):
    from recon_amd.gpgnn import GPGNN
    torch.manual_seed(0)
    emb = np.random.RandomState(0).randn(2000, 50).astype(np.float32)          # frozen (models/models.py:102-105): not part of the step
    m = GPGNN(dict(STAGE_B_PARAMS), emb, max_sent_len=36, n_out=353).to(dev)
    return m, [p for p in m.parameters() if p.requires_grad]


SETS = {"stage_a": (stage_a_params, "sgd"), "convkb": (convkb_params, "adam"), "stage_b": (stage_b_params, "adam")}


def make(kind, which, params, clip):
    from recon_amd import optim
    if which == "torch":
        opt = torch.optim.SGD(params, lr=1e-3) if kind == "sgd" else torch.optim.Adam(params, lr=1e-3, weight_decay=1e-5)
        if clip is None:
            return opt.step
        return lambda: (torch.nn.utils.clip_grad_norm_(params, clip), opt.step())
    if kind == "sgd":
        return optim.SGD(params, lr=1e-3, max_grad_norm=clip).step
    return optim.Adam(params, lr=1e-3, weight_decay=1e-5, max_grad_norm=clip).step


def wall_per_step(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / STEPS * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.jsonl"))
    ap.add_argument("--sets", default=",".join(SETS))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    for name in a.sets.split(","):
        build, kind = SETS[name]
        for clip in (None, CLIP):
            steps = {}
            for which in ("torch", "recon"):                                  # each optimizer owns a copy of the parameters, same gradients
                model, params = build(dev)
                g = torch.Generator().manual_seed(1)
                for p in params:
                    p.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(dev)
                steps[which] = (make(kind, which, params, clip), model)
            for which in steps:
                for _ in range(WARMUP):
                    steps[which][0]()
            times = {"torch": [], "recon": []}
            for r in range(REPEATS):
                for which in (("torch", "recon") if r % 2 == 0 else ("recon", "torch")):
                    times[which].append(wall_per_step(steps[which][0]))
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = max(max(v) - min(v) for v in times.values())
            line = {"set": name, "optimizer": kind, "clip": clip, "tensors": len(params), "elements": sum(p.numel() for p in params),
                    "torch_us_median": round(med["torch"], 2), "recon_us_median": round(med["recon"], 2), "spread_us": round(spread, 2),
                    "torch_us": [round(x, 2) for x in times["torch"]], "recon_us": [round(x, 2) for x in times["recon"]],
                    "torch_launches": count_launches(steps["torch"][0], iters=5), "recon_launches": count_launches(steps["recon"][0], iters=5),
                    "recon_faster_beyond_spread": bool(med["torch"] - med["recon"] > spread), "warmup": WARMUP, "steps": STEPS, "repeats": REPEATS}
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
