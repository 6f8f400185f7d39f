"""Forward + backward of the GAT_sep_space stage-A loss at the stage-A size (14 541 entities, 237 relations with 1 / k sizes, D = 200, 2 000
positives, ratio 2), three legs alternated in one process, device events, the median of 7 samples of 20 iterations each:

  a  the composition the package offered before: rel_rows_mm four times plus torch ops, positives tiled as the reference tiles them
  b  the same with the positives carried into relation space once (deduplicated by hand)
  c  recon_amd.sep_space.batch_gat_loss

    python tools/sep_gat_loss_bench.py                 # one JSON line
    python tools/sep_gat_loss_bench.py --only c --samples 1 --iters 5      # what a kernel trace wraps
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", default="abc")
    a = ap.parse_args()
    from recon_amd.graph import trust
    from recon_amd.sep_space import batch_gat_loss, rel_rows_mm
    dev = torch.device("cuda:0")
    n_ent, n_rel, D, n_pos, ratio = 14541, 237, 200, 2000, 2
    reps = 2 * ratio
    M = n_pos * (reps + 1)
    w = 1.0 / np.arange(1, n_rel + 1)
    sizes = np.floor(M * w / w.sum()).astype(np.int64)
    sizes[0] += M - sizes.sum()
    rs = np.random.RandomState(0)
    tri = np.stack([rs.randint(0, n_ent, M), np.repeat(np.arange(n_rel), sizes)[rs.permutation(M)], rs.randint(0, n_ent, M)], 1)
    tri = trust(torch.from_numpy(tri).to(dev), bound=n_ent, rel_bound=n_rel)        # as the sampler vouches for its batches: no host read
    gen = torch.Generator().manual_seed(0)
    E = torch.randn(n_ent, D, generator=gen).to(dev).requires_grad_(True)
    Rel = (0.5 * torch.randn(n_rel, D, generator=gen)).to(dev).requires_grad_(True)
    W = (torch.randn(n_rel, D, D, generator=gen) / D ** 0.5).to(dev).requires_grad_(True)
    gat = type("Gat", (), {"W_ent2rel": W, "nonlinearity_ent2rel": torch.tanh})
    fn = torch.nn.MarginRankingLoss(margin=1.0)
    y = -torch.ones(reps * n_pos, device=dev)
    rel_col = trust(tri[:, 1].contiguous(), bound=n_rel)
    pos_t = tri[:n_pos].repeat(reps, 1)
    pos_rel = trust(pos_t[:, 1].contiguous(), bound=n_rel)

    def norm(t, r):
        h = torch.tanh(rel_rows_mm(E[t[:, 0]], r, W))
        tl = torch.tanh(rel_rows_mm(E[t[:, 2]], r, W))
        return torch.norm(h + Rel[t[:, 1]] - tl, p=1, dim=1)

    def leg_a():
        return fn(norm(pos_t, pos_rel), norm(tri[n_pos:], rel_col[n_pos:]), y)

    def leg_b():
        return fn(norm(tri[:n_pos], rel_col[:n_pos]).repeat(reps), norm(tri[n_pos:], rel_col[n_pos:]), y)

    def leg_c():
        return batch_gat_loss(fn, tri, E, Rel, gat, valid_invalid_ratio_gat=ratio)

    legs = {k: f for k, f in (("a", leg_a), ("b", leg_b), ("c", leg_c)) if k in a.only}

    def step(f):
        E.grad = Rel.grad = W.grad = None
        loss = f()
        loss.backward()
        return loss

    first = {}
    for k, f in legs.items():                                                         # warm-up, and the bits of a step
        for _ in range(3):
            loss = step(f)
        first[k] = [t.clone() for t in (loss.detach(), E.grad, Rel.grad, W.grad)]
    times = {k: [] for k in legs}
    for _ in range(a.samples):
        for k, f in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                loss = step(f)
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) * 1e3 / a.iters)
    out = {"shape": {"n_ent": n_ent, "n_rel": n_rel, "D": D, "n_pos": n_pos, "ratio": ratio, "largest_relation": int(sizes[0])},
           "samples": a.samples, "iters": a.iters}
    for k in legs:
        out[k] = {"median_us": float(np.median(times[k])), "min_us": float(np.min(times[k])), "max_us": float(np.max(times[k]))}
    if "c" in legs:
        again = [loss.detach(), E.grad, Rel.grad, W.grad] if list(legs)[-1] == "c" else None
        if again is not None:
            out["c"]["bitwise_equal_to_first_step"] = all(torch.equal(x.view(torch.int32), y_.view(torch.int32)) for x, y_ in zip(first["c"], again))
        if "a" in legs:
            out["c"]["loss_minus_a"] = float(first["c"][0] - first["a"][0])
            out["accepted_c_median_below_a_min"] = out["c"]["median_us"] < out["a"]["min_us"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
