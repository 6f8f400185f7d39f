"""Forward + backward of recon_amd.translation_residuals (csrc/rel_trans.hip) against the op chain it replaced, timed in one process.

    python tools/translation_bench.py [--rounds 5] [--out FILE]

One JSON line per shape (M, n_out, ent_dim, rel_dim): median and minimum milliseconds of forward + backward (gradient for `rel` only, as
in RECON) and of the forward and the backward alone for the fused op, and torch.cuda.max_memory_allocated above the inputs for each path.
The two paths alternate round by round on the same random data."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(3600, 353, 200, 200), (300, 353, 200, 200)]


def timed(fn, parts=False):
    """(ms of fn(), peak bytes above what was allocated before); fn returns (out, g_out)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    out, g_out = fn()
    e[1].record()
    out.backward(g_out)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[2]), e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recon_amd import translation_residuals
    from recon_amd.translation import _chain
    d = torch.device("cuda:0")
    lines = []
    for M, n_out, ent_dim, rel_dim in SHAPES:
        g = torch.Generator().manual_seed(M)
        emb = (torch.randn(M, 2 * ent_dim, generator=g) * 0.5).to(d)
        W = (torch.randn(n_out, ent_dim, rel_dim, generator=g) / ent_dim ** 0.5).to(d)
        rel = (torch.randn(n_out, rel_dim, generator=g) * 0.5).to(d).requires_grad_(True)
        g_out = torch.randn(M, n_out, generator=g).to(d)
        head, tail = emb[:, :ent_dim], emb[:, ent_dim:]
        paths = {"fused": lambda: (translation_residuals(head, tail, W, rel), g_out), "chain": lambda: (_chain(head, tail, W, rel), g_out)}
        res = {k: [] for k in paths}
        for rnd in range(a.rounds + 1):                                   # round 0 warms up
            for k, fn in paths.items():
                rel.grad = None
                r = timed(fn)
                if rnd:
                    res[k].append(r)
        line = {"shape": [M, n_out, ent_dim, rel_dim], "rounds": a.rounds}
        for k, rs in res.items():
            for i, name in enumerate(("fwd_bwd_ms", "fwd_ms", "bwd_ms")):
                line["%s_%s_median" % (k, name)] = round(statistics.median(r[i] for r in rs), 4)
                line["%s_%s_min" % (k, name)] = round(min(r[i] for r in rs), 4)
            line["%s_peak_bytes" % k] = max(r[3] for r in rs)
        line["speedup_median"] = round(line["chain_fwd_bwd_ms_median"] / line["fused_fwd_bwd_ms_median"], 3)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
