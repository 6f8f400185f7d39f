"""recon_amd.pair_transitions (csrc/pair_trans.hip) against the stock lines it replaces in GPGNN.forward / RECON_EAC.relation_features, timed
in one process.

    python tools/transitions_bench.py [--rounds 7] [--out profiles/transitions_bench.jsonl]

One JSON line per (batch size B, projection style): M = 72 B pair states (C = 72 ordered entity pairs of 9 nodes) of K = 512 at the
reference's widths (model_params.json: units1 = 256, embedding_dim = 8, so N1 = 256), untied with L = 3 projections under relu and tied
with L = 1 under tanh.  Paths: `chain`, the stock lines (per layer nn.Linear's F.linear on the vendor GEMM, then the activation), and `op`,
alternating round by round on the same data, x and every parameter requiring a gradient.  Per path: median and minimum milliseconds of the
forward alone and of forward + backward (device events), the launches of one forward + backward (kernels, memsets and copies the profiler
sees on the device) and torch.cuda.max_memory_allocated above the inputs.  Also the op's forward under no_grad, the bytes of its backward
workspace, the forward's fp32 matrix operations and the largest difference of the two paths' outputs.  Lines are appended to --out."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BATCHES = [5, 50]
STYLES = [("untied", 3, "relu"), ("tied", 1, "tanh")]
C, K, N1 = 72, 512, 256


def timed(fn, g_outs):
    """(forward ms, forward + backward ms, peak bytes above what was allocated before) of fn() and its backward."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    outs = fn()
    e[1].record()
    torch.autograd.backward(list(outs), g_outs)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[0].elapsed_time(e[2]), torch.cuda.max_memory_allocated() - base


def timed_forward(fn):
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    with torch.no_grad():
        fn()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1])


def launches(fn, g_outs):
    """Device-side events (kernels, memsets, copies) of one forward + backward, or None where the profiler is not available."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            torch.autograd.backward(list(fn()), g_outs)
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == DeviceType.CUDA)
    except Exception:                                                      # the count is a by-product: the timings do not depend on it
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recon_amd import _lib, pair_transitions
    d = torch.device("cuda:0")
    lines = []
    for B in BATCHES:
        for style, L, act in STYLES:
            g = torch.Generator().manual_seed(B + L)
            s = 1.0 / math.sqrt(K)
            x = torch.randn(B, C, K, generator=g).to(d).requires_grad_(True)
            Ws = [((torch.rand(N1, K, generator=g) * 2 - 1) * s).to(d).requires_grad_(True) for _ in range(L)]
            bs = [((torch.rand(N1, generator=g) * 2 - 1) * s).to(d).requires_grad_(True) for _ in range(L)]
            g_outs = [torch.randn(B, C, N1, generator=g).to(d) for _ in range(L)]
            leaves = [x] + Ws + bs

            def chain():
                outs = []
                for W, b in zip(Ws, bs):
                    T = F.linear(x, W, b)
                    if act != "linear":
                        T = getattr(F, act)(T)
                    outs.append(T)
                return outs

            def op():
                return pair_transitions(x, Ws, bs, act)

            paths = {"op": op, "chain": chain}
            res = {k: [] for k in paths}
            nograd = []
            for rnd in range(a.rounds + 1):                               # round 0 warms up
                for k, fn in paths.items():
                    for t in leaves:
                        t.grad = None
                    r = timed(fn, g_outs)
                    if rnd:
                        res[k].append(r)
                t = timed_forward(op)
                if rnd:
                    nograd.append(t)
            M = B * C
            lib = _lib.lib()
            line = {"B": B, "C": C, "M": M, "K": K, "N1": N1, "L": L, "style": style, "act": act, "rounds": a.rounds,
                    "input_bytes": sum(t.numel() for t in leaves) * 4, "output_bytes": L * M * N1 * 4,
                    "workspace_bytes_bwd": lib.recon_pair_transitions_workspace_bytes(M, K, N1, L, 1), "forward_flop": 2 * M * K * N1 * L,
                    "op_fwd_nograd_ms_median": round(statistics.median(nograd), 4), "op_fwd_nograd_ms_min": round(min(nograd), 4)}
            with torch.no_grad():
                line["max_abs_diff_op_chain"] = max((u - v).abs().max().item() for u, v in zip(op(), chain()))
            for k, rs in res.items():
                for i, name in enumerate(("fwd_ms", "fwd_bwd_ms")):
                    line["%s_%s_median" % (k, name)] = round(statistics.median(r[i] for r in rs), 4)
                    line["%s_%s_min" % (k, name)] = round(min(r[i] for r in rs), 4)
                line["%s_peak_bytes" % k] = max(r[2] for r in rs)
                for t in leaves:
                    t.grad = None
                line["%s_launches_fwd_bwd" % k] = launches(paths[k], g_outs)
            line["speedup_fwd_bwd_median"] = round(line["chain_fwd_bwd_ms_median"] / line["op_fwd_bwd_ms_median"], 3)
            line["op_median_below_chain_min"] = line["op_fwd_bwd_ms_median"] < line["chain_fwd_bwd_ms_min"]
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
