#!/usr/bin/env python3
"""Three float32 GraphConvolutions over a ragged batch (recon_amd/gcn_layers.py _GcnRaggedFunction, csrc/gcn_ragged.hip) beside what a float32
user had before: tools/secondary.py powerlaw_mixed_stack_bf16's batch — 64 graphs, n ~ U{16..256}, width 256, three layers — as
  ragged        the new path: x [N, 256] with a float32 RaggedAdjacency
  padded_copy   every graph padded to [B, n_max, n_max] through the dense float32 layer, the pad and unpad copies included
  padded        the same without the copies (input, result and gradient stay padded)
  host_loop     one 2-D dense call per graph and layer
  ragged_bf16   the bfloat16 ragged layer, for context
forward and forward + backward, median / minimum over alternating rounds (tools/op_bench.py), launches per layer, bytes allocated above
the inputs, and for `ragged` the aggregate kernel's time against its own bytes and FLOPs.  One JSON line per leg and one for the kernel,
appended to --out.

    python tools/gcn_ragged_bench.py --rounds 10 --out profiles/gcn_ragged_bench.jsonl"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import op_bench  # noqa: E402


def batch(B, lo, hi):
    """powerlaw_mixed_stack_bf16's graphs: sizes U{lo..hi}, min(4096, 16 n) power-law edges + identity, row-normalised; float32."""
    rs = np.random.RandomState(0)
    mats = []
    for _ in range(B):
        n = int(rs.randint(lo, hi + 1))
        e = min(4096, 16 * n)
        p = 1.0 / np.arange(1, n + 1)
        p /= p.sum()
        dl, sl = rs.choice(n, size=e, p=p), rs.randint(0, n, size=e)
        a = torch.zeros(n, n)
        a[torch.from_numpy(dl), torch.from_numpy(sl)] = 1.0
        a += torch.eye(n)
        mats.append(a / a.sum(-1, keepdim=True))
    return mats


def kernel_ms(fn, g_out, needle):
    """{kernel name: [milliseconds per launch]} of the kernels whose name holds `needle`, in one forward + backward."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn().backward(g_out)
        torch.cuda.synchronize()
    found = {}
    for ev in prof.events():
        if ev.device_type == DeviceType.CUDA and needle in ev.name:
            us = getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)
            found.setdefault(ev.name, []).append(us / 1e3)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    from recon_amd.gcn_layers import GraphConvolution, RaggedAdjacency
    dv = torch.device("cuda:0")
    mats = batch(o.graphs, 16, 256)
    sizes = [m.shape[0] for m in mats]
    B, N, D, n_max = len(sizes), sum(sizes), o.width, max(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, D, generator=g).to(dv).requires_grad_(True)
    G = torch.randn(N, D, generator=g).to(dv)
    torch.manual_seed(0)
    layers = [GraphConvolution(D, D).to(dv) for _ in range(o.layers)]
    layers16 = [GraphConvolution(D, D).to(torch.bfloat16).to(dv) for _ in range(o.layers)]
    mats_d = [m.to(dv) for m in mats]
    rag = RaggedAdjacency.from_dense(mats_d)
    rag16 = RaggedAdjacency.from_dense([m.to(torch.bfloat16) for m in mats_d])
    x16 = x.detach().to(torch.bfloat16).requires_grad_(True)
    adj_pad = torch.zeros(B, n_max, n_max, device=dv)
    for b, m in enumerate(mats_d):
        adj_pad[b, :m.shape[0], :m.shape[0]] = m
    rows = torch.cat([torch.arange(n) + b * n_max for b, n in enumerate(sizes)]).to(dv)        # the padded batch's real rows
    x_pad = torch.zeros(B * n_max, D, device=dv)
    x_pad[rows] = x.detach()
    x_pad = x_pad.view(B, n_max, D).requires_grad_(True)
    G_pad = torch.zeros(B * n_max, D, device=dv)
    G_pad[rows] = G
    G_pad = G_pad.view(B, n_max, D)

    def through(ls, h, adj):
        for l in ls:
            h = l(h, adj)
        return h

    def padded_copy():
        h = torch.zeros(B * n_max, D, device=dv).index_copy(0, rows, x).view(B, n_max, D)
        return through(layers, h, adj_pad).reshape(B * n_max, D)[rows]

    def host_loop():
        hs = [x[ptr[b]:ptr[b + 1]] for b in range(B)]
        for l in layers:
            hs = [l(h, m) for h, m in zip(hs, mats_d)]
        return torch.cat(hs)

    legs = {
        "ragged": (lambda: through(layers, x, rag), G),
        "padded_copy": (padded_copy, G),
        "padded": (lambda: through(layers, x_pad, adj_pad), G_pad),
        "host_loop": (host_loop, G),
        "ragged_bf16": (lambda: through(layers16, x16, rag16), G.to(torch.bfloat16)),
    }
    leaves = [x, x16, x_pad] + [p for l in layers + layers16 for p in l.parameters()]

    def clear():
        for t in leaves:
            t.grad = None

    res = {k: [] for k in legs}
    for rnd in range(o.rounds + 1):                       # round 0 warms up; the legs alternate within a round
        for k, (fn, g_out) in legs.items():
            clear()
            r = op_bench.timed(fn, g_out)
            if rnd:
                res[k].append(r)
    shape = dict(graphs=B, nodes=N, n_max=n_max, adj_cells=int(sum(n * n for n in sizes)), padded_adj_cells=B * n_max * n_max, width=D,
                 layers=o.layers, rounds=o.rounds)
    lines = []
    for k, rs in res.items():
        line = dict(tool="gcn_ragged_bench", leg=k, **shape)
        op_bench.put_ms(line, "fwd_ms", (r[0] for r in rs))
        op_bench.put_ms(line, "fwd_bwd_ms", (r[1] for r in rs))
        line["peak_bytes_above_inputs"] = max(r[2] for r in rs)
        clear()
        n_launch = op_bench.launches(*legs[k])
        line["launches_fwd_bwd_per_layer"] = None if n_launch is None else round(n_launch / o.layers, 1)
        lines.append(json.dumps(line))
        print(lines[-1])
    try:                                                   # the aggregate kernel against its own traffic: adj_b, the operand rows, the result rows
        clear()
        per = kernel_ms(*legs["ragged"], "k_gcn_ragged_aggregate")
        cells = shape["adj_cells"]
        for name, ms in per.items():
            masked = "ILb1ELb1" in name or "<true, true" in name
            nbytes = 4 * (cells + (3 if masked else 2) * N * D)
            flops = 2.0 * cells * D
            t = statistics.median(ms)
            line = dict(tool="gcn_ragged_bench", leg="aggregate_kernel", instance="backward" if masked else "forward", launches=len(ms),
                        ms_median=round(t, 4), ms_min=round(min(ms), 4), bytes=nbytes, flops=flops, gbytes_per_s=round(nbytes / t / 1e6, 1),
                        gflops_per_s=round(flops / t / 1e6, 1), **shape)
            lines.append(json.dumps(line))
            print(lines[-1])
    except Exception as exc:                               # no profiler: the legs above stand on their own
        print("aggregate kernel times not available: %r" % (exc,))
    op_bench.write_lines(o.out, lines)


if __name__ == "__main__":
    main()
