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
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from op_bench import put_ms, run_rounds, summarise, wiring_rule, write_lines  # noqa: E402

BATCHES = [5, 50]
STYLES = [("untied", 3, "relu"), ("tied", 1, "tanh")]
C, K, N1 = 72, 512, 256


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

            def clear_grads():
                for t in leaves:
                    t.grad = None

            paths = {"op": op, "chain": chain}
            res, nograd = run_rounds(paths, g_outs, clear_grads, a.rounds, nograd=op)
            M = B * C
            lib = _lib.lib()
            line = {"B": B, "C": C, "M": M, "K": K, "N1": N1, "L": L, "style": style, "act": act, "rounds": a.rounds,
                    "input_bytes": sum(t.numel() for t in leaves) * 4, "output_bytes": L * M * N1 * 4,
                    "workspace_bytes_bwd": lib.recon_pair_transitions_workspace_bytes(M, K, N1, L, 1), "forward_flop": 2 * M * K * N1 * L}
            put_ms(line, "op_fwd_nograd_ms", nograd)
            with torch.no_grad():
                line["max_abs_diff_op_chain"] = max((u - v).abs().max().item() for u, v in zip(op(), chain()))
            summarise(line, res, paths, g_outs, clear_grads)
            wiring_rule(line)
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
