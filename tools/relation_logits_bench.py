"""recon_amd.relation_logits (csrc/rel_head.hip) against the stock lines it replaces in RECON_EAC_KGGAT.forward / RECON.forward, timed in one
process.

    python tools/relation_logits_bench.py [--rounds 7] [--out profiles/relation_logits_bench.jsonl]

One JSON line per (batch size B, form): M = 72 B pair rows (C = 72 ordered entity pairs of 9 nodes) at the reference's widths
(model_params.json: 2 d L = 48 propagation features, 2 x 200 KB-GAT columns, n_out = 353 as in negative_sampling_test).  Forms: `recon`
(blocks 48 and 400 and the scattered 353 with every row present, Mnz = M: the op's most expensive case and the one the wiring rule is
taken at), `recon_half` (Mnz = M / 2, every other row: the share of present rows in the real data is not known here), `kggat` (48, 400)
and `single` (48 alone, which the models leave to linear3).  The propagation features, the translation scores, the weight and the bias
require a gradient, the KB-GAT columns do not.  Paths: `chain`, the stock lines (`zeros`, `index_put`, `cat`, F.linear on the vendor GEMM),
and `op`, alternating round by round on the same data.  Per path: median and minimum milliseconds of the forward alone and of forward +
backward (device events), the launches of one forward + backward (kernels, memsets and copies the profiler sees on the device) and
torch.cuda.max_memory_allocated above the inputs.  Also the op's forward under no_grad, the bytes of its backward workspace, the
forward's fp32 matrix operations and the largest difference of the two paths' outputs.  Lines are appended to --out."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from op_bench import put_ms, run_rounds, summarise, wiring_rule, write_lines  # noqa: E402

BATCHES = [5, 50]
C, K_REL, K_GAT, N = 72, 48, 400, 353
#        form          dense widths     scattered width, share of present rows
FORMS = [("recon", (K_REL, K_GAT), (N, 1.0)), ("recon_half", (K_REL, K_GAT), (N, 0.5)), ("kggat", (K_REL, K_GAT), None), ("single", (K_REL,), None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recon_amd import _lib, relation_logits
    from recon_amd.relation_head import _chain
    d = torch.device("cuda:0")
    lines = []
    for B in BATCHES:
        for form, widths, sc in FORMS:
            M = B * C
            Kt = sum(widths) + (sc[0] if sc else 0)
            g = torch.Generator().manual_seed(B + Kt)
            s = 1.0 / math.sqrt(Kt)
            blocks = [torch.randn(B, C, K, generator=g).to(d).requires_grad_(i == 0) for i, K in enumerate(widths)]
            W = ((torch.rand(N, Kt, generator=g) * 2 - 1) * s).to(d).requires_grad_(True)
            b = ((torch.rand(N, generator=g) * 2 - 1) * s).to(d).requires_grad_(True)
            scattered = pos = None
            Mnz = 0
            if sc:
                pos = torch.arange(0, M, round(1 / sc[1])).to(d)
                Mnz = pos.shape[0]
                scattered = torch.randn(Mnz, sc[0], generator=g).to(d).requires_grad_(True)
            g_out = torch.randn(B, C, N, generator=g).to(d)
            leaves = [t for t in blocks + [W, b, scattered] if t is not None]

            def chain():
                return _chain(blocks, W, b, scattered, pos)

            def op():
                return relation_logits(blocks, W, b, scattered, pos)

            def clear_grads():
                for t in leaves:
                    t.grad = None

            paths = {"op": op, "chain": chain}
            res, nograd = run_rounds(paths, g_out, clear_grads, a.rounds, nograd=op)
            line = {"B": B, "C": C, "M": M, "form": form, "widths": list(widths), "K_s": sc[0] if sc else 0, "Mnz": Mnz, "Kt": Kt, "N": N,
                    "rounds": a.rounds, "input_bytes": sum(t.numel() for t in leaves) * 4, "output_bytes": M * N * 4,
                    "workspace_bytes_bwd": _lib.lib().recon_relation_logits_workspace_bytes(M, len(widths), Kt, N, 1),
                    "forward_flop": 2 * M * Kt * N}
            put_ms(line, "op_fwd_nograd_ms", nograd)
            with torch.no_grad():
                line["max_abs_diff_op_chain"] = (op() - chain()).abs().max().item()
            summarise(line, res, paths, g_out, clear_grads)
            wiring_rule(line)
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
