"""recon_amd.entity_line_pool (csrc/line_pool.hip) against the stock lines it replaces in EntityEmbedding.forward, timed in one process.

    python tools/line_pool_bench.py [--rounds 7] [--out profiles/line_pool_bench.jsonl]

One JSON line per U (entities of a batch): 45 and 450 (up to 9 entities per graph at batch sizes 5, which model_params.json has, and 50)
at the reference's widths (train.py:253: 32 context lines; model_params.json: 2 x 50 line-state channels, entity_embed_dim 8,
entity_conv_filter_size 1), suffix masks with 1..32 valid lines, every input requiring a gradient.  The wiring rule is taken at U = 450.  Paths: `chain`, the stock lines (permute, the vendor convolution, `masked_fill`, `max`),
and `op`, alternating round by round on the same data.  Per path: median and minimum milliseconds of the forward alone and of forward +
backward (device events), the launches of one forward + backward (kernels, memsets and copies the profiler sees on the device) and
torch.cuda.max_memory_allocated above the inputs.  Also the op's forward under no_grad, the bytes of its backward workspace, the bytes of
the [U, E, P] tensor it does not write and the largest difference of the two paths' outputs.  Lines are appended to --out."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from op_bench import put_ms, run_rounds, summarise, wiring_rule, write_lines  # noqa: E402

ENTITIES = [45, 450]
LN, C, E, K = 32, 100, 8, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recon_amd import _lib, entity_line_pool
    from recon_amd.line_pool import _chain
    d = torch.device("cuda:0")
    lines = []
    for U in ENTITIES:
        g = torch.Generator().manual_seed(U)
        P, s = LN - K + 1, 1.0 / math.sqrt(C * K)
        states = torch.randn(U, LN, C, generator=g).to(d).requires_grad_(True)
        weight = ((torch.rand(E, C, K, generator=g) * 2 - 1) * s).to(d).requires_grad_(True)
        bias = ((torch.rand(E, generator=g) * 2 - 1) * s).to(d).requires_grad_(True)
        mask = (torch.arange(P)[None, :] >= torch.randint(1, P + 1, (U, 1), generator=g)).to(d)
        g_out = torch.randn(U, E, generator=g).to(d)
        leaves = [states, weight, bias]

        def chain():
            return _chain(states, weight, bias, mask)

        def op():
            return entity_line_pool(states, weight, bias, mask)

        def clear_grads():
            for t in leaves:
                t.grad = None

        paths = {"op": op, "chain": chain}
        res, nograd = run_rounds(paths, g_out, clear_grads, a.rounds, nograd=op)
        line = {"U": U, "Ln": LN, "C": C, "E": E, "k": K, "rounds": a.rounds, "input_bytes": sum(t.numel() for t in leaves) * 4 + mask.numel(),
                "output_bytes": U * E * 4, "unwritten_conv_bytes": U * E * P * 4,
                "workspace_bytes_bwd": _lib.lib().recon_line_pool_workspace_bytes(U, LN, C, E, K), "forward_flop": 2 * U * P * C * K * E}
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
