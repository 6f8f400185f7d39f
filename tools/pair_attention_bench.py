"""recon_amd.pair_context_attention (csrc/pair_attn.hip) against the batched torch form and against the loop of models/baselines.py:86-111
it replaces in ContextAware.forward, timed in one process.

    python tools/pair_attention_bench.py [--rounds 7] [--out profiles/pair_attention_bench.jsonl]

One JSON line per batch size B at the reference's widths (C = 72 ordered pairs of 9 nodes, D = 2 units1 = 512).  Paths, alternating
round by round on the same data, states and weight requiring a gradient: `op`; `chain`, the batched torch form (`pair_attention._chain`:
matmul, bmm, masked_fill, softmax, bmm, cat); `loop`, the reference's loop as it stands (tests/pair_attention_checks.loop).  Per path:
median and minimum milliseconds of the forward alone and of forward + backward (device events), the launches of one forward + backward
(kernels, memsets and copies the profiler sees on the device) and torch.cuda.max_memory_allocated above the inputs.  Also the op's forward
under no_grad, the ratio of the loop's median to the op's and the largest difference of the op's output from the other two.  Lines are
appended to --out."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from op_bench import put_ms, run_rounds, summarise, wiring_rule, write_lines  # noqa: E402

BATCHES = [5, 50]
C, D = 72, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pair_attention_checks import inputs, loop
    from recon_amd import _lib, pair_context_attention
    from recon_amd.pair_attention import _chain
    d = torch.device("cuda:0")
    lines = []
    for B in BATCHES:
        states, weight, g_out = inputs(B, C, D)
        states, weight, g_out = states.to(d).requires_grad_(True), weight.to(d).requires_grad_(True), g_out.to(d)
        leaves = [states, weight]

        def clear_grads():
            for t in leaves:
                t.grad = None

        paths = {"op": lambda: pair_context_attention(states, weight), "chain": lambda: _chain(states, weight), "loop": lambda: loop(states, weight)}
        res, nograd = run_rounds(paths, g_out, clear_grads, a.rounds, nograd=paths["op"])
        line = {"B": B, "C": C, "D": D, "rounds": a.rounds, "input_bytes": sum(t.numel() for t in leaves) * 4, "output_bytes": B * C * 2 * D * 4,
                "saved_p_bytes": B * C * C * 4, "workspace_bytes_bwd": _lib.lib().recon_pair_attention_workspace_bytes(B, C, D, 1),
                "loop_cat_bytes_fwd": C * B * (C - 1) * D * 4}
        put_ms(line, "op_fwd_nograd_ms", nograd)
        with torch.no_grad():
            out = paths["op"]()
            line["max_abs_diff_op_chain"] = (out - paths["chain"]()).abs().max().item()
            line["max_abs_diff_op_loop"] = (out - paths["loop"]()).abs().max().item()
        summarise(line, res, paths, g_out, clear_grads)
        line["speedup_over_loop_fwd_bwd_median"] = round(line["loop_fwd_bwd_ms_median"] / line["op_fwd_bwd_ms_median"], 3)
        wiring_rule(line)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
