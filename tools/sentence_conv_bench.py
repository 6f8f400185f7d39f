"""recon_amd.sentence_conv_pool (csrc/sent_conv.hip) against the stock lines of models/baselines.py:237-247 (CNN) and :297-308 (PCNN) it
replaces, timed in one process.

    python tools/sentence_conv_bench.py [--rounds 7] [--out profiles/sentence_conv_bench.jsonl]

One JSON line per (form, B, p) at the reference's widths (T = 36, Dw = 50, Dp = 3, E = 256): the CNN form with windows (3, 5, 7) and tanh,
the PCNN form with k = 3 and relu, each at B = 50 (model_params.json's batch) and B = 3600 (the pairs of a batch of the graph models), each
without factors (p = 0) and with word and pooled factors of p = 0.5 (fp32 factors, the same for both paths).  Paths, alternating round by
round on the same data, both position tables, every weight and every bias requiring a gradient: `op`; `chain`, the stock lines
(tests/sentence_conv_checks.lines: the reference's own, PCNN's `.repeat` of the mask included); `fallback`, what the op and the models run
without the kernels (`sentence_conv._chain`: the same lines with the mask broadcast).  Per path: median and minimum milliseconds of the
forward alone and of forward + backward (device events), the launches of one forward + backward and torch.cuda.max_memory_allocated above the inputs.  Also the op's forward under
no_grad and the largest difference of the op's output from the chain's.  Lines are appended to --out."""
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

T, DW, DP, E = 36, 50, 3, 256
FORMS = {"cnn": (3, 5, 7), "pcnn": (3,)}
BATCHES = [50, 3600]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sentence_conv_checks import default_activation, inputs, lines as stock
    from recon_amd import sentence_conv_pool
    from recon_amd.sentence_conv import _chain
    d = torch.device("cuda:0")
    out_lines = []
    for form, ks in FORMS.items():
        for B in BATCHES:
            shape = (form, B, T, DW, DP, E, ks)
            c = inputs(shape)
            act = default_activation(shape)
            fixed = [c["sentence"].to(d), c["positions"].to(d), c["word_table"].to(d)]
            leaves = [c["pos_table_0"].to(d).requires_grad_(True), c["pos_table_1"].to(d).requires_grad_(True)]
            ws, bs = [w.to(d).requires_grad_(True) for w in c["weights"]], [b.to(d).requires_grad_(True) for b in c["biases"]]
            seg = None if c["segments"] is None else c["segments"].to(d)
            g_out = c["g_out"].to(d)

            def clear_grads():
                for t in leaves + ws + bs:
                    t.grad = None
            for p_drop in (0.0, 0.5):
                kw = dict(segments=seg, activation=act, keep=c["keep"].to(d) if p_drop else None, pool_keep=c["pool_keep"].to(d) if p_drop else None)
                paths = {"op": lambda: sentence_conv_pool(*fixed, *leaves, ws, bs, **kw), "chain": lambda: stock(*fixed, *leaves, ws, bs, **kw),
                         "fallback": lambda: _chain(*fixed, *leaves, ws, bs, **kw)}
                res, nograd = run_rounds(paths, g_out, clear_grads, a.rounds, nograd=paths["op"])
                line = {"form": form, "B": B, "T": T, "Dw": DW, "Dp": DP, "E": E, "windows": list(ks), "p": p_drop, "rounds": a.rounds,
                        "output_bytes": g_out.numel() * 4, "x_bytes": B * T * (DW + 2 * DP) * 4,
                        "conv_output_bytes": sum(B * E * (T if form == "pcnn" else T - k + 1) for k in ks) * 4}
                put_ms(line, "op_fwd_nograd_ms", nograd)
                with torch.no_grad():
                    line["max_abs_diff_op_chain"] = (paths["op"]() - paths["chain"]()).abs().max().item()
                summarise(line, res, paths, g_out, clear_grads)
                wiring_rule(line)
                line["op_median_below_fallback_min"] = line["op_fwd_bwd_ms_median"] < line["fallback_fwd_bwd_ms_min"]
                out_lines.append(json.dumps(line))
                print(out_lines[-1], flush=True)
    write_lines(a.out, out_lines)


if __name__ == "__main__":
    main()
