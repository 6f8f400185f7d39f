"""Forward + backward of recon_amd.translation_residuals (csrc/rel_trans.hip) against the op chain it replaced, timed in one process.

    python tools/translation_bench.py [--rounds 5] [--out FILE]

One JSON line per shape (M, n_out, ent_dim, rel_dim): median and minimum milliseconds of forward + backward (gradient for `rel` only, as
in RECON) and of the forward and the backward alone for the fused op, and torch.cuda.max_memory_allocated above the inputs for each path.
The two paths alternate round by round on the same random data."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from op_bench import put_ms, run_rounds, write_lines  # noqa: E402

SHAPES = [(3600, 353, 200, 200), (300, 353, 200, 200)]


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
        paths = {"fused": lambda: translation_residuals(head, tail, W, rel), "chain": lambda: _chain(head, tail, W, rel)}
        res, _ = run_rounds(paths, g_out, lambda: setattr(rel, "grad", None), a.rounds)
        line = {"shape": [M, n_out, ent_dim, rel_dim], "rounds": a.rounds}
        for k, rs in res.items():
            put_ms(line, k + "_fwd_bwd_ms", (r[1] for r in rs))
            put_ms(line, k + "_fwd_ms", (r[0] for r in rs))
            put_ms(line, k + "_bwd_ms", (r[1] - r[0] for r in rs))        # the same two events' difference
            line["%s_peak_bytes" % k] = max(r[2] for r in rs)
        line["speedup_median"] = round(line["chain_fwd_bwd_ms_median"] / line["fused_fwd_bwd_ms_median"], 3)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    write_lines(a.out, lines, mode="w")


if __name__ == "__main__":
    main()
