"""recon_amd.context_line_states (csrc/ctx_lstm.hip) against the stock lines it replaces in EntityEmbedding.forward, timed in one process.

    python tools/ctx_lstm_bench.py [--rounds 7] [--out profiles/ctx_lstm_bench.jsonl]

One JSON line per number of entities U: S = 32 U context lines of T = 32 words at the reference's widths (model_params.json: word vectors
of 50, char features of 50, hidden 50; a 4 000-row word table, frozen as in the stage-B models).  Paths: `chain`, the stock lines
(embedding, cat, nn.LSTM on MIOpen, the h_n reshape), and `op`, alternating round by round on the same data.  Per path: median and minimum
milliseconds of the forward alone and of forward + backward (device events), the launches of one forward + backward (kernels, memsets and
copies the profiler sees on the device) and torch.cuda.max_memory_allocated above the inputs.  Also the bytes of the op's saved state and
workspaces, and the largest difference of the two paths' outputs.  Lines are appended to --out."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from op_bench import run_rounds, summarise, wiring_rule, write_lines  # noqa: E402

ENTITIES = [45, 450]
LINES, T, DW, FC, H, VW = 32, 32, 50, 50, 50, 4000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recon_amd import _lib, context_line_states
    d = torch.device("cuda:0")
    lines = []
    for U in ENTITIES:
        S = LINES * U
        g = torch.Generator().manual_seed(U)
        torch.manual_seed(U)
        lstm = nn.LSTM(DW + FC, H, 1, batch_first=True, bidirectional=True).to(d).train()
        words = torch.randint(0, VW, (S, T), generator=g).to(d)
        table = torch.randn(VW, DW, generator=g).to(d)
        feat = torch.tanh(torch.randn(S, T, FC, generator=g)).to(d).requires_grad_(True)
        g_out = torch.randn(S, 2 * H, generator=g).to(d)

        def chain():
            _, (h_n, _) = lstm(torch.cat((F.embedding(words, table), feat), -1))
            return h_n.view(1, 2, S, H)[-1].permute(1, 0, 2).reshape(S, 2 * H)

        def op():
            return context_line_states(lstm, feat, words, table)

        def clear_grads():
            lstm.zero_grad(set_to_none=True)
            feat.grad = None

        paths = {"op": op, "chain": chain}
        res, _ = run_rounds(paths, g_out, clear_grads, a.rounds)
        geo = (S, T, DW, FC, H)
        L = _lib.lib()
        with torch.no_grad():
            diff = (op() - chain()).abs().max().item()
        line = {"entities": U, "S": S, "T": T, "Dw": DW, "Fc": FC, "H": H, "rounds": a.rounds, "input_bytes": feat.numel() * 4 + words.numel() * 8,
                "concatenated_input_bytes": S * T * (DW + FC) * 4, "lstm_output_bytes": S * T * 2 * H * 4,
                "saved_bytes": L.recon_ctx_lstm_saved_bytes(*geo), "workspace_bytes_fwd": L.recon_ctx_lstm_workspace_bytes(*geo, 0),
                "workspace_bytes_bwd": L.recon_ctx_lstm_workspace_bytes(*geo, 1), "max_abs_diff_op_chain": diff}
        summarise(line, res, paths, g_out, clear_grads)
        wiring_rule(line)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
