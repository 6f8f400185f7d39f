"""recon_amd.pair_sentence_states (csrc/sent_lstm.hip) against the stock lines it replaces in GPGNN.encode, timed in one process.

    python tools/sent_lstm_bench.py [--rounds 7] [--out profiles/sent_lstm_bench.jsonl]

One JSON line per (batch size B, dropout p): S = 72 B sequences (C = 72 ordered entity pairs of 9 nodes) of T = 36 words at the reference's
widths (train.py, model_params.json: word vectors of 50, position vectors of 3, hidden 256; a 4 000-row word table, frozen as in every
stage-B model).  Paths: `chain`, the stock lines (the sentence copied per pair, both embeddings, nn.Dropout at p > 0, cat, nn.LSTM on
MIOpen, the two rows), and `op` (at p > 0 with its own packed draw, `draw_packed_keep`, inside the timed region), alternating round by
round on the same data.  Per path: median and minimum milliseconds of the forward alone and of forward + backward (device events), the
launches of one forward + backward (kernels, memsets and copies the profiler sees on the device) and torch.cuda.max_memory_allocated above
the inputs.  Also the op's forward under no_grad (nothing saved), the bytes of its saved state and workspaces, the forward's fp32 matrix
operations, and without dropout the largest difference of the two paths' outputs.  Lines are appended to --out."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from op_bench import put_ms, run_rounds, summarise, wiring_rule, write_lines  # noqa: E402

BATCHES = [5, 50]
DROPOUT = [0.0, 0.5]
C, T, DW, P, H, VW, VP = 72, 36, 50, 3, 256, 4000, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recon_amd import _lib, pair_sentence_states
    from recon_amd.char_features import draw_packed_keep
    d = torch.device("cuda:0")
    lines = []
    for B in BATCHES:
        for p in DROPOUT:
            g = torch.Generator().manual_seed(B)
            torch.manual_seed(B)
            rnn = nn.LSTM(DW + P, H, 1, batch_first=True, bidirectional=True).to(d).train()
            sentence = torch.randint(0, VW, (B, T), generator=g).to(d)
            markers = torch.randint(0, VP, (B, C, T), generator=g).to(d)
            table = torch.randn(VW, DW, generator=g).to(d)
            pos = torch.randn(VP, P, generator=g).to(d).requires_grad_(True)
            g_out = torch.randn(B, C, 2 * H, generator=g).to(d)
            drop = nn.Dropout(p).train()

            def chain():
                expanded = torch.transpose(sentence.expand(C, B, T), 0, 1)
                word = drop(F.embedding(expanded.contiguous().view(-1, T), table, padding_idx=0).view(B, C, T, -1))
                posv = F.embedding(markers.contiguous().view(-1, T), pos, padding_idx=0).view(B, C, T, -1)
                merged = torch.cat([word, posv], dim=3)
                rnn_output, _ = rnn(merged.view(-1, T, merged.size(-1)))
                return torch.cat([rnn_output[:, -1, :H], rnn_output[:, 0, H:]], dim=1).view(B, C, -1)

            def op():
                keep = draw_packed_keep(B * C, T, DW, p, d) if p > 0 else None
                return pair_sentence_states(rnn, sentence, markers, table, pos, keep)

            def clear_grads():
                rnn.zero_grad(set_to_none=True)
                pos.grad = None

            paths = {"op": op, "chain": chain}
            res, nograd = run_rounds(paths, g_out, clear_grads, a.rounds, nograd=op)
            geo = (B, C, T, DW, P, H)
            L = _lib.lib()
            flop = 2 * B * C * T * 2 * (DW + P + H) * 4 * H
            line = {"B": B, "C": C, "S": B * C, "T": T, "Dw": DW, "P": P, "H": H, "dropout": p, "rounds": a.rounds,
                    "input_bytes": sentence.numel() * 8 + markers.numel() * 8, "concatenated_input_bytes": B * C * T * (DW + P) * 4,
                    "lstm_output_bytes": B * C * T * 2 * H * 4, "saved_bytes": L.recon_sent_lstm_saved_bytes(*geo),
                    "workspace_bytes_fwd": L.recon_sent_lstm_workspace_bytes(*geo, VP, 0),
                    "workspace_bytes_bwd": L.recon_sent_lstm_workspace_bytes(*geo, VP, 1), "forward_flop": flop}
            put_ms(line, "op_fwd_nograd_ms", nograd)
            if p == 0:
                with torch.no_grad():
                    line["max_abs_diff_op_chain"] = (op() - chain()).abs().max().item()
            summarise(line, res, paths, g_out, clear_grads)
            wiring_rule(line)
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
