"""recon_amd.char_word_features (csrc/char_cnn.hip) against the stock sequence it replaced in EntityEmbedding.forward, timed in one process.

    python tools/char_features_bench.py [--rounds 5] [--out profiles/char_features_bench.jsonl]

One JSON line per (entities U, mode): S = 32 U sequences of 32 words at the reference's widths (model_params.json: char_embed_dim 50,
char_feature_size 50, conv_filter_size 3, max_char_len 10; 90 characters).  Modes: eval (no dropout: the table form) and train (p = 0.5:
the stock path is dropout(embedding(chars)); the op's path draws the factors on a ones tensor, as CharEmbeddings.draw_keep does, and
hands them over as `keep`, which runs the stock chain; a third path, op_packed, draws packed bits with draw_packed_keep, the draw inside
the timed region, and runs the masked kernels of csrc/char_mask.hip).  Per path: median and minimum milliseconds of the forward alone and
of forward + backward (device events), the launches of one forward + backward (kernels, memsets and copies the profiler sees on the
device) and torch.cuda.max_memory_allocated above the inputs; for op_packed also the draw alone.  The paths alternate round by round on
the same data.  Lines are appended to --out."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from op_bench import run_rounds, summarise, write_lines  # noqa: E402

ENTITIES = [45, 450]
LINES, WORDS, MAX_CHAR, CFS, C, FO, V, P = 32, 32, 10, 3, 50, 50, 90, 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recon_amd import _lib, char_word_features
    from recon_amd.char_features import draw_packed_keep
    d = torch.device("cuda:0")
    span = MAX_CHAR + CFS - 1
    lines = []
    for U in ENTITIES:
        S = LINES * U
        g = torch.Generator().manual_seed(U)
        lens = torch.randint(1, MAX_CHAR + 1, (S, WORDS), generator=g)
        live = (torch.arange(span)[None, None, :] < lens[:, :, None]) & (torch.arange(WORDS)[None, :, None] < torch.randint(0, WORDS + 1, (S, 1, 1), generator=g))
        chars = torch.zeros(S, CFS - 1 + WORDS * span, dtype=torch.int64)
        chars[:, :WORDS * span] = (torch.randint(1, V, (S, WORDS, span), generator=g) * live).view(S, -1)
        chars = chars.to(d)
        E = torch.randn(V, C, generator=g)
        E[0] = 0
        E = E.to(d).requires_grad_(True)
        Wc = (torch.randn(FO, C, CFS, generator=g) * (2.0 / (C * CFS + FO * CFS)) ** 0.5).to(d).requires_grad_(True)
        b = (0.1 * torch.randn(FO, generator=g)).to(d).requires_grad_(True)
        g_out = torch.randn(S, WORDS, FO, generator=g).to(d)
        Lc = chars.shape[1]

        def stock(train):
            x = F.dropout(F.embedding(chars, E, padding_idx=0), P, train).permute(0, 2, 1)
            return torch.tanh(F.max_pool1d(F.conv1d(x, Wc, b), span, span)).permute(0, 2, 1)

        def op(train):
            keep = F.dropout(torch.ones(S, Lc, C, device=d), P, True) if train else None
            return char_word_features(chars, E, Wc, b, span, keep=keep)

        def op_packed():
            return char_word_features(chars, E, Wc, b, span, keep=draw_packed_keep(S, Lc, C, P, d))

        def draw_ms():
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            e[0].record()
            draw_packed_keep(S, Lc, C, P, d)
            e[1].record()
            torch.cuda.synchronize()
            return e[0].elapsed_time(e[1])

        def clear_grads():
            E.grad = Wc.grad = b.grad = None

        for mode in ("eval", "train"):
            paths = {"op": lambda: op(mode == "train"), "chain": lambda: stock(mode == "train")}
            if mode == "train":
                paths["op_packed"] = op_packed
            res, _ = run_rounds(paths, g_out, clear_grads, a.rounds)
            geo = (S, WORDS, span, CFS, V, C, FO)
            line = {"entities": U, "S": S, "words": WORDS, "mode": mode, "rounds": a.rounds,
                    "compulsory_bytes": chars.numel() * 8 + S * WORDS * FO * 4, "gathered_embedding_bytes": S * Lc * C * 4,
                    "workspace_bytes_fwd": _lib.lib().recon_char_features_workspace_bytes(*geo, 0),
                    "workspace_bytes_bwd": _lib.lib().recon_char_features_workspace_bytes(*geo, 1)}
            summarise(line, res, paths, g_out, clear_grads)
            if mode == "train":
                geo_m = _lib.lib().recon_char_masked_workspace_bytes
                line.update({"packed_bits_bytes": S * Lc * ((C + 31) // 32) * 4, "packed_workspace_bytes_fwd": geo_m(*geo, 0),
                             "packed_workspace_bytes_bwd": geo_m(*geo, 1),
                             "op_packed_draw_ms_median": round(statistics.median(draw_ms() for _ in range(a.rounds + 1)), 4),
                             "speedup_packed_fwd_bwd_median": round(line["chain_fwd_bwd_ms_median"] / line["op_packed_fwd_bwd_ms_median"], 3)})
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
