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
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ENTITIES = [45, 450]
LINES, T, DW, FC, H, VW = 32, 32, 50, 50, 50, 4000


def timed(fn, g_out):
    """(forward ms, forward + backward ms, peak bytes above what was allocated before) of fn() and its backward."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    out = fn()
    e[1].record()
    out.backward(g_out)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[0].elapsed_time(e[2]), torch.cuda.max_memory_allocated() - base


def launches(fn, g_out):
    """Device-side events (kernels, memsets, copies) of one forward + backward, or None where the profiler is not available."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn().backward(g_out)
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == DeviceType.CUDA)
    except Exception:                                                      # the count is a by-product: the timings do not depend on it
        return None


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

        paths = {"op": op, "chain": chain}
        res = {k: [] for k in paths}
        for rnd in range(a.rounds + 1):                                   # round 0 warms up
            for k, fn in paths.items():
                lstm.zero_grad(set_to_none=True)
                feat.grad = None
                r = timed(fn, g_out)
                if rnd:
                    res[k].append(r)
        geo = (S, T, DW, FC, H)
        L = _lib.lib()
        with torch.no_grad():
            diff = (op() - chain()).abs().max().item()
        line = {"entities": U, "S": S, "T": T, "Dw": DW, "Fc": FC, "H": H, "rounds": a.rounds, "input_bytes": feat.numel() * 4 + words.numel() * 8,
                "concatenated_input_bytes": S * T * (DW + FC) * 4, "lstm_output_bytes": S * T * 2 * H * 4,
                "saved_bytes": L.recon_ctx_lstm_saved_bytes(*geo), "workspace_bytes_fwd": L.recon_ctx_lstm_workspace_bytes(*geo, 0),
                "workspace_bytes_bwd": L.recon_ctx_lstm_workspace_bytes(*geo, 1), "max_abs_diff_op_chain": diff}
        for k, rs in res.items():
            for i, name in enumerate(("fwd_ms", "fwd_bwd_ms")):
                line["%s_%s_median" % (k, name)] = round(statistics.median(r[i] for r in rs), 4)
                line["%s_%s_min" % (k, name)] = round(min(r[i] for r in rs), 4)
            line["%s_peak_bytes" % k] = max(r[2] for r in rs)
            lstm.zero_grad(set_to_none=True)
            feat.grad = None
            line["%s_launches_fwd_bwd" % k] = launches(paths[k], g_out)
        line["speedup_fwd_bwd_median"] = round(line["chain_fwd_bwd_ms_median"] / line["op_fwd_bwd_ms_median"], 3)
        line["op_median_below_chain_min"] = line["op_fwd_bwd_ms_median"] < line["chain_fwd_bwd_ms_min"]
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
