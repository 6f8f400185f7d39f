"""recon_amd.relation_objective (csrc/objective.hip) against the stock lines it replaces in the stage-B loops (train.py:232, :309-324), timed
in one process.

    python tools/relation_objective_bench.py [--rounds 7] [--iterations 200] [--out profiles/relation_objective_bench.jsonl]

One JSON line per M (pair rows of a batch): 360 and 3 600 (72 ordered pairs of 9 nodes at batch sizes 5, which model_params.json has, and
50) at n_out = 353, logits ~ 4 N(0, 1) requiring a gradient, labels like the reference's: about 70 % ignore_index = 0, about 20 %
empty_label = 1, the rest uniform over the other classes.  The wiring rule is taken at M = 3 600.

Device time, paths `chain` (`recon_amd.objective._chain`: F.cross_entropy, torch.max, the softmax probability of the prediction and the
counters as tensor ops) and `op`, alternating round by round on the same data: median and minimum milliseconds of the forward alone and of
forward + backward (device events), the launches of one forward + backward (kernels, memsets and copies the profiler sees on the device)
and torch.cuda.max_memory_allocated above the inputs; also the op's forward under no_grad and the bytes of its workspace.

Wall clock, `stock_loop` against `op_loop`: --iterations iterations of the objective's part of a training iteration, timed on the host
from the first call to the end of ONE final synchronise, as microseconds per iteration (median and minimum over --rounds runs).  Both
upload the batch's labels from a numpy array, as train.py:309 does, and run the loss's backward.  `stock_loop` is train.py:309-324 as it
stands: the loss, `torch.max`, two `.tolist()`s, the numpy filter and a Python count per pair (written here from
utils/evaluation_utils.py:17-59's description), `f1 += add_f1` on the host.  `op_loop` is relation_objective with a RelationMetrics and no
host read until the run's end.  Device events do not see the stall of the `.tolist()`s; this does.  Each is measured alone and again
behind --queued-ms (default 1.0) milliseconds of queued device work per iteration (square fp32 matmuls, a stand-in for the model's
forward), where a host that does not stall runs ahead of the device.  The two loops' f1 sums are compared bit for bit.  Lines are appended
to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from op_bench import put_ms, run_rounds, summarise, wiring_rule, write_lines  # noqa: E402

ROWS = [360, 3600]
N_OUT, IGNORE, EMPTY = 353, 0, 1


def instance_f1(predicted, gold, empty):
    """The batch F1 over two lists: the share of the non-empty entries of one list that the other list matches, both ways round, and
    their harmonic mean."""
    def share(first, second):
        count = hits = 0
        for a, b in zip(first, second):
            if a != empty:
                count += 1
                if a == b:
                    hits += 1
        return float(hits) / count if count > 0 else 0
    prec, rec = share(predicted, gold), share(gold, predicted)
    return 2.0 * prec * rec / (prec + rec) if prec + rec > 0 else 0


def queued_work(d, ms):
    """A function that queues about `ms` milliseconds of matmuls (None for 0), and the milliseconds it measured."""
    if ms <= 0:
        return None, 0.0
    a = torch.randn(2048, 2048, device=d)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.mm(a, a)
    torch.cuda.synchronize()
    e[0].record()
    for _ in range(20):
        torch.mm(a, a)
    e[1].record()
    torch.cuda.synchronize()
    one = e[0].elapsed_time(e[1]) / 20
    reps = max(1, round(ms / one))

    def work():
        for _ in range(reps):
            torch.mm(a, a)
    return work, reps * one


def wall_us(step, iterations, rounds):
    """Microseconds per iteration of `step(i)`, from the first call to the end of one final synchronise; round 0 warms up."""
    out = []
    for rnd in range(rounds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iterations):
            step(i)
        torch.cuda.synchronize()
        if rnd:
            out.append((time.perf_counter() - t0) / iterations * 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--queued-ms", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recon_amd import RelationMetrics, _lib, relation_objective
    from recon_amd.objective import _chain
    d = torch.device("cuda:0")
    lines = []
    for M in ROWS:
        g = torch.Generator().manual_seed(M)
        logits = (torch.randn(M, N_OUT, generator=g) * 4).to(d).requires_grad_(True)
        u = torch.rand(M, generator=g)
        other = torch.randint(2, N_OUT, (M,), generator=g)
        labels_host = torch.where(u < 0.7, torch.full((M,), IGNORE), torch.where(u < 0.9, torch.full((M,), EMPTY), other)).numpy()
        labels = torch.from_numpy(labels_host).to(d)
        g_out = torch.ones((), device=d)

        def chain():
            return _chain(logits, labels, IGNORE, EMPTY).loss

        def op():
            return relation_objective(logits, labels, IGNORE, EMPTY).loss

        def clear_grads():
            logits.grad = None

        paths = {"op": op, "chain": chain}
        res, nograd = run_rounds(paths, g_out, clear_grads, a.rounds, nograd=op)
        line = {"M": M, "n_out": N_OUT, "rounds": a.rounds, "kept_rows": int((labels_host != IGNORE).sum()),
                "non_empty_gold": int(((labels_host != IGNORE) & (labels_host != EMPTY)).sum()), "input_bytes": M * N_OUT * 4 + M * 8,
                "output_bytes": 4 + M * 8 + M * 4 + 32 + 8, "unwritten_log_softmax_bytes": M * N_OUT * 4,
                "workspace_bytes_fwd": _lib.lib().recon_relation_objective_workspace_bytes(M, N_OUT), "saved_bytes": M * 4 + 32}
        put_ms(line, "op_fwd_nograd_ms", nograd)
        with torch.no_grad():
            line["abs_diff_loss_op_chain"] = (op() - chain()).abs().item()
        summarise(line, res, paths, g_out, clear_grads)
        wiring_rule(line)
        line["op_slower_than_chain_on_device"] = line["op_fwd_bwd_ms_median"] > line["chain_fwd_bwd_ms_median"]

        # ---- wall clock per iteration: train.py:309-324 as it stands against the op with an accumulator
        loss_func = torch.nn.CrossEntropyLoss(ignore_index=IGNORE)
        metrics = RelationMetrics(d)
        host = {"f1": 0}
        for name, ms in (("alone", 0.0), ("queued", a.queued_ms)):
            work, measured = queued_work(d, ms)

            def stock_step(i):
                if work:
                    work()
                logits.grad = None
                lab = labels_host
                loss = loss_func(logits, torch.from_numpy(lab.astype(int)).view(-1).to(d))
                loss.backward()
                _, predicted = torch.max(logits, dim=1)
                lab = lab.reshape(-1).tolist()
                predicted = predicted.data.tolist()
                p_indices = np.array(lab) != 0
                predicted = np.array(predicted)[p_indices].tolist()
                lab = np.array(lab)[p_indices].tolist()
                host["f1"] += instance_f1(predicted, lab, EMPTY)

            def op_step(i):
                if work:
                    work()
                logits.grad = None
                res = relation_objective(logits, torch.from_numpy(labels_host.astype(int)).view(-1).to(d), IGNORE, EMPTY, metrics=metrics)
                res.loss.backward()

            host["f1"] = 0
            stock = wall_us(stock_step, a.iterations, a.rounds)
            f1_stock = host["f1"]
            metrics.reset()
            ours = wall_us(op_step, a.iterations, a.rounds)
            r = metrics.result()
            assert r.batches == a.iterations * (a.rounds + 1)
            line["%s_queued_ms_per_iteration" % name] = round(measured, 4)
            for k, v in (("stock_loop", stock), ("op_loop", ours)):
                line["%s_%s_us_per_iteration_median" % (k, name)] = round(statistics.median(v), 2)
                line["%s_%s_us_per_iteration_min" % (k, name)] = round(min(v), 2)
            line["%s_wall_speedup_median" % name] = round(statistics.median(stock) / statistics.median(ours), 3)
            line["%s_f1_sums_equal_bits" % name] = f1_stock == r.f1_sum
        line["iterations"] = a.iterations
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    write_lines(a.out, lines)


if __name__ == "__main__":
    main()
