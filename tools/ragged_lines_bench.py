"""A stage-B training iteration of `RECON` at the reference's widths with the batcher's padded entity-context batch against its ragged one
(`ContextBatcher.batch(..., ragged_lines=True)`), both legs in one process.

The model, the optimizer and the sentences are tools/stage_b_iter_bench.py's (batch 50, n = 9 nodes, T = 36 tokens, packed word and char
dropout, `recon_amd.optim.Adam(max_grad_norm=0.25)`, `run_epoch` from device-resident data).  Three synthetic context tables over the
same entities, each with 31 table lines for ALL_ZERO — unique entity 0 of every batch — so that every batch has one 32-line entity and
P_b = 32:

    a  every entity has 32 lines (the surface form and 31 table lines): nothing to leave out
    b  line counts uniform in 2 .. 12
    c  line counts uniform in 1 .. 4

Per table: milliseconds per training iteration of either leg (an epoch's wall clock, ending in a synchronize, over its iterations; the
legs alternate round by round, round 0 warms up and is dropped), device launches per iteration, the share of present lines, and the
conditions of the issue: (a) the ragged median exceeds the padded median by no more than the padded leg's median - minimum; (b), (c) the
ragged median lies below the padded minimum (the wiring rule of section 28).

    python tools/ragged_lines_bench.py [--rounds 7] [--out profiles/ragged_lines_bench.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -o ragged_lines -- python tools/ragged_lines_bench.py --profile-epochs 2      # a run of its own
    python tools/ragged_lines_bench.py --condense DIR/ragged_lines_results.db [--out profiles/ragged_lines_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from context_batch_checks import build, random_batch, random_dataset  # noqa: E402
from op_bench import put_ms, write_lines  # noqa: E402
from stage_a_iter_bench import count_launches  # noqa: E402
from stage_b_iter_bench import N_OUT, N_WORDS, PARAMS, make_model  # noqa: E402

TABLES = {"a_all_32": (32, 32), "b_2_to_12": (2, 12), "c_1_to_4": (1, 4)}
ENCODER = ("k_char_", "k_keep_bits", "k_ctx_lstm_", "k_lp_")            # the entity-context encoder's kernels, by name


def set_line_counts(ds, rng, lo, hi):
    """Every entity's context rewritten to a line count (the surface form included) uniform in lo .. hi: a description, then instances, then
    aliases (at most 15 each), the texts as `random_dataset` draws them (one description in ten has 34 tokens, so T_b = 32 as in section
    28's dataset); ALL_ZERO gets 31 table lines."""
    pool = ds["pool"]
    text = lambda n: " ".join(pool[int(i)] for i in rng.integers(0, len(pool), n))
    ctx = {}
    for name in ds["entity2idx"]:
        m = 31 if name == "ALL_ZERO" else int(rng.integers(lo, hi + 1)) - 1
        if m == 0:
            continue
        kinds = min(15, m // 2)
        ctx[name] = {"desc": text(int(rng.integers(1, 7)) if rng.random() < 0.9 else 34), "instances": [{"label": text(int(rng.integers(1, 4)))} for _ in range(kinds)],
                     "aliases": [text(int(rng.integers(1, 4))) for _ in range(m - 1 - kinds)]}
    ds["context_wikidata"] = ctx


def make_dataset(N, n, T, seed, lo, hi, zipf=1.33, fill=None):       # about 450 unique entities per batch of 50, as section 28 measured
    """fill: what writes the entities' context in place of `set_line_counts` (tools/word_forms_bench.py's adverse table)."""
    C = n * (n - 1)
    rng = np.random.default_rng(seed)
    ds = random_dataset(rng, 1500, PARAMS["gat_entity_embedding_dim"])
    (fill or set_line_counts)(ds, rng, lo, hi)
    ids, sf = random_batch(np.random.default_rng(seed + 1), ds, N, C, zipf=zipf)
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    rng = np.random.default_rng(seed + 2)
    sentences = rng.integers(1, N_WORDS, (N, T)).astype(np.int32)
    markers = rng.integers(0, 4, (N, C, T)).astype(np.int8)
    labels = np.where(ids[:, :, 0] == -1, 0, rng.integers(1, N_OUT, (N, C))).astype(np.int16)
    return ds, (sentences, markers, labels, np.full(N, n, dtype=np.int32), ids.astype(np.int32), sf, None), surface_ids, tables


class RaggedBatcher:
    """`run_epoch` calls batcher.batch(ids, surface_ids, index_dtype): the same batcher with ragged_lines=True."""

    def __init__(self, batcher):
        self.batcher = batcher

    def batch(self, entity_indices, surface_ids, index_dtype=torch.int64):
        return self.batcher.batch(entity_indices, surface_ids, index_dtype, ragged_lines=True)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def condense(db, out):
    """The profiler run's dispatch records (a rocpd SQLite database) -> per table and leg the encoder kernels' and all kernels'
    microseconds per iteration.  An iteration starts at its k_sb_slice; the run's order is, per table, one warm-up epoch of either leg,
    then the padded epochs, then the ragged ones — an iteration with a k_cb_scan is a ragged one."""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, start, end from kernels order by start"))
    starts = [i for i, r in enumerate(rows) if "k_sb_slice" in r[0]] + [len(rows)]
    its = []
    for a, b in zip(starts[:-1], starts[1:]):
        part = rows[a:b]
        its.append(("ragged" if any("k_cb_scan" in r[0] for r in part) else "padded", sum(e - s for nm, s, e in part if any(k in nm for k in ENCODER)),
                    sum(e - s for _, s, e in part), len(part)))
    # runs of equal legs: per table warm-up padded, warm-up ragged, measured padded, measured ragged
    runs, lines = [], []
    for it in its:
        if runs and runs[-1][0][0] == it[0]:
            runs[-1].append(it)
        else:
            runs.append([it])
    assert len(runs) == 4 * len(TABLES), [(r[0][0], len(r)) for r in runs]
    for t, name in enumerate(TABLES):
        line = {"tool": "ragged_lines_bench", "what": "rocprofv3 --kernel-trace, a run of its own", "table": name}
        for run in runs[4 * t + 2:4 * t + 4]:
            leg, n = run[0][0], len(run)
            line["%s_iterations" % leg] = n
            line["%s_encoder_kernels_us_per_iteration" % leg] = round(sum(r[1] for r in run) / n / 1e3, 1)
            line["%s_all_kernels_us_per_iteration" % leg] = round(sum(r[2] for r in run) / n / 1e3, 1)
            line["%s_dispatches_per_iteration" % leg] = round(sum(r[3] for r in run) / n, 1)
        lines.append(json.dumps(line))
        print(lines[-1])
    write_lines(out, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sentences", type=int, default=500)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--tables", default=",".join(TABLES))
    ap.add_argument("--profile-epochs", type=int, default=0, help="per table one warm-up epoch of either leg, then this many padded and this many ragged epochs (for a profiler)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--condense", metavar="DB", help="no GPU work: the profiler run's database -> the encoder kernels' time per table and leg")
    a = ap.parse_args()
    if a.condense:
        return condense(a.condense, a.out)
    from recon_amd import ContextBatcher, RelationMetrics, StageBData, run_epoch
    from recon_amd.optim import Adam
    dev = torch.device("cuda:0")
    N, bs, n, T = a.sentences, a.batch, 9, 36
    iters = N // bs
    model, lines = None, []
    for name in a.tables.split(","):
        lo, hi = TABLES[name]
        ds, as_indices, surface_ids, tables = make_dataset(N, n, T, 2024, lo, hi)
        if model is None:
            model = make_model(len(ds["char2idx"]), dev)
        batcher = ContextBatcher(tables.to(dev))
        data = StageBData.from_indices(as_indices, surface_ids).to(dev)
        opt = Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-4, weight_decay=0, max_grad_norm=0.25)
        metrics = RelationMetrics(dev)
        order = torch.from_numpy(np.random.default_rng(1).permutation(N).astype(np.int64)).to(dev)
        model.train()
        legs = {"padded": lambda: run_epoch(model, data, bs, order=order, batcher=batcher, optimizer=opt, metrics=metrics),
                "ragged": lambda: run_epoch(model, data, bs, order=order, batcher=RaggedBatcher(batcher), optimizer=opt, metrics=metrics)}
        if a.profile_epochs:
            for k, epochs in (("padded", 1), ("ragged", 1), ("padded", a.profile_epochs), ("ragged", a.profile_epochs)):
                for _ in range(epochs):
                    legs[k]()
            metrics.result()
            torch.cuda.synchronize()
            continue
        # the batches' sizes: entities, the padded rows U P_b and the present lines L
        U = P = L = 0
        for i in range(iters):
            sl = data.take(order, i * bs, bs)
            r = batcher.batch(sl.entity_indices, sl.surface_ids, ragged_lines=True).context_mask
            U, P, L = U + r.U, max(P, r.n_max), L + r.total
            assert r.n_max == 32
        times = {k: [] for k in legs}
        for rnd in range(a.rounds + 1):
            for k, fn in legs.items():
                ms = wall(fn) / iters
                if rnd:
                    times[k].append(ms)
            metrics.reset()
        line = {"tool": "ragged_lines_bench", "device": torch.cuda.get_device_name(0), "model": "RECON", "table": name, "line_counts": [lo, hi], "N": N,
                "B": bs, "n": n, "T": T, "n_out": N_OUT, "iterations_per_epoch": iters, "rounds": a.rounds, "entities_per_batch": round(U / iters, 1),
                "P_b": P, "padded_rows_per_batch": round(32 * U / iters, 1), "present_lines_per_batch": round(L / iters, 1),
                "present_share": round(L / (32.0 * U), 4), "unit": "ms per training iteration (an epoch's wall clock, ending in a synchronize, over its iterations)"}
        for k, v in times.items():
            put_ms(line, k + "_ms", v)
        for k, fn in legs.items():
            c = count_launches(fn, iters=1)
            line[k + "_launches_per_iteration"] = None if c is None else round(c / iters, 1)
        line["ragged_over_padded_median"] = round(line["ragged_ms_median"] / line["padded_ms_median"], 4)
        line["padded_median_minus_min"] = round(line["padded_ms_median"] - line["padded_ms_min"], 4)
        if lo == hi == 32:     # the same rows: only the scan and the offset lookups are added
            line["ragged_median_within_padded_spread"] = line["ragged_ms_median"] - line["padded_ms_median"] <= line["padded_median_minus_min"]
        else:                  # the wiring rule of section 28
            line["ragged_median_below_padded_min"] = line["ragged_ms_median"] < line["padded_ms_min"]
        lines.append(json.dumps(line))
        print(lines[-1])
    if not a.profile_epochs:
        write_lines(a.out, lines)


if __name__ == "__main__":
    main()
