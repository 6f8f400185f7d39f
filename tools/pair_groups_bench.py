"""A stage-B iteration of `GPGNN` and `RECON` at the reference's widths with `distinct_pair_sequences` off (dense: B C = 3 600 sequences
through the sentence encoder) against on (mapped: the S_d distinct ones), both legs in one process.

The models, the optimizer and the sentences are tools/stage_b_iter_bench.py's (batch 50, n = 9 nodes, T = 36 tokens, n_out = 353, packed
word and char dropout, `recon_amd.optim.Adam(max_grad_norm=0.25)`, `run_epoch` from device-resident data); `RECON` also takes
`ragged_lines=True` on section 34's table (b) (line counts uniform in 2 .. 12).  Synthetic datasets in which every sentence has k entities:
its k (k - 1) present pairs hold a marker row of their own, every other of the 72 slots the all-zero row, as
parsing/legacy_sp_models.py:294-326 leaves them:

    k9   S_d = 3 600 per batch: nothing is shared        k3   S_d = 350
    k5   S_d = 50 x 21                                    k2   S_d = 150
    mix  k uniform in 2 .. 5

Per model and dataset: milliseconds per training iteration and per evaluation iteration of either leg (an epoch's wall clock, ending in
a synchronize, over its iterations; the legs alternate round by round, round 0 warms up and is dropped), device launches per iteration,
S_d per batch, and the conditions of the issue under section 28's wiring rule: for k <= 5 and the mix the mapped median lies below the
dense minimum; at k = 9 the mapped median exceeds the dense median by no more than the dense leg's median - minimum.

    python tools/pair_groups_bench.py [--rounds 7] [--out profiles/pair_groups_bench.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -o pair_groups -- python tools/pair_groups_bench.py --models GPGNN --profile-epochs 2      # a run of its own
    python tools/pair_groups_bench.py --models GPGNN --condense DIR/pair_groups_results.db [--out profiles/pair_groups_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from context_batch_checks import build, random_batch, random_dataset  # noqa: E402
from op_bench import put_ms, write_lines  # noqa: E402
from pair_groups_checks import entity_markers, slot_of  # noqa: E402
from ragged_lines_bench import RaggedBatcher, set_line_counts, wall  # noqa: E402
from stage_a_iter_bench import count_launches  # noqa: E402
from stage_b_iter_bench import N_OUT, N_WORDS, PARAMS, make_model  # noqa: E402

DATASETS = {"k9": (9, 9), "k5": (5, 5), "k3": (3, 3), "k2": (2, 2), "mix_2_to_5": (2, 5)}
ENCODER = ("k_sent_lstm_", "k_pg_")                      # the sentence encoder's kernels, by name


def make_gpgnn(dev):
    from recon_amd.gpgnn import GPGNN
    torch.manual_seed(0)
    m = GPGNN(dict(PARAMS), np.random.RandomState(0).randn(N_WORDS, 50).astype(np.float32), 36, N_OUT)
    m.packed_word_dropout = True
    return m.to(dev)


def make_dataset(N, n, T, seed, lo, hi):
    """Every sentence has k entities, k uniform in lo .. hi: markers as the preprocessing writes them, ids and labels for the present pairs
    alone (the absent ones are (-1, -1) with label 0), the entities' context on section 34's table (b)."""
    C = n * (n - 1)
    rng = np.random.default_rng(seed)
    ds = random_dataset(rng, 1500, PARAMS["gat_entity_embedding_dim"])
    set_line_counts(ds, rng, 2, 12)
    ks = rng.integers(lo, hi + 1, N)
    markers = entity_markers(N, ks.tolist(), T, n=n, seed=seed + 3).astype(np.int8)
    present = np.zeros((N, C), dtype=bool)
    for b, k in enumerate(ks):
        for i in range(k):
            for j in range(k):
                if i != j:
                    present[b, slot_of(i, j, n)] = True
    ids, sf = random_batch(np.random.default_rng(seed + 1), ds, N, C, zipf=1.33, pad_share=0.0)
    ids[~present] = -1
    for b, c in zip(*np.nonzero(~present)):
        sf[b, c, 0] = sf[b, c, 1] = ["ALL_ZEROS"]
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    rng = np.random.default_rng(seed + 2)
    sentences = rng.integers(1, N_WORDS, (N, T)).astype(np.int32)
    labels = np.where(present, rng.integers(1, N_OUT, (N, C)), 0).astype(np.int16)
    return ds, (sentences, markers, labels, ks.astype(np.int32), ids.astype(np.int32), sf, None), surface_ids, tables


def condense(db, out, models, datasets):
    """The profiler run's dispatch records (a rocpd SQLite database) -> per model, dataset and leg the sentence-encoder kernels' and all
    kernels' microseconds per training iteration.  An iteration starts at its k_sb_slice; the run's order is, per model and dataset, one
    warm-up epoch of either leg, then the dense epochs, then the mapped ones — an iteration with a k_pg_scan is a mapped one."""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, start, end from kernels order by start"))
    starts = [i for i, r in enumerate(rows) if "k_sb_slice" in r[0]] + [len(rows)]
    its = []
    for a, b in zip(starts[:-1], starts[1:]):
        part = rows[a:b]
        its.append(("mapped" if any("k_pg_scan" in r[0] for r in part) else "dense", sum(e - s for nm, s, e in part if any(k in nm for k in ENCODER)),
                    sum(e - s for _, s, e in part), len(part)))
    runs, lines = [], []
    for it in its:
        if runs and runs[-1][0][0] == it[0]:
            runs[-1].append(it)
        else:
            runs.append([it])
    cases = [(m, d) for m in models for d in datasets]
    assert len(runs) == 4 * len(cases), [(r[0][0], len(r)) for r in runs]
    for t, (model, name) in enumerate(cases):
        line = {"tool": "pair_groups_bench", "what": "rocprofv3 --kernel-trace, a run of its own", "model": model, "dataset": name}
        for run in runs[4 * t + 2:4 * t + 4]:
            leg, n = run[0][0], len(run)
            line["%s_iterations" % leg] = n
            line["%s_sentence_encoder_kernels_us_per_iteration" % leg] = round(sum(r[1] for r in run) / n / 1e3, 1)
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
    ap.add_argument("--models", default="GPGNN,RECON")
    ap.add_argument("--datasets", default=",".join(DATASETS))
    ap.add_argument("--profile-epochs", type=int, default=0, help="per model and dataset one warm-up epoch of either leg, then this many dense and this many mapped epochs (for a profiler)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--condense", metavar="DB", help="no GPU work: the profiler run's database -> the sentence-encoder kernels' time per model, dataset and leg")
    a = ap.parse_args()
    models, names = a.models.split(","), a.datasets.split(",")
    if a.condense:
        return condense(a.condense, a.out, models, names)
    from recon_amd import ContextBatcher, RelationMetrics, StageBData, run_epoch
    from recon_amd.optim import Adam
    dev = torch.device("cuda:0")
    N, bs, n, T = a.sentences, a.batch, 9, 36
    iters = N // bs
    lines = []
    made = {name: make_dataset(N, n, T, 2024, *DATASETS[name]) for name in names}
    for which in models:
        model = make_gpgnn(dev) if which == "GPGNN" else make_model(len(made[names[0]][0]["char2idx"]), dev)
        for name in names:
            ds, as_indices, surface_ids, tables = made[name]
            batcher = RaggedBatcher(ContextBatcher(tables.to(dev))) if which == "RECON" else None
            data = StageBData.from_indices(as_indices if which == "RECON" else as_indices[:4], surface_ids if which == "RECON" else None).to(dev)
            opt = Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-4, weight_decay=0, max_grad_norm=0.25)
            metrics = RelationMetrics(dev)
            order = torch.from_numpy(np.random.default_rng(1).permutation(N).astype(np.int64)).to(dev)

            def epoch(on, train):
                model.distinct_pair_sequences = on
                model.train(train)
                run_epoch(model, data, bs, order=order, batcher=batcher, optimizer=opt if train else None, metrics=metrics)
            legs = {"dense": False, "mapped": True}
            if a.profile_epochs:
                for k, epochs in (("dense", 1), ("mapped", 1), ("dense", a.profile_epochs), ("mapped", a.profile_epochs)):
                    for _ in range(epochs):
                        epoch(legs[k], True)
                metrics.result()
                torch.cuda.synchronize()
                continue
            S_d = int(data.distinct_counts()[order[:iters * bs]].sum())
            line = {"tool": "pair_groups_bench", "device": torch.cuda.get_device_name(0), "model": which, "dataset": name, "entities_per_sentence": list(DATASETS[name]),
                    "N": N, "B": bs, "n": n, "T": T, "n_out": N_OUT, "iterations_per_epoch": iters, "rounds": a.rounds, "sequences_per_batch": bs * n * (n - 1),
                    "distinct_sequences_per_batch": round(S_d / iters, 1), "distinct_share": round(S_d / (iters * bs * n * (n - 1.0)), 4),
                    "unit": "ms per iteration (an epoch's wall clock, ending in a synchronize, over its iterations)"}
            for phase, train in (("train", True), ("eval", False)):
                times = {k: [] for k in legs}
                for rnd in range(a.rounds + 1):
                    for k, on in legs.items():
                        ms = wall(lambda: epoch(on, train)) / iters
                        if rnd:
                            times[k].append(ms)
                    metrics.reset()
                for k, v in times.items():
                    put_ms(line, "%s_%s_ms" % (k, phase), v)
                for k, on in legs.items():
                    c = count_launches(lambda: epoch(on, train), iters=1)
                    line["%s_%s_launches_per_iteration" % (k, phase)] = None if c is None else round(c / iters, 1)
                d_med, d_min, m_med = line["dense_%s_ms_median" % phase], line["dense_%s_ms_min" % phase], line["mapped_%s_ms_median" % phase]
                line["mapped_over_dense_%s_median" % phase] = round(m_med / d_med, 4)
                line["dense_%s_median_minus_min" % phase] = round(d_med - d_min, 4)
                if DATASETS[name] == (9, 9):   # the same sequences: only the grouping, the compact copies and the expansion are added
                    line["%s_mapped_median_within_dense_spread" % phase] = m_med - d_med <= d_med - d_min
                else:                          # the wiring rule of section 28
                    line["%s_mapped_median_below_dense_min" % phase] = m_med < d_min
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del model
    if not a.profile_epochs:
        write_lines(a.out, lines)


if __name__ == "__main__":
    main()
