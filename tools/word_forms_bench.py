"""A stage-B training iteration of `RECON` at the reference's widths with the batcher's dense char block against its distinct word forms
(`ContextBatcher.batch(..., word_forms=True)`), in the padded and in the ragged line form, all four legs in one
process.

The model, the optimizer, the sentences and the tables a, b and c are tools/ragged_lines_bench.py's (batch 50, n = 9 nodes, T = 36
tokens, packed word and char dropout, `recon_amd.optim.Adam(max_grad_norm=0.25)`, `run_epoch` from device-resident data).  An adverse
table d has c's line counts, every table line 32 tokens long and every token of a description, a label or an alias a string of its own:
apart from form 0 (the empty slots of the surface-form lines and of the padding lines) only the five words `entity_lines` puts in front
of a label or an alias ("instance of", "also known as") are shared.

Per table and leg pair (padded, ragged) one line: milliseconds per training iteration of the dense and the forms leg (an epoch's wall
clock, ending in a synchronize, over its iterations; the legs alternate round by round, round 0 warms up and is dropped), device launches
per iteration, S_d / n_slots, and on a, b and c the condition of the issue: the forms leg's median lies below the dense leg's minimum
(the wiring rule of section 28).  On d the difference is recorded, not judged.

    python tools/word_forms_bench.py [--rounds 7] [--out profiles/word_forms_bench.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -o word_forms -- python tools/word_forms_bench.py --profile-epochs 2       # a run of its own
    python tools/word_forms_bench.py --condense DIR/word_forms_results.db [--out profiles/word_forms_bench.jsonl]
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

from op_bench import put_ms, write_lines  # noqa: E402
from ragged_lines_bench import TABLES as RAGGED_TABLES, make_dataset, wall  # noqa: E402
from stage_a_iter_bench import count_launches  # noqa: E402
from stage_b_iter_bench import N_OUT, make_model  # noqa: E402

TABLES = dict(RAGGED_TABLES, d_unique_tokens=RAGGED_TABLES["c_1_to_4"])
LEGS = ("padded", "padded_forms", "ragged", "ragged_forms")
CHAR = ("k_char_", "k_keep_bits")                                 # the char-CNN family, by kernel name
FORMS = ("k_wf_", "k_pg_expand", "k_cb_forms_")                   # what the forms add: the copy, its backward, the marking and the scan


def set_unique_tokens(ds, rng, lo, hi):
    """c's line counts; every table line 32 tokens (`entity_lines` cuts at max_sent_len = 32) and every token below a string of its own."""
    fresh = iter(range(10 ** 9))
    text = lambda n: " ".join("u%d" % next(fresh) for _ in range(n))
    ctx = {}
    for name in ds["entity2idx"]:
        m = 31 if name == "ALL_ZERO" else int(rng.integers(lo, hi + 1)) - 1
        if m == 0:
            continue
        kinds = min(15, m // 2)
        ctx[name] = {"desc": text(32), "instances": [{"label": text(30)} for _ in range(kinds)], "aliases": [text(29) for _ in range(m - 1 - kinds)]}
    ds["context_wikidata"] = ctx


def condense(db, out):
    """The profiler run's dispatch records (a rocpd SQLite database) -> per table and leg the char-CNN family's, the forms' own and all
    kernels' microseconds per iteration.  An iteration starts at its k_sb_slice; a ragged one holds a k_cb_scan, a forms one a
    k_cb_forms_scan.  The run's order is, per table, one warm-up epoch of each leg in LEGS order, then the measured epochs in that order."""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, start, end from kernels order by start"))
    starts = [i for i, r in enumerate(rows) if "k_sb_slice" in r[0]] + [len(rows)]
    its = []
    for a, b in zip(starts[:-1], starts[1:]):
        part = rows[a:b]
        leg = ("ragged" if any("k_cb_scan" in r[0] for r in part) else "padded") + ("_forms" if any("k_cb_forms_scan" in r[0] for r in part) else "")
        its.append((leg, sum(e - s for nm, s, e in part if any(k in nm for k in CHAR)), sum(e - s for nm, s, e in part if any(k in nm for k in FORMS)),
                    sum(e - s for _, s, e in part), len(part)))
    runs, lines = [], []
    for it in its:
        if runs and runs[-1][0][0] == it[0]:
            runs[-1].append(it)
        else:
            runs.append([it])
    assert len(runs) == 2 * len(LEGS) * len(TABLES), [(r[0][0], len(r)) for r in runs]
    for t, name in enumerate(TABLES):
        line = {"tool": "word_forms_bench", "what": "rocprofv3 --kernel-trace, a run of its own", "table": name}
        for run in runs[2 * len(LEGS) * t + len(LEGS):2 * len(LEGS) * (t + 1)]:
            leg, n = run[0][0], len(run)
            line["%s_iterations" % leg] = n
            line["%s_char_kernels_us_per_iteration" % leg] = round(sum(r[1] for r in run) / n / 1e3, 1)
            line["%s_forms_kernels_us_per_iteration" % leg] = round(sum(r[2] for r in run) / n / 1e3, 1)
            line["%s_all_kernels_us_per_iteration" % leg] = round(sum(r[3] for r in run) / n / 1e3, 1)
            line["%s_dispatches_per_iteration" % leg] = round(sum(r[4] for r in run) / n, 1)
        lines.append(json.dumps(line))
        print(lines[-1])
    write_lines(out, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sentences", type=int, default=500)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--tables", default=",".join(TABLES))
    ap.add_argument("--profile-epochs", type=int, default=0, help="per table one warm-up epoch of each leg, then this many epochs of each (for a profiler)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--condense", metavar="DB", help="no GPU work: the profiler run's database -> the char-CNN kernels' time per table and leg")
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
        ds, as_indices, surface_ids, tables = make_dataset(N, n, T, 2024, lo, hi, fill=set_unique_tokens if name.startswith("d_") else None)
        if model is None:
            model = make_model(len(ds["char2idx"]), dev)
        tables = tables.to(dev)
        batchers = {"padded": ContextBatcher(tables), "padded_forms": ContextBatcher(tables, word_forms=True),
                    "ragged": ContextBatcher(tables, ragged_lines=True), "ragged_forms": ContextBatcher(tables, ragged_lines=True, word_forms=True)}
        data = StageBData.from_indices(as_indices, surface_ids).to(dev)
        opt = Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-4, weight_decay=0, max_grad_norm=0.25)
        metrics = RelationMetrics(dev)
        order = torch.from_numpy(np.random.default_rng(1).permutation(N).astype(np.int64)).to(dev)
        model.train()
        legs = {k: (lambda b=b: run_epoch(model, data, bs, order=order, batcher=b, optimizer=opt, metrics=metrics)) for k, b in batchers.items()}
        if a.profile_epochs:
            for epochs in (1, a.profile_epochs):
                for k in LEGS:
                    for _ in range(epochs):
                        legs[k]()
            metrics.result()
            torch.cuda.synchronize()
            continue
        # the batches' sizes: word slots and distinct forms of either line form
        sizes = {"padded": [0, 0], "ragged": [0, 0]}
        for i in range(iters):
            sl = data.take(order, i * bs, bs)
            for k in sizes:
                f = batchers[k + "_forms"].batch(sl.entity_indices, sl.surface_ids).context_chars
                sizes[k][0] += f.n_slots
                sizes[k][1] += f.total
        # what the occurrence lists cost per batch (a stable torch.sort of slot_form and a searchsorted; the last batch's forms, 20 calls)
        from recon_amd.word_forms import occurrence_lists
        sort_us = {}
        for k in sizes:
            f = batchers[k + "_forms"].batch(sl.entity_indices, sl.surface_ids).context_chars
            occurrence_lists(f.slot_form, f.total)
            sort_us[k] = round(wall(lambda: [occurrence_lists(f.slot_form, f.total) for _ in range(20)]) / 20 * 1e3, 1)
        # what a batcher call costs, host and device, with the last batch's ids (20 calls behind a warm-up, a synchronize at the end): with
        # the forms it holds the flags' clearing, the marking, the one-workgroup scan over the table's forms and the occurrence lists
        batch_us = {}
        for k, b in batchers.items():
            b.batch(sl.entity_indices, sl.surface_ids)
            batch_us[k] = round(wall(lambda: [b.batch(sl.entity_indices, sl.surface_ids) for _ in range(20)]) / 20 * 1e3, 1)
        times = {k: [] for k in legs}
        for rnd in range(a.rounds + 1):
            for k in LEGS:
                ms = wall(legs[k]) / iters
                if rnd:
                    times[k].append(ms)
            metrics.reset()
        launches = {k: count_launches(legs[k], iters=1) for k in LEGS}
        for k in ("padded", "ragged"):
            line = {"tool": "word_forms_bench", "device": torch.cuda.get_device_name(0), "model": "RECON", "table": name, "lines": k, "line_counts": [lo, hi],
                    "N": N, "B": bs, "n": n, "T": T, "n_out": N_OUT, "iterations_per_epoch": iters, "rounds": a.rounds, "table_forms": tables.dims["NFm"],
                    "word_slots_per_batch": round(sizes[k][0] / iters, 1), "forms_per_batch": round(sizes[k][1] / iters, 1),
                    "forms_over_slots": round(sizes[k][1] / max(sizes[k][0], 1), 5), "occurrence_lists_us_per_batch": sort_us[k],
                    "dense_batcher_call_us": batch_us[k], "forms_batcher_call_us": batch_us[k + "_forms"],
                    "unit": "ms per training iteration (an epoch's wall clock, ending in a synchronize, over its iterations)"}
            put_ms(line, "dense_ms", times[k])
            put_ms(line, "forms_ms", times[k + "_forms"])
            for leg, key in ((k, "dense"), (k + "_forms", "forms")):
                line[key + "_launches_per_iteration"] = None if launches[leg] is None else round(launches[leg] / iters, 1)
            line["forms_over_dense_median"] = round(line["forms_ms_median"] / line["dense_ms_median"], 4)
            if name.startswith("d_"):      # recorded, not judged: the switch is off by default
                line["forms_median_minus_dense_median"] = round(line["forms_ms_median"] - line["dense_ms_median"], 4)
            else:                          # the wiring rule of section 28
                line["forms_median_below_dense_min"] = line["forms_ms_median"] < line["dense_ms_min"]
            lines.append(json.dumps(line))
            print(lines[-1])
    if not a.profile_epochs:
        write_lines(a.out, lines)


if __name__ == "__main__":
    main()
