"""A whole stage-B iteration of `RECON` at the reference's widths, from device-resident data (`recon_amd.run_epoch`) and by the
hand-written loop of INTEGRATION.md (host slices, pageable uploads, device gathers), in one process.

A synthetic dataset of N = 1 000 sentences: n = 9 nodes (72 pairs), T = 36 tokens, Zipf entity ids with about 450 unique entities per
batch of 50 (tools/context_batch_bench.py's dataset), contexts of 1-32 lines, G = 200; `RECON` with model_params.json's sizes, n_out = 353,
packed word and char dropout on, `recon_amd.optim.Adam(max_grad_norm=0.25)`.  The legs, alternating round by round (round 0 warms up and
is dropped; every timing ends with a synchronize):

    a  run_epoch: a training epoch, milliseconds per iteration and device launches per iteration
    b  the hand-written loop, the same
    c  `take` alone over the epoch's batches: the kernel, torch indexing of the device-resident arrays, host slices plus uploads
    d  an evaluation pass (no_grad) with `EpochRows.append` against the `.cpu()[rows].tolist()` lines of the test loop, and the collection
       alone over recorded outputs

    python tools/stage_b_iter_bench.py [--rounds 7] [--out profiles/stage_b_iter_bench.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -o stage_b_iter -- python tools/stage_b_iter_bench.py --profile-epochs 2      # leg (a) alone, a run of its own
    python tools/stage_b_iter_bench.py --condense DIR/stage_b_iter_results.db profiles/stage_b_iter_kernel_stats.csv
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

from context_batch_bench import make_case  # noqa: E402
from context_batch_checks import build, random_batch  # noqa: E402
from op_bench import put_ms, write_lines  # noqa: E402
from stage_a_iter_bench import count_launches  # noqa: E402

# the reference's model_params.json (the keys RECON reads)
PARAMS = {"max_num_nodes": 9, "embedding_dim": 8, "layer_number": 3, "projection_style": "untie", "non-linear1": "relu", "non-linear": "tanh",
          "dropout1": 0.5, "position_emb": 3, "units1": 256, "rnn1_layers": 1, "bidirectional": 1, "batch_size": 50, "conv_filter_size": 3,
          "entity_conv_filter_size": 1, "hidden_dim_ent": 50, "num_entEmb_layers": 1, "is_bidirectional_ent": 1, "drop_out_rate_ent": 0.5,
          "entity_embed_dim": 8, "char_embed_dim": 50, "char_feature_size": 50, "max_char_len": 10, "gat_entity_embedding_dim": 200}
N_OUT, N_WORDS, REL_DIM = 353, 2000, 200


def make_model(n_chars, dev):
    from recon_amd.gpgnn import RECON
    torch.manual_seed(0)
    rs = np.random.RandomState(0)
    emb = rs.randn(N_WORDS, 50).astype(np.float32)
    G = PARAMS["gat_entity_embedding_dim"]
    rel = {str(i): [float(v) for v in rs.randn(REL_DIM) * 0.5] for i in range(N_OUT)}
    W_all = (rs.randn(N_OUT, G, REL_DIM) / G ** 0.5).astype(np.float32)
    m = RECON(dict(PARAMS), emb, 36, N_OUT, list(range(n_chars)), rel, W_all, {i: "P%d" % i for i in range(N_OUT)}, {"P%d" % i: str(i) for i in range(N_OUT)})
    m.packed_word_dropout = True
    m.entity_embedding_module.packed_char_dropout = True
    return m.to(dev)


def make_dataset(N, B, n, T, seed):
    """(ds, as_indices, surface_ids, tables): tools/context_batch_bench.py's entities and Zipf exponent, N sentences of them."""
    C = n * (n - 1)
    ds, (_, zipf, _, _) = make_case(B, C, PARAMS["gat_entity_embedding_dim"], 450, seed)
    rng = np.random.default_rng(seed + 2)
    ids, sf = random_batch(rng, ds, N, C, zipf=zipf)
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    sentences = rng.integers(1, N_WORDS, (N, T)).astype(np.int32)
    markers = rng.integers(0, 4, (N, C, T)).astype(np.int8)
    labels = np.where(ids[:, :, 0] == -1, 0, rng.integers(1, N_OUT, (N, C))).astype(np.int16)
    counts = np.full(N, n, dtype=np.int32)
    return ds, (sentences, markers, labels, counts, ids.astype(np.int32), sf, None), surface_ids, tables, zipf


def hand_written(model, as_indices, entity_indices_d, surface_ids_d, batcher, bs, indices, opt, metrics, dev, collect=False):
    """INTEGRATION.md's loops before StageBData: train.py:247-251 on the host, the uploads of :261-262 and :309, the two device gathers in
    front of `batcher.batch`; with `collect` the two [M] copies and `.tolist()`s of the test loop."""
    from recon_amd import relation_objective
    N = as_indices[0].shape[0]
    kept = []
    for i in range(int(N / bs)):
        at = indices[i * bs:(i + 1) * bs]
        sentence_input = torch.from_numpy(as_indices[0][at].astype(int)).to(dev)
        entity_markers = torch.from_numpy(as_indices[1][at].astype(int)).to(dev)
        labels = as_indices[2][at]
        if opt is not None:
            opt.zero_grad()
        rows = torch.from_numpy(at).to(dev)
        batch = batcher.batch(entity_indices_d[rows], surface_ids_d[rows])
        output = model(sentence_input, entity_markers, as_indices[3][at], *batch.model_args())
        res = relation_objective(output, torch.from_numpy(labels.astype(int)).to(dev), ignore_index=0, empty_label=1, metrics=metrics)
        if opt is not None:
            res.loss.backward()
            opt.step()
        if collect:
            keep = (torch.from_numpy(labels.reshape(-1).astype(int)) != 0).nonzero().squeeze(1)
            kept.append((res.predicted.cpu()[keep].tolist(), res.confidence.cpu()[keep].tolist()))
    return kept


def condense(db, out, skip_epochs, iters):
    """The profiler run's dispatch records (a rocpd SQLite database) -> rocprofv3's stats columns per kernel over the iterations behind
    the first `skip_epochs` epochs (an iteration starts at its k_sb_slice), and the span, busy time and gaps per iteration on stdout."""
    import collections
    import csv
    import sqlite3
    import statistics
    rows = list(sqlite3.connect(db).execute("select name, start, end from kernels order by start"))
    starts = [i for i, r in enumerate(rows) if "k_sb_slice" in r[0]]
    meas = rows[starts[skip_epochs * iters]:]
    n = len(starts) - skip_epochs * iters
    busy, (_, lo, hi) = 0, meas[0]
    for _, s, e in meas[1:]:
        if s > hi:
            busy, lo, hi = busy + hi - lo, s, e
        else:
            hi = max(hi, e)
    busy += hi - lo
    span = meas[-1][2] - meas[0][1]
    by = collections.defaultdict(list)
    for name, s, e in meas:
        by[name].append(e - s)
    total = sum(sum(v) for v in by.values())
    with open(out, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "StdDev"])
        for name, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
            w.writerow([name, len(v), sum(v), round(sum(v) / len(v), 6), round(100.0 * sum(v) / total, 2), min(v), max(v), round(statistics.pstdev(v), 6)])
    print(json.dumps({"iterations": n, "span_us_per_iteration": round(span / n / 1e3, 1), "kernels_us_per_iteration": round(busy / n / 1e3, 1),
                      "gaps_us_per_iteration": round((span - busy) / n / 1e3, 1), "dispatches_per_iteration": round(len(meas) / n, 1)}))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sentences", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--profile-epochs", type=int, default=0, help="only run leg (a) for this many epochs behind one warm-up epoch (for a profiler)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--condense", nargs=2, metavar=("DB", "CSV"), help="no GPU work: the profiler run's database -> the per-kernel table, its warm-up epoch left out")
    a = ap.parse_args()
    if a.condense:
        return condense(a.condense[0], a.condense[1], 1, a.sentences // a.batch)
    from recon_amd import ContextBatcher, EpochRows, RelationMetrics, StageBData, relation_objective, run_epoch, stage_b
    from recon_amd.optim import Adam
    dev = torch.device("cuda:0")
    N, bs, n, T = a.sentences, a.batch, 9, 36
    C, iters = n * (n - 1), a.sentences // a.batch
    ds, as_indices, surface_ids, tables, zipf = make_dataset(N, bs, n, T, 2024)
    batcher = ContextBatcher(tables.to(dev))
    data = StageBData.from_indices(as_indices, surface_ids).to(dev)
    entity_indices_d = torch.from_numpy(as_indices[4].astype(np.int64)).to(dev)
    surface_ids_d = torch.from_numpy(surface_ids).to(dev)
    model = make_model(len(ds["char2idx"]), dev)
    opt = Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=1e-4, weight_decay=0, max_grad_norm=0.25)
    metrics, rows = RelationMetrics(dev), EpochRows.for_data(data)
    rng = np.random.default_rng(1)
    order = rng.permutation(N).astype(np.int64)
    order_d = torch.from_numpy(order).to(dev)

    def leg_a():
        model.train()
        run_epoch(model, data, bs, order=order_d, batcher=batcher, optimizer=opt, metrics=metrics)

    def leg_b():
        model.train()
        hand_written(model, as_indices, entity_indices_d, surface_ids_d, batcher, bs, order, opt, metrics, dev)

    if a.profile_epochs:
        for _ in range(1 + a.profile_epochs):
            leg_a()
        metrics.result()
        torch.cuda.synchronize()
        return

    def take_kernel():
        for i in range(iters):
            data.take(order_d, i * bs, bs)

    def take_torch():
        prev, stage_b._KERNELS = stage_b._KERNELS, False
        try:
            for i in range(iters):
                data.take(order_d, i * bs, bs)
        finally:
            stage_b._KERNELS = prev

    def take_host():
        for i in range(iters):
            at = order[i * bs:(i + 1) * bs]
            torch.from_numpy(as_indices[0][at].astype(int)).to(dev)
            torch.from_numpy(as_indices[1][at].astype(int)).to(dev)
            torch.from_numpy(as_indices[2][at].astype(int)).view(-1).to(dev)
            r = torch.from_numpy(at).to(dev)
            entity_indices_d[r], surface_ids_d[r]

    def eval_rows():
        model.eval()
        rows.reset()
        run_epoch(model, data, bs, batcher=batcher, metrics=metrics, rows=rows)
        rows.result()

    def eval_host():
        model.eval()
        with torch.no_grad():
            hand_written(model, as_indices, entity_indices_d, surface_ids_d, batcher, bs, np.arange(N), None, metrics, dev, collect=True)

    # recorded outputs of one evaluation pass, for the collection alone
    model.eval()
    recorded = []
    with torch.no_grad():
        for i in range(iters):
            sl = data.take(None, i * bs, bs)
            out = model(sl.sentence_input, sl.entity_markers, sl.num_entities, *batcher.batch(sl.entity_indices, sl.surface_ids).model_args())
            recorded.append((relation_objective(out, sl.labels, empty_label=1), sl, as_indices[2][i * bs:(i + 1) * bs]))
    torch.cuda.synchronize()

    def collect_rows():
        rows.reset()
        for res, sl, _ in recorded:
            rows.append(res, sl)
        rows.result()

    def collect_host():
        for res, _, labels in recorded:
            keep = (torch.from_numpy(labels.reshape(-1).astype(int)) != 0).nonzero().squeeze(1)
            res.predicted.cpu()[keep].tolist(), res.confidence.cpu()[keep].tolist()

    legs = {"a_run_epoch": leg_a, "b_hand_written": leg_b, "c_take_kernel": take_kernel, "c_take_torch": take_torch, "c_take_host": take_host,
            "d_eval_rows": eval_rows, "d_eval_host": eval_host, "d_collect_rows": collect_rows, "d_collect_host": collect_host}
    times = {k: [] for k in legs}
    for rnd in range(a.rounds + 1):
        for k, fn in legs.items():
            ms = wall(fn) / iters
            if rnd:
                times[k].append(ms)
        metrics.reset()
    line = {"tool": "stage_b_iter_bench", "device": torch.cuda.get_device_name(0), "model": "RECON", "N": N, "B": bs, "n": n, "C": C, "T": T, "n_out": N_OUT,
            "G": PARAMS["gat_entity_embedding_dim"], "zipf": zipf, "iterations_per_epoch": iters, "kept_pairs": data.kept_pairs, "rounds": a.rounds,
            "unit": "ms per iteration (an epoch's wall clock, ending in a synchronize, over its iterations)",
            "dataset_device_bytes": sum(t.numel() * t.element_size() for t in data.arrays.values())}
    for k, v in times.items():
        put_ms(line, k + "_ms", v)
    line["a_launches_per_iteration"] = count_launches(leg_a, iters=1)
    line["b_launches_per_iteration"] = count_launches(leg_b, iters=1)
    for k in ("a_launches_per_iteration", "b_launches_per_iteration"):
        line[k] = None if line[k] is None else round(line[k] / iters, 1)
    line["b_over_a_median"] = round(line["b_hand_written_ms_median"] / line["a_run_epoch_ms_median"], 4)
    line["a_median_below_b_min"] = line["a_run_epoch_ms_median"] < line["b_hand_written_ms_min"]
    # the wiring rule: the kernel is the default where its median lies below the torch-primitive form's minimum in the same process
    line["take_kernel_median_below_torch_min"] = line["c_take_kernel_ms_median"] < line["c_take_torch_ms_min"]
    line["take_kernel_median_below_host_min"] = line["c_take_kernel_ms_median"] < line["c_take_host_ms_min"]
    line["collect_rows_median_below_host_min"] = line["d_collect_rows_ms_median"] < line["d_collect_host_ms_min"]
    line["eval_rows_median_below_host_min"] = line["d_eval_rows_ms_median"] < line["d_eval_host_ms_min"]
    text = json.dumps(line)
    print(text)
    write_lines(a.out, [text])


if __name__ == "__main__":
    main()
