#!/usr/bin/env python3
"""Link-prediction evaluation of the GAT_sep_space ConvKB scorer at FB15k-237 size (14 541 entities, 237 relations, ~310 k known triples,
20 466 test triples, D = 200; synthetic tables, relation sizes skewed 1/k): the HIP kernels of recon_amd.kg_sep and, in the same process,
the reference's torch formulation (SpKBGATConvOnly.batch_test with the [T, D, D] gather of W_ent2rel, 100 rows per call as
get_validation_cnfmat tiles it) on a subset of the rows, extrapolated to all of them.  Device events, warm-up, legs alternated inside every
repeat, medians.  Prints one JSON line.

Legs:
  tables         recon_kgsep_tables for all 237 relations over all entities, chunk by chunk (1 GiB budget: 46 relations per launch)
  rank           recon_kgsep_rank, head and tail side, every chunk, tables resident (filters built once, outside the timing)
  rank_call      kg_sep.rank_entities end to end (filters, chunk tables, both sides)
  rel_scores     kg_sep.relation_scores end to end: [Q, R] (tables over the queries' entities + the dense kernel)
  torch_rows     the reference's batch_test on --torch-rows rows of the relation-scores tiling

    python tools/kg_sep_eval_bench.py [--repeats 5] [--torch-rows 20000]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recon_amd import _lib, kg_eval, kg_sep                       # noqa: E402
from recon_amd.gat_layers import ConvKB                            # noqa: E402

MFMA_F32_PEAK = 157.3e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-rows", type=int, default=20000)
    ap.add_argument("--legs", default="tables,rank,rank_call,rel_scores,torch_rows")
    a = ap.parse_args()
    legs = a.legs.split(",")
    n_ent, n_rel, n_known, n_test, D = 14541, 237, 310116, 20466, 200
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    E = torch.randn(n_ent, D, generator=g).to(dev)
    R = torch.randn(n_rel, D, generator=g).to(dev)
    rel = torch.multinomial(1.0 / torch.arange(1, n_rel + 1, dtype=torch.float64), n_known, replacement=True, generator=g)
    known = torch.stack([torch.randint(0, n_ent, (n_known,), generator=g), rel, torch.randint(0, n_ent, (n_known,), generator=g)], 1).to(dev)
    test = known[torch.randperm(n_known, generator=g)[:n_test].to(dev)]
    torch.manual_seed(0)
    conv = ConvKB(D, 3, 1, 50, 0.0, 0.2).to(dev).eval()
    gat = types.SimpleNamespace(W_ent2rel=(torch.randn(n_rel, D, D, generator=g) / D ** 0.5).to(dev), nonlinearity_ent2rel=torch.tanh)
    scorer = kg_sep.sep_scorer(E, R, conv, gat)
    L = _lib.lib()

    # resident tables of every relation (5.5 GB), chunked as rank_entities chunks them
    chunks = kg_sep.plan_chunks(range(n_rel), n_ent, D)
    rel_t = [torch.tensor(c, dtype=torch.int64, device=dev) for c in chunks]
    tabs = [kg_sep.relation_tables(scorer, c) for c in chunks]

    def build_tables():
        for r, (P_h, P_t) in zip(rel_t, tabs):
            _lib.check(L.recon_kgsep_tables(scorer.E.data_ptr(), n_ent, None, n_ent, scorer.W_ent2rel.data_ptr(), n_rel, r.data_ptr(), r.numel(),
                                            scorer.W1.data_ptr(), D, P_h.data_ptr(), P_t.data_ptr(), _lib.current_stream()), "recon_kgsep_tables")

    # the queries of each chunk, sorted by relation, with their filters (plumbing, built once)
    order = torch.argsort(test[:, 1], stable=True)
    ts = test[order].contiguous()
    counts = torch.bincount(ts[:, 1], minlength=n_rel).tolist()
    start = [sum(counts[:r]) for r in range(n_rel)]
    work = []
    for c, r, (P_h, P_t) in zip(chunks, rel_t, tabs):
        q0, q1 = start[c[0]], start[c[-1]] + counts[c[-1]]
        tq = ts[q0:q1].contiguous()
        seg = torch.tensor([0] + [start[x] + counts[x] - q0 for x in c], dtype=torch.int64, device=dev)
        for s in (kg_eval.SLOT_HEAD, kg_eval.SLOT_TAIL):
            f = kg_eval.build_filter(known, tq, s, (n_ent, n_rel))
            ws_floats = L.recon_convkb_rank_workspace_floats(tq.shape[0], D)
            work.append((s, tq, seg, r, P_h, P_t, f, torch.empty(ws_floats, device=dev), ws_floats, torch.empty(tq.shape[0], dtype=torch.int64, device=dev),
                         torch.empty(tq.shape[0], device=dev)))

    def rank_kernels():
        for s, tq, seg, r, P_h, P_t, f, ws, ws_floats, rk, st in work:
            _lib.check(L.recon_kgsep_rank(s, tq.shape[0], tq.data_ptr(), seg.data_ptr(), r.numel(), P_h.data_ptr(), scorer.P_r.data_ptr(),
                                          P_t.data_ptr(), n_ent, n_rel, D, scorer.b1.data_ptr(), scorer.w2.data_ptr(), scorer.b2.data_ptr(),
                                          scorer.slope, f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), ws.data_ptr(), ws_floats, rk.data_ptr(),
                                          st.data_ptr(), _lib.current_stream()), "recon_kgsep_rank")

    # the reference's formulation: rows of the relation-scores tiling, 100 per batch_test call, W_ent2rel gathered per row
    Wg = gat.W_ent2rel
    pred = test[:, None, :].repeat(1, n_rel, 1)
    pred[:, :, 1] = torch.arange(n_rel, device=dev)
    pred = pred.reshape(-1, 3)
    rows_t = min(a.torch_rows, pred.shape[0]) // 100 * 100

    def torch_rows():
        with torch.no_grad():
            for i in range(0, rows_t, 100):
                b = pred[i:i + 100]
                W = Wg[b[:, 1]]
                src = torch.tanh(torch.bmm(E[b[:, 0]].unsqueeze(1), W)).squeeze()
                dst = torch.tanh(torch.bmm(E[b[:, 2]].unsqueeze(1), W)).squeeze()
                conv(torch.cat((src, R[b[:, 1]], dst), dim=1))

    fns = {"tables": build_tables, "rank": rank_kernels, "rank_call": lambda: kg_sep.rank_entities(scorer, test, known),
           "rel_scores": lambda: kg_sep.relation_scores(scorer, test), "torch_rows": torch_rows}
    for leg in legs:                                                    # warm-up
        fns[leg]()
    torch.cuda.synchronize()
    ms = {leg: [] for leg in legs}
    for _ in range(a.repeats):
        for leg in legs:
            ms[leg].append(event_ms(fns[leg]))
    med = {leg: statistics.median(v) for leg, v in ms.items()}
    flop = 2.0 * 3 * n_rel * n_ent * D * D
    out = {"workload": "kg_sep FB15k-237-sized: %d entities, %d relations, %d known, %d test triples, D=%d, %d table chunks"
                       % (n_ent, n_rel, n_known, n_test, D, len(chunks)),
           "repeats": a.repeats, "ms_all": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
    if "tables" in med:
        out.update(tables_ms=round(med["tables"], 4), tables_tflops=flop / (med["tables"] * 1e-3) / 1e12,
                   tables_floor_ms=round(flop / MFMA_F32_PEAK * 1e3, 3), tables_share_of_peak=flop / MFMA_F32_PEAK / (med["tables"] * 1e-3))
    if "rank" in med:
        out.update(rank_both_sides_ms=round(med["rank"], 4), rank_per_side_ms=round(med["rank"] / 2, 4),
                   elem_evals_per_s=2 * n_test * n_ent * D / (med["rank"] * 1e-3))
    if "rank_call" in med:
        out["rank_entities_call_ms"] = round(med["rank_call"], 3)
    if "rel_scores" in med:
        out["relation_scores_call_ms"] = round(med["rel_scores"], 3)
    if "torch_rows" in med:
        per_row = med["torch_rows"] / rows_t
        out.update(torch_rows_measured=rows_t, torch_ms_measured=round(med["torch_rows"], 3),
                   torch_relation_scores_ms_extrapolated=round(per_row * n_test * n_rel, 1),
                   torch_entity_ranks_ms_extrapolated=round(per_row * 2 * n_test * n_ent, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
