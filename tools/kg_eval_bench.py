#!/usr/bin/env python3
"""Link-prediction evaluation of the ConvKB scorer at FB15k-237 size (14 541 entities, 237 relations, ~310 k known triples, 20 466 test
triples, D = 200; synthetic tables): (a) the three projections, (b) filtered entity ranking, head and tail side, (c) relation scores
[Q, R] and filtered relation ranks — on the HIP kernels of recon_amd.kg_eval — and, in the same process, the torch-on-GPU formulation of
the tail-side ranking (chunked gather + ConvKB + comparison counts with the filter applied) on a subset of the queries, extrapolated to
all of them.  Device events, warm-up, median over repeats.  Prints one JSON line.

    python tools/kg_eval_bench.py [--repeats 5] [--torch-queries 1024]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recon_amd import kg_eval                                  # noqa: E402
from recon_amd.gat_layers import ConvKB                          # noqa: E402


def timed(fn, repeats, warmup=1):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-queries", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=16, help="queries per torch chunk")
    a = ap.parse_args()
    n_ent, n_rel, n_known, n_test, D = 14541, 237, 310116, 20466, 200
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    E = torch.randn(n_ent, D, generator=g).to(dev)
    R = torch.randn(n_rel, D, generator=g).to(dev)
    known = torch.stack([torch.randint(0, n_ent, (n_known,), generator=g), torch.randint(0, n_rel, (n_known,), generator=g),
                         torch.randint(0, n_ent, (n_known,), generator=g)], 1).to(dev)
    test = known[torch.randperm(n_known, generator=g)[:n_test].to(dev)]
    torch.manual_seed(0)
    conv = ConvKB(D, 3, 1, 50, 0.0, 0.2).to(dev).eval()

    proj = kg_eval.convkb_projections(E, R, conv)
    t_proj = timed(lambda: kg_eval.convkb_projections(E, R, conv), a.repeats)
    # filters built once (plumbing); the timed part is the rank kernels
    filt = {s: kg_eval.build_filter(known, test, s, (n_ent, n_rel)) for s in (kg_eval.SLOT_HEAD, kg_eval.SLOT_TAIL, kg_eval.SLOT_RELATION)}
    from recon_amd import _lib
    L = _lib.lib()
    ws_floats = L.recon_convkb_rank_workspace_floats(n_test, D)
    ws = torch.empty(ws_floats, device=dev)
    ranks = torch.empty(n_test, dtype=torch.int64, device=dev)
    s_true = torch.empty(n_test, device=dev)

    def rank(slot):
        f = filt[slot]
        _lib.check(L.recon_convkb_rank(slot, n_test, test.data_ptr(), proj.P_h.data_ptr(), proj.P_r.data_ptr(), proj.P_t.data_ptr(), n_ent, n_rel, D,
                                       proj.b1.data_ptr(), proj.w2.data_ptr(), proj.b2.data_ptr(), proj.slope, f[0].data_ptr(), f[1].data_ptr(),
                                       f[2].data_ptr(), ws.data_ptr(), ws_floats, ranks.data_ptr(), s_true.data_ptr(), _lib.current_stream()),
                   "recon_convkb_rank")
    t_head = timed(lambda: rank(kg_eval.SLOT_HEAD), a.repeats)
    t_tail = timed(lambda: rank(kg_eval.SLOT_TAIL), a.repeats)
    rank(kg_eval.SLOT_TAIL)
    ranks_tail = ranks.clone()
    s_tail = s_true.clone()
    t_rel_scores = timed(lambda: kg_eval.relation_scores(proj, test), a.repeats)
    t_rel_rank = timed(lambda: rank(kg_eval.SLOT_RELATION), a.repeats)
    t_full = timed(lambda: kg_eval.rank_entities(proj, test, known), max(1, a.repeats // 2))

    # torch on the GPU, tail side, the first --torch-queries queries: gather + ConvKB + counts, the filter as a dense mask per chunk
    Qt, ch = min(a.torch_queries, n_test), a.chunk
    ids, begin, end = filt[kg_eval.SLOT_TAIL]
    cand = torch.arange(n_ent, device=dev)

    def torch_rank():
        out = []
        with torch.no_grad():
            for q0 in range(0, Qt, ch):
                q = test[q0:q0 + ch]
                n = q.shape[0]
                conv_input = torch.cat((E[q[:, 0]].repeat_interleave(n_ent, 0), R[q[:, 1]].repeat_interleave(n_ent, 0), E[cand].repeat(n, 1)), 1)
                S = conv(conv_input).view(n, n_ent)
                st = conv(torch.cat((E[q[:, 0]], R[q[:, 1]], E[q[:, 2]]), 1))
                cnt = end[q0:q0 + n] - begin[q0:q0 + n]
                rows = torch.repeat_interleave(torch.arange(n, device=dev), cnt)
                pos = torch.arange(rows.numel(), device=dev) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt) + torch.repeat_interleave(begin[q0:q0 + n], cnt)
                excl = torch.zeros(n, n_ent, dtype=torch.bool, device=dev)
                excl[rows, ids[pos]] = True
                out.append(1 + ((S > st) & ~excl).sum(1))
        return torch.cat(out)
    t_torch = timed(torch_rank, max(1, a.repeats // 2))
    agree = (torch_rank() == ranks_tail[:Qt]).float().mean().item()
    elems = n_test * n_ent * D
    print(json.dumps({
        "workload": "kg_eval FB15k-237-sized: %d entities, %d relations, %d known, %d test triples, D=%d" % (n_ent, n_rel, n_known, n_test, D),
        "projections_ms": round(t_proj, 4),
        "rank_head_ms": round(t_head, 4), "rank_tail_ms": round(t_tail, 4),
        "rank_entities_call_ms": round(t_full, 4),
        "relation_scores_ms": round(t_rel_scores, 4), "relation_rank_ms": round(t_rel_rank, 4),
        "elem_evals_per_s_tail": elems / (t_tail * 1e-3),
        "torch_tail_ms_measured": round(t_torch, 3), "torch_tail_queries": Qt,
        "torch_tail_ms_extrapolated": round(t_torch * n_test / Qt, 1),
        "torch_elem_evals_per_s": Qt * n_ent * D / (t_torch * 1e-3),
        "torch_rank_agreement": agree,
        "s_true_finite": bool(torch.isfinite(s_tail).all().item()),
    }))


if __name__ == "__main__":
    main()
