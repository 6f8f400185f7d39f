"""Device evaluation of the GAT_sep_space ConvKB scorer (csrc/kg_sep.hip and the relation-segmented kernels of csrc/kg_eval.hip through
recon_amd.kg_sep / sep_space.SpKBGATConvOnly): parity with the reference's get_validation_pred / relation scores / forward, per-relation
tables against fp64, bit-exact agreement with recon_amd.kg_eval run one relation at a time, an FB15k-237-sized run, argument rejection."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = 2.0 ** -24


def _model(n_ent, n_rel, D, seed):
    """A sep shell with random weights on the device and a model_gat stand-in: (model_conv, model_gat)."""
    from recon_amd.sep_space import SpKBGATConvOnly
    torch.manual_seed(seed)
    m = SpKBGATConvOnly(torch.randn(n_ent, 8), torch.randn(n_rel, 8), [1, D], [1, D], 0.0, 0.0, 0.2, 0.2, [D, 1], 50).to(DEV).eval()
    with torch.no_grad():
        m.convKB.fc1.weight.normal_(0, D ** -0.5)
        m.convKB.fc1.bias.normal_(0, 0.5)
        m.convKB.fc2.weight.normal_(0, D ** -0.5)
    gat = types.SimpleNamespace(W_ent2rel=(torch.randn(n_rel, D, D) / D ** 0.5).to(DEV), nonlinearity_ent2rel=torch.tanh)
    return m, gat


def _tables64(scorer, r, ids=None):
    """fp64 P_h^r, P_t^r over the entity rows ids (None: all) and their elementwise fp32 error bound.
    T = tanh(E W_r): the product is an fma chain over D terms (|dX| <= D eps sum |e w|), tanh is 1-Lipschitz and tanhf adds a few ulp (8 eps,
    absolute: |T| <= 1); P = T W^T adds its own chain (D eps |T| |W|^T) to the propagated |dT| |W|^T.  Doubled for second-order slack."""
    D = scorer.D
    E = scorer.E.double() if ids is None else scorer.E.double()[ids]
    W = scorer.W_ent2rel[r].double()
    X = E @ W
    T = torch.tanh(X)
    dT = (D + 2) * EPS32 * (E.abs() @ W.abs()) + 8 * EPS32
    W1 = scorer.W1.double()
    out = []
    for Wx in (W1[:, :D], W1[:, 2 * D:]):
        P = T @ Wx.T
        tau = dT @ Wx.abs().T + (D + 2) * EPS32 * ((T.abs() + dT) @ Wx.abs().T)
        out += [P, 2 * tau]
    return out                                                                    # P_h64, tau_h, P_t64, tau_t


def _sep_scores64(scorer, tabs, queries, slot):
    """fp64 scores of queries [Q, 3] (one relation, tables tabs = _tables64 over all entities) against every candidate of `slot`, with the
    error bound of the fp32 path: kg_eval's score bound on the fp32 magnitudes plus sum_d |w2| (dPa + dPb + dPc) from the tables."""
    Ph, th, Pt, tt = tabs
    P = [Ph, scorer.P_r.double(), Pt]
    T = [th, torch.zeros_like(scorer.P_r, dtype=torch.float64), tt]
    b1, w2, b2 = scorer.b1.double(), scorer.w2.double(), scorer.b2.double()
    ca, cb = (1, 2) if slot == 0 else (0, 1)
    qa, qb = queries[:, ca], queries[:, cb]
    u = P[ca][qa] + P[cb][qb] + b1
    x = u[:, None, :] + P[slot][None, :, :]
    s = (w2 * torch.where(x > 0, x, scorer.slope * x)).sum(-1) + b2
    mag = (P[ca][qa].abs() + P[cb][qb].abs() + b1.abs())[:, None, :] + P[slot].abs()[None, :, :]
    tau = 2 * ((scorer.D + 4) * EPS32 * (w2.abs() * mag).sum(-1) + EPS32 * s.abs())
    tau += (w2.abs() * (T[ca][qa] + T[cb][qb])).sum(-1)[:, None] + (T[slot] @ w2.abs())[None, :]
    return s, tau


def _excluded(known, queries, slot, n_slot):
    ks = set(map(tuple, known.tolist()))
    m = torch.zeros(len(queries), n_slot, dtype=torch.bool)
    for q, tri in enumerate(queries.tolist()):
        for c in range(n_slot):
            x = list(tri)
            x[slot] = c
            m[q, c] = tuple(x) in ks
    return m


def test_kg_sep_reference_parity():
    from recon_amd import kg_eval, kg_sep
    from recon_amd.sep_space import SpKBGATConvOnly
    g = load_golden("kgsep1")
    D = g["sd__final_entity_embeddings"].shape[1]
    m = SpKBGATConvOnly(torch.randn(int(g["n_ent"]), 8), torch.randn(int(g["n_rel"]), 8), [D // 2, D], [D // 2, D], 0.0, 0.0, 0.2, 0.2, [2, 2], 50)
    m.load_state_dict({k: torch.from_numpy(g["sd__" + k]) for k in m.state_dict()}, strict=True)
    m = m.to(DEV).eval()
    gat = types.SimpleNamespace(W_ent2rel=torch.from_numpy(g["gat__W_ent2rel"]).to(DEV), nonlinearity_ent2rel=torch.tanh)
    test = torch.from_numpy(g["test"]).to(DEV)
    known = torch.from_numpy(g["known"]).to(DEV)
    rel = m.relation_scores(gat, test)
    ref = torch.from_numpy(g["rel_scores"])
    assert rel.shape == ref.shape
    torch.testing.assert_close(rel.cpu(), ref, rtol=1e-5, atol=1e-5)
    with torch.no_grad():
        true_rel = torch.from_numpy(g["rel_scores"][np.arange(len(g["test"])), g["test"][:, 1]])[:, None]
        torch.testing.assert_close(m.batch_test(test, gat).cpu(), true_rel, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m(None, None, torch.from_numpy(g["fwd_batch"]).to(DEV), gat).cpu(), torch.from_numpy(g["fwd_out"]),
                                   rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(m.batch_test(test[:1], gat).cpu(), true_rel[:1], rtol=1e-5, atol=1e-5)     # one row (the reference fails here)
    metrics = m.evaluate(gat, test, known, unique_entities=torch.from_numpy(g["unique"]).to(DEV))
    names = ("hits@100", "hits@10", "hits@3", "hits@1", "mean_rank", "mean_reciprocal_rank")
    for sec in ("head", "tail", "cumulative"):
        assert [metrics[sec][k] for k in names] == g["metrics_" + sec].tolist(), sec
    scorer = m._scorer(gat)
    rh, rt, _ = kg_sep.rank_entities(scorer, test, known, unique_entities=g["unique"])
    assert rh.cpu().tolist() == g["ranks_head64"].tolist() and rt.cpu().tolist() == g["ranks_tail64"].tolist()
    assert kg_eval.link_prediction_metrics(rh, rt) == metrics


def test_kg_sep_shell_trains():
    """Gradients of the shell's torch ConvKB reach fc1 / fc2 and a W_ent2rel parameter (the reference's train_conv loop runs on it)."""
    m, gat = _model(30, 4, 16, seed=5)
    gat.W_ent2rel = torch.nn.Parameter(gat.W_ent2rel)
    m.train()
    batch = torch.tensor([[1, 0, 2], [3, 3, 4], [5, 1, 1]], device=DEV)
    m(None, None, batch, gat).sum().backward()
    for p in (m.convKB.fc1.weight, m.convKB.fc2.weight, gat.W_ent2rel):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and p.grad.abs().sum() > 0
    assert gat.W_ent2rel.grad[2].abs().sum() == 0                                  # relation 2 is in no triple


@pytest.mark.parametrize("D", [1, 37, 144, 145, 200, 257, 304, 305, 512])       # 144 | 145, 304 | 305: the row-block switches of k_kgs_tables
def test_kg_sep_tables_fp64_band_and_deterministic(D):
    from recon_amd import kg_sep
    n_ent, n_rel = 101, 5
    m, gat = _model(n_ent, n_rel, D, seed=D)
    scorer = m._scorer(gat)
    g = torch.Generator().manual_seed(D)
    ids = torch.randint(0, n_ent, (77,), generator=g)                             # odd U, duplicates
    ids[5] = ids[40] = ids[76] = 7
    rels = [3, 0, 4, 3]
    P_h, P_t = kg_sep.relation_tables(scorer, rels, ids.to(DEV))
    P_h2, P_t2 = kg_sep.relation_tables(scorer, rels, ids.to(DEV))
    assert torch.equal(P_h.view(torch.int32), P_h2.view(torch.int32)) and torch.equal(P_t.view(torch.int32), P_t2.view(torch.int32))
    assert torch.equal(P_h[0].view(torch.int32), P_h[3].view(torch.int32))        # a repeated relation: the same table
    assert torch.equal(P_h[:, 5].view(torch.int32), P_h[:, 76].view(torch.int32))  # a repeated id: the same row
    for k, r in enumerate(rels):
        Ph64, th, Pt64, tt = _tables64(scorer, r, ids.to(DEV))
        for got, want, tau in ((P_h[k], Ph64, th), (P_t[k], Pt64, tt)):
            err = (got.double() - want).abs()
            assert bool((err <= tau).all()), (D, r, float((err / tau).max()))
    A_h, _ = kg_sep.relation_tables(scorer, [4])                                  # ids None: every entity row, in order
    assert torch.equal(A_h[0, ids.to(DEV)].view(torch.int32), P_h[2].view(torch.int32))


def _segment_case(n_ent, n_rel, seed):
    """Queries whose relations hold 0, 1, 64, 65, 130 and a few queries; fully filtered head and tail queries; duplicate known triples."""
    rs = np.random.RandomState(seed)
    per_rel = {0: 0, 1: 1, 2: 64, 3: 65, 4: 130, 5: 3, 6: 0, 7: 17, 8: 2}
    q = [np.stack([rs.randint(0, n_ent, k), np.full(k, r), rs.randint(0, n_ent, k)], 1) for r, k in per_rel.items() if k]
    queries = np.concatenate(q)[rs.permutation(sum(per_rel.values()))]
    known = np.concatenate([queries[::2], rs.randint(0, [n_ent, n_rel, n_ent], size=(900, 3))])
    known = np.concatenate([known, known[:100]])
    h, r, t = queries[0]
    full = [[c, r, t] for c in range(n_ent)] + [[queries[1, 0], queries[1, 1], c] for c in range(n_ent)]
    known = np.concatenate([known, np.array(full)])
    queries = np.concatenate([queries, [[n_ent - 1, 8, n_ent - 1]]])              # the last ids
    return torch.from_numpy(known), torch.from_numpy(queries)


@pytest.mark.parametrize("D", [37, 200])
def test_kg_sep_segmented_equals_kg_eval_per_relation(D):
    from recon_amd import kg_eval, kg_sep
    n_ent, n_rel = 203, 9
    m, gat = _model(n_ent, n_rel, D, seed=D + 1)
    scorer = m._scorer(gat)
    known, queries = _segment_case(n_ent, n_rel, seed=D)
    qd, kd = queries.to(DEV), known.to(DEV)
    budget = 3 * 2 * 4 * n_ent * D                                                # three relations per chunk: several chunks
    for filtered in (False, True):
        rh, rt, s_tail = kg_sep.rank_entities(scorer, qd, kd if filtered else None, budget_bytes=budget)
        rh2, _, s_head = kg_sep.rank_entities(scorer, qd, kd if filtered else None, side="head", budget_bytes=2 * 4 * n_ent * D)
        assert torch.equal(rh, rh2)
        for r in range(n_rel):
            sel = (queries[:, 1] == r).nonzero().reshape(-1)
            if not len(sel):
                continue
            P_h, P_t = kg_sep.relation_tables(scorer, [r])
            proj = kg_sep.relation_projections(scorer, P_h, P_t, 0)
            for slot, got_r, got_s in ((kg_eval.SLOT_HEAD, rh, s_head), (kg_eval.SLOT_TAIL, rt, s_tail)):
                want_r, want_s = kg_eval.rank_slot(proj, qd[sel.to(DEV)], slot, kd if filtered else None)
                assert torch.equal(got_r[sel.to(DEV)], want_r), (r, slot, filtered)
                assert torch.equal(got_s[sel.to(DEV)].view(torch.int32), want_s.view(torch.int32)), (r, slot, filtered)
        if filtered:
            assert rh[0].item() == 1 and rt[1].item() == 1                         # every candidate of these queries filtered
    # dense relation scores against kg_eval.slot_scores on the same per-relation tables (the queries' entities only)
    S = kg_sep.relation_scores(scorer, qd, budget_bytes=2 * (2 * 4 * n_ent * D))    # two relations per chunk
    ue = torch.unique(torch.cat([qd[:, 0], qd[:, 2]]))
    rows = torch.stack([torch.searchsorted(ue, qd[:, 0].contiguous()), qd[:, 1], torch.searchsorted(ue, qd[:, 2].contiguous())], 1)
    for r in range(n_rel):
        P_h, P_t = kg_sep.relation_tables(scorer, [r], ue)
        want = kg_eval.slot_scores(kg_sep.relation_projections(scorer, P_h, P_t, 0), rows, kg_eval.SLOT_RELATION, c0=r, C=1)
        assert torch.equal(S[:, r:r + 1].view(torch.int32), want.view(torch.int32)), r
    # filtered relation ranks: the dense matrix with the tie rule and the brute-force filter
    ranks, s_true = kg_sep.rank_relations(scorer, qd, kd)
    Sc = S.cpu()
    excl = _excluded(known, queries, kg_eval.SLOT_RELATION, n_rel)
    assert torch.equal(s_true.cpu(), Sc[torch.arange(len(queries)), queries[:, 1]])
    assert torch.equal(ranks.cpu(), 1 + ((Sc > s_true.cpu()[:, None]) & ~excl).sum(1))


def test_kg_sep_at_size():
    from recon_amd import kg_eval, kg_sep
    n_ent, n_rel, D, Q = 14541, 237, 200, 3000
    m, gat = _model(n_ent, n_rel, D, seed=11)
    scorer = m._scorer(gat)
    g = torch.Generator().manual_seed(4)
    zipf = 1.0 / torch.arange(1, n_rel + 1, dtype=torch.float64)                   # skewed relation sizes, as in FB15k-237
    rel = torch.multinomial(zipf, 310000, replacement=True, generator=g)
    known = torch.stack([torch.randint(0, n_ent, (310000,), generator=g), rel, torch.randint(0, n_ent, (310000,), generator=g)], 1).to(DEV)
    queries = known[torch.randperm(known.shape[0], generator=g)[:Q].to(DEV)]
    rh, rt, s = kg_sep.rank_entities(scorer, queries, known)
    rh2, rt2, s2 = kg_sep.rank_entities(scorer, queries, known)
    assert torch.equal(rh, rh2) and torch.equal(rt, rt2) and torch.equal(s.view(torch.int32), s2.view(torch.int32))
    assert int(rh.min()) >= 1 and int(rh.max()) <= n_ent and int(rt.min()) >= 1 and int(rt.max()) <= n_ent
    sub = torch.arange(0, Q, Q // 256)[:256].to(DEV)
    qs = queries[sub]
    for slot, ranks in ((kg_eval.SLOT_HEAD, rh[sub]), (kg_eval.SLOT_TAIL, rt[sub])):
        ids, begin, end = kg_eval.build_filter(known, qs, slot, (n_ent, n_rel))
        for r in torch.unique(qs[:, 1]).tolist():
            tabs = _tables64(scorer, r)
            for i in (qs[:, 1] == r).nonzero().reshape(-1).tolist():
                s64, tau = _sep_scores64(scorer, tabs, qs[i:i + 1], slot)
                keep = torch.ones(n_ent, dtype=torch.bool, device=DEV)
                keep[ids[begin[i]:end[i]]] = False
                tid = int(qs[i, slot])
                st, tt = s64[0, tid], tau[0, tid]
                lo = 1 + int(((s64[0] > st + tau[0] + tt) & keep).sum())
                hi = 1 + int(((s64[0] > st - tau[0] - tt) & keep).sum())
                assert lo <= int(ranks[i]) <= hi, (slot, i, lo, int(ranks[i]), hi)


def test_kg_sep_rejects_bad_arguments():
    from recon_amd import _lib, kg_sep
    m, gat = _model(20, 3, 16, seed=2)
    scorer = m._scorer(gat)
    L = _lib.lib()
    P = torch.empty(1, 20, 16, device=DEV)
    rel = torch.tensor([0], device=DEV)
    args = lambda D, Rc: (scorer.E.data_ptr(), 20, None, 20, scorer.W_ent2rel.data_ptr(), 3, rel.data_ptr(), Rc, scorer.W1.data_ptr(), D,
                          P.data_ptr(), P.data_ptr(), _lib.current_stream())
    assert L.recon_kgsep_tables(*args(513, 1)) == -2                              # D > 512
    assert L.recon_kgsep_tables(*args(0, 1)) == -1
    assert L.recon_kgsep_tables(*args(16, -1)) == -1
    assert L.recon_kgsep_tables(*args(16, 0)) == 0                                # nothing to do
    tri = torch.tensor([[1, 0, 2]], device=DEV)
    seg = torch.tensor([0, 1], device=DEV)
    out_r = torch.empty(1, dtype=torch.int64, device=DEV)
    out_s = torch.empty(1, device=DEV)
    ws = torch.empty(64, device=DEV)
    rank = lambda slot, ws_floats: L.recon_kgsep_rank(slot, 1, tri.data_ptr(), seg.data_ptr(), 1, P.data_ptr(), scorer.P_r.data_ptr(), P.data_ptr(),
                                                      20, 3, 16, scorer.b1.data_ptr(), scorer.w2.data_ptr(), scorer.b2.data_ptr(), 0.01, None, None,
                                                      None, ws.data_ptr(), ws_floats, out_r.data_ptr(), out_s.data_ptr(), _lib.current_stream())
    assert rank(1, 64) == -1                                                      # the relation slot has no per-relation candidate table
    assert rank(2, 8) == -4                                                       # workspace too small
    S = torch.empty(1, 3, device=DEV)
    assert L.recon_kgsep_scores(1, tri.data_ptr(), rel.data_ptr(), 1, P.data_ptr(), scorer.P_r.data_ptr(), P.data_ptr(), 20, 3, 16,
                                scorer.b1.data_ptr(), scorer.w2.data_ptr(), scorer.b2.data_ptr(), 0.01, S.data_ptr(), 2, None) == -1   # ldS < n_rel
    for bad in ([[20, 0, 1]], [[0, 3, 1]], [[-1, 0, 1]]):
        with pytest.raises(ValueError):
            kg_sep.rank_entities(scorer, torch.tensor(bad, device=DEV))
        with pytest.raises(ValueError):
            kg_sep.relation_scores(scorer, torch.tensor(bad, device=DEV))
    with pytest.raises(ValueError):
        kg_sep.relation_tables(scorer, [3])
    with pytest.raises(ValueError):
        kg_sep.relation_tables(scorer, [0], torch.tensor([20], device=DEV))
    with pytest.raises(ValueError):
        kg_sep.rank_entities(scorer, tri, budget_bytes=100)
    with pytest.raises(RuntimeError):
        m.batch_test(tri.cpu(), gat)
    torch.cuda.synchronize()
