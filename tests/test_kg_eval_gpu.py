"""Link-prediction evaluation on the device (csrc/kg_eval.hip through recon_amd.kg_eval): parity with the reference's
get_validation_pred / relation scores, exact self-consistency of the fused rank kernel with the library's own dense scores, fp64 bands,
an FB15k-237-sized run, determinism and argument rejection."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = 2.0 ** -24


def _proj(n_ent, n_rel, D, seed, slope=0.01):
    from recon_amd.kg_eval import ConvKBProjections
    g = torch.Generator(device="cpu").manual_seed(seed)
    f = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return ConvKBProjections(f(n_ent, D), f(n_rel, D), f(n_ent, D), f(D), f(D) / D ** 0.5, f(1), slope, n_ent, n_rel, D)


def _excluded_mask(known, queries, slot, n_slot):
    """[Q, n_slot] bool: candidate c of query q is a known triple (brute force over Python sets)."""
    ks = set(map(tuple, known.tolist()))
    m = torch.zeros(len(queries), n_slot, dtype=torch.bool)
    for q, tri in enumerate(queries.tolist()):
        for c in range(n_slot):
            x = list(tri)
            x[slot] = c
            m[q, c] = tuple(x) in ks
    return m


def _scores64(proj, queries, slot, cand):
    """fp64 scores (on the device, returned on the CPU) of queries [Q, 3] against candidate ids `cand`, and the fp32 error bound tau of each score."""
    P = [proj.P_h.double(), proj.P_r.double(), proj.P_t.double()]
    b1, w2, b2 = proj.b1.double(), proj.w2.double(), proj.b2.double()
    queries, cand = queries.to(DEV), cand.to(DEV)
    ca, cb = (1, 2) if slot == 0 else ((0, 2) if slot == 1 else (0, 1))
    u = P[ca][queries[:, ca]] + P[cb][queries[:, cb]] + b1                       # [Q, D]
    x = u[:, None, :] + P[slot][cand][None, :, :]                                 # [Q, C, D]
    s = (w2 * torch.where(x > 0, x, proj.slope * x)).sum(-1) + b2
    # tau: u takes two fp32 roundings (|du| <= 2 eps (|Pa| + |Pb| + |b1|)), x = u + p one more, slope * x one, and the fma chain over D terms
    # adds at most D eps sum |w y| (gamma_D, first order); leaky is 1-Lipschitz for slope <= 1.  Per term that is at most
    # (D + 4) eps |w_d| (|Pa_d| + |Pb_d| + |b1_d| + |p_d|); the final + b2 adds eps |s|.  Doubled for second-order slack.
    mag = (P[ca][queries[:, ca]].abs() + P[cb][queries[:, cb]].abs() + b1.abs())[:, None, :] + P[slot][cand].abs()[None, :, :]
    tau = 2 * ((proj.D + 4) * EPS32 * (w2.abs() * mag).sum(-1) + EPS32 * s.abs())
    return s.cpu(), tau.cpu()


def _case_queries(n_ent, n_rel, seed):
    rs = np.random.RandomState(seed)
    known = rs.randint(0, [n_ent - 1, n_rel, n_ent - 1], size=(600, 3))
    known[:2, 1] = 0                                                             # the fully filtered groups stay off the last-id query's
    known = np.concatenate([known, known[:100]])                                 # duplicate known triples
    full = [[known[0, 0], known[0, 1], c] for c in range(n_ent)]                  # query 0: every tail candidate filtered
    full += [[c, known[1, 1], known[1, 2]] for c in range(n_ent)]                 # query 1: every head candidate filtered
    full += [[known[2, 0], r, known[2, 2]] for r in range(n_rel)]                 # query 2: every relation filtered
    known = np.concatenate([known, np.array(full)])
    queries = np.concatenate([known[:3], known[rs.randint(3, 700, 20)], rs.randint(0, [n_ent, n_rel, n_ent], size=(8, 3)),
                              [[n_ent - 1, n_rel - 1, n_ent - 1]]])              # last query: the last ids, empty filters
    return torch.from_numpy(known), torch.from_numpy(queries)


def test_kg_eval_reference_parity():
    from recon_amd.models import SpKBGATConvOnly
    from recon_amd import kg_eval
    g = load_golden("kgeval1")
    D = g["sd__final_entity_embeddings"].shape[1]
    m = SpKBGATConvOnly(torch.randn(int(g["n_ent"]), 8), torch.randn(int(g["n_rel"]), 8), [D // 2, D], [D // 2, D], 0.0, 0.0, 0.2, 0.2, [2, 2], 50)
    m.load_state_dict({k: torch.from_numpy(g["sd__" + k]) for k in m.state_dict()}, strict=True)
    m = m.to(DEV).eval()
    test = torch.from_numpy(g["test"]).to(DEV)
    known = torch.from_numpy(g["known"]).to(DEV)
    proj = kg_eval.convkb_projections(m.final_entity_embeddings, m.final_relation_embeddings, m.convKB)
    rel = kg_eval.relation_scores(proj, test)
    ref = torch.from_numpy(g["rel_scores"])
    assert rel.shape == ref.shape
    torch.testing.assert_close(rel.cpu(), ref, rtol=1e-5, atol=1e-6)
    with torch.no_grad():
        torch.testing.assert_close(m.batch_test(test).cpu(), torch.from_numpy(g["rel_scores"][np.arange(len(g["test"])), g["test"][:, 1]])[:, None],
                                   rtol=1e-5, atol=1e-6)
    metrics = m.evaluate(test, known, unique_entities=torch.from_numpy(g["unique"]).to(DEV))
    names = ("hits@100", "hits@10", "hits@3", "hits@1", "mean_rank", "mean_reciprocal_rank")
    for sec in ("head", "tail", "cumulative"):
        assert [metrics[sec][k] for k in names] == g["metrics_" + sec].tolist(), sec
    rh, rt, _ = kg_eval.rank_entities(proj, test, known, unique_entities=g["unique"])
    assert rh.cpu().tolist() == g["ranks_head64"].tolist() and rt.cpu().tolist() == g["ranks_tail64"].tolist()


@pytest.mark.parametrize("D", [1, 37, 200, 257])
def test_kg_eval_rank_self_consistent_and_fp64_band(D):
    from recon_amd import kg_eval
    n_ent, n_rel = 203, 11                                                       # neither a multiple of the 64-candidate tile
    proj = _proj(n_ent, n_rel, D, seed=D)
    known, queries = _case_queries(n_ent, n_rel, seed=D)
    qd, kd = queries.to(DEV), known.to(DEV)
    for slot in (kg_eval.SLOT_HEAD, kg_eval.SLOT_RELATION, kg_eval.SLOT_TAIL):
        n_slot = n_rel if slot == kg_eval.SLOT_RELATION else n_ent
        S = kg_eval.slot_scores(proj, qd, slot).cpu()
        s_true_dense = S[torch.arange(len(queries)), queries[:, slot]]
        excl = _excluded_mask(known, queries, slot, n_slot)
        s64, tau = _scores64(proj, queries, slot, torch.arange(n_slot))
        s64_true = s64[torch.arange(len(queries)), queries[:, slot]][:, None]
        t64_true = tau[torch.arange(len(queries)), queries[:, slot]][:, None]
        for filtered in (False, True):
            ranks, s_true = kg_eval.rank_slot(proj, qd, slot, kd if filtered else None)
            ranks, s_true = ranks.cpu(), s_true.cpu()
            assert torch.equal(s_true.view(torch.int32), s_true_dense.view(torch.int32)), (slot, filtered)
            keep = ~excl if filtered else torch.ones_like(excl)
            want = 1 + ((S > s_true[:, None]) & keep).sum(1)
            assert torch.equal(ranks, want), (slot, filtered)
            lo = 1 + ((s64 > s64_true + tau + t64_true) & keep).sum(1)
            hi = 1 + ((s64 > s64_true - tau - t64_true) & keep).sum(1)
            assert bool(((ranks >= lo) & (ranks <= hi)).all()), (slot, filtered)
            if filtered:
                assert ranks[{0: 1, 1: 2, 2: 0}[slot]].item() == 1                   # every candidate of that query filtered
                assert excl[-1].sum() == 0                                           # the last-id query has an empty filter


def test_kg_eval_at_size_and_deterministic():
    from recon_amd import kg_eval
    n_ent, n_rel, D, Q = 14541, 237, 200, 2048
    proj = _proj(n_ent, n_rel, D, seed=7)
    g = torch.Generator(device="cpu").manual_seed(3)
    known = torch.stack([torch.randint(0, n_ent, (310000,), generator=g), torch.randint(0, n_rel, (310000,), generator=g),
                         torch.randint(0, n_ent, (310000,), generator=g)], 1).to(DEV)
    queries = known[torch.randperm(known.shape[0], generator=g)[:Q].to(DEV)]
    for slot in (kg_eval.SLOT_HEAD, kg_eval.SLOT_TAIL):
        ranks, s_true = kg_eval.rank_slot(proj, queries, slot, known)
        ranks2, s_true2 = kg_eval.rank_slot(proj, queries, slot, known)
        assert torch.equal(ranks, ranks2) and torch.equal(s_true.view(torch.int32), s_true2.view(torch.int32))
        ids, begin, end = kg_eval.build_filter(known, queries, slot, (n_ent, n_rel))
        excl = torch.zeros(Q, n_ent, dtype=torch.bool, device=DEV)
        cnt = end - begin
        rows = torch.repeat_interleave(torch.arange(Q, device=DEV), cnt)
        pos = torch.arange(int(cnt.sum()), device=DEV) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt) + torch.repeat_interleave(begin, cnt)
        excl[rows, ids[pos]] = True
        want = torch.ones(Q, dtype=torch.int64, device=DEV)
        for c0 in range(0, n_ent, 4096):
            C = min(4096, n_ent - c0)
            S = kg_eval.slot_scores(proj, queries, slot, c0, C)
            want += ((S > s_true[:, None]) & ~excl[:, c0:c0 + C]).sum(1)
        assert torch.equal(ranks, want), slot
        sub = torch.arange(0, Q, Q // 64)[:64]
        q64 = queries[sub.to(DEV)].cpu()
        keep = ~excl[sub.to(DEV)].cpu()
        for k in range(0, 64, 2):                                                  # two queries at a time: ~50 MB per fp64 temporary
            s64, tau = _scores64(proj, q64[k:k + 2], slot, torch.arange(n_ent))
            i = torch.arange(2)
            st, tt = s64[i, q64[k:k + 2, slot]][:, None], tau[i, q64[k:k + 2, slot]][:, None]
            lo = 1 + ((s64 > st + tau + tt) & keep[k:k + 2]).sum(1)
            hi = 1 + ((s64 > st - tau - tt) & keep[k:k + 2]).sum(1)
            r = ranks[sub[k:k + 2].to(DEV)].cpu()
            assert bool(((r >= lo) & (r <= hi)).all()), (slot, k)


def test_kg_eval_rejects_bad_arguments():
    from recon_amd import _lib, kg_eval
    from recon_amd.models import SpKBGATConvOnly
    proj = _proj(50, 4, 16, seed=1)
    L = _lib.lib()
    tri = torch.tensor([[1, 2, 3]], device=DEV)
    out_r = torch.empty(1, dtype=torch.int64, device=DEV)
    out_s = torch.empty(1, device=DEV)
    ws = torch.empty(64, device=DEV)
    args = lambda slot, Q, D, slope: (slot, Q, tri.data_ptr(), proj.P_h.data_ptr(), proj.P_r.data_ptr(), proj.P_t.data_ptr(), 50, 4, D,
                                      proj.b1.data_ptr(), proj.w2.data_ptr(), proj.b2.data_ptr(), slope, None, None, None, ws.data_ptr(), 64,
                                      out_r.data_ptr(), out_s.data_ptr(), _lib.current_stream())
    assert L.recon_convkb_rank(*args(2, 1, -3, 0.01)) == -1                    # negative D
    assert L.recon_convkb_rank(*args(3, 1, 16, 0.01)) == -1                    # no such slot
    assert L.recon_convkb_rank(*args(2, -1, 16, 0.01)) == -1                   # negative Q
    assert L.recon_convkb_rank(*args(2, 1, 16, 1.5)) == -2                     # slope outside [0, 1]
    assert L.recon_convkb_rank(*args(2, 5, 16, 0.01)[:17] + (4,) + args(2, 5, 16, 0.01)[18:]) == -4   # workspace too small
    assert L.recon_convkb_scores(1, 1, tri.data_ptr(), proj.P_h.data_ptr(), proj.P_r.data_ptr(), proj.P_t.data_ptr(), 50, 4, 16,
                                 proj.b1.data_ptr(), proj.w2.data_ptr(), proj.b2.data_ptr(), 0.01, 2, 3, out_s.data_ptr(), 3, None) == -1   # c0 + C > n_rel
    for bad in ([[50, 0, 1]], [[0, 4, 1]], [[-1, 0, 1]]):
        with pytest.raises(ValueError):
            kg_eval.rank_entities(proj, torch.tensor(bad, device=DEV))
    with pytest.raises(RuntimeError):
        kg_eval.rank_entities(proj, tri.cpu())
    m = SpKBGATConvOnly(torch.randn(50, 8), torch.randn(4, 8), [8, 16], [8, 16], 0.0, 0.0, 0.2, 0.2, [2, 2], 50)
    with pytest.raises(RuntimeError):
        m.evaluate(tri.cpu(), tri.cpu())
    with pytest.raises(RuntimeError):
        m.batch_test(tri.cpu())
    torch.cuda.synchronize()
