"""Link-prediction evaluation of the GAT_sep_space ConvKB scorer on the device: filtered entity ranks, relation scores
and filtered relation ranks of SpKBGATConvOnly (GAT_sep_space/models.py:247-339), which carries both entities of a triple into its relation's
space, e' = tanh(E[e] W_ent2rel[r]), before ConvKB.

    scorer = sep_scorer(model_conv.final_entity_embeddings, model_conv.final_relation_embeddings, model_conv.convKB, model_gat)
    ranks_head, ranks_tail, s_true = rank_entities(scorer, test_triples, known_triples, unique_entities=...)
    S = relation_scores(scorer, test_triples)                       # [Q, R]: get_validation_cnfmat's scores (GAT_sep_space/create_batch.py:1360-1390)

With fc1.weight = [W_h | W_r | W_t] the entity tables of recon_amd.kg_eval become per relation, P_h^r = tanh(E W_ent2rel[r]) W_h^T and
P_t^r = tanh(E W_ent2rel[r]) W_t^T (csrc/kg_sep.hip); P_r = Rel W_r^T is kg_eval's.  The tables are built for chunks of relations under a
byte budget, and the relation-segmented kernels of csrc/kg_eval.hip score every (query, candidate) pair with kg_eval's one score routine on
the tables of the query's relation: a score here is bit-identical to kg_eval's on ConvKBProjections(P_h^r, P_r, P_t^r, ...).
"""
from collections import namedtuple

import torch

from . import _lib
from . import kg_eval as _kge

MAX_D = 512                                           # recon_kgsep_tables
DEFAULT_BUDGET = 1 << 30                              # bytes of P_h^r + P_t^r per chunk: 46 relations at 14 541 entities x D = 200

SepScorer = namedtuple("SepScorer", "E W_ent2rel W1 P_r b1 w2 b2 slope n_ent n_rel D")


def _is_tanh(f):
    return f is torch.tanh or f is torch.nn.functional.tanh or f is torch.Tensor.tanh or isinstance(f, torch.nn.Tanh)


def check_ent2rel(model_gat, n_rel, D):
    """W_ent2rel [n_rel, D, D] and a tanh nonlinearity_ent2rel (the device kernels hard-code tanh); ValueError otherwise."""
    W = getattr(model_gat, "W_ent2rel", None)
    if not torch.is_tensor(W) or W.dim() != 3 or tuple(W.shape) != (n_rel, D, D):
        raise ValueError("model_gat.W_ent2rel: [%d, %d, %d] (num_relation, D, D) expected, got %s"
                         % (n_rel, D, D, None if not torch.is_tensor(W) else tuple(W.shape)))
    if not _is_tanh(getattr(model_gat, "nonlinearity_ent2rel", None)):
        raise ValueError("model_gat.nonlinearity_ent2rel: the device evaluation of the GAT_sep_space scorer supports torch.tanh only")
    if D > MAX_D:
        raise ValueError("GAT_sep_space evaluation: D = %d, at most %d supported" % (D, MAX_D))
    return W


def sep_scorer(entity_emb, relation_emb, convkb, model_gat):
    """Everything the kernels read: E, W_ent2rel, fc1.weight (in place, ldb = 3 D), P_r = Rel W_r^T (recon_sgemm_ex, as
    kg_eval.convkb_projections), b1, w2, b2 and nl1's slope.  Arguments are checked before any device work."""
    D = _kge._check_shapes(entity_emb, relation_emb, convkb, "sep_scorer")
    N, R = entity_emb.shape[0], relation_emb.shape[0]
    W = check_ent2rel(model_gat, R, D)
    _lib.require_gpu(entity_emb, relation_emb, W, convkb.fc1.weight, convkb.fc1.bias, convkb.fc2.weight, convkb.fc2.bias)
    W1, b1, w2, b2, slope = _kge._detached_weights(convkb)
    P_r = _kge._project(relation_emb.detach().float().contiguous(), W1, 1)
    return SepScorer(entity_emb.detach().float().contiguous(), W.detach().float().contiguous(), W1, P_r, b1, w2, b2, slope, N, R, D)


def plan_chunks(relations, n_rows, D, budget_bytes=DEFAULT_BUDGET):
    """Split `relations` (ids, in order) into consecutive chunks whose tables P_h^r + P_t^r ([n_rows, D] fp32 each) fit budget_bytes."""
    per = 2 * 4 * int(n_rows) * int(D)
    if per > budget_bytes:
        raise ValueError("plan_chunks: one relation's tables take %d bytes, more than the budget of %d" % (per, budget_bytes))
    k = max(1, min(65535, budget_bytes // max(per, 1)))
    rel = list(relations)
    return [rel[i:i + k] for i in range(0, len(rel), k)]


def relation_tables(scorer, rel_ids, ids=None):
    """(P_h, P_t), fp32 [len(rel_ids), U, D]: the tables of the relations rel_ids over the entity rows ids (int64, None: all entities)."""
    dev = scorer.E.device
    rel = torch.as_tensor(rel_ids, dtype=torch.int64, device=dev).reshape(-1).contiguous()
    if rel.numel() and (int(rel.min()) < 0 or int(rel.max()) >= scorer.n_rel):
        raise ValueError("relation_tables: a relation id lies outside [0, %d)" % scorer.n_rel)
    if ids is not None:
        ids = torch.as_tensor(ids, dtype=torch.int64, device=dev).reshape(-1).contiguous()
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= scorer.n_ent):
            raise ValueError("relation_tables: an entity id lies outside [0, %d)" % scorer.n_ent)
    U = scorer.n_ent if ids is None else ids.numel()
    P_h = torch.empty(rel.numel(), U, scorer.D, device=dev, dtype=torch.float32)
    P_t = torch.empty_like(P_h)
    with _lib.on_device(dev):
        _lib.check(_lib.lib().recon_kgsep_tables(scorer.E.data_ptr(), scorer.n_ent, _lib.ptr(ids), U, scorer.W_ent2rel.data_ptr(), scorer.n_rel,
                                                 rel.data_ptr(), rel.numel(), scorer.W1.data_ptr(), scorer.D, P_h.data_ptr(), P_t.data_ptr(),
                                                 _lib.current_stream()), "recon_kgsep_tables")
    return P_h, P_t


def relation_projections(scorer, P_h, P_t, k):
    """kg_eval.ConvKBProjections of local relation k of a chunk's tables: what recon_amd.kg_eval scores the same pairs with."""
    return _kge.ConvKBProjections(P_h[k], scorer.P_r, P_t[k], scorer.b1, scorer.w2, scorer.b2, scorer.slope, P_h.shape[1], scorer.n_rel, scorer.D)


def _check(scorer, triples, name="test_triples"):
    return _kge._check_triples(triples, scorer.E, scorer.n_ent, scorer.n_rel, name)


def _rank_chunk(scorer, t, rel, seg, P_h, P_t, slot, filt, ranks, scores):
    L = _lib.lib()
    Q = t.shape[0]
    ws, ws_floats = _kge._rank_workspace(Q, scorer.D, t.device)
    with _lib.on_device(t.device):
        _lib.check(L.recon_kgsep_rank(slot, Q, t.data_ptr(), seg.data_ptr(), rel.numel(), P_h.data_ptr(), scorer.P_r.data_ptr(), P_t.data_ptr(),
                                      P_h.shape[1], scorer.n_rel, scorer.D, scorer.b1.data_ptr(), scorer.w2.data_ptr(), scorer.b2.data_ptr(),
                                      scorer.slope, _lib.ptr(filt[0]), _lib.ptr(filt[1]), _lib.ptr(filt[2]), ws.data_ptr(), ws_floats,
                                      ranks.data_ptr(), scores.data_ptr(), _lib.current_stream()), "recon_kgsep_rank")


def rank_entities(scorer, test_triples, known_triples=None, side="both", unique_entities=None, budget_bytes=DEFAULT_BUDGET):
    """Filtered (known_triples given) or raw head / tail ranks of the sep scorer: (ranks_head, ranks_tail, true_scores) as
    kg_eval.rank_entities, with the queries dropped by unique_entities removed first.  The queries are sorted by relation; each chunk's
    tables (all entities) are built once and serve both sides."""
    sides = _kge._entity_slots(side)
    t = _kge._keep_unique(_check(scorer, test_triples), unique_entities)
    k = None if known_triples is None else _check(scorer, known_triples, "known_triples")
    Q, dev = t.shape[0], t.device
    ranks = {s: torch.empty(Q, dtype=torch.int64, device=dev) for s in sides}
    true = torch.empty(Q, dtype=torch.float32, device=dev)
    order = torch.argsort(t[:, 1], stable=True)
    ts = t[order].contiguous()
    counts = torch.bincount(ts[:, 1], minlength=scorer.n_rel)
    start = torch.cumsum(counts, 0) - counts
    present = torch.nonzero(counts).reshape(-1).tolist()
    cnt, st = counts.tolist(), start.tolist()
    for chunk in plan_chunks(present, scorer.n_ent, scorer.D, budget_bytes):
        q0, q1 = st[chunk[0]], st[chunk[-1]] + cnt[chunk[-1]]
        tq = ts[q0:q1]
        seg = torch.tensor([0] + [st[r] + cnt[r] - q0 for r in chunk], dtype=torch.int64, device=dev)
        P_h, P_t = relation_tables(scorer, chunk)
        rel = torch.tensor(chunk, dtype=torch.int64, device=dev)
        for s in sides:
            filt = (None, None, None) if k is None else _kge.build_filter(k, tq, s, (scorer.n_ent, scorer.n_rel))
            r_out = torch.empty(q1 - q0, dtype=torch.int64, device=dev)
            s_out = torch.empty(q1 - q0, dtype=torch.float32, device=dev)
            _rank_chunk(scorer, tq, rel, seg, P_h, P_t, s, filt, r_out, s_out)
            ranks[s][order[q0:q1]] = r_out
            true[order[q0:q1]] = s_out
        del P_h, P_t
    return ranks.get(_kge.SLOT_HEAD), ranks.get(_kge.SLOT_TAIL), true


def relation_scores(scorer, test_triples, budget_bytes=DEFAULT_BUDGET):
    """[Q, R]: every test triple scored with every relation, the `scores` of get_validation_cnfmat (GAT_sep_space/create_batch.py:1360-1390)
    before its view(-1, num_rels).  The tables cover the queries' entities only; the triples are remapped to table rows."""
    t = _check(scorer, test_triples)
    Q, dev = t.shape[0], t.device
    S = torch.empty(Q, scorer.n_rel, dtype=torch.float32, device=dev)
    if Q == 0:
        return S
    ue = torch.unique(torch.cat([t[:, 0], t[:, 2]]))
    rows = torch.stack([torch.searchsorted(ue, t[:, 0].contiguous()), t[:, 1], torch.searchsorted(ue, t[:, 2].contiguous())], 1).contiguous()
    L = _lib.lib()
    for chunk in plan_chunks(range(scorer.n_rel), ue.numel(), scorer.D, budget_bytes):
        P_h, P_t = relation_tables(scorer, chunk, ue)
        rel = torch.tensor(chunk, dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.recon_kgsep_scores(Q, rows.data_ptr(), rel.data_ptr(), rel.numel(), P_h.data_ptr(), scorer.P_r.data_ptr(), P_t.data_ptr(),
                                            ue.numel(), scorer.n_rel, scorer.D, scorer.b1.data_ptr(), scorer.w2.data_ptr(), scorer.b2.data_ptr(),
                                            scorer.slope, S.data_ptr(), scorer.n_rel, _lib.current_stream()), "recon_kgsep_scores")
        del P_h, P_t
    return S


def rank_relations(scorer, test_triples, known_triples=None, budget_bytes=DEFAULT_BUDGET):
    """Ranks of the true relation among all relations, raw or filtered, from the dense relation scores with kg_eval's tie rule
    (1 + #{r' not excluded : S[q, r'] > S[q, r]}): (ranks, true_scores).  Exact: every score comes from the one score routine."""
    t = _check(scorer, test_triples)
    S = relation_scores(scorer, t, budget_bytes)
    Q = t.shape[0]
    s_true = S[torch.arange(Q, device=t.device), t[:, 1]]
    above = S > s_true[:, None]
    if known_triples is not None and Q:
        ids, begin, end = _kge.build_filter(_check(scorer, known_triples, "known_triples"), t, _kge.SLOT_RELATION, (scorer.n_ent, scorer.n_rel))
        cnt = end - begin
        qi = torch.repeat_interleave(torch.arange(Q, device=t.device), cnt)
        pos = torch.arange(int(cnt.sum()), device=t.device) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt) + torch.repeat_interleave(begin, cnt)
        above[qi, ids[pos]] = False
    return 1 + above.sum(1), s_true
