"""Link-prediction evaluation of the ConvKB scorer on the device: what Corpus.get_validation_pred (GAT/create_batch.py:905-1199) and the
scoring half of get_validation_cnfmat (:1365-1420) compute with Python loops, np.tile and a torch.sort per test triple.

    proj = convkb_projections(model.final_entity_embeddings, model.final_relation_embeddings, model.convKB)
    ranks_head, ranks_tail, s_true = rank_entities(proj, test_triples, known_triples, unique_entities=...)
    metrics = link_prediction_metrics(ranks_head, ranks_tail)

fc1 is split along its concatenated input ([e_h; r; e_t] -> three D x D projections, recon_sgemm_ex on strided slices of W1); the
candidates are then scored, counted against the true score and filtered by the fused rank kernel of csrc/kg_eval.hip (no Q x N score
matrix, no sort).  Rank rule: 1 + #{candidates outside the filter scoring strictly above the true triple}, i.e. the true triple wins ties,
as it does at index 0 of the reference's descending sort.  Filters (valid_triples_dict) are built once, on the device, as sorted int64 keys.
"""
from collections import namedtuple

import torch

from . import _lib

SLOT_HEAD, SLOT_RELATION, SLOT_TAIL = 0, 1, 2          # RECON_KGE_* (include/recon_hip.h): the column of the triple that is replaced
_QUERY_CHUNK = 65535                                  # recon_convkb_scores: queries per call

ConvKBProjections = namedtuple("ConvKBProjections", "P_h P_r P_t b1 w2 b2 slope n_ent n_rel D")


def _check_ids(triples, n_ent, n_rel, name):
    """One device reduction and one host sync: every id of the [rows, 3] triples inside its table."""
    if triples.numel():
        lo, hi = triples.amin(0).tolist(), triples.amax(0).tolist()
        if min(lo) < 0 or hi[0] >= n_ent or hi[2] >= n_ent or hi[1] >= n_rel:
            raise ValueError("%s: an id lies outside its table (%d entities, %d relations)" % (name, n_ent, n_rel))


def _check_triples(triples, table, n_ent, n_rel, name="test_triples"):
    """The triples as contiguous int64 [Q, 3] on the device of `table` (a GPU tensor), every id inside its table."""
    _lib.require_gpu(triples, table)
    if triples.dim() != 2 or triples.shape[1] != 3:
        raise ValueError("%s: [Q, 3] (head, relation, tail) expected" % name)
    t = triples.to(device=table.device, dtype=torch.int64).contiguous()
    _check_ids(t, n_ent, n_rel, name)
    return t


def _check_shapes(entity_emb, relation_emb, convkb, who):
    """D of entity [N, D] and relation [R, D] tables scored by a ConvKB module with fc1 [D, 3D] and fc2 [1, D]; ValueError otherwise."""
    if entity_emb.dim() != 2 or relation_emb.dim() != 2 or relation_emb.shape[1] != entity_emb.shape[1]:
        raise ValueError("%s: entity [N, D] and relation [R, D] tables expected" % who)
    D = entity_emb.shape[1]
    if tuple(convkb.fc1.weight.shape) != (D, 3 * D) or tuple(convkb.fc2.weight.shape) != (1, D):
        raise ValueError("%s: fc1 [D, 3D], fc2 [1, D] expected" % who)
    return D


def _detached_weights(convkb):
    """fc1.weight, b1, w2 (flat) and b2 ([1]) of a ConvKB module as detached contiguous fp32 tensors, and the slope of its LeakyReLU nl1."""
    return (convkb.fc1.weight.detach().float().contiguous(), convkb.fc1.bias.detach().float().contiguous(),
            convkb.fc2.weight.detach().float().reshape(-1).contiguous(), convkb.fc2.bias.detach().float().reshape(1).contiguous(),
            float(convkb.nl1.negative_slope))


def _project(T, W1, k):
    """T W_k^T, fp32 [rows of T, D], with W_k block k of W1 = [W_h | W_r | W_t] (recon_sgemm_ex on the strided slice)."""
    n, D = T.shape
    P = torch.empty(n, D, device=T.device, dtype=torch.float32)
    with _lib.on_device(T.device):
        _lib.check(_lib.lib().recon_sgemm_ex(n, D, D, T.data_ptr(), D, 0, W1.data_ptr() + 4 * k * D, 3 * D, 1, P.data_ptr(), D, None,
                                             _lib.current_stream()), "recon_sgemm_ex")
    return P


def convkb_projections(entity_emb, relation_emb, convkb):
    """P_h = E W_h^T, P_r = Rel W_r^T, P_t = E W_t^T with fc1.weight = [W_h | W_r | W_t] (each [D, D], read in place: ldb = 3 D), plus b1, w2,
    b2 (device) and the LeakyReLU slope of convkb.nl1 (nn.LeakyReLU(): 0.01, whatever alpha_conv says — GAT/layers.py:24)."""
    _lib.require_gpu(entity_emb, relation_emb, convkb.fc1.weight, convkb.fc1.bias, convkb.fc2.weight, convkb.fc2.bias)
    D = _check_shapes(entity_emb, relation_emb, convkb, "convkb_projections")
    E = entity_emb.detach().float().contiguous()
    R = relation_emb.detach().float().contiguous()
    W1, b1, w2, b2, slope = _detached_weights(convkb)
    return ConvKBProjections(_project(E, W1, 0), _project(R, W1, 1), _project(E, W1, 2), b1, w2, b2, slope, E.shape[0], R.shape[0], D)


def filter_keys(triples, slot, sizes):
    """int64 key of every triple that sorts each query's excluded ids of `slot` into one contiguous run: tail (r, h, t), head (r, t, h),
    relation (h, t, r) — group columns first, the candidate id last.  sizes: (n_ent, n_rel)."""
    n_ent, n_rel = sizes
    n = (n_ent, n_rel, n_ent)
    cols = {SLOT_TAIL: (1, 0), SLOT_HEAD: (1, 2), SLOT_RELATION: (0, 2)}[slot]
    if n[cols[0]] * n[cols[1]] * n[slot] >= 1 << 62:
        raise ValueError("filter_keys: tables too large for int64 keys")
    return (triples[:, cols[0]] * n[cols[1]] + triples[:, cols[1]]) * n[slot] + triples[:, slot]


def build_filter(known_triples, queries, slot, sizes):
    """(ids, begin, end): the excluded ids of query q of `slot` are ids[begin[q]:end[q]] — the candidates c for which the query triple with
    c in the slot is one of known_triples (duplicates removed).  torch ops on the tensors' device."""
    n_slot = sizes[0] if slot != SLOT_RELATION else sizes[1]
    keys = torch.unique(filter_keys(known_triples, slot, sizes))          # sorted
    group = filter_keys(queries, slot, sizes) - queries[:, slot]          # the key of candidate 0
    begin = torch.searchsorted(keys, group)
    end = torch.searchsorted(keys, group + n_slot)
    return keys % n_slot, begin, end


def _rank_workspace(Q, D, device):
    """(workspace, floats) of recon_convkb_rank / recon_kgsep_rank for Q queries."""
    floats = _lib.lib().recon_convkb_rank_workspace_floats(Q, D)
    return torch.empty(floats, dtype=torch.float32, device=device), floats


def rank_slot(proj, triples, slot, known_triples=None):
    """Ranks (int64 [Q]) and true scores (fp32 [Q]) of the queries `triples` with column `slot` replaced by every id of its table; filtered by
    known_triples (the union of train, valid and test: valid_triples_dict) or raw (None)."""
    t = _check_triples(triples, proj.P_h, proj.n_ent, proj.n_rel)
    Q = t.shape[0]
    dev = t.device
    ranks = torch.empty(Q, dtype=torch.int64, device=dev)
    scores = torch.empty(Q, dtype=torch.float32, device=dev)
    if Q == 0:
        return ranks, scores
    filt = (None, None, None)
    if known_triples is not None:
        k = _check_triples(known_triples, proj.P_h, proj.n_ent, proj.n_rel, "known_triples")
        filt = build_filter(k, t, slot, (proj.n_ent, proj.n_rel))
    L = _lib.lib()
    ws, ws_floats = _rank_workspace(Q, proj.D, dev)
    with _lib.on_device(dev):
        _lib.check(L.recon_convkb_rank(slot, Q, t.data_ptr(), proj.P_h.data_ptr(), proj.P_r.data_ptr(), proj.P_t.data_ptr(), proj.n_ent, proj.n_rel,
                                       proj.D, proj.b1.data_ptr(), proj.w2.data_ptr(), proj.b2.data_ptr(), proj.slope, _lib.ptr(filt[0]),
                                       _lib.ptr(filt[1]), _lib.ptr(filt[2]), ws.data_ptr(), ws_floats, ranks.data_ptr(), scores.data_ptr(),
                                       _lib.current_stream()), "recon_convkb_rank")
    return ranks, scores


def _keep_unique(triples, unique_entities):
    """The reference's `continue` (GAT/create_batch.py:937-938): a query whose head or tail is not in unique_entities is dropped."""
    if unique_entities is None:
        return triples
    ue = torch.as_tensor(unique_entities, dtype=torch.int64, device=triples.device)
    keep = torch.isin(triples[:, 0], ue) & torch.isin(triples[:, 2], ue)
    return triples[keep]


def _entity_slots(side):
    """The slots that rank_entities' `side` ('both', 'head' or 'tail') ranks, head first."""
    if side not in ("both", "head", "tail"):
        raise ValueError("side: 'both', 'head' or 'tail'")
    return tuple(slot for slot, name in ((SLOT_HEAD, "head"), (SLOT_TAIL, "tail")) if side in ("both", name))


def rank_entities(proj, test_triples, known_triples=None, side="both", unique_entities=None):
    """Filtered (known_triples given) or raw entity ranks of every test triple: (ranks_head, ranks_tail, true_scores), device tensors; a side
    not asked for is None.  true_scores: s* of the tail pass (of the head pass when side == "head")."""
    slots = _entity_slots(side)
    t = _keep_unique(_check_triples(test_triples, proj.P_h, proj.n_ent, proj.n_rel), unique_entities)
    ranks, s = {}, None
    for slot in slots:
        ranks[slot], s = rank_slot(proj, t, slot, known_triples)
    return ranks.get(SLOT_HEAD), ranks.get(SLOT_TAIL), s


def rank_relations(proj, test_triples, known_triples=None):
    """Ranks of the true relation among all relations (relation slot), raw or filtered: (ranks, true_scores)."""
    return rank_slot(proj, test_triples, SLOT_RELATION, known_triples)


def slot_scores(proj, triples, slot, c0=0, C=None):
    """Dense scores S[q, j] = s(q with column `slot` = c0 + j), fp32 [Q, C] (the same score routine as the rank kernel: bit-identical)."""
    t = _check_triples(triples, proj.P_h, proj.n_ent, proj.n_rel)
    n_slot = proj.n_rel if slot == SLOT_RELATION else proj.n_ent
    C = n_slot - c0 if C is None else C
    S = torch.empty(t.shape[0], C, dtype=torch.float32, device=t.device)
    L = _lib.lib()
    with _lib.on_device(t.device):
        for q0 in range(0, t.shape[0], _QUERY_CHUNK):
            tq = t[q0:q0 + _QUERY_CHUNK]
            _lib.check(L.recon_convkb_scores(slot, tq.shape[0], tq.data_ptr(), proj.P_h.data_ptr(), proj.P_r.data_ptr(), proj.P_t.data_ptr(),
                                             proj.n_ent, proj.n_rel, proj.D, proj.b1.data_ptr(), proj.w2.data_ptr(), proj.b2.data_ptr(), proj.slope,
                                             c0, C, S[q0:].data_ptr(), C, _lib.current_stream()), "recon_convkb_scores")
    return S


def relation_scores(proj, test_triples):
    """[Q, R]: every test triple scored with every relation — the reference's `scores.view(-1, num_rels)` (GAT/create_batch.py:1369-1416)."""
    return slot_scores(proj, test_triples, SLOT_RELATION)


def _side_metrics(ranks, n):
    ranks = [int(r) for r in ranks]
    recip = [1.0 / r for r in ranks]
    return {"hits@100": sum(r <= 100 for r in ranks) / float(n), "hits@10": sum(r <= 10 for r in ranks) / n,
            "hits@3": sum(r <= 3 for r in ranks) / n, "hits@1": sum(r == 1 for r in ranks) / n,
            "mean_rank": sum(ranks) / len(ranks), "mean_reciprocal_rank": sum(recip) / len(recip)}


def link_prediction_metrics(ranks_head, ranks_tail):
    """Hits@100/10/3/1, mean rank and mean reciprocal rank per side and their cumulative averages, with the reference's formulas
    (GAT/create_batch.py:1100-1199; both sides' hit rates are divided by the number of head ranks, as there)."""
    rh = ranks_head.tolist() if torch.is_tensor(ranks_head) else list(ranks_head)
    rt = ranks_tail.tolist() if torch.is_tensor(ranks_tail) else list(ranks_tail)
    if not rh or len(rh) != len(rt):
        raise ValueError("link_prediction_metrics: two non-empty rank lists of one length expected")
    head, tail = _side_metrics(rh, len(rh)), _side_metrics(rt, len(rh))
    return {"head": head, "tail": tail, "cumulative": {k: (head[k] + tail[k]) / 2 for k in head}}
