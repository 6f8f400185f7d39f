#!/usr/bin/env python3
"""Generate tests/golden/kgsep1.npz by RUNNING THE REFERENCE (CPU): the link-prediction evaluation of the GAT_sep_space ConvKB scorer.

Reference entry points executed (unmodified, imported from where they lie):
  GAT_sep_space/models.py:91-245   SpKBGATModified (model_gat: W_ent2rel, nonlinearity_ent2rel = torch.tanh)
  GAT_sep_space/models.py:247-339  SpKBGATConvOnly (constructor, state_dict, forward / batch_test(batch, model_gat) -> ConvKB.forward)
  GAT_sep_space/create_batch.py:17-86     Corpus (valid_triples_dict, test_indices)
  GAT_sep_space/create_batch.py:905-1199  Corpus.get_validation_pred: filtered head / tail ranks and the printed hits@100/10/3/1, MR, MRR.
                                It calls model.batch_test(x) with one argument; a two-line adapter hands model_gat to the sep scorer's
                                batch_test.  .cuda() is the identity for the call and the printed averages are parsed, as in
                                gen_golden_kgeval.py.
  GAT_sep_space/create_batch.py:1360-1390 the relation-prediction tiling of get_validation_cnfmat, scored by batch_test(..., model_gat) 100 rows
                                at a time (Q R = 360, so no call sees a single row and the bare .squeeze() keeps its [T, D] shape)

The synthetic KG is reseeded until no candidate outside a query's filter scores within 1e-4 (relative) of the true triple in an fp64
recomputation, so the fixture does not depend on how a sort orders ties.  The fp64 ranks are stored too.

Usage:  python tests/golden/gen_golden_kgsep.py          (rewrites tests/golden/kgsep1.npz; needs the reference)
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import REF, _install_shims, save, synthetic_kg  # noqa: E402
from gen_golden_kgeval import _parse  # noqa: E402

N_ENT, N_REL, N_TEST, N_VALID = 300, 6, 60, 60
HEADS, DIM = 2, 12                          # D = entity_out_dim[0] * nheads_GAT[0] = 24
TIE_REL = 1e-4


def _import_ref():
    sep = os.path.join(REF, "GAT_sep_space")
    sys.path.insert(0, sep)
    try:
        for k in ("layers", "models", "create_batch"):
            sys.modules.pop(k, None)
        models = importlib.import_module("models")
        cb = importlib.import_module("create_batch")
    finally:
        sys.path.remove(sep)
    assert models.__file__.startswith(sep) and cb.__file__.startswith(sep)
    return models, cb


class _Adapter:
    """get_validation_pred calls model.batch_test(x); the sep scorer needs model_gat as well."""

    def __init__(self, conv, gat):
        self.conv, self.gat = conv, gat

    def batch_test(self, x):
        return self.conv.batch_test(x, self.gat)


def _scores64(conv, gat, h, r, t):
    """The sep scorer in fp64 on id arrays: tanh(E[e] W_ent2rel[r]) for both entities, then ConvKB (fc1, LeakyReLU 0.01, fc2)."""
    E = conv.final_entity_embeddings.detach().double()
    R = conv.final_relation_embeddings.detach().double()
    W = gat.W_ent2rel.detach().double()[r]
    eh = torch.tanh(torch.bmm(E[h].unsqueeze(1), W)).squeeze(1)
    et = torch.tanh(torch.bmm(E[t].unsqueeze(1), W)).squeeze(1)
    x = torch.cat([eh, R[r], et], 1)
    k = conv.convKB
    y = torch.nn.functional.leaky_relu(x @ k.fc1.weight.detach().double().T + k.fc1.bias.detach().double(), 0.01)
    return (y @ k.fc2.weight.detach().double().T + k.fc2.bias.detach().double()).reshape(-1)


def _ranks64(conv, gat, test, known, unique):
    """Filtered ranks of the kept test triples in fp64, and the smallest relative gap between a true score and an unfiltered candidate."""
    ks = set(map(tuple, known.tolist()))
    rh, rt, gap = [], [], np.inf
    cand = torch.arange(N_ENT)
    for h, r, t in test.tolist():
        if h not in unique or t not in unique:
            continue
        for side, out in ((0, rh), (2, rt)):
            tri = [[c if side == 0 else h, r, c if side == 2 else t] for c in range(N_ENT)]
            keep = torch.tensor([tuple(x) not in ks for x in tri])
            s = _scores64(conv, gat, torch.tensor([x[0] for x in tri]), torch.full((N_ENT,), r), torch.tensor([x[2] for x in tri]))
            s_true = s[h if side == 0 else t]
            sc = s[cand[keep]]
            if sc.numel():
                gap = min(gap, ((sc - s_true).abs() / max(abs(s_true.item()), 1e-30)).min().item())
            out.append(1 + int((sc > s_true).sum()))
    return np.array(rh, np.int64), np.array(rt, np.int64), gap


def main():
    if not os.path.isdir(REF):
        sys.exit("the reference is not mounted here; golden vectors can only be regenerated in the build container")
    torch.set_num_threads(4)
    _install_shims()
    if "sklearn" not in sys.modules:                          # create_batch.py imports sklearn.metrics (the confusion matrix only)
        sk, skm = types.ModuleType("sklearn"), types.ModuleType("sklearn.metrics")
        skm.multilabel_confusion_matrix = None
        sk.metrics = skm
        sys.modules.setdefault("sklearn", sk)
        sys.modules.setdefault("sklearn.metrics", skm)
    models, cb = _import_ref()
    for seed in range(200):
        h, r, t = synthetic_kg(N_ENT, N_REL, 1300, seed)
        tri = np.unique(np.stack([h, r, t], 1), axis=0)
        rs = np.random.RandomState(seed)
        tri = tri[rs.permutation(len(tri))]
        test, valid, train = tri[:N_TEST], tri[N_TEST:N_TEST + N_VALID], tri[N_TEST + N_VALID:]
        dropped = np.array([test[0, 0], test[1, 2], test[2, 0]])                   # a few test triples leave through unique_entities
        unique = sorted(set(range(N_ENT)) - set(dropped.tolist()))
        torch.manual_seed(seed)
        ent0, rel0 = torch.randn(N_ENT, 8), torch.randn(N_REL, 8)
        gat = models.SpKBGATModified(ent0, rel0, [DIM, DIM * HEADS], [DIM * HEADS, DIM * HEADS], 0.0, 0.2, [HEADS, HEADS], None)
        conv = models.SpKBGATConvOnly(ent0, rel0, [DIM, DIM * HEADS], [DIM, DIM * HEADS], 0.0, 0.0, 0.2, 0.2, [HEADS, HEADS], 50)
        gat.eval()
        conv.eval()
        rh64, rt64, gap = _ranks64(conv, gat, test, tri, set(unique))
        if gap > TIE_REL and len(rh64) < N_TEST:
            break
    else:
        sys.exit("no seed without near ties")
    print("seed %d: %d of %d test triples kept, smallest relative gap %.2e" % (seed, len(rh64), N_TEST, gap))

    as_list = lambda a: [tuple(x) for x in a.tolist()]
    adj = ([0], [0], [0])
    e2i = {"e%d" % i: i for i in range(N_ENT)}
    r2i = {"r%d" % i: i for i in range(N_REL)}
    args = types.SimpleNamespace(entities_per_batch=5, partial_2hop=False, data="synthetic")
    uniq_names = ["e%d" % i for i in unique]
    C = cb.Corpus(args, (as_list(train), adj), (as_list(valid), adj), (as_list(test), adj), e2i, r2i, None, 8, 2, uniq_names, uniq_names,
                  None, None, None, get_2hop=False, get_1hop=False)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        buf = io.StringIO()
        with torch.no_grad(), contextlib.redirect_stdout(buf):
            C.get_validation_pred(args, _Adapter(conv, gat), unique)
        # relation prediction: the tiling of get_validation_cnfmat (:1360-1390), 100 rows per batch_test call
        pred = np.tile(np.expand_dims(test.copy(), 1), (1, N_REL, 1))
        for rel_id in range(N_REL):
            pred[:, rel_id, 1] = rel_id
        pred = pred.reshape(-1, 3)
        assert len(pred) % 100 != 1
        with torch.no_grad():
            rel_scores = torch.cat([conv.batch_test(torch.LongTensor(pred[i:i + 100]), gat) for i in range(0, len(pred), 100)]).view(-1, N_REL)
            fwd_batch = torch.LongTensor(tri[::7][:50])
            fwd_out = conv(None, None, fwd_batch, gat)
    finally:
        torch.Tensor.cuda = cuda
    printed = _parse(buf.getvalue())
    assert abs(printed["head"][4] - rh64.mean()) < 1e-9 and abs(printed["tail"][4] - rt64.mean()) < 1e-9, (printed, rh64.mean(), rt64.mean())
    sd = conv.state_dict()
    arrays = {"sd__" + k: v.detach().numpy() for k, v in sd.items()}
    save("kgsep1", sd_keys=np.array(list(sd.keys())), gat__W_ent2rel=gat.W_ent2rel.detach().numpy(), test=test, known=tri,
         unique=np.array(unique, np.int64), n_ent=np.array(N_ENT), n_rel=np.array(N_REL), ranks_head64=rh64, ranks_tail64=rt64,
         metrics_head=printed["head"], metrics_tail=printed["tail"], metrics_cumulative=printed["cumulative"], rel_scores=rel_scores.numpy(),
         fwd_batch=fwd_batch.numpy(), fwd_out=fwd_out.numpy(), **arrays)


if __name__ == "__main__":
    main()
