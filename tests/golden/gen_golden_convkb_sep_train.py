#!/usr/bin/env python3
"""Generate tests/golden/convkb_sep_train1.npz by RUNNING THE REFERENCE (CPU): stage B of the GAT_sep_space tree, one training step of its
ConvKB scorer.

Reference entry points executed (unmodified, imported from where they lie):
  GAT_sep_space/create_batch.py:17-86    Corpus (train_indices, valid_triples_dict)
  GAT_sep_space/create_batch.py:103-260  Corpus.get_iteration_batch(1): that tree's train_conv passes the iteration number
                                         (GAT_sep_space/main.py:845), so the recorded batch is the second one, ratio 4
  GAT_sep_space/models.py:91-245         SpKBGATModified (model_gat: W_ent2rel, nonlinearity_ent2rel = torch.tanh)
  GAT_sep_space/models.py:247-324        SpKBGATConvOnly (constructor, forward(Corpus_, adj, batch, model_gat) -> ConvKB.forward)

The step around them follows train_conv (GAT_sep_space/main.py:803-905): frozen tables, Adam over the scorer's parameters only, the
class-weighted BCE on the scores, backward and one optimizer step.  model_gat is not stepped; W_ent2rel is frozen here so that its dead
gradient is not computed.  The batch is stored with its layout signature (per row: base positive, replaced column or -1, value), as in
gen_golden_convkb_train.py: a device sampler cannot replay numpy's stream.

Usage:  python tests/golden/gen_golden_convkb_sep_train.py          (rewrites tests/golden/convkb_sep_train1.npz; needs the reference)
"""
import contextlib
import importlib
import importlib.machinery
import io
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import REF, _install_shims, save  # noqa: E402
from gen_golden_convkb_train import _signature  # noqa: E402

N_ENT, N_REL, B, RATIO = 40, 12, 8, 4
HEADS, DIM = 2, 12                          # D = entity_out_dim[0] * nheads_GAT[0] = 24
LR, WEIGHT_DECAY = 1e-3, 1e-5


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


def _kg():
    rs = np.random.RandomState(9)
    pairs = {}                                                               # one relation per (head, tail) pair: no relation give-up
    while len(pairs) < 150:
        pairs.setdefault((int(rs.randint(N_ENT)), int(rs.randint(N_ENT))), int(rs.randint(N_REL)))
    tri = sorted((h, r, t) for (h, t), r in pairs.items())
    tri = [tri[i] for i in rs.permutation(len(tri))]
    return tri[:100], tri[100:120], tri[120:]


def _weighted_bce(scores, values, ratio):
    """Positives (value +1) weigh 1, negatives (value -1) weigh 1 / (2 ratio); mean of the weighted logistic losses."""
    target = (values.view(-1) + 1) / 2
    weight = target + (1 - target) / (2 * ratio)
    return torch.nn.functional.binary_cross_entropy_with_logits(scores.view(-1), target, weight=weight)


def main():
    if not os.path.isdir(REF):
        sys.exit("the reference is not mounted here; golden vectors can only be regenerated in the build container")
    torch.set_num_threads(4)
    _install_shims()
    if "sklearn" not in sys.modules:                          # create_batch.py imports sklearn.metrics (the confusion matrix only)
        sk, skm = types.ModuleType("sklearn"), types.ModuleType("sklearn.metrics")
        sk.__spec__ = importlib.machinery.ModuleSpec("sklearn", None)           # torch.optim's import of dynamo looks specs up
        skm.__spec__ = importlib.machinery.ModuleSpec("sklearn.metrics", None)
        skm.multilabel_confusion_matrix = None
        sk.metrics = skm
        sys.modules.setdefault("sklearn", sk)
        sys.modules.setdefault("sklearn.metrics", skm)
    models, cb = _import_ref()
    train, valid, test = _kg()
    adj = ([0], [0], [0])
    names = ["e%d" % i for i in range(N_ENT)]
    args = types.SimpleNamespace(entities_per_batch=5, partial_2hop=False, data="synthetic")
    with contextlib.redirect_stdout(io.StringIO()):
        C = cb.Corpus(args, (train, adj), (valid, adj), (test, adj), {n: i for i, n in enumerate(names)},
                      {"r%d" % i: i for i in range(N_REL)}, None, B, RATIO, names, names, None, None, None, get_2hop=False, get_1hop=False)
    np.random.seed(17)
    idx, val = C.get_iteration_batch(1)
    idx, val = idx.astype(np.int64), val.reshape(-1).astype(np.float32)
    pos = C.train_indices[B:2 * B].astype(np.int64)
    base, col, v = _signature(pos, idx, val)
    assert (col[B:] >= 0).all()                                              # every corruption replaced a column

    torch.manual_seed(5)
    ent0, rel0 = torch.randn(N_ENT, 8), torch.randn(N_REL, 8)
    gat = models.SpKBGATModified(ent0, rel0, [DIM, DIM * HEADS], [DIM * HEADS, DIM * HEADS], 0.0, 0.2, [HEADS, HEADS], None)
    conv = models.SpKBGATConvOnly(ent0, rel0, [DIM, DIM * HEADS], [DIM, DIM * HEADS], 0.0, 0.0, 0.2, 0.2, [HEADS, HEADS], 50)
    conv.train()
    conv.final_entity_embeddings.requires_grad = False
    conv.final_relation_embeddings.requires_grad = False
    gat.W_ent2rel.requires_grad = False
    sd0 = {k: t.detach().clone() for k, t in conv.state_dict().items()}
    opt = torch.optim.Adam(conv.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
    preds = conv(C, C.train_adj_matrix, torch.LongTensor(idx), gat)
    opt.zero_grad()
    loss = _weighted_bce(preds, torch.from_numpy(val), RATIO)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in conv.named_parameters() if p.grad is not None}
    assert sorted(grads) == ["convKB.fc1.bias", "convKB.fc1.weight", "convKB.fc2.bias", "convKB.fc2.weight"], sorted(grads)
    opt.step()
    out = {"train": np.array(train, np.int64), "valid": np.array(valid, np.int64), "test": np.array(test, np.int64), "n_ent": np.array(N_ENT),
           "n_rel": np.array(N_REL), "batch_size": np.array(B), "iter": np.array(1), "ratio": np.array(RATIO), "positives": pos,
           "indices": idx, "values": v, "base": base, "col": col, "gat__W_ent2rel": gat.W_ent2rel.detach().numpy(),
           "sd_keys": np.array(list(sd0.keys())), "preds": preds.detach().numpy().reshape(-1), "loss": np.array(loss.item(), np.float32),
           "lr": np.array(LR), "weight_decay": np.array(WEIGHT_DECAY)}
    out.update({"sd__" + k: t.numpy() for k, t in sd0.items()})
    out.update({"grad__" + k: t.numpy() for k, t in grads.items()})
    out.update({"after__" + k: conv.state_dict()[k].detach().numpy() for k in grads})
    save("convkb_sep_train1", **out)


if __name__ == "__main__":
    main()
