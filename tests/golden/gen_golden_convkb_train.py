#!/usr/bin/env python3
"""Generate tests/golden/convkb_train1.npz by RUNNING THE REFERENCE (CPU): stage B of KB-GAT, the training of the ConvKB scorer.

Reference entry points executed (unmodified, imported from where they lie):
  GAT/create_batch.py:17-86     Corpus (train_indices, train_values, valid_triples_dict)
  GAT/create_batch.py:103-260   Corpus.get_iteration_batch: the positives and their filtered corruptions, for ratio 4 and 3 (iter_num 0)
                                and for the short last batch (iter_num 1 of a train set of batch_size + 3 triples)
  GAT/models.py:240-304         SpKBGATConvOnly (constructor, forward -> ConvKB.forward, GAT/layers.py:41-46)
  GAT/main.py:741-742, :750-751, :793-843   the training step of train_conv: frozen tables, Adam(lr, weight_decay), preds, the weighted
                                BCE (restated line for line: it sits inside train_conv's loop), backward, one optimizer step

The numpy stream of the reference cannot be matched by a device sampler, so each batch is stored with its layout signature: per row the
base positive, the replaced column (-1: none) and the value.  The KG links one (head, tail) pair by every relation, and two of the
positives are on that pair, so the reference's give-up rule for relation draws fires on them deterministically.

Usage:  python tests/golden/gen_golden_convkb_train.py          (rewrites tests/golden/convkb_train1.npz; needs the reference)
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

N_ENT, N_REL, B = 40, 12, 8
HEADS, DIM = 2, 12                          # D = entity_out_dim[0] * nheads_GAT[0] = 24
FULL_H, FULL_T = 3, 7                       # (FULL_H, r, FULL_T) is known for every relation r
LR, WEIGHT_DECAY = 1e-3, 1e-5


def _import_ref():
    gat = os.path.join(REF, "GAT")
    sys.path.insert(0, gat)
    try:
        for k in ("layers", "models", "create_batch"):
            sys.modules.pop(k, None)
        models = importlib.import_module("models")
        cb = importlib.import_module("create_batch")
    finally:
        sys.path.remove(gat)
    assert models.__file__.startswith(REF) and cb.__file__.startswith(REF)
    return models, cb


def _kg():
    rs = np.random.RandomState(5)
    pairs = {}                                                               # one relation per (head, tail) pair: a give-up elsewhere
    while len(pairs) < 150:                                                  # would need 12 draws in a row of that relation (p ~ 1e-13)
        pairs.setdefault((int(rs.randint(N_ENT)), int(rs.randint(N_ENT))), int(rs.randint(N_REL)))
    pairs.pop((FULL_H, FULL_T), None)
    full = [(FULL_H, r, FULL_T) for r in range(N_REL)]
    tri = sorted((h, r, t) for (h, t), r in pairs.items())
    order = rs.permutation(len(tri))
    tri = [tri[i] for i in order]
    train = tri[:100]
    train[1], train[4] = full[0], full[2]                                    # two positives of every batch on the saturated pair
    rest = [x for x in full if x not in train]
    train = train + rest[:4]
    valid = tri[100:120] + rest[4:]
    test = tri[120:]
    return train, valid, test


def _corpus(cb, train, valid, test, ratio):
    adj = ([0], [0], [0])
    e2i = {"e%d" % i: i for i in range(N_ENT)}
    r2i = {"r%d" % i: i for i in range(N_REL)}
    args = types.SimpleNamespace(entities_per_batch=5, partial_2hop=False, data="synthetic")
    names = list(e2i)
    with contextlib.redirect_stdout(io.StringIO()):
        return cb.Corpus(args, (train, adj), (valid, adj), (test, adj), e2i, r2i, None, B, ratio, names, names, None, None, None,
                         get_2hop=False, get_1hop=False)


def _signature(pos, idx, val):
    """(base positive, replaced column or -1, value) of every row of a reference batch."""
    b = len(pos)
    base = np.array([o if o < b else (o - b) % b for o in range(len(idx))], np.int64)
    diff = idx != pos[base]
    assert (diff.sum(1) <= 1).all()
    col = np.where(diff.any(1), diff.argmax(1), -1).astype(np.int64)
    return base, col, val.reshape(-1).astype(np.float32)


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
    out = {"train": np.array(train, np.int64), "valid": np.array(valid, np.int64), "test": np.array(test, np.int64),
           "n_ent": np.array(N_ENT), "n_rel": np.array(N_REL), "batch_size": np.array(B)}
    batches = {}
    for name, ratio, n_train, iter_num in (("r4", 4, len(train), 0), ("r3", 3, len(train), 0), ("short", 4, B + 3, 1)):
        C = _corpus(cb, train[:n_train], valid + train[n_train:], test, ratio)
        np.random.seed(11 + ratio)
        idx, val = C.get_iteration_batch(iter_num)
        idx, val = idx.copy(), val.copy()
        lo = B * iter_num
        pos = C.train_indices[lo:lo + B].astype(np.int64)
        base, col, v = _signature(pos, idx.astype(np.int64), val)
        out.update({name + "_ratio": np.array(ratio), name + "_n_train": np.array(n_train), name + "_iter": np.array(iter_num),
                    name + "_positives": pos, name + "_indices": idx.astype(np.int64), name + "_values": v, name + "_base": base,
                    name + "_col": col})
        batches[name] = (idx, val, ratio)
        print("%-5s ratio %d: %d rows, %d replaced, %d give-ups" % (name, ratio, len(idx), (col >= 0).sum(),
                                                                    ((col < 0) & (np.arange(len(idx)) >= len(pos))).sum()))
    give_ups = (out["r4_col"][B:] < 0).sum()
    assert give_ups == 2 * 4, give_ups                                       # every relation row of the two saturated positives, no other

    # one training step of train_conv on the recorded ratio-4 batch
    torch.manual_seed(3)
    m = models.SpKBGATConvOnly(torch.randn(N_ENT, 8), torch.randn(N_REL, 8), [DIM, DIM * HEADS], [DIM, DIM * HEADS], 0.0, 0.0, 0.2, 0.2,
                               [HEADS, HEADS], 50)
    m.train()
    m.final_entity_embeddings.requires_grad = False                          # main.py:741-742
    m.final_relation_embeddings.requires_grad = False
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ratio = 4
    optimizer = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
    bce_loss = torch.nn.functional.binary_cross_entropy_with_logits
    train_indices, train_values = batches["r4"][0], batches["r4"][1]
    train_indices = torch.LongTensor(train_indices)
    train_values = torch.FloatTensor(train_values)
    preds = m(None, None, train_indices)
    optimizer.zero_grad()
    train_values = train_values.view(-1)
    train_values = (train_values + 1) / 2
    train_values = train_values.float()
    preds = preds.view(-1)
    weights = train_values + (1 - train_values) * 1 / (ratio * 2)
    loss = bce_loss(preds, train_values.float(), weight=weights)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    assert sorted(grads) == ["convKB.fc1.bias", "convKB.fc1.weight", "convKB.fc2.bias", "convKB.fc2.weight"], sorted(grads)
    optimizer.step()
    out.update({"sd__" + k: v.numpy() for k, v in sd0.items()})
    out.update({"grad__" + k: v.numpy() for k, v in grads.items()})
    out.update({"after__" + k: m.state_dict()[k].detach().numpy() for k in grads})
    out.update({"sd_keys": np.array(list(sd0.keys())), "step_indices": train_indices.numpy(), "step_values": batches["r4"][1].reshape(-1),
                "step_ratio": np.array(ratio), "preds": preds.detach().numpy(), "loss": np.array(loss.item(), np.float32),
                "lr": np.array(LR), "weight_decay": np.array(WEIGHT_DECAY)})
    save("convkb_train1", **out)


if __name__ == "__main__":
    main()
