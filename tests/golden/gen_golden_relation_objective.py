"""Fixture of the stage-B objective (tests/golden/relation_objective1.npz), written where the reference tree is available.

An "epoch" of six small batches (M <= 24 rows, n_out <= 7) goes through the lines of train.py:232 and :309-324 on the CPU: torch's
`CrossEntropyLoss(ignore_index=0)`, `torch.max`, the `labels != 0` filter and the reference's own
`utils.evaluation_utils.evaluate_instance_based(..., empty_label=1)`, with the running `f1 += add_f1`.  The batches: an ordinary one, one
with every label ignored, one where nothing is predicted non-empty, one where no gold label is non-empty, one with an exact tie (a copied
column, the tie deciding rows whose gold label is either of the two), and another ordinary one.  Recorded per batch i: logits_i (fp32),
labels_i, loss_i and d_logits_i (fp64, from the logits cast to fp64), predicted_i, confidence_i (the fp64 softmax probability of the
prediction), prec_i, rec_i, f1_i (the reference's doubles), counts_i (kept, n_pred, n_gold, n_ok by a plain loop) and f1_sum_i (the running
sum after the batch).  Arrays only; nothing of the reference's text is stored.
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
IGNORE, EMPTY = 0, 1


def _labels(g, M, n, p_ignore=0.5, p_empty=0.25):
    u = torch.rand(M, generator=g)
    other = torch.randint(2, n, (M,), generator=g) if n > 2 else torch.full((M,), EMPTY)
    lab = torch.where(u < p_ignore, torch.full((M,), IGNORE), torch.where(u < p_ignore + p_empty, torch.full((M,), EMPTY), other))
    return lab.to(torch.int64)


def _toward(g, x, lab, p=0.6, by=3.0):
    """The logits with `by` added at the label's column in a share p of the rows: predictions that are partly right."""
    hit = (torch.rand(x.shape[0], generator=g) < p).to(x.dtype) * by
    return x + hit.unsqueeze(1) * torch.nn.functional.one_hot(lab, x.shape[1]).to(x.dtype)


def _batches():
    g = torch.Generator().manual_seed(53)
    out = []
    lab = _labels(g, 24, 7)                                               # ordinary
    out.append((_toward(g, torch.randn(24, 7, generator=g) * 2, lab), lab))
    x = torch.randn(8, 5, generator=g) * 2                                # every label ignored
    out.append((x, torch.full((8,), IGNORE, dtype=torch.int64)))
    x = torch.randn(12, 5, generator=g)                                   # nothing predicted non-empty: the empty column wins every row
    x[:, EMPTY] += 9
    out.append((x, _labels(g, 12, 5, 0.3, 0.2)))
    x = torch.randn(10, 4, generator=g) * 2                               # no gold label non-empty
    lab = _labels(g, 10, 4, 0.4, 0.6)
    lab[lab > EMPTY] = EMPTY
    out.append((x, lab))
    x = torch.randn(9, 6, generator=g)                                    # an exact tie: column 3 is a copy of column 2 and the pair wins
    x[:, 2] += 5
    x[:, 3] = x[:, 2]
    lab = torch.tensor([2, 3, 2, 3, 0, 1, 2, 3, 5], dtype=torch.int64)
    out.append((x, lab))
    lab = _labels(g, 17, 3, 0.4, 0.2)                                     # ordinary, odd sizes
    out.append((_toward(g, torch.randn(17, 3, generator=g) * 3, lab), lab))
    return out


def _counts(predicted, labels):
    kept = n_pred = n_gold = n_ok = 0
    for p, l in zip(predicted, labels):
        if l == IGNORE:
            continue
        kept += 1
        n_pred += p != EMPTY
        n_gold += l != EMPTY
        n_ok += l != EMPTY and p == l
    return [kept, n_pred, n_gold, n_ok]


def main():
    sys.path.insert(0, HERE)
    import gen_golden
    ref = gen_golden.REF
    sys.path.insert(0, ref)
    from utils import evaluation_utils
    assert evaluation_utils.__file__.startswith(ref)
    loss_func = nn.CrossEntropyLoss(ignore_index=IGNORE)
    arrays = {"n_batches": np.int64(6), "ignore_index": np.int64(IGNORE), "empty_label": np.int64(EMPTY)}
    f1 = 0
    for i, (x, lab) in enumerate(_batches()):
        xd = x.double().requires_grad_(True)
        loss = loss_func(xd, lab)                                         # train.py:309
        loss.backward()
        _, predicted = torch.max(x, dim=1)                                # train.py:317-322
        assert torch.equal(predicted, torch.max(xd, dim=1)[1])
        labels = lab.numpy().reshape(-1).tolist()
        pred = predicted.tolist()
        p_indices = np.array(labels) != 0
        pred_kept = np.array(pred)[p_indices].tolist()
        labels_kept = np.array(labels)[p_indices].tolist()
        prec, rec, add_f1 = evaluation_utils.evaluate_instance_based(pred_kept, labels_kept, empty_label=EMPTY)      # train.py:324
        f1 += add_f1
        conf = torch.softmax(xd.detach(), dim=1).gather(1, predicted.unsqueeze(1)).squeeze(1)
        arrays.update({"logits_%d" % i: x.numpy(), "labels_%d" % i: lab.numpy(), "loss_%d" % i: np.float64(loss.item()),
                       "d_logits_%d" % i: xd.grad.numpy(), "predicted_%d" % i: predicted.numpy(), "confidence_%d" % i: conf.numpy(),
                       "prec_%d" % i: np.float64(prec), "rec_%d" % i: np.float64(rec), "f1_%d" % i: np.float64(add_f1),
                       "counts_%d" % i: np.array(_counts(pred, labels), dtype=np.int64), "f1_sum_%d" % i: np.float64(f1)})
    c = [arrays["counts_%d" % i] for i in range(6)]
    assert c[1][0] == 0 and np.isnan(arrays["loss_1"]) and not arrays["d_logits_1"].any()
    assert c[2][1] == 0 and c[2][0] > 0 and c[2][2] > 0 and c[3][2] == 0 and c[3][0] > 0 and c[3][1] > 0
    assert (arrays["predicted_4"] == 2).all() and (arrays["logits_4"][:, 2] == arrays["logits_4"][:, 3]).all()
    assert all(0 < arrays["f1_%d" % i] < 1 for i in (0, 4, 5))
    path = os.path.join(HERE, "relation_objective1.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %-28s %5.1f KB" % ("relation_objective1.npz", os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
