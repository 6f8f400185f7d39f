"""Training of the GAT_sep_space ConvKB scorer on the device: stage B of that tree, train_conv (GAT_sep_space/main.py:769-921), over frozen
tables and a frozen W_ent2rel.

    model_gat.W_ent2rel.requires_grad_(False)                          # train_conv never steps it: its optimizer holds model_conv's (:808-809)
    filt = TripleFilter(known_triples, n_ent, n_rel)                     # train + valid + test: valid_triples_dict
    for iters in range(num_iters_per_epoch):
        idx, val = iteration_batch(train_indices, train_values, iters, batch_size, filt, ratio)   # main.py:845 passes iter_num = iters
        loss = sep_convkb_bce_loss(model_conv, model_gat, idx, val, ratio)                        # forward + weighted BCE (:879-901)
        optimizer.zero_grad(); loss.backward(); optimizer.step()        # gradients reach convKB.fc1 / convKB.fc2 only

Batches come from recon_amd.kg_train unchanged: GAT_sep_space/create_batch.py:103-260 is the GAT tree's sampler line for line.  Unlike the
GAT tree, whose train_conv always passes iter_num = 0, this tree's passes the iteration number.

The scorer carries both entities of a triple into its relation's space, e' = tanh(E[e] W_ent2rel[r]) (GAT_sep_space/models.py:311-324).
One kernel (csrc/kg_sep.hip, recon_kgsep_ent2rel) writes those rows for a batch of M triples as a [2 M, D] table T, heads then tails, with
the triples remapped to (m, r, M + m); the fused ConvKB forward and backward of recon_amd.kg_train then run unchanged on E := T.  No
[M, D, D] gather of W_ent2rel, no gradient for it: the step is bitwise reproducible.  SpKBGATConvOnly.forward keeps its torch arithmetic.
"""
import torch

from . import _lib
from . import kg_train as _kgt
from .kg_eval import _check_ids, _check_shapes
from .kg_sep import MAX_D, check_ent2rel

_FP32 = "%s: fp32 tables, W_ent2rel and weights expected"
_W_FROZEN = ("model_gat.W_ent2rel requires grad, but the device step computes no gradient for it: train_conv never steps it (its optimizer "
             "holds model_conv.parameters() only, GAT_sep_space/main.py:808-809).  Freeze it first: model_gat.W_ent2rel.requires_grad_(False)")


def ent2rel_rows(E, W_ent2rel, triples, check_ids=True):
    """(T, remapped): T fp32 [2 M, D] with T[m] = tanh(E[h_m] W_ent2rel[r_m]) and T[M + m] = tanh(E[t_m] W_ent2rel[r_m]) (the two rows
    GAT_sep_space/models.py:312-320 builds per triple), remapped int64 [M, 3] = (m, r_m, M + m).  E fp32 [n_ent, D], W_ent2rel fp32
    [n_rel, D, D] laid out [in][out] (x . W), triples int32 / int64 [M, 3] on the device.  check_ids=False skips the range check (one host
    sync); an id outside its table then gives a NaN row."""
    _lib.require_gpu(E, W_ent2rel)
    tri = _kgt._triples(triples, "triples")
    if E.dim() != 2 or W_ent2rel.dim() != 3 or tuple(W_ent2rel.shape[1:]) != (E.shape[1], E.shape[1]):
        raise ValueError("ent2rel_rows: E [n_ent, D] and W_ent2rel [n_rel, D, D] expected")
    _lib.require_gpu(E, W_ent2rel, dtype=torch.float32, wrong_dtype=(ValueError, _FP32 % "ent2rel_rows"))
    n_ent, n_rel, D = E.shape[0], W_ent2rel.shape[0], E.shape[1]
    if n_ent < 1 or n_rel < 1 or D < 1:
        raise ValueError("ent2rel_rows: non-empty tables expected")
    if D > MAX_D:
        raise ValueError("ent2rel_rows: D = %d, at most %d supported" % (D, MAX_D))
    if check_ids:
        _check_ids(tri, n_ent, n_rel, "triples")
    M, dev = tri.shape[0], tri.device
    T = torch.empty(2 * M, D, dtype=torch.float32, device=dev)
    remapped = torch.empty(M, 3, dtype=torch.int64, device=dev)
    if M == 0:
        return T, remapped
    rel = tri[:, 1].to(torch.int64).clamp(0, n_rel - 1)                # an id outside W_ent2rel sorts under a real relation, then scores NaN
    order = torch.argsort(rel.repeat(2), stable=True)
    seg = torch.zeros(n_rel + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(rel, minlength=n_rel) * 2, 0, out=seg[1:])
    E, W = E.detach().contiguous(), W_ent2rel.detach().contiguous()
    with _lib.on_device(dev):
        _lib.check(_lib.lib().recon_kgsep_ent2rel(tri.data_ptr(), tri.element_size(), M, E.data_ptr(), n_ent, W.data_ptr(), n_rel, D,
                                                  order.data_ptr(), seg.data_ptr(), T.data_ptr(), remapped.data_ptr(), _lib.current_stream()),
                   "recon_kgsep_ent2rel")
    return T, remapped


def _params(model_conv, model_gat):
    """Every check before device work: frozen tables and W_ent2rel, W_ent2rel's shape and tanh, GPU and fp32 tensors."""
    E, R = model_conv.final_entity_embeddings, model_conv.final_relation_embeddings
    if E.requires_grad or R.requires_grad:
        raise RuntimeError("recon_amd.kg_sep_train: " + _kgt._FROZEN)
    D = _check_shapes(E, R, model_conv.convKB, "recon_amd.kg_sep_train")
    W = check_ent2rel(model_gat, R.shape[0], D)
    if W.requires_grad:
        raise RuntimeError("recon_amd.kg_sep_train: " + _W_FROZEN)
    E, R, W1, b1, w2, b2, slope = _kgt._params(model_conv)
    _lib.require_gpu(W, dtype=torch.float32, wrong_dtype=(ValueError, _FP32 % "recon_amd.kg_sep_train"))
    return E, R, W, W1, b1, w2, b2, slope


def sep_convkb_scores(model_conv, model_gat, triples, check_ids=True):
    """preds [M, 1] of SpKBGATConvOnly.forward(..., model_gat) (GAT_sep_space/models.py:311-324) on the HIP kernels, differentiable in
    convKB.fc1 / convKB.fc2.  model_gat: anything with W_ent2rel [R, D, D] (frozen) and a tanh nonlinearity_ent2rel.  check_ids=False skips
    the range check (one host sync); an id outside its table then scores NaN."""
    E, R, W, W1, b1, w2, b2, slope = _params(model_conv, model_gat)
    tri = _kgt._triples(triples, "triples")
    if check_ids:
        _check_ids(tri, E.shape[0], R.shape[0], "triples")
    T, rem = ent2rel_rows(E, W, tri, check_ids=False)
    return _kgt._Scores.apply(rem, T, R, slope, W1, b1, w2, b2)


def sep_convkb_bce_loss(model_conv, model_gat, indices, values, ratio, check_ids=True):
    """train_conv's loss (GAT_sep_space/main.py:893-901): y = (v + 1) / 2, w = y + (1 - y) / (2 ratio), binary_cross_entropy_with_logits(preds,
    y, weight=w), mean reduction — kg_train.convkb_bce_loss's loss on the stacked table T, backward through its fixed-order kernel."""
    ratio = int(ratio)
    if ratio < 1:
        raise ValueError("sep_convkb_bce_loss: ratio >= 1 expected (the reference's weights divide by 2 ratio)")
    E, R, W, W1, b1, w2, b2, slope = _params(model_conv, model_gat)
    tri = _kgt._triples(indices, "indices")
    _lib.require_gpu(values)
    val = values.reshape(-1).to(torch.float32).contiguous()
    if val.numel() != tri.shape[0]:
        raise ValueError("sep_convkb_bce_loss: one value per triple expected")
    if tri.shape[0] == 0:
        raise ValueError("sep_convkb_bce_loss: an empty batch has no mean")
    if check_ids:
        _check_ids(tri, E.shape[0], R.shape[0], "indices")
    T, rem = ent2rel_rows(E, W, tri, check_ids=False)
    return _kgt._BCELoss.apply(rem, T, R, slope, val, ratio, W1, b1, w2, b2)
