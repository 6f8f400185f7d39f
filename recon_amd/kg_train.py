"""Training of the ConvKB scorer on the device: stage B of KB-GAT, train_conv (GAT/main.py:707-860), with the batches built on the device.

    filt = TripleFilter(known_triples, n_ent, n_rel)                     # train + valid + test: valid_triples_dict
    for iters in range(num_iters_per_epoch):
        idx, val = iteration_batch(train_indices, train_values, 0, batch_size, filt, ratio)   # main.py:785 always passes iter_num = 0
        loss = convkb_bce_loss(model, idx, val, ratio)                  # forward + weighted BCE (main.py:793, :833-840)
        optimizer.zero_grad(); loss.backward(); optimizer.step()        # gradients reach convKB.fc1 / convKB.fc2 only

The corruption kernel restates Corpus.get_iteration_batch / get_iteration_triples_batch (GAT/create_batch.py:103-351) with the same row
layout, value rule and give-up rule, filtered by binary search in sorted int64 keys; its random stream is a counter-based function of a
seed drawn from torch's CPU generator (torch.manual_seed reproduces a run, no host sync).  The scorer's forward and backward read the
frozen tables in place and reduce in one fixed order (csrc/kg_train.hip).  SpKBGATConvOnly.forward / batch_test keep their torch arithmetic.
"""
import torch

from . import _lib
from .kg_eval import SLOT_TAIL, _check_ids, _check_shapes, filter_keys

MAX_D = 512                          # recon_convkb_train_*: 1 <= D <= MAX_D
ENTITY_DRAW_CAP = 1 << 16            # recon_kg_corrupt: entity draws per row before it gives up
_FROZEN = ("the embedding tables must be frozen, as train_conv freezes them (GAT/main.py:741-742): "
           "model.final_entity_embeddings.requires_grad = False; model.final_relation_embeddings.requires_grad = False")


def _triples(triples, name):
    _lib.require_gpu(triples)
    if triples.dim() != 2 or triples.shape[1] != 3 or triples.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s: int32 or int64 [rows, 3] (head, relation, tail) expected" % name)
    return triples.contiguous()


_WORKSPACES = {}


def _workspace(dev, kind, floats):
    """Zero-filled once, grown when needed: the kernels leave their arrival counters at zero."""
    key = (dev.index, kind)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < floats:
        ws = torch.zeros(max(floats, 1), dtype=torch.float32, device=dev)
        _WORKSPACES[key] = ws
    return ws


class TripleFilter:
    """The known triples (valid_triples_dict: train + valid + test) as sorted unique int64 keys (r n_ent + h) n_ent + t on the device
    (kg_eval.filter_keys, tail order).  `capped` counts, on the device, the corrupted rows that gave up after ENTITY_DRAW_CAP draws
    (cumulative over every corrupt_batch call with this filter; read it with capped_rows(), which syncs)."""

    def __init__(self, known_triples, n_ent, n_rel):
        t = _triples(known_triples, "known_triples").to(torch.int64)
        self.n_ent, self.n_rel = int(n_ent), int(n_rel)
        if self.n_ent < 1 or self.n_rel < 1:
            raise ValueError("TripleFilter: n_ent, n_rel >= 1 expected")
        _check_ids(t, self.n_ent, self.n_rel, "known_triples")
        self.keys = torch.unique(filter_keys(t, SLOT_TAIL, (self.n_ent, self.n_rel)))
        self.capped = torch.zeros(1, dtype=torch.int64, device=t.device)

    @property
    def device(self):
        return self.keys.device

    def key(self, triples):
        t = triples.to(torch.int64)
        return filter_keys(t, SLOT_TAIL, (self.n_ent, self.n_rel))

    def contains(self, triples):
        """bool [rows]: the triple is a known one."""
        return torch.isin(self.key(triples), self.keys)

    def capped_rows(self):
        return int(self.capped.item())


def _seed(generator):
    """A 64-bit seed from torch's CPU generator (no device work, no sync)."""
    s = torch.randint(-(1 << 63), (1 << 63) - 1, (), dtype=torch.int64, generator=generator, device="cpu").item()
    return s & ((1 << 64) - 1)


def corrupt_batch(positives, values, filt, ratio, generator=None, check_ids=True):
    """(indices int64 [B (2 ratio + 1), 3], values fp32 [B (2 ratio + 1)]): the positives followed by their filtered corruptions, laid out as
    get_iteration_batch lays them out (GAT/create_batch.py:103-260; include/recon_hip.h, recon_kg_corrupt).  positives int32 / int64 [B, 3],
    values [B] or [B, 1]; generator: a CPU torch.Generator (None: the default one).  check_ids=False skips the range check of the
    positives (one host sync) for callers whose positives are already checked."""
    if not isinstance(filt, TripleFilter):
        raise TypeError("corrupt_batch: filt must be a TripleFilter")
    ratio = int(ratio)
    if ratio < 0:
        raise ValueError("corrupt_batch: ratio >= 0 expected")
    pos = _triples(positives, "positives")
    _lib.require_gpu(values)
    val = values.reshape(-1).to(torch.float32).contiguous()
    if val.numel() != pos.shape[0]:
        raise ValueError("corrupt_batch: one value per positive expected")
    if pos.device != filt.device:
        raise ValueError("corrupt_batch: positives and filter on different devices")
    if check_ids:
        _check_ids(pos, filt.n_ent, filt.n_rel, "positives")
    B = pos.shape[0]
    rows = B * (2 * ratio + 1)
    idx = torch.empty(rows, 3, dtype=torch.int64, device=pos.device)
    out = torch.empty(rows, dtype=torch.float32, device=pos.device)
    seed = _seed(generator)
    L = _lib.lib()
    with _lib.on_device(pos.device):
        _lib.check(L.recon_kg_corrupt(pos.data_ptr(), pos.element_size(), val.data_ptr(), B, ratio, filt.keys.data_ptr(), filt.keys.numel(),
                                      filt.n_ent, filt.n_rel, seed, idx.data_ptr(), out.data_ptr(), filt.capped.data_ptr(),
                                      _lib.current_stream()), "recon_kg_corrupt")
    return idx, out


def iteration_batch(train_indices, train_values, iter_num, batch_size, filt, ratio, generator=None, check_ids=True):
    """get_iteration_batch(iter_num) (GAT/create_batch.py:103-260) on the device: positives [batch_size iter_num, batch_size (iter_num + 1))
    of train_indices, or up to its end when that runs past it (the short last batch, :182-196), then corrupt_batch.  The reference's
    train_conv always passes iter_num = 0 (GAT/main.py:785: every iteration corrupts the first batch_size triples of the epoch's shuffle);
    which iter_num to pass is the caller's choice."""
    n = train_indices.shape[0]
    lo = batch_size * iter_num
    hi = lo + batch_size if (iter_num + 1) * batch_size <= n else n
    return corrupt_batch(train_indices[lo:hi], train_values[lo:hi], filt, ratio, generator=generator, check_ids=check_ids)


def _params(model):
    E, R = model.final_entity_embeddings, model.final_relation_embeddings
    if E.requires_grad or R.requires_grad:
        raise RuntimeError("recon_amd.kg_train: " + _FROZEN)
    conv = model.convKB
    W1, b1, w2, b2 = conv.fc1.weight, conv.fc1.bias, conv.fc2.weight, conv.fc2.bias
    _lib.require_gpu(E, R, W1, b1, w2, b2)
    _check_shapes(E, R, conv, "recon_amd.kg_train")
    _lib.require_gpu(E, R, W1, b1, w2, b2, dtype=torch.float32, wrong_dtype=(ValueError, "recon_amd.kg_train: fp32 tables and weights expected"))
    return E.detach().contiguous(), R.detach().contiguous(), W1, b1, w2, b2, float(conv.nl1.negative_slope)


def _forward(tri, E, R, W1, b1, w2, b2, slope, values=None, ratio=0):
    M, D = tri.shape[0], E.shape[1]
    dev = tri.device
    z = torch.empty(M, D, dtype=torch.float32, device=dev)
    s = torch.empty(M, dtype=torch.float32, device=dev)
    gs = loss = ws = None
    ws_floats = 0
    if values is not None:
        gs = torch.empty(M, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
    L = _lib.lib()
    if values is not None and M > 0:
        ws_floats = L.recon_convkb_train_fwd_workspace_floats(M, D)
        ws = _workspace(dev, "fwd", ws_floats)
    with _lib.on_device(dev):
        _lib.check(L.recon_convkb_train_fwd(tri.data_ptr(), tri.element_size(), M, E.data_ptr(), R.data_ptr(), E.shape[0], R.shape[0], D,
                                            W1.detach().contiguous().data_ptr(), b1.detach().contiguous().data_ptr(),
                                            w2.detach().contiguous().data_ptr(), b2.detach().contiguous().data_ptr(), slope, z.data_ptr(),
                                            s.data_ptr(), _lib.ptr(values), ratio, None, _lib.ptr(gs), _lib.ptr(loss), _lib.ptr(ws), ws_floats,
                                            _lib.current_stream()), "recon_convkb_train_fwd")
    return z, s, gs, loss


def _backward(tri, E, R, w2, slope, z, g_s, g_scale, W1, b1, b2):
    M, D = tri.shape[0], E.shape[1]
    dev = tri.device
    dW1, db1 = torch.empty_like(W1), torch.empty_like(b1)
    dw2, db2 = torch.empty(1, D, dtype=torch.float32, device=dev), torch.empty_like(b2)
    L = _lib.lib()
    ws_floats = L.recon_convkb_train_bwd_workspace_floats(M, D)
    ws = _workspace(dev, "bwd", ws_floats) if ws_floats else None
    with _lib.on_device(dev):
        _lib.check(L.recon_convkb_train_bwd(tri.data_ptr(), tri.element_size(), M, E.data_ptr(), R.data_ptr(), E.shape[0], R.shape[0], D,
                                            w2.detach().contiguous().data_ptr(), slope, z.data_ptr(), g_s.data_ptr(), _lib.ptr(g_scale),
                                            dW1.data_ptr(), db1.data_ptr(), dw2.data_ptr(), db2.data_ptr(), _lib.ptr(ws), ws_floats,
                                            _lib.current_stream()), "recon_convkb_train_bwd")
    return dW1, db1, dw2, db2


class _Scores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tri, E, R, slope, W1, b1, w2, b2):
        z, s, _, _ = _forward(tri, E, R, W1, b1, w2, b2, slope)
        ctx.save_for_backward(tri, E, R, z, W1, b1, w2, b2)
        ctx.slope = slope
        return s.view(-1, 1)

    @staticmethod
    def backward(ctx, g):
        tri, E, R, z, W1, b1, w2, b2 = ctx.saved_tensors
        g_s = g.reshape(-1).to(torch.float32).contiguous()
        dW1, db1, dw2, db2 = _backward(tri, E, R, w2, ctx.slope, z, g_s, None, W1, b1, b2)
        return None, None, None, None, dW1, db1, dw2, db2


class _BCELoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tri, E, R, slope, values, ratio, W1, b1, w2, b2):
        z, _, gs, loss = _forward(tri, E, R, W1, b1, w2, b2, slope, values, ratio)
        ctx.save_for_backward(tri, E, R, z, gs, W1, b1, w2, b2)
        ctx.slope = slope
        return loss

    @staticmethod
    def backward(ctx, g):
        tri, E, R, z, gs, W1, b1, w2, b2 = ctx.saved_tensors
        g_scale = g.reshape(1).to(torch.float32).contiguous()
        dW1, db1, dw2, db2 = _backward(tri, E, R, w2, ctx.slope, z, gs, g_scale, W1, b1, b2)
        return None, None, None, None, None, None, dW1, db1, dw2, db2


def convkb_scores(model, triples, check_ids=True):
    """preds [M, 1] of SpKBGATConvOnly.forward (GAT/models.py:291-296) on the HIP kernels, differentiable in convKB.fc1 / convKB.fc2 (the
    tables must be frozen: main.py:741-742).  check_ids=False skips the range check (one host sync); an id outside its table then scores
    NaN."""
    E, R, W1, b1, w2, b2, slope = _params(model)
    tri = _triples(triples, "triples")
    if check_ids:
        _check_ids(tri, E.shape[0], R.shape[0], "triples")
    return _Scores.apply(tri, E, R, slope, W1, b1, w2, b2)


def convkb_bce_loss(model, indices, values, ratio, check_ids=True):
    """train_conv's loss (GAT/main.py:793, :833-840) as one forward launch: y = (v + 1) / 2, w = y + (1 - y) / (2 ratio),
    binary_cross_entropy_with_logits(preds, y, weight=w), mean reduction; backward through the fixed-order backward kernel."""
    ratio = int(ratio)
    if ratio < 1:
        raise ValueError("convkb_bce_loss: ratio >= 1 expected (the reference's weights divide by 2 ratio)")
    E, R, W1, b1, w2, b2, slope = _params(model)
    tri = _triples(indices, "indices")
    _lib.require_gpu(values)
    val = values.reshape(-1).to(torch.float32).contiguous()
    if val.numel() != tri.shape[0]:
        raise ValueError("convkb_bce_loss: one value per triple expected")
    if tri.shape[0] == 0:
        raise ValueError("convkb_bce_loss: an empty batch has no mean")
    if check_ids:
        _check_ids(tri, E.shape[0], R.shape[0], "indices")
    return _BCELoss.apply(tri, E, R, slope, val, ratio, W1, b1, w2, b2)
