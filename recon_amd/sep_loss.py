"""The stage-A loss of the GAT_sep_space tree — GAT_sep_space/main.py:347-391, what its train_gat differentiates on every iteration
(:552-561) and the only place where W_ent2rel learns.

    from recon_amd.sep_space import batch_gat_loss        # instead of the function GAT_sep_space/main.py defines
    loss = batch_gat_loss(gat_loss_func, train_indices, entity_embed, relation_embed, model_gat)

`batch_gat_loss` has the reference's signature (its module-level `args.valid_invalid_ratio_gat` is the keyword `valid_invalid_ratio_gat`,
default 2 as in its run scripts).  With a `torch.nn.MarginRankingLoss` (mean reduction), GPU float32 tables and a tanh
`nonlinearity_ent2rel` the batch's triples are carried into relation space ONCE each (recon_kgsep_ent2rel: the reference tiles the
positives 2 * ratio times first), the norms, terms and their mean are two launches, and the backward runs through the map on exact-fp32
MFMA (csrc/kg_sep.hip: k_kgsl_rows, k_kgsl_wgrad) with every sum in one fixed order: the step is bitwise reproducible.  Anything else
runs the reference's own op sequence on `rel_rows_mm` and `gather_rows`.
"""
import torch

from . import _lib
from .graph import trust
from .kg_sep import MAX_D, _is_tanh
from .losses import _validate


_NAME = "recon_amd.sep_space.batch_gat_loss"          # for losses._validate's message; its n_rel here: the rows of relation_embed AND of W_ent2rel


def _walk(tri, n_rel):
    """The relation-ordered walk over the 2 M items (heads, then tails) as kg_sep_train.ent2rel_rows builds it: no host read."""
    rel = tri[:, 1].clamp(0, n_rel - 1)
    order = torch.argsort(rel.repeat(2), stable=True)
    seg = torch.zeros(n_rel + 1, dtype=torch.int64, device=tri.device)
    torch.cumsum(torch.bincount(rel, minlength=n_rel) * 2, 0, out=seg[1:])
    return order, seg


def _forward(E, Rel, W, tri, n_pos, reps, margin):
    """(T, norms, terms, loss, order, seg) on contiguous, detached fp32 device tensors."""
    dev, M, D, n_rel = E.device, tri.shape[0], E.shape[1], W.shape[0]
    order, seg = _walk(tri, n_rel)
    T = torch.empty(2 * M, D, dtype=torch.float32, device=dev)
    remapped = torch.empty(M, 3, dtype=torch.int64, device=dev)
    norms = torch.empty(M, dtype=torch.float32, device=dev)
    terms = torch.empty(n_pos * reps, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    L = _lib.lib()
    with _lib.on_device(dev):
        _lib.check(L.recon_kgsep_ent2rel(tri.data_ptr(), 8, M, E.data_ptr(), E.shape[0], W.data_ptr(), n_rel, D, order.data_ptr(), seg.data_ptr(),
                                         T.data_ptr(), remapped.data_ptr(), _lib.current_stream()), "recon_kgsep_ent2rel")
        _lib.check(L.recon_kgsep_gat_loss_fwd(tri.data_ptr(), n_pos, reps, T.data_ptr(), Rel.data_ptr(), Rel.shape[0], D, float(margin), norms.data_ptr(),
                                              terms.data_ptr(), loss.data_ptr(), _lib.current_stream()), "recon_kgsep_gat_loss_fwd")
    return T, norms, terms, loss, order, seg


def _backward(E, Rel, W, tri, n_pos, reps, order, seg, T, terms, g, need_e, need_rel, need_w):
    """(g_rows [2 M, D] or None, g_Rel or None, g_W or None): recon_kgsep_gat_loss_bwd; what is not needed is not computed."""
    dev, M, D, n_rel = E.device, tri.shape[0], E.shape[1], W.shape[0]
    L = _lib.lib()
    ws = torch.empty(L.recon_kgsep_gat_loss_bwd_workspace_bytes(M) // 4, dtype=torch.float32, device=dev)
    g_rows = torch.empty(2 * M, D, dtype=torch.float32, device=dev) if need_e else None
    g_W = torch.empty_like(W) if need_w else None
    g_Rel = None
    if need_rel:                                                          # rows beyond W_ent2rel's relations have no triples: zeros
        g_Rel = torch.empty_like(Rel) if Rel.shape[0] <= n_rel else torch.zeros_like(Rel)
    with _lib.on_device(dev):
        _lib.check(L.recon_kgsep_gat_loss_bwd(tri.data_ptr(), n_pos, reps, E.data_ptr(), E.shape[0], Rel.data_ptr(), Rel.shape[0], W.data_ptr(), n_rel, D,
                                              order.data_ptr(), seg.data_ptr(), T.data_ptr(), terms.data_ptr(), g.data_ptr(), ws.data_ptr(),
                                              ws.numel() * 4, _lib.ptr(g_rows), _lib.ptr(g_W), _lib.ptr(g_Rel), _lib.current_stream()),
                   "recon_kgsep_gat_loss_bwd")
    return g_rows, g_Rel, g_W


class _SepTransEMarginLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, entity_embed, relation_embed, W_ent2rel, train_indices, n_pos, reps, margin):
        E, Rel, W, tri = (entity_embed.detach().contiguous(), relation_embed.detach().contiguous(), W_ent2rel.detach().contiguous(),
                          train_indices.contiguous())
        T, _, terms, loss, order, seg = _forward(E, Rel, W, tri, n_pos, reps, margin)
        if any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(E, Rel, W, tri, T, terms, order, seg)
            ctx.meta = (n_pos, reps)
        return loss

    @staticmethod
    def backward(ctx, g):
        from .gat_layers import _rowsum_keyed
        E, Rel, W, tri, T, terms, order, seg = ctx.saved_tensors
        n_pos, reps = ctx.meta
        need_e, need_rel, need_w = ctx.needs_input_grad[:3]
        g = g.contiguous().to(torch.float32)
        g_rows, g_Rel, g_W = _backward(E, Rel, W, tri, n_pos, reps, order, seg, T, terms, g, need_e, need_rel, need_w)
        g_E = None
        if need_e:                                                        # the fixed-order keyed row sum over the item rows: heads, then tails
            ids = torch.cat([tri[:, 0], tri[:, 2]])
            keys = torch.stack([ids, ids])
            trust(keys, bound=E.shape[0])                                 # copies of ids that were validated (or vouched for) by the caller
            g_E = _rowsum_keyed(g_rows, keys, E.shape[0])
        return g_E, g_Rel, g_W, None, None, None, None


def _split(train_indices, valid_invalid_ratio_gat):
    reps = 2 * int(valid_invalid_ratio_gat)
    return reps, int(train_indices.shape[0] / (reps + 1))


def _shapes_ok(train_indices, entity_embed, relation_embed, W, n_pos, reps):
    """What the kernels take: fp32 tensors on one GPU, E [n_ent, D], Rel [n_rel', D], W [n_rel, D, D] with 1 <= D <= 512, int64 triples
    [n_pos * (1 + reps), 3]."""
    if not (torch.is_tensor(W) and entity_embed.is_cuda and relation_embed.device == entity_embed.device and W.device == entity_embed.device):
        return False
    if not (entity_embed.dtype == relation_embed.dtype == W.dtype == torch.float32 and train_indices.dtype == torch.int64):
        return False
    if not (entity_embed.dim() == 2 and relation_embed.dim() == 2 and W.dim() == 3 and train_indices.dim() == 2 and train_indices.shape[1] == 3):
        return False
    D = entity_embed.shape[1]
    return (1 <= D <= MAX_D and relation_embed.shape[1] == D and tuple(W.shape[1:]) == (D, D) and W.shape[0] >= 1 and entity_embed.shape[0] >= 1 and
            relation_embed.shape[0] >= 1 and reps >= 1 and n_pos > 0 and train_indices.shape[0] == n_pos * (reps + 1))


def _fused(gat_loss_func, train_indices, entity_embed, relation_embed, model_gat, n_pos, reps):
    return (isinstance(gat_loss_func, torch.nn.MarginRankingLoss) and gat_loss_func.reduction == "mean" and
            _is_tanh(getattr(model_gat, "nonlinearity_ent2rel", None)) and
            _shapes_ok(train_indices, entity_embed, relation_embed, getattr(model_gat, "W_ent2rel", None), n_pos, reps))


def gat_loss_parts(train_indices, entity_embed, relation_embed, W_ent2rel, margin, valid_invalid_ratio_gat=2):
    """(T, norms, terms, loss) of a batch on the device kernels, for tests and tools: T fp32 [2 M, D] (heads, then tails, each triple in its
    relation's space), norms [M] = |(T[i] + Rel[r_i]) - T[M + i]|_1, terms [n_pos * 2 * ratio], loss [] = their mean.  fp32 GPU tensors,
    int64 train_indices [n_pos * (1 + 2 * ratio), 3]; ids are range-checked unless the producer vouched for them."""
    _lib.require_gpu(entity_embed, relation_embed, W_ent2rel, dtype=torch.float32)
    reps, n_pos = _split(train_indices, valid_invalid_ratio_gat)
    tri = train_indices.to(entity_embed.device)
    if not _shapes_ok(tri, entity_embed, relation_embed, W_ent2rel, n_pos, reps):
        raise ValueError("gat_loss_parts: E [n_ent, D], Rel [n_rel', D], W_ent2rel [n_rel, D, D] with D <= %d and int64 triples "
                         "[n_pos * (1 + 2 * ratio), 3] expected" % MAX_D)
    _validate(tri, entity_embed.shape[0], min(relation_embed.shape[0], W_ent2rel.shape[0]), _NAME)
    return _forward(entity_embed.detach().contiguous(), relation_embed.detach().contiguous(), W_ent2rel.detach().contiguous(), tri.contiguous(),
                    n_pos, reps, margin)[:4]


def batch_gat_loss(gat_loss_func, train_indices, entity_embed, relation_embed, model_gat, valid_invalid_ratio_gat=2):
    """GAT_sep_space/main.py:347-391.  train_indices int64 [T, 3]: the positive triples, then 2 * valid_invalid_ratio_gat corrupted copies
    of them; model_gat: anything with W_ent2rel [n_rel, D, D] (laid out [in][out], x . W) and nonlinearity_ent2rel."""
    reps, n_pos = _split(train_indices, valid_invalid_ratio_gat)
    if entity_embed.is_cuda and train_indices.device != entity_embed.device:
        train_indices = train_indices.to(entity_embed.device)            # the reference indexes a CUDA table with a CPU LongTensor
    W = model_gat.W_ent2rel
    if _fused(gat_loss_func, train_indices, entity_embed, relation_embed, model_gat, n_pos, reps):
        _validate(train_indices, entity_embed.shape[0], min(relation_embed.shape[0], W.shape[0]), _NAME)
        return _SepTransEMarginLoss.apply(entity_embed, relation_embed, W, train_indices, n_pos, reps, float(gat_loss_func.margin))
    # the reference's op sequence (any loss function, any dtype, any nonlinearity): rows through gather_rows and products through rel_rows_mm
    # where they are GPU float32
    from .gat_layers import gather_rows
    from .sep_space import rel_rows_mm

    def rows(t, i):                                                      # chosen per table: each may live elsewhere / in another dtype
        if t.is_cuda and t.dtype == torch.float32:
            return gather_rows(t, i.to(t.device).contiguous())
        return t[i.to(t.device)]

    def ent2rel(x, rel):
        if x.is_cuda and x.dtype == torch.float32 and W.is_cuda and W.dtype == torch.float32 and x.shape[1] <= 1024 and W.shape[2] <= 512:
            return model_gat.nonlinearity_ent2rel(rel_rows_mm(x, rel.to(x.device).contiguous(), W))
        return model_gat.nonlinearity_ent2rel(torch.bmm(x.unsqueeze(1), W[rel.to(W.device)]).squeeze(1))

    def norm(tr):
        x = ent2rel(rows(entity_embed, tr[:, 0]), tr[:, 1]) + rows(relation_embed, tr[:, 1]) - ent2rel(rows(entity_embed, tr[:, 2]), tr[:, 1])
        return torch.norm(x, p=1, dim=1)

    pos_norm = norm(train_indices[:n_pos].repeat(reps, 1))
    neg_norm = norm(train_indices[n_pos:])
    y = -torch.ones(reps * n_pos, device=entity_embed.device)
    return gat_loss_func(pos_norm, neg_norm, y)
