"""The `GAT_sep_space` variant of the stage-A model (reference GAT_sep_space/models.py:91-245): `SpKBGATModified` with one more
trainable tensor, `W_ent2rel` [num_relation, D, D] (D = entity_out_dim_1 * nheads), that carries an entity embedding into the space
of a triple's relation before the translation loss (`tanh(e W_r)`, GAT_sep_space/main.py:359-364, :372-377) and before ConvKB
(GAT_sep_space/models.py:316-320).  Encoder, forward / batch_test signatures and every other state_dict key are the GAT tree's
(recon_amd/models.py); a checkpoint written by GAT_sep_space/main.py loads with strict=True.

    from recon_amd.sep_space import SpKBGATModified          # instead of `from models import SpKBGATModified` in GAT_sep_space/main.py

Stage B of that tree, `SpKBGATConvOnly` (GAT_sep_space/models.py:247-339), scores a triple after carrying both entities into its relation's
space; its forward / batch_test take model_gat for W_ent2rel.  The class below keeps that interface and the state_dict, and its `evaluate`
and `relation_scores` run on the device (recon_amd.kg_sep).

Stage A's loss of that tree, `batch_gat_loss(gat_loss_func, train_indices, entity_embed, relation_embed, model_gat)`
(GAT_sep_space/main.py:347-391), is re-exported here from recon_amd.sep_loss:

    from recon_amd.sep_space import batch_gat_loss           # instead of the function GAT_sep_space/main.py defines
"""
import torch
import torch.nn as nn

from . import _lib
from . import models as _models
from .graph import trusted


class SpKBGATModified(_models.SpKBGATModified):
    def __init__(self, initial_entity_emb, initial_relation_emb, entity_out_dim, relation_out_dim, drop_GAT, alpha, nheads_GAT,
                 initial_entity_emb_params=None):
        super().__init__(initial_entity_emb, initial_relation_emb, entity_out_dim, relation_out_dim, drop_GAT, alpha, nheads_GAT,
                         initial_entity_emb_params)
        wide = self.entity_out_dim_1 * self.nheads_GAT_1
        self.W_ent2rel = nn.Parameter(torch.zeros(size=(self.num_relation, wide, wide)))                 # :136-138
        nn.init.xavier_uniform_(self.W_ent2rel.data, gain=1.414)
        self.nonlinearity_ent2rel = torch.tanh                                                           # :139

    def ent2rel(self, entity_rows, relation_ids):
        """`nonlinearity_ent2rel(bmm(entity_rows.unsqueeze(1), W_ent2rel[relation_ids])).squeeze(1)` (GAT_sep_space/main.py:360-364)
        without the [T, D, D] gather the reference materialises (160 KB per triple at D = 200): rows are walked in relation order, rows of
        one relation share the passes over its matrix (csrc/rel_mm.hip: one launch forward, two backward, no host read)."""
        return self.nonlinearity_ent2rel(rel_rows_mm(entity_rows, relation_ids, self.W_ent2rel))


class SpKBGATConvOnly(_models.SpKBGATConvOnly):
    """The GAT_sep_space ConvKB scorer (GAT_sep_space/models.py:247-339): the GAT tree's constructor and state_dict keys
    (final_entity_embeddings, final_relation_embeddings, convKB.*), so `conv/trained_*.pth` of that tree loads with strict=True.
    forward / batch_test take model_gat — anything with W_ent2rel [R, D, D] (laid out [in][out], x . W) and nonlinearity_ent2rel — and
    score [e_h' | r | e_t'] with e' = nonlinearity_ent2rel(E[e] . W_ent2rel[r]) through ConvKB in torch; the per-row products run on
    rel_rows_mm (no [T, D, D] gather) and gradients reach convKB and W_ent2rel as in the reference.
    Deviation: the reference squeezes the [T, 1, D] products with a bare .squeeze(), so a one-row batch fails in torch.cat; here a one-row
    batch scores like any other."""

    def _score(self, batch_inputs, model_gat):
        if not self.final_entity_embeddings.is_cuda or not batch_inputs.is_cuda:
            raise RuntimeError("recon_amd: SpKBGATConvOnly expects GPU tensors (this package has no CPU path)")
        W = model_gat.W_ent2rel
        rel = batch_inputs[:, 1]
        head = model_gat.nonlinearity_ent2rel(rel_rows_mm(self.final_entity_embeddings[batch_inputs[:, 0], :], rel, W))      # :316-320
        tail = model_gat.nonlinearity_ent2rel(rel_rows_mm(self.final_entity_embeddings[batch_inputs[:, 2], :], rel, W))
        return self.convKB(torch.cat((head, self.final_relation_embeddings[rel], tail), dim=1))

    def forward(self, Corpus_, adj, batch_inputs, model_gat):
        return self._score(batch_inputs, model_gat)

    def batch_test(self, batch_inputs, model_gat):
        return self._score(batch_inputs, model_gat)

    def _scorer(self, model_gat):
        from . import kg_sep
        return kg_sep.sep_scorer(self.final_entity_embeddings, self.final_relation_embeddings, self.convKB, model_gat)

    def evaluate(self, model_gat, test_triples, known_triples, unique_entities=None):
        """Filtered head and tail ranking of test_triples against known_triples (train + valid + test: valid_triples_dict), the metrics
        Corpus.get_validation_pred prints (GAT_sep_space/create_batch.py:905-1199) for this scorer: kg_eval.link_prediction_metrics' dict."""
        from . import kg_eval, kg_sep
        with torch.no_grad():
            rh, rt, _ = kg_sep.rank_entities(self._scorer(model_gat), test_triples, known_triples, unique_entities=unique_entities)
        return kg_eval.link_prediction_metrics(rh, rt)

    def relation_scores(self, model_gat, test_triples):
        """[Q, R]: every test triple scored with every relation, the `scores` of get_validation_cnfmat (GAT_sep_space/create_batch.py:1360-1390)
        before its view(-1, num_rels)."""
        from . import kg_sep
        with torch.no_grad():
            return kg_sep.relation_scores(self._scorer(model_gat), test_triples)


class _RelRowsMM(torch.autograd.Function):
    """out[t] = x[t] . W[rel[t]]   (x [T, D], W [R, D, Dout], rel [T] int64 in [0, R))"""

    @staticmethod
    def forward(ctx, x, rel, W):
        T, D = x.shape
        R, _, Dout = W.shape
        xc, Wc, relc = x.contiguous(), W.contiguous(), rel.contiguous()
        out = torch.empty(T, Dout, dtype=torch.float32, device=x.device)
        order = torch.argsort(relc, stable=True).to(torch.int32)
        if T:
            with _lib.on_device(x.device):
                _lib.check(_lib.lib().recon_rel_rows_mm(xc.data_ptr(), order.data_ptr(), relc.data_ptr(), Wc.data_ptr(), T, D, Dout, 0, out.data_ptr(),
                                                        _lib.current_stream()), "recon_rel_rows_mm")
        ctx.save_for_backward(xc, relc, Wc, order)
        return out

    @staticmethod
    def backward(ctx, g):
        xc, relc, Wc, order = ctx.saved_tensors
        T, D = xc.shape
        R, _, Dout = Wc.shape
        g = g.contiguous()
        g_x = g_W = None
        with _lib.on_device(g.device):
            if ctx.needs_input_grad[0]:
                g_x = torch.empty_like(xc)
                if T:
                    _lib.check(_lib.lib().recon_rel_rows_mm(g.data_ptr(), order.data_ptr(), relc.data_ptr(), Wc.data_ptr(), T, Dout, D, 1, g_x.data_ptr(),
                                                            _lib.current_stream()), "recon_rel_rows_mm")
            if ctx.needs_input_grad[2]:
                if not T:
                    return g_x, None, torch.zeros_like(Wc)
                g_W = torch.empty_like(Wc)
                seg = torch.zeros(R + 1, dtype=torch.int32, device=g.device)
                seg[1:] = torch.cumsum(torch.bincount(relc, minlength=R), 0)
                _lib.check(_lib.lib().recon_rel_rows_mm_wgrad(xc.data_ptr(), g.data_ptr(), order.data_ptr(), seg.data_ptr(), R, D, Dout, g_W.data_ptr(),
                                                              _lib.current_stream()), "recon_rel_rows_mm_wgrad")
        return g_x, None, g_W


def rel_rows_mm(x, rel, W):
    """Per-row product with the matrix its relation selects: `torch.bmm(x.unsqueeze(1), W[rel]).squeeze(1)` (GAT_sep_space/main.py:359-364)
    on the device kernels of csrc/rel_mm.hip.  float32, x [T, D], W [R, D, Dout] with D <= 1024, Dout <= 512; relation ids outside [0, R)
    raise (asynchronously, like an out-of-range index on the device does in the reference)."""
    if not x.is_cuda:
        raise RuntimeError("rel_rows_mm needs device tensors (there is no CPU path)")
    if x.dtype != torch.float32 or W.dtype != torch.float32 or rel.dtype != torch.int64:
        raise TypeError("rel_rows_mm takes float32 rows / matrices and int64 relation ids")
    if x.dim() != 2 or W.dim() != 3 or rel.shape != (x.shape[0],) or W.shape[1] != x.shape[1]:
        raise ValueError("rel_rows_mm: x [T, D], rel [T], W [R, D, Dout]")
    if x.shape[1] > 1024 or W.shape[2] > 512:
        raise ValueError("rel_rows_mm: D <= 1024 and Dout <= 512")
    if rel.numel() and not trusted(rel, limit=W.shape[0]):
        torch._assert_async(((rel >= 0) & (rel < W.shape[0])).all())
    return _RelRowsMM.apply(x, rel, W)


# the stage-A loss of this tree (GAT_sep_space/main.py:347-391) on the device: recon_amd/sep_loss.py, DESIGN.md section 14
from .sep_loss import batch_gat_loss, gat_loss_parts  # noqa: E402,F401
