"""Callers of the hot path, shaped like the reference's model classes so that checkpoints and call
sites carry over.  `SpGAT` mirrors GAT/models.py:11-88 (same constructor, forward signature and
state_dict keys: attention_i.a / attention_i.a_2 / W / out_att.a / out_att.a_2) but runs all heads
in ONE fused launch instead of a Python loop over H layers."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .gat_layers import ConvKB, SpGraphAttentionLayer, gat_heads, cat_edge_embed, gather_rows, gather_rows_pair, small_mm, IndexedRows, set_weight_grad_destination
from .graph import prepare_graph, trust, trusted, trust_bounds
from .sampler import prune_batch_launch

# SpKBGATModified: drop the edges into rows that its mask discards before the layers run (sampler.prune_edges); 0 = evaluate every row, as
# the reference does (tests compare both)
PRUNE_DEAD_ROWS = os.environ.get("RECON_KBGAT_PRUNE", "1") != "0"
KEEP_PRUNED_POSITIONS = False   # also return the surviving edges' positions (SpKBGATModified._pruned_pos): tests replay recorded per-edge dropout factors through them


class _AliasHeadParams(torch.autograd.Function):
    """[H,D,W] / [H,D] tensors that ALIAS the per-head parameters (which SpGAT keeps as views of two fused
    buffers): no copy in forward, and backward hands each head its slice of the fused gradient."""

    @staticmethod
    def forward(ctx, A, A2, *params):
        ctx.nheads = len(params) // 2
        return A.detach(), A2.detach()

    @staticmethod
    def backward(ctx, gA, gA2):
        return (None, None) + gA.unbind(0) + gA2.split(1, 0)        # one call each: 2 H views cost ~2 us apiece when sliced one by one


class SpGAT(nn.Module):
    def __init__(self, num_nodes, nfeat, nhid, relation_dim, dropout, alpha, nheads):
        super().__init__()
        self.dropout = dropout
        self.dropout_layer = nn.Dropout(self.dropout)
        self.attentions = [SpGraphAttentionLayer(num_nodes, nfeat, nhid, relation_dim, dropout=dropout,
                                                 alpha=alpha, concat=True) for _ in range(nheads)]
        for i, attention in enumerate(self.attentions):
            self.add_module('attention_{}'.format(i), attention)
        self.W = nn.Parameter(torch.zeros(size=(relation_dim, nheads * nhid)))
        nn.init.xavier_uniform_(self.W.data, gain=1.414)
        self.out_att = SpGraphAttentionLayer(num_nodes, nhid * nheads, nheads * nhid, nheads * nhid,
                                             dropout=dropout, alpha=alpha, concat=False)
        self.alpha = alpha

    def fused_head_params(self):
        """The H heads' `a` / `a_2` as one [H,D,2F+R] / [H,D] pair for the fused launch.  The per-head
        nn.Parameters (state_dict keys attention_i.a / attention_i.a_2, as in the reference) are kept as views of
        two fused buffers, so this is an alias, not a per-step torch.stack; whenever something replaced a
        parameter's storage (.to(), a fresh load) the buffers are rebuilt and the parameters re-pointed."""
        atts = self.attentions
        fused = getattr(self, "_fused_heads", None)
        params = [att.a for att in atts] + [att.a_2 for att in atts]
        ok = fused is not None
        if ok:
            A, A2, ptrs = fused                                       # ptrs: where every parameter must still live (no views made here)
            ok = all(p.data_ptr() == q for p, q in zip(params, ptrs))
        if not ok:
            with torch.no_grad():
                A = torch.stack([att.a.data for att in atts]).contiguous()
                A2 = torch.cat([att.a_2.data for att in atts], dim=0).contiguous()
                for i, att in enumerate(atts):
                    att.a.data = A[i]
                    att.a_2.data = A2[i:i + 1]
            params = [att.a for att in atts] + [att.a_2 for att in atts]
            self._fused_heads = (A, A2, [p.data_ptr() for p in params])
        bucket = getattr(self, "_head_grad_bucket", None)
        if bucket is not None:                                          # the heads' weight gradients land in the bucket's own storage
            bound = getattr(self, "_head_grad_bound", None)
            if bound is None or bound[0] != A.data_ptr():
                ra, ra2 = bucket.region([att.a for att in atts]), bucket.region([att.a_2 for att in atts])
                ok = ra is not None and ra2 is not None and ra.device == A.device
                bound = self._head_grad_bound = (A.data_ptr(), (ra.view_as(A), ra2.view_as(A2)) if ok else None)
            # The destination is claimed by the FIRST backward that runs after a release (gat_layers._weight_grad_tensors decides there, not
            # here: two forwards before one backward both see .grad None).  It is released only by a forward that finds every gradient
            # None — nothing live views the bucket region then; with gradients still in place (accumulation) the claim stands and the
            # next backward returns fresh tensors for autograd to add.
            if bound[1] is not None:
                set_weight_grad_destination(A, *bound[1], release=all(p.grad is None for p in params))
            else:
                set_weight_grad_destination(A, None, None)
        return _AliasHeadParams.apply(A, A2, *params)

    def write_head_gradients_into(self, bucket):
        """Let the H heads' backward write d a / d a_2 straight into `bucket` (dist.FlatGradBucket) — possible when the bucket holds
        attention_0.a .. attention_{H-1}.a back to back and likewise the a_2 (build it from `head_parameters()`); then autograd assigns views
        of the bucket as the parameters' gradients and bucket.pack() / allreduce_mean() copy nothing.  Returns whether the layout allows it."""
        self._head_grad_bucket, self._head_grad_bound = bucket, None
        return (bucket.region([att.a for att in self.attentions]) is not None and
                bucket.region([att.a_2 for att in self.attentions]) is not None)

    def head_parameters(self):
        """The heads' parameters in the order that lets a gradient bucket alias the fused gradients: every a, then every a_2."""
        return [att.a for att in self.attentions] + [att.a_2 for att in self.attentions]

    def heads_forward(self, x, edge_list, edge_embed, edge_list_nhop, edge_embed_nhop):
        """The H-head attention stage (GAT/models.py:71-72) as one fused call."""
        graph = prepare_graph(edge_list, edge_list_nhop, x.shape[0])
        ee, ee_index = cat_edge_embed(edge_embed, edge_list_nhop, edge_embed_nhop)
        a, a2 = self.fused_head_params()                                  # [H, D, 2F+R], [H, D]
        iid = getattr(self, "iid_keep_draws", False) and all(att.plain_draws() for att in self.attentions)
        if iid:                                                           # the edge list is the caller's own (pruned): all heads' factors in one draw
            keep = self.attentions[0].draw_keeps_iid(len(self.attentions), graph.E, x.device)
        else:
            keeps = [att.draw_keep(graph.E, x.device) for att in self.attentions]   # reference draw order
            keep = torch.cat(keeps, dim=0) if keeps[0] is not None else None
        return gat_heads(x, ee, a, a2, graph, keep, self.alpha, True,
                         keep_max=self.attentions[0].keep_bound() if keep is not None else None, ee_index=ee_index, keep_iid=iid and keep is not None)

    def forward(self, Corpus_, entity_embeddings, relation_embed, edge_list, edge_type, edge_embed,
                edge_list_nhop, edge_type_nhop):
        x = entity_embeddings
        has_nhop = edge_type_nhop.shape[0] != 0
        if edge_embed is None:
            # what every caller in the reference passes is relation_embed[edge_type] (GAT/models.py:156, :212): with None the layer reads
            # the relation table in place instead of an E x R copy of it
            edge_embed = IndexedRows(relation_embed, edge_type)
        if has_nhop:
            # relation_embed[edge_type_nhop[:, 0]] + relation_embed[edge_type_nhop[:, 1]] (:64-65) as one op: one gather-and-add forward, one
            # segment sum over both columns' keys backward (two gather_rows: two key tensors, two CSR builds, two sums and an add per table)
            edge_embed_nhop = gather_rows_pair(relation_embed, edge_type_nhop)
        else:
            edge_embed_nhop = torch.tensor([])
        x = self.heads_forward(x, edge_list, edge_embed, edge_list_nhop, edge_embed_nhop)
        x = self.dropout_layer(x)
        out_relation_1 = small_mm(relation_embed.to(self.W.dtype), self.W)    # (a reduced-precision relation table meets the fp32 parameter here)
        edge_embed = IndexedRows(out_relation_1, edge_type)               # out_relation_1[edge_type] (:79), read in place by the layer
        if has_nhop:
            edge_embed_nhop = gather_rows_pair(out_relation_1, edge_type_nhop)
        else:
            edge_embed_nhop = torch.tensor([])
        x = self.out_att(x, edge_list, edge_embed, edge_list_nhop, edge_embed_nhop, elu=True)        # F.elu(out_att(...)), :86-87, in the epilogue
        return x, out_relation_1


class _SkipMaskNormalize(torch.autograd.Function):
    """F.normalize(ew + mask.unsqueeze(-1) * skip, p=2, dim=1) — the tail of GAT/models.py:177-180 — as one launch each way (csrc/norm.hip)."""

    @staticmethod
    def forward(ctx, ew, skip, mask):
        ew, skip = ew.contiguous(), skip.contiguous()
        N, Cw = ew.shape
        y = torch.empty_like(ew)
        norm = torch.empty(N, dtype=torch.float32, device=ew.device)
        with _lib.on_device(ew.device):
            _lib.check(_lib.lib().recon_rows_normalize_fwd(ew.data_ptr(), skip.data_ptr(), mask.data_ptr(), N, Cw, 1e-12, y.data_ptr(), norm.data_ptr(),
                                                           _lib.current_stream()), "recon_rows_normalize_fwd")
        ctx.save_for_backward(y, norm, mask)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, norm, mask = ctx.saved_tensors
        gy = gy.contiguous()
        N, Cw = y.shape
        gt = torch.empty_like(y)
        gs = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        with _lib.on_device(y.device):
            _lib.check(_lib.lib().recon_rows_normalize_bwd(gy.data_ptr(), y.data_ptr(), norm.data_ptr(), mask.data_ptr(), N, Cw, 1e-12, gt.data_ptr(),
                                                           _lib.ptr(gs), _lib.current_stream()), "recon_rows_normalize_bwd")
        return gt, gs, None


def normalize_rows_(t):
    """t <- F.normalize(t, p=2, dim=1) in place (no gradient): GAT/models.py:160, one launch."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()):
        t.copy_(F.normalize(t, p=2, dim=1))
        return t
    with _lib.on_device(t.device):
        _lib.check(_lib.lib().recon_rows_normalize_fwd(t.data_ptr(), None, None, t.shape[0], t.shape[1], 1e-12, t.data_ptr(), None, _lib.current_stream()),
                   "recon_rows_normalize_fwd")
    return t


class SpKBGATModified(nn.Module):
    """Stage-A KB-GAT model, shaped like GAT/models.py:91-239 (same constructor, `forward` / `batch_test`
    signatures and state_dict keys: final_entity_embeddings, final_relation_embeddings, entity_embeddings,
    relation_embeddings, sparse_gat_1.*, W_entities).  The whole entity table goes through the fused SpGAT
    above with one entity batch's 1-hop + 2-hop edges; rows outside the batch keep only the W_entities skip
    connection; outputs are L2-normalised.  Inputs must already live on the GPU."""

    def __init__(self, initial_entity_emb, initial_relation_emb, entity_out_dim, relation_out_dim, drop_GAT, alpha,
                 nheads_GAT, initial_entity_emb_params=None):
        super().__init__()
        self.num_nodes, self.entity_in_dim = initial_entity_emb.shape
        self.entity_out_dim_1, self.entity_out_dim_2 = entity_out_dim[0], entity_out_dim[1]
        self.nheads_GAT_1, self.nheads_GAT_2 = nheads_GAT[0], nheads_GAT[1]
        self.num_relation, self.relation_dim = initial_relation_emb.shape
        self.relation_out_dim_1 = relation_out_dim[0]
        self.drop_GAT = drop_GAT
        self.alpha = alpha
        wide = self.entity_out_dim_1 * self.nheads_GAT_1
        self.final_entity_embeddings = nn.Parameter(torch.randn(self.num_nodes, wide))
        self.final_relation_embeddings = nn.Parameter(torch.randn(self.num_relation, wide))
        self.entity_embeddings = nn.Parameter(initial_entity_emb)
        self.relation_embeddings = nn.Parameter(initial_relation_emb)
        self.sparse_gat_1 = SpGAT(self.num_nodes, self.entity_in_dim, self.entity_out_dim_1, self.relation_dim,
                                  self.drop_GAT, self.alpha, self.nheads_GAT_1)
        self.W_entities = nn.Parameter(torch.zeros(size=(self.entity_in_dim, wide)))
        nn.init.xavier_uniform_(self.W_entities.data, gain=1.414)

    def _nhop(self, train_indices_nhop, dev):
        """2-hop quadruples (source, rel_1, rel_2, target) -> edges target <- source typed (rel_1, rel_2), GAT/models.py:145-148, on `dev`.
        The derived tensors are kept per quadruple tensor (identity + version).  In the reference's training loop every iteration
        brings a NEW quadruple tensor (GAT/main.py:494-508: `get_batch_nhop_neighbors_all` + `.cuda()`), so this cache only helps
        callers that re-use a batch (evaluation over a fixed split, benchmarks of the cached regime); what keeps the fresh-tensor
        regime cheap is that tensors marked by `graph.trust` (the sampler's batches) are never validated with a host round trip."""
        if train_indices_nhop.shape[0] == 0:
            return torch.tensor([]), torch.tensor([])
        key = (train_indices_nhop.data_ptr(), train_indices_nhop._version, tuple(train_indices_nhop.shape), str(dev))
        hit = getattr(self, "_nhop_cache", None)
        if hit is None or hit[0] != key:
            q = train_indices_nhop.to(dev)
            edge_nhop, type_nhop = torch.stack((q[:, 3], q[:, 0])).contiguous(), q[:, 1:3].contiguous()
            if trusted(train_indices_nhop):
                eb, rb = trust_bounds(train_indices_nhop)                 # entity ids in columns 0 / 3, relation ids in 1 / 2
                trust(edge_nhop, bound=eb)
                trust(type_nhop, bound=rb)
            hit = (key, edge_nhop, type_nhop, train_indices_nhop)
            self._nhop_cache = hit
        return hit[1], hit[2]

    def _encode(self, Corpus_, entity_embeddings, relation_embeddings, batch_entities, adj, train_indices_nhop):
        edge_list, edge_type = adj[0], adj[1]
        dev = entity_embeddings.device
        edge_list, edge_type = edge_list.to(dev), edge_type.to(dev)
        self._pruned_pos = None
        self.sparse_gat_1.iid_keep_draws = self.sparse_gat_1.out_att.iid_keep_draws = False
        quads = train_indices_nhop
        prune = (PRUNE_DEAD_ROWS and entity_embeddings.is_cuda and edge_list.dtype == torch.int64 and edge_list.dim() == 2 and edge_list.shape[1] > 0 and
                 (quads.shape[0] == 0 or (quads.dtype == torch.int64 and quads.dim() == 2 and quads.shape[1] == 4)))
        if prune:
            # :177-178 keep `mask * out_entity_1`: the edges into rows that neither the mask keeps nor a kept row reads are dropped up front
            # (sampler.prune_batch: one launch makes the mask, reads the n-hop edges out of the quadruples and writes both lists' survivors side by
            # side); both layers then see the same, much smaller graph and every kept row comes out as before.
            # Kept per (edge tensors, quadruples, batch entities) identity + version, like the graph cache: a caller that re-uses a batch re-uses
            # the pruned tensors (and with them the prepared graph); a fresh batch per iteration — the reference's loop — prunes once per iteration
            ver = lambda t: (t.data_ptr(), t._version, tuple(t.shape)) if torch.is_tensor(t) else None
            key = (ver(edge_list), ver(edge_type), ver(quads), ver(batch_entities), str(dev), KEEP_PRUNED_POSITIONS)
            hit = getattr(self, "_prune_cache", None)
            ew = None
            if hit is None or hit[0] != key:
                q = quads.to(dev) if quads.shape[0] else quads
                if quads.shape[0] and trusted(quads):
                    trust(q, bound=trust_bounds(quads)[0], rel_bound=trust_bounds(quads)[1])
                finish = prune_batch_launch(batch_entities, edge_list, edge_type, q, entity_embeddings.shape[0], want_pos=KEEP_PRUNED_POSITIONS,
                                            table_rows=relation_embeddings.shape[0])
                # the host waits for the prune kernel's counts: the skip connection's product (:177) does not depend on them and goes out first
                ew = small_mm(entity_embeddings, self.W_entities)
                hit = self._prune_cache = (key, finish(), (edge_list, edge_type, quads, batch_entities))      # the inputs pin their identities
            mask, edge_list, edge_type, edge_list_nhop, edge_type_nhop = hit[1][:5]
            self._pruned_pos = hit[1][5] if KEEP_PRUNED_POSITIONS else None
            # the layers' per-edge dropout factors cannot be the reference's edge for edge on a pruned list: drawn in one call per layer
            self.sparse_gat_1.iid_keep_draws = self.sparse_gat_1.out_att.iid_keep_draws = True
        else:
            ew = None
            edge_list_nhop, edge_type_nhop = self._nhop(train_indices_nhop, dev)
            mask = torch.zeros(entity_embeddings.shape[0], device=dev)
            mask[batch_entities.to(dev)] = 1.0           # the reference takes torch.unique first (:167-170): same mask, but a host round trip
        # :156 `edge_embed = self.relation_embeddings[edge_type]`: None lets SpGAT read the relation table in place (IndexedRows)
        out_entity, out_relation = self.sparse_gat_1(Corpus_, entity_embeddings, relation_embeddings, edge_list, edge_type,
                                                     None, edge_list_nhop, edge_type_nhop)
        if ew is None:
            ew = small_mm(entity_embeddings, self.W_entities)
        if ew.dtype == torch.float32 and out_entity.dtype == torch.float32:
            return _SkipMaskNormalize.apply(ew, out_entity, mask), out_relation, mask      # :177-180 in one launch each way
        out_entity = ew + mask.unsqueeze(-1) * out_entity
        return F.normalize(out_entity, p=2, dim=1), out_relation, mask

    def forward(self, Corpus_, batch_entities, adj, train_indices_nhop):
        normalize_rows_(self.entity_embeddings.data)                                                    # :160, in place
        out_entity, out_relation, mask = self._encode(Corpus_, self.entity_embeddings, self.relation_embeddings,
                                                      batch_entities, adj, train_indices_nhop)
        self.final_entity_embeddings.data = out_entity.data
        self.final_relation_embeddings.data = out_relation.data
        return out_entity, out_relation, mask

    def batch_test(self, Corpus_, batch_entities, adj, train_indices_nhop, entity_embeddings):
        ent = F.normalize(entity_embeddings.data, p=2, dim=1).detach()
        return self._encode(Corpus_, ent, self.relation_embeddings.detach(), batch_entities, adj, train_indices_nhop)


class SpKBGATConvOnly(nn.Module):
    """The ConvKB scorer over frozen final embeddings (GAT/models.py:240-304): same constructor, state_dict keys (final_entity_embeddings,
    final_relation_embeddings, convKB.*) and torch arithmetic in forward / batch_test, so `conv/trained_*.pth` loads with strict=True and
    training stays as it is.  `evaluate` runs the link-prediction evaluation on the HIP kernels of recon_amd.kg_eval."""

    def __init__(self, initial_entity_emb, initial_relation_emb, entity_out_dim, relation_out_dim, drop_GAT, drop_conv, alpha, alpha_conv,
                 nheads_GAT, conv_out_channels):
        super().__init__()
        self.num_nodes = initial_entity_emb.shape[0]
        self.entity_in_dim = initial_entity_emb.shape[1]
        self.entity_out_dim_1 = entity_out_dim[0]
        self.nheads_GAT_1 = nheads_GAT[0]
        self.entity_out_dim_2 = entity_out_dim[1]
        self.nheads_GAT_2 = nheads_GAT[1]
        self.num_relation = initial_relation_emb.shape[0]
        self.relation_dim = initial_relation_emb.shape[1]
        self.relation_out_dim_1 = relation_out_dim[0]
        self.drop_GAT = drop_GAT
        self.drop_conv = drop_conv
        self.alpha = alpha
        self.alpha_conv = alpha_conv
        self.conv_out_channels = conv_out_channels
        D = self.entity_out_dim_1 * self.nheads_GAT_1
        self.final_entity_embeddings = nn.Parameter(torch.randn(self.num_nodes, D))
        self.final_relation_embeddings = nn.Parameter(torch.randn(self.num_relation, D))
        self.convKB = ConvKB(D, 3, 1, self.conv_out_channels, self.drop_conv, self.alpha_conv)

    def _score(self, batch_inputs):
        if not self.final_entity_embeddings.is_cuda or not batch_inputs.is_cuda:
            raise RuntimeError("recon_amd: SpKBGATConvOnly expects GPU tensors (this package has no CPU path)")
        conv_input = torch.cat((self.final_entity_embeddings[batch_inputs[:, 0], :], self.final_relation_embeddings[batch_inputs[:, 1]],
                                self.final_entity_embeddings[batch_inputs[:, 2], :]), dim=1)
        return self.convKB(conv_input)

    def forward(self, Corpus_, adj, batch_inputs):
        return self._score(batch_inputs)

    def batch_test(self, batch_inputs):
        return self._score(batch_inputs)

    def evaluate(self, test_triples, known_triples, unique_entities=None):
        """Filtered head and tail ranking of test_triples against known_triples (train + valid + test: valid_triples_dict) and the metrics
        Corpus.get_validation_pred prints (GAT/create_batch.py:905-1199): recon_amd.kg_eval.link_prediction_metrics' dict."""
        from . import kg_eval
        with torch.no_grad():
            proj = kg_eval.convkb_projections(self.final_entity_embeddings, self.final_relation_embeddings, self.convKB)
            rh, rt, _ = kg_eval.rank_entities(proj, test_triples, known_triples, unique_entities=unique_entities)
        return kg_eval.link_prediction_metrics(rh, rt)
