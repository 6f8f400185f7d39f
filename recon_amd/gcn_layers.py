"""Drop-in replacement for the reference module `models/layers.py`: `GraphConvolution` (same
constructor, `forward(input, adj)`, parameters `weight` [in,out] / `bias` [out] with the reference's
uniform(-1/sqrt(out), 1/sqrt(out)) init) and `SparseMM`, running in csrc/prop.hip + gemm_f32.hip.

    from recon_amd.gcn_layers import GraphConvolution          # models/models.py:8

bfloat16 tensors (`layer.to(torch.bfloat16)`, bf16 input / adj) take the bf16 MFMA path of csrc/gemm_b16.hip / gcn_b16.hip:
bf16 storage, fp32 accumulation, what torch.mm does for bf16 operands.

Extension over the reference: `forward` also accepts a batch, input [B,n,in] with adj [B,n,n]
(the reference's torch.mm only takes the 2-D single-graph form).  Any n is accepted (the aggregate kernel tiles
the adjacency in 32 x 32 blocks); B <= 65 535 graphs per call.

Second extension: graphs of DIFFERENT sizes in one call, `forward(input [N, in], RaggedAdjacency(values, sizes))`, in bfloat16
(csrc/gcn_b16.hip) and in float32 (csrc/gcn_ragged.hip: the dense layer's GEMMs over all N rows, the per-graph aggregate and g_adj on
the exact-fp32 matrix cores); input and adjacency values share one dtype."""
import ctypes as C
import os
import math
from collections import namedtuple

import torch
from torch.nn.parameter import Parameter
from torch.nn.modules.module import Module

from . import _lib
from . import gat_layers as _gl        # the GEMM-family switch (_GEMM_BX3) is ONE module-level setting for GAT and GCN


def _f32_args(B, n, I, O, x3, adj3, weight, bias, sup, out, w_split):
    """recon_gcn_args (include/recon_hip.h) of a launch, and of a backward's `fwd` field."""
    return _lib.GcnArgs(B=B, n=n, in_features=I, out_features=O, x=x3.data_ptr(), adj=adj3.data_ptr(), weight=weight.data_ptr(),
                        bias=_lib.ptr(bias), support=sup.data_ptr(), out=out.data_ptr(), w_split=_lib.ptr(w_split))


class _GcnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj, weight, bias):
        _lib.require_gpu(x, adj, weight, bias, dtype=torch.float32)
        x3 = x.contiguous().view(-1, x.shape[-2], x.shape[-1])
        adj3 = adj.contiguous().view(-1, adj.shape[-2], adj.shape[-1])
        weight = weight.contiguous()
        B, n, I = x3.shape
        O = weight.shape[1]
        if adj3.shape != (B, n, n) or weight.shape[0] != I:
            raise ValueError("GraphConvolution: inconsistent shapes")
        dev = x.device
        sup = torch.empty(B, n, O, dtype=torch.float32, device=dev)
        # allocated in the caller's shape and returned AS IS: the tensor saved for the backward (its sign is the ReLU mask)
        # is the tensor the caller holds, so an in-place edit of the result is caught by autograd's version check
        out = torch.empty(x.shape[:-1] + (O,), dtype=torch.float32, device=dev)
        w_split = None
        mode = _gl._GEMM_BX3                                  # split-precision GEMMs (fp32-accurate, csrc/gemm_bx3.hip): auto | 1 | 0
        if mode == "1" or (mode != "0" and 2.0 * B * n * I * O >= 2.0e9):    # small products do not pay for the term-plane launches
            w_split = torch.empty(_lib.lib().recon_gcn_split_bytes(I, O), dtype=torch.uint8, device=dev)
        args = _f32_args(B, n, I, O, x3, adj3, weight, bias, sup, out, w_split)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().recon_gcn_fwd(C.byref(args), _lib.current_stream()), "recon_gcn_fwd")
        ctx.save_for_backward(x3, adj3, weight, bias, sup, out, w_split)
        ctx.shapes = (tuple(x.shape), tuple(adj.shape))
        return out

    @staticmethod
    def backward(ctx, gout):
        x3, adj3, weight, bias, sup, out, w_split = ctx.saved_tensors
        B, n, I = x3.shape
        O = weight.shape[1]
        dev = gout.device
        L = _lib.lib()
        f32 = dict(dtype=torch.float32, device=dev)
        gout = gout.contiguous()
        nx, nadj, nw, nb = ctx.needs_input_grad
        g_sup = torch.empty(B, n, O, **f32)
        partial = torch.empty(L.recon_gcn_bwd_partial_floats(B, n, I, O), **f32)
        g_x = torch.empty(B, n, I, **f32) if nx else None
        g_adj = torch.empty(B, n, n, **f32) if nadj else None
        g_w = torch.empty(I, O, **f32) if nw else None
        g_b = torch.empty(O, **f32) if (nb and bias is not None) else None
        gs_split = (torch.empty(L.recon_gcn_bwd_split_bytes(B, n, O), dtype=torch.uint8, device=dev)
                    if (w_split is not None and g_w is not None) else None)
        args = _lib.GcnBwdArgs(fwd=_f32_args(B, n, I, O, x3, adj3, weight, bias, sup, out, w_split), grad_out=gout.data_ptr(),
                               g_support=g_sup.data_ptr(), partial=partial.data_ptr(), g_x=_lib.ptr(g_x), g_adj=_lib.ptr(g_adj),
                               g_weight=_lib.ptr(g_w), g_bias=_lib.ptr(g_b), gs_split=_lib.ptr(gs_split))
        with _lib.on_device(dev):
            _lib.check(L.recon_gcn_bwd(C.byref(args), _lib.current_stream()), "recon_gcn_bwd")
        xs, adjs = ctx.shapes
        return (g_x.view(xs) if g_x is not None else None, g_adj.view(adjs) if g_adj is not None else None, g_w, g_b)


def _up8(v):
    return (v + 7) // 8 * 8


# the layouts a kernel reads in place, as rules: (row stride a multiple of, byte alignment of the first row, pad columns are multiplied)
_MFMA = (8, 16, True)            # the GEMMs' rows: ld % 8 == 0, ld >= up8(feat), 16-byte aligned, and the pad columns feat .. up8(feat) are READ
_MFMA_UNREAD = (8, 16, False)    # the same rows where nothing multiplies the pad columns (a gradient's, or a kernel that masks its K tail)
_MASKED = (2, 4, False)          # rows a kernel with masked row tails reads: ld even, ld >= feat, 4-byte aligned


def _row_stride(t, feat, rule):
    """Row stride ld of a [..., n, feat] bf16 tensor whose rows are feat contiguous elements at ONE regular stride that `rule` admits — a
    contiguous tensor with feat % 8 == 0, or the padded views this module hands out.  None: the tensor has to be repacked."""
    mult, align, pads_read = rule
    if t.dim() < 2 or t.stride(-1) != 1:
        return None
    if pads_read and feat % 8 and not getattr(t, "_recon_padded", False):
        # the kernels read the pad columns feat .. round_up(feat, 8) of every row (times zero weights): only rows THIS module wrote have
        # zeros there — somebody else's `buf[..., :feat]` may carry inf / NaN in them, and 0 * NaN would poison the result
        return None
    ld = t.stride(-2)
    if ld % mult or ld < feat or t.data_ptr() % align:         # a multiple of 8 that is >= feat is >= up8(feat)
        return None
    rows = t.shape[-2]
    for d in range(t.dim() - 3, -1, -1):                       # leading dims must continue the same row sequence
        if t.shape[d] != 1 and t.stride(d) != rows * ld:
            return None
        rows *= t.shape[d]
    return ld


def _rows_view(t, feat, pads_read=True):
    return _row_stride(t, feat, _MFMA if pads_read else _MFMA_UNREAD)


def _packed_rows(t, feat, zero_pad):
    """[rows, ld] bf16 buffer holding t's rows (ld = feat rounded up to 8); pad columns zeroed when the kernels multiply them."""
    ld = _up8(feat)
    t2 = t.reshape(-1, feat)
    if ld == feat:
        return t2.contiguous(), ld
    buf = (torch.zeros if zero_pad else torch.empty)(t2.shape[0], ld, dtype=torch.bfloat16, device=t.device)
    buf[:, :feat] = t2
    return buf, ld


def _rows_or_packed(t, feat, rule, zero_pad):
    """(tensor, ld): t's rows where they lie if `rule` admits them, else a packed copy."""
    ld = _row_stride(t, feat, rule)
    return (t, ld) if ld is not None else _packed_rows(t, feat, zero_pad)


def _grad_rows(gout, feat, rule):
    """(tensor, ld) of a gradient as bf16 rows; its pad columns are never read, so a copy leaves them unwritten."""
    if gout.dtype != torch.bfloat16:
        gout = gout.to(torch.bfloat16)
    return _rows_or_packed(gout, feat, rule, False)


def _strides(lead, ld):
    """Strides of a [*lead, feat] view over rows of stride ld (lead = leading dims ending with the row dim)."""
    st, acc = [], ld
    for d in reversed(lead):
        st.append(acc)
        acc *= d
    return tuple(reversed(st)) + (1,)


def _padded_result(out_p, lead, feat, ld, zero_tail):
    """The [rows, ld] result buffer as the caller's [*lead, feat]: a plain view, or (feat < ld) a strided one tagged `_recon_padded`, whose
    pad columns the next layer and the backward read in place (zero_tail: the kernel did not write them as zeros itself).  The view
    starts where out_p starts (as_strided keeps the storage offset: the last layer of a stack's buffer)."""
    if ld == feat:
        return out_p.view(lead + (feat,))
    if zero_tail:
        out_p[:, feat:].zero_()
    out = out_p.as_strided(lead + (feat,), _strides(lead, ld))
    out._recon_padded = True
    return out


def _grad_view(g, shape, feat, ld):
    """A [rows, ld] gradient buffer (or None) in the caller's `shape`; untagged: nothing reads a gradient's pad columns, which stay unwritten."""
    if g is None:
        return None
    return g.view(shape) if ld == feat else g.as_strided(shape, _strides(shape[:-1], ld))


_FUSED = os.environ.get("RECON_GCN_FUSED", "1") != "0"
_FUSED_MAX_N = 32            # csrc/gcn_b16.hip gcn_fused_ok / recon_gcn_b16_stack_fwd: `a->n <= 32` (one 32-row tile per graph)
_FUSED_MAX_WIDTH = 320       # csrc/gcn_b16.hip `kFusedNT * 16` (kFusedNT = 20 column tiles): `a->ldo <= kFusedNT * 16`


def _fits_int32(B, n, I, O):        # csrc/gcn_b16.hip gcn_fused_ok: `B * n * ld * 2 < 0x7fffffff` for ldx and ldo (the fused kernels index bytes in 32 bits)
    return B * n * _up8(max(I, O)) * 2 < 2 ** 31 - 1


class _PlaneCache(dict):
    """Repacked weights kept across calls: (weight data_ptr, version, in, out, device) -> (planes, weight).  The key is identity + version:
    an in-place update through the tensor bumps the version and misses; one through `.data` does NOT — drop() / clear() are for that.  The
    entry keeps `weight` alive (its data_ptr is the key); at 64 entries the next insertion empties the cache first."""

    def find(self, weight, I, O, dev):
        """(key, the planes kept under it or None)"""
        key = (weight.data_ptr(), weight._version, I, O, dev)
        return key, self.get(key, (None,))[0]

    def put(self, key, planes, weight):
        if len(self) >= 64:
            self.clear()
        self[key] = (planes, weight)

    def drop(self, weight):
        """Forget what belongs to this weight tensor (by identity, or by address)."""
        for k in [k for k, v in self.items() if v[1] is weight or k[0] == weight.data_ptr()]:
            self.pop(k, None)


_PLANES_CACHE = os.environ.get("RECON_GCN_PLANES_CACHE", "1") != "0"
_PLANES = _PlaneCache()            # the layer's planes (recon_gcn_b16_fwd's w_planes) of frozen eval()-mode layers: invalidate_planes()
_STACK_PLANES = _PlaneCache()      # gcn_stack()'s transposed planes (recon_gcn_b16_transposed_planes): invalidate_stack_planes()


def invalidate_stack_planes():
    """Drop the repacked weights gcn_stack() keeps (after an in-place write through `weight.data`)."""
    _STACK_PLANES.clear()


# stands in for autograd's ctx when a forward body runs outside autograd (torch.no_grad()): the bodies only READ needs_input_grad, and this
# value cannot be written to — one instance serves every call
_NO_GRAD_CTX = namedtuple("_NoGradCtx", "needs_input_grad")((False,) * 5)


def _require_bf16(message, *tensors):
    for t in tensors:
        if t is not None and (not t.is_cuda or t.dtype != torch.bfloat16):
            raise TypeError(message)


def _b16_args(B, n, I, O, xr, ldx, adj, weight, bias, sup, out_p, o8, planes, planes_ready, ragged=None, total_rows=0):
    """recon_gcn_b16_args (include/recon_hip.h) of a launch and of a backward's `fwd` field (planes_ready = 1: the forward filled them)."""
    a = _lib.GcnB16Args(B=B, n=n, in_features=I, out_features=O, x=xr.data_ptr(), ldx=ldx, adj=adj.data_ptr(),
                        weight=weight.data_ptr(), bias=_lib.ptr(bias), support=_lib.ptr(sup), lds=o8, out=out_p.data_ptr(), ldo=o8,
                        w_planes=planes.data_ptr(), w_planes_valid=planes_ready)
    if ragged is not None:
        a.node_ptr, a.adj_ptr, a.total_rows = ragged[0].data_ptr(), ragged[1].data_ptr(), total_rows
    return a


# The geometry value that tells a dense batch from a ragged one in the two bodies below: (rows, B, n, ragged, lead, adj_shape, partial, what).
# rows: node rows of x; B, n: graphs and (largest) graph size; ragged: the ragged batch's (node_ptr, adj_ptr) tensors, else None; lead: the leading
# shape of x and of the result; adj_shape: g_adj's; partial: (B, n, extra) for the backward's scratch, recon_gcn_b16_bwd_partial_floats(B, n, in,
# out) + extra * out floats; what: suffix of the entries' names.  A plain tuple, unpacked once per body: building a named one cost the no_grad
# layer path a microsecond per call
def _b16_forward(ctx, geo, x, adj, weight, bias, keep_planes):
    """The forward of both bf16 Functions.  Reads ctx.needs_input_grad and nothing else of ctx; returns (result, tensors to save, meta)."""
    rows, B, n, ragged, lead, _, _, what = geo
    need = ctx.needs_input_grad
    I, O, dev, L = x.shape[-1], weight.shape[1], x.device, _lib.lib()
    o8, bf = _up8(O), dict(dtype=torch.bfloat16, device=dev)
    # `support` = x @ W is only needed again for d adj; without it the dense forward is ONE kernel (k_gcn_b16_fused_fwd) that keeps it in registers
    fused = ragged is None and not need[1] and n <= _FUSED_MAX_N and o8 <= _FUSED_MAX_WIDTH and _fits_int32(B, n, I, O) and _FUSED
    # inference through the fused kernel: it masks the K tail, so what lies behind a row's last feature is never multiplied — anybody's
    # padded rows, and unpadded ones (4-byte aligned), are read in place; training keeps rows it can hand to the weight-gradient GEMM
    masked = fused and not any(need)
    rule = _MFMA_UNREAD if masked else _MFMA
    xr, ldx = x, _row_stride(x, I, rule)
    if ldx is None and masked and I % 2 == 0 and x.is_contiguous() and x.data_ptr() % 16 == 0:
        ldx = I                                                # ... contiguous even rows too, which no rule admits
    elif ldx is None:
        xr, ldx = _packed_rows(x, I, zero_pad=True)
    sup = None if fused else torch.empty(rows, o8, **bf)
    out_p = torch.empty(rows, o8, **bf)
    weight = weight.contiguous()
    # W^T / W repacked for the matrix cores: every call, or kept across calls for a module in eval() mode (`keep_planes`, _PLANES)
    frozen = _PLANES_CACHE and keep_planes and not need[2]
    key, planes = _PLANES.find(weight, I, O, dev) if frozen else (None, None)
    hit = planes is not None
    if not hit:
        planes = torch.empty(L.recon_gcn_b16_planes_bytes(I, O), dtype=torch.uint8, device=dev)
    args = _b16_args(B, n, I, O, xr, ldx, adj, weight, bias, sup, out_p, o8, planes, 1 if hit else 0, ragged, rows)
    with _lib.on_device(dev):
        _lib.check(L.recon_gcn_b16_fwd(C.byref(args), _lib.current_stream()), "recon_gcn_b16_fwd" + what)
    if frozen and not hit:
        _PLANES.put(key, planes, weight)
    return (_padded_result(out_p, lead, O, o8, not fused), (xr, adj, weight, bias, sup, out_p, planes), (geo, I, O, ldx, o8))


def _b16_backward(ctx, gout):
    """The backward of both bf16 Functions: (g_x, g_adj, g_weight, g_bias, None for the fifth argument)."""
    xr, adj, weight, bias, sup, out_p, planes = ctx.saved_tensors
    geo, I, O, ldx, o8 = ctx.meta
    rows, B, n, ragged, lead, adj_shape, (pB, pn, extra), what = geo
    dev, L = gout.device, _lib.lib()
    bf = dict(dtype=torch.bfloat16, device=dev)
    nx, nadj, nw, nb = ctx.needs_input_grad[:4]
    gr, ldg = _grad_rows(gout, O, _MFMA_UNREAD)
    i8 = _up8(I)
    g_sup = torch.empty(rows, o8, **bf)
    partial = torch.empty(L.recon_gcn_b16_bwd_partial_floats(pB, pn, I, O) + extra * O, dtype=torch.float32, device=dev)
    g_x = torch.empty(rows, i8, **bf) if nx else None
    g_adj = torch.empty(adj_shape, **bf) if nadj else None
    g_w = torch.empty(I, O, **bf) if nw else None
    g_b = torch.empty(O, **bf) if (nb and bias is not None) else None
    args = _lib.GcnB16BwdArgs(fwd=_b16_args(B, n, I, O, xr, ldx, adj, weight, bias, sup, out_p, o8, planes, 1, ragged, rows), grad_out=gr.data_ptr(), ldg=ldg,
                              g_support=g_sup.data_ptr(), partial=partial.data_ptr(), g_x=_lib.ptr(g_x), ldgx=i8, g_adj=_lib.ptr(g_adj),
                              g_weight=_lib.ptr(g_w), g_bias=_lib.ptr(g_b), zeros=_lib.zero_page(dev).data_ptr())
    with _lib.on_device(dev):
        _lib.check(L.recon_gcn_b16_bwd(C.byref(args), _lib.current_stream()), "recon_gcn_b16_bwd" + what)
    return _grad_view(g_x, lead + (I,), I, i8), g_adj, g_w, g_b, None


def _keep(ctx, result):
    """A forward body's (result, tensors, meta) onto autograd's ctx."""
    out, saved, ctx.meta = result
    ctx.save_for_backward(*saved)
    return out


def _dense_forward(ctx, x, adj, weight, bias, keep_planes=False):
    _require_bf16("recon_amd: the bfloat16 GraphConvolution path needs bfloat16 GPU tensors for input, adj, weight and bias", x, adj, weight, bias)
    n, I = x.shape[-2], x.shape[-1]
    B = x.numel() // (n * I) if x.numel() else 0
    adj3 = adj.contiguous().view(-1, n, n) if adj.numel() else adj.reshape(0, n, n)
    if adj3.shape[0] != B or weight.shape[0] != I:
        raise ValueError("GraphConvolution: inconsistent shapes")
    geo = (B * n, B, n, None, x.shape[:-1], tuple(adj.shape), (B, n, 0), "")
    return _b16_forward(ctx, geo, x, adj3, weight, bias, keep_planes)


class _GcnB16Function(torch.autograd.Function):
    """The layer on bfloat16 tensors (BASELINE.json configs[2]): bf16 storage, fp32 accumulation, the three feature products on
    the bf16 matrix cores (csrc/gemm_b16.hip, gcn_b16.hip).  Feature counts that are not multiples of 8 live in row-padded
    buffers; the result is returned as a [..., :out] view of one, which the next layer reads in place."""

    @staticmethod
    def forward(ctx, x, adj, weight, bias, keep_planes=False):
        return _keep(ctx, _dense_forward(ctx, x, adj, weight, bias, keep_planes))

    backward = staticmethod(_b16_backward)


class RaggedAdjacency:
    """A batch of graphs of DIFFERENT sizes for GraphConvolution (BASELINE.json configs[4]: power-law graphs of up to 256 nodes each):
    graph b owns node rows node_ptr[b] .. node_ptr[b+1] of the layer's input [N, in] and a dense n_b x n_b adjacency stored at
    values[adj_ptr[b] : adj_ptr[b] + n_b^2] (row major).  Equivalent to the reference layer (models/layers.py:57-63) applied to each graph,
    i.e. to one block-diagonal adjacency over all N nodes.  `values` is a bfloat16 or a float32 GPU tensor — the dtype of the layer's input
    and parameters — and may require grad."""

    def __init__(self, values, sizes):
        sizes = [int(v) for v in sizes]
        if any(v <= 0 for v in sizes):
            raise ValueError("RaggedAdjacency: every graph needs at least one node")
        self.sizes = sizes
        self.B = len(sizes)
        self.n_max = max(sizes) if sizes else 0
        self.total_rows = sum(sizes)
        if values.dim() != 1 or values.numel() != sum(v * v for v in sizes):
            raise ValueError("RaggedAdjacency: `values` must be the flat concatenation of the graphs' n_b x n_b adjacencies")
        self.values = values
        npt = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)
        apt = torch.tensor([0] + [v * v for v in sizes], dtype=torch.int64).cumsum(0)
        self.node_ptr = npt.to(dtype=torch.int32, device=values.device)
        self.adj_ptr = apt.to(device=values.device)

    @classmethod
    def from_dense(cls, mats):
        """From a list of [n_b, n_b] tensors."""
        return cls(torch.cat([m.reshape(-1) for m in mats]), [m.shape[0] for m in mats])

    def block(self, b):
        o, n = int(self.adj_ptr[b]), self.sizes[b]
        return self.values[o:o + n * n].view(n, n)

    def row_tiles(self):
        """The float32 kernels' work list, built once from `sizes`: [tiles, 2] int32 on the values' device, one (graph, row tile) pair per
        32 rows of every graph (include/recon_hip.h: recon_gcn_ragged_fwd's `tiles`)."""
        t = self.__dict__.get("_row_tiles")
        if t is None:
            pairs = [(b, i) for b, n in enumerate(self.sizes) for i in range((n + 31) // 32)]
            t = self._row_tiles = torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2).to(self.values.device)
        return t


class _GcnRaggedFunction(torch.autograd.Function):
    """GraphConvolution over a ragged batch in float32 (csrc/gcn_ragged.hip): x @ W, g_support @ W^T and x^T @ g_support over all node
    rows at once on the dense layer's GEMMs (the same `_GEMM_BX3` switch), the aggregate and g_adj per graph on the exact-fp32 matrix
    cores.  `x` is read in place through a row-strided view."""

    @staticmethod
    def forward(ctx, x, values, weight, bias, ragged):
        _lib.require_gpu(x, values, weight, bias, dtype=torch.float32)
        if x.dim() != 2 or x.shape[0] != ragged.total_rows or weight.shape[0] != x.shape[1]:
            raise ValueError("GraphConvolution (ragged): input must be [total nodes, in_features]")
        if ragged.B > _lib.MAX_BATCH:
            raise NotImplementedError("GraphConvolution (ragged): more than %d graphs per call" % _lib.MAX_BATCH)
        N, I, O, B, dev, L = x.shape[0], x.shape[1], weight.shape[1], ragged.B, x.device, _lib.lib()
        # allocated and returned AS IS: the tensor saved for the backward (its sign is the ReLU mask) is the tensor the caller holds, so an
        # in-place edit of the result is caught by autograd's version check (_GcnFunction's rule)
        out = torch.empty(N, O, dtype=torch.float32, device=dev)
        ctx.ragged = ragged
        if N == 0 or B == 0:                                  # nothing to launch
            ctx.save_for_backward(x, values, weight, bias, out, out, None)
            ctx.ldx = I
            return out
        _lib.check(L.recon_gcn_ragged_supported(B, N, ragged.n_max, I, O), "recon_gcn_ragged_supported")
        xr, ldx = _lib.rows_in_place(x, I)
        values, weight = values.contiguous(), weight.contiguous()
        sup = torch.empty(N, O, dtype=torch.float32, device=dev)
        w_split = None
        mode = _gl._GEMM_BX3                                  # the dense layer's switch and rule (_GcnFunction.forward), over all N rows
        if mode == "1" or (mode != "0" and 2.0 * N * I * O >= 2.0e9):
            w_split = _lib.workspace(L.recon_gcn_split_bytes(I, O), dev)
        tiles = ragged.row_tiles()
        with _lib.on_device(dev):
            _lib.check(L.recon_gcn_ragged_fwd(xr.data_ptr(), ldx, values.data_ptr(), weight.data_ptr(), _lib.ptr(bias), ragged.node_ptr.data_ptr(),
                                              ragged.adj_ptr.data_ptr(), tiles.data_ptr(), tiles.shape[0], B, N, ragged.n_max, I, O, sup.data_ptr(),
                                              out.data_ptr(), _lib.ptr(w_split), _lib.current_stream()), "recon_gcn_ragged_fwd")
        ctx.save_for_backward(xr, values, weight, bias, sup, out, w_split)
        ctx.ldx = ldx
        return out

    @staticmethod
    def backward(ctx, gout):
        xr, values, weight, bias, sup, out, w_split = ctx.saved_tensors
        ragged, ldx = ctx.ragged, ctx.ldx
        N, I, O, B, dev, L = xr.shape[0], xr.shape[1], weight.shape[1], ragged.B, gout.device, _lib.lib()
        f32 = dict(dtype=torch.float32, device=dev)
        nx, nadj, nw, nb = ctx.needs_input_grad[:4]
        g_x = torch.empty(N, I, **f32) if nx else None
        g_adj = torch.empty(values.shape, **f32) if nadj else None
        g_w = torch.empty(I, O, **f32) if nw else None
        g_b = torch.empty(O, **f32) if (nb and bias is not None) else None
        if N == 0 or B == 0:                                  # no rows: the parameters' gradients are sums over nothing
            for g in (g_w, g_b):
                if g is not None:
                    g.zero_()
            return g_x, g_adj, g_w, g_b, None
        gout = gout.contiguous()
        g_sup = torch.empty(N, O, **f32)
        partial = torch.empty(L.recon_gcn_ragged_bwd_partial_floats(B, N, I, O), **f32)
        gs_split = _lib.workspace(L.recon_gcn_bwd_split_bytes(1, N, O), dev) if (w_split is not None and g_w is not None) else None
        tiles = ragged.row_tiles()
        with _lib.on_device(dev):
            _lib.check(L.recon_gcn_ragged_bwd(xr.data_ptr(), ldx, values.data_ptr(), weight.data_ptr(), ragged.node_ptr.data_ptr(),
                                              ragged.adj_ptr.data_ptr(), tiles.data_ptr(), tiles.shape[0], B, N, ragged.n_max, I, O, sup.data_ptr(),
                                              out.data_ptr(), _lib.ptr(w_split), gout.data_ptr(), g_sup.data_ptr(), partial.data_ptr(), _lib.ptr(g_x),
                                              _lib.ptr(g_adj), _lib.ptr(g_w), _lib.ptr(g_b), _lib.ptr(gs_split), _lib.current_stream()),
                       "recon_gcn_ragged_bwd")
        return g_x, g_adj, g_w, g_b, None


class _GcnB16RaggedFunction(torch.autograd.Function):
    """GraphConvolution over a ragged batch in bfloat16: x @ W over all node rows at once (bf16 matrix cores), the aggregate per graph."""

    @staticmethod
    def forward(ctx, x, values, weight, bias, ragged):
        _require_bf16("recon_amd: the ragged GraphConvolution path needs bfloat16 GPU tensors for input, adjacency values, weight and bias", x, values, weight, bias)
        if x.dim() != 2 or x.shape[0] != ragged.total_rows or weight.shape[0] != x.shape[1]:
            raise ValueError("GraphConvolution (ragged): input must be [total nodes, in_features]")
        if ragged.B > _lib.MAX_BATCH:
            raise NotImplementedError("GraphConvolution (ragged): more than %d graphs per call" % _lib.MAX_BATCH)
        N = x.shape[0]
        geo = (N, ragged.B, ragged.n_max, (ragged.node_ptr, ragged.adj_ptr), (N,), tuple(values.shape), (1, N, ragged.B), " (ragged)")
        return _keep(ctx, _b16_forward(ctx, geo, x, values.contiguous(), weight, bias, False))

    backward = staticmethod(_b16_backward)


class SparseMM(torch.autograd.Function):
    """models/layers.py:9-32 is a legacy (non-static) autograd Function for `mm` that current torch can no
    longer run; this static equivalent keeps the name and the gradients dA = g B^T, dB = A^T g."""

    @staticmethod
    def forward(ctx, matrix1, matrix2):
        ctx.save_for_backward(matrix1, matrix2)
        return _mm(matrix1, matrix2, False, False)

    @staticmethod
    def backward(ctx, grad_output):
        matrix1, matrix2 = ctx.saved_tensors
        g1 = _mm(grad_output, matrix2, False, True) if ctx.needs_input_grad[0] else None
        g2 = _mm(matrix1, grad_output, True, False) if ctx.needs_input_grad[1] else None
        return g1, g2


def _mm(a, b, a_t, b_t):
    """op(a) op(b): fp32 GPU matrices on this library's fp32 matrix-core GEMM (recon_sgemm_ex); anything else (the class is kept for
    name compatibility and is also importable on a CPU-only host) on torch.mm."""
    if a.is_cuda and b.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 2 and b.dim() == 2:
        from .gat_layers import _sgemm_ex
        return _sgemm_ex(a.contiguous(), a_t, b.contiguous(), b_t)
    return torch.mm(a.t() if a_t else a, b.t() if b_t else b)


def _ptrs(base, offsets):
    return (C.c_void_p * len(offsets))(*[base + o for o in offsets])


def _stack_args(B, n, I, D, nl, x, ldx, x_rows, ldxr, adj3, ws, bs, planes, poff, acts, o8, **backward):
    """recon_gcn_b16_stack_train_args (include/recon_hip.h) as the forward fills it; the backward adds its own fields by name (`backward`).
    x / ldx: the rows layer 0 reads; x_rows / ldxr: where the kernel leaves their aligned copy (None: x already is one)."""
    return _lib.GcnB16StackTrainArgs(B=B, n=n, in_features=I, hidden=D, L=nl, x=x.data_ptr(), ldx=ldx, x_rows=_lib.ptr(x_rows), ldxr=ldxr,
                                     adj=adj3.data_ptr(), weight=_lib.ptr_array(ws), bias=_lib.ptr_array(bs), planes=_ptrs(planes.data_ptr(), poff),
                                     acts=_ptrs(acts.data_ptr(), [l * B * n * o8 * 2 for l in range(nl)]), ldo=o8, **backward)


class _GcnB16StackFunction(torch.autograd.Function):
    """`for l in layers: x = l(x, adj)` with gradients, as one launch forward and three launches backward (csrc/gcn_b16.hip:
    k_gcn_b16_stack_fwd keeping every layer's result; k_gcn_b16_stack_bwd; one split-K launch + one second pass for all weight and bias
    gradients): models/layers.py:57-63 applied L times.  Output, g_x and g_bias are bit-equal to the loop over _GcnB16Function, g_W up to
    the summation order of its split-K partials.  `adj` gets no gradient here (gcn_stack() routes such calls through the loop).
    Host side: one allocation per KIND of buffer (results, repacked weights, g_support, gradients), not per layer — at cfg 3a the loop's
    ~40 small allocations and launches were as long as its kernels."""

    @staticmethod
    def forward(ctx, x, adj, n_layers, *params):
        ws, bs = list(params[0::2]), list(params[1::2])
        n, I, D = x.shape[-2], x.shape[-1], ws[0].shape[1]
        B = x.numel() // (n * I)
        dev, L, o8 = x.device, _lib.lib(), _up8(D)
        # rows the weight-gradient GEMM of layer 0 can read: 16-byte aligned, stride % 8 == 0 (its pad columns only reach rows of the product
        # that are never stored, so they need no zeros; the forward kernel masks its own K tail)
        ldx = _rows_view(x, I, pads_read=False)
        xr, xin, ldin = x, x, ldx
        if ldx is None:
            ldin = _row_stride(x, I, _MASKED)
            if ldin is not None and x.data_ptr() % 16 == 0:          # the forward kernel reads x where it lies and leaves the aligned copy itself
                ldx = _up8(I)
                xr = torch.empty(B * n, ldx, dtype=torch.bfloat16, device=dev)
            else:
                xr, ldx = _packed_rows(x, I, zero_pad=False)
                xin, ldin = xr, ldx
        adj3 = adj.contiguous().view(-1, n, n)
        ws = [w.contiguous() for w in ws]
        acts = torch.empty(n_layers, B * n, o8, dtype=torch.bfloat16, device=dev)
        pb = [(L.recon_gcn_b16_planes_bytes(w.shape[0], D) + 255) // 256 * 256 for w in ws]
        poff = [sum(pb[:l]) for l in range(n_layers)]
        planes = torch.empty(sum(pb), dtype=torch.uint8, device=dev)
        args = _stack_args(B, n, I, D, n_layers, xin, ldin, xr if xr is not xin else None, ldx, adj3, ws, bs, planes, poff, acts, o8)
        with _lib.on_device(dev):
            _lib.check(L.recon_gcn_b16_stack_train_fwd(C.byref(args), _lib.current_stream()), "recon_gcn_b16_stack_train_fwd")
        ctx.save_for_backward(xr, adj3, acts, planes, *ws, *[b for b in bs if b is not None])
        ctx.meta = (B, n, I, D, n_layers, ldx, o8, tuple(x.shape), [b is not None for b in bs], poff)
        return _padded_result(acts[n_layers - 1], x.shape[:-1], D, o8, zero_tail=False)

    @staticmethod
    def backward(ctx, gout):
        B, n, I, D, nl, ldx, o8, xs, has_b, poff = ctx.meta
        sv = ctx.saved_tensors
        (xr, adj3, acts, planes), ws, it = sv[:4], sv[4:4 + nl], iter(sv[4 + nl:])
        bs = [next(it) if h else None for h in has_b]
        dev, L = gout.device, _lib.lib()
        bf = dict(dtype=torch.bfloat16, device=dev)
        gr, ldg = _grad_rows(gout, D, _MASKED)                      # read in place through masked loads: any even row stride
        i8 = I if I % 4 == 0 else _up8(I)                           # g_x leaves the kernel as 8-byte stores: a dense [.., I] result where I % 4 == 0
        need, rows = ctx.needs_input_grad, B * n
        g_sup = torch.empty(nl, rows, o8, **bf)
        partial = torch.empty(L.recon_gcn_b16_stack_bwd_partial_floats(B, n, I, D, nl), dtype=torch.float32, device=dev)
        g_x = torch.empty(rows, i8, **bf) if need[0] else None
        # the parameters' gradients: one buffer [g_W_0 | g_W_1 .. | g_b_0 ..], handed back as views
        wn = [w.shape[0] * D for w in ws]
        gbuf = torch.empty(sum(wn) + nl * D, **bf)
        g_w = [gbuf[sum(wn[:l]):sum(wn[:l + 1])].view(ws[l].shape[0], D) if need[3 + 2 * l] else None for l in range(nl)]
        g_b = [gbuf[sum(wn) + l * D:sum(wn) + (l + 1) * D] if (bs[l] is not None and need[4 + 2 * l]) else None for l in range(nl)]
        args = _stack_args(B, n, I, D, nl, xr, ldx, None, 0, adj3, ws, bs, planes, poff, acts, o8, grad_out=gr.data_ptr(), ldg=ldg,
                           g_support=_ptrs(g_sup.data_ptr(), [l * rows * o8 * 2 for l in range(nl)]), partial=partial.data_ptr(), g_x=_lib.ptr(g_x),
                           ldgx=i8, g_weight=_lib.ptr_array(g_w), g_bias=_lib.ptr_array(g_b), zeros=_lib.zero_page(dev).data_ptr())
        with _lib.on_device(dev):
            _lib.check(L.recon_gcn_b16_stack_train_bwd(C.byref(args), _lib.current_stream()), "recon_gcn_b16_stack_train_bwd")
        return (_grad_view(g_x, xs, I, i8), None, None, *[g for l in range(nl) for g in (g_w[l], g_b[l])])


def _layer_loop(x, adj, layers):
    for l in layers:
        x = l(x, adj)
    return x


def _stack_form(x, adj, layers, need_grad):
    """How gcn_stack() runs a dense batch: "train" (_GcnB16StackFunction), "infer" (recon_gcn_b16_stack_fwd), or None: layer by layer."""
    if not (len(layers) >= 2 and len(layers) <= 8 and x.is_cuda and x.dtype == torch.bfloat16 and adj.dtype == torch.bfloat16
            and x.dim() in (2, 3) and os.environ.get("RECON_GCN_STACK", "1") != "0" and not (need_grad and adj.requires_grad)):
        return None
    n, I, D = x.shape[-2], x.shape[-1], layers[0].out_features
    B = x.numel() // (n * I) if x.numel() else 0
    # the fused kernels' shapes with 8-byte adjacency / bias loads (csrc/gcn_b16.hip recon_gcn_b16_stack_fwd: n % 4, hidden % 4, `a->B > 65535 * 4`)
    if not (B > 0 and n <= _FUSED_MAX_N and n % 4 == 0 and D % 4 == 0 and _up8(D) <= _FUSED_MAX_WIDTH and layers[0].in_features == I
            and all(l.in_features == D and l.out_features == D for l in layers[1:])
            and all(l.weight.dtype == torch.bfloat16 and (l.bias is None or l.bias.data_ptr() % 8 == 0) for l in layers)
            and adj.is_contiguous() and adj.data_ptr() % 8 == 0
            and adj.numel() == B * n * n and _fits_int32(B, n, I, D) and B <= 4 * _lib.MAX_BATCH):
        return None
    if need_grad:       # recon_gcn_b16_stack_train_bwd: `in_features > 16 * kFusedNT` is unsupported (g_x of layer 0 is one tile)
        return "train" if _up8(I) <= _FUSED_MAX_WIDTH and os.environ.get("RECON_GCN_STACK_TRAIN", "1") != "0" else None
    return "infer" if x.is_contiguous() and I % 2 == 0 and x.data_ptr() % 16 == 0 else None


def gcn_stack(x, adj, layers):
    """`for l in layers: x = l(x, adj)` — the reference's stacks of GraphConvolutions over one adjacency (models/layers.py:57-63 applied
    len(layers) times) — as ONE launch where that is possible: bfloat16 tensors, graphs of n <= 32 nodes with n % 4 == 0, every layer
    hidden -> hidden after the first with hidden % 4 == 0, hidden <= 320.  The activations of a graph stay in LDS between the layers
    (csrc/gcn_b16.hip: k_gcn_b16_stack_fwd); with gradients (anything but `adj` requiring grad, in_features <= 320) the forward also keeps
    every layer's result and the backward is the mirror-image kernel + one weight-gradient GEMM per layer (_GcnB16StackFunction).  Results
    and gradients are bit-equal to the loop, which is also what runs for every other case.  Repacked weights are kept per weight tensor (identity + version); call
    invalidate_stack_planes() after writing through `weight.data`.
    A RaggedAdjacency (graphs of different sizes, x [total nodes, in]) runs layer by layer in bfloat16 and in float32 alike: the same
    calls as the loop, hence the same bits."""
    layers = list(layers)
    if isinstance(adj, RaggedAdjacency):        # graphs of different sizes: layer by layer (GEMM over all rows + aggregate per graph;
        return _layer_loop(x, adj, layers)      # the one-kernel form of a bf16 layer was measured and is no faster there)
    need_grad = torch.is_grad_enabled() and (x.requires_grad or adj.requires_grad or any(p.requires_grad for l in layers for p in l.parameters()))
    form = _stack_form(x, adj, layers, need_grad)
    if form is None:
        return _layer_loop(x, adj, layers)
    if form == "train":
        return _GcnB16StackFunction.apply(x, adj, len(layers), *[p for l in layers for p in (l.weight, l.bias)])
    n, I, D = x.shape[-2], x.shape[-1], layers[0].out_features
    B, dev, L, o8 = x.numel() // (n * I), x.device, _lib.lib(), _up8(D)
    planes = []
    with _lib.on_device(dev):
        for l in layers:
            w = l.weight
            key, pl = _STACK_PLANES.find(w, l.in_features, D, dev)
            if pl is None:
                kp = (l.in_features + 31) // 32 * 32
                pl = torch.empty(D * kp, dtype=torch.bfloat16, device=dev)
                _lib.check(L.recon_gcn_b16_transposed_planes(w.detach().contiguous().data_ptr(), l.in_features, D, pl.data_ptr(), _lib.current_stream()),
                           "recon_gcn_b16_transposed_planes")
                _STACK_PLANES.put(key, pl, w)
            planes.append(pl)
        out_p = torch.empty(B * n, o8, dtype=torch.bfloat16, device=dev)
        args = _lib.GcnB16StackArgs(B=B, n=n, in_features=I, hidden=D, L=len(layers), x=x.data_ptr(), ldx=I, adj=adj.data_ptr(),
                                    w_planes=_lib.ptr_array(planes), bias=_lib.ptr_array([l.bias for l in layers]), out=out_p.data_ptr(), ldo=o8)
        rc = L.recon_gcn_b16_stack_fwd(C.byref(args), _lib.current_stream())
    if rc == -2:                                # RECON_ERR_UNSUPPORTED: layer by layer
        return _layer_loop(x, adj, layers)
    _lib.check(rc, "recon_gcn_b16_stack_fwd")
    return _padded_result(out_p, x.shape[:-1], D, o8, zero_tail=False)


class GraphConvolution(Module):
    """Simple GCN layer, models/layers.py:35-68: relu(adj @ (input @ weight) + bias)."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.weight = Parameter(torch.Tensor(in_features, out_features))
        if bias:
            self.bias = Parameter(torch.Tensor(out_features))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1. / math.sqrt(self.weight.size(1))
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)
        self.invalidate_planes()

    def invalidate_planes(self):
        """Drop the repacked copies of `weight` an eval()-mode bfloat16 layer keeps across calls.  Needed after an in-place write through
        `weight.data` (which autograd's version counter does not see); reset_parameters, load_state_dict and .to() / .cuda() call it.
        Only the layer's own planes: what gcn_stack() keeps of the same weight goes with invalidate_stack_planes()."""
        _PLANES.drop(self.weight)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self.invalidate_planes()

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_planes()
        return super()._apply(fn, *args, **kwargs)

    def forward(self, input, adj):
        if isinstance(adj, RaggedAdjacency):                  # graphs of different sizes: input [total nodes, in], bfloat16 or float32
            if input.dtype != adj.values.dtype and {input.dtype, adj.values.dtype} == {torch.float32, torch.bfloat16}:
                raise TypeError("GraphConvolution (ragged): input is %s but the adjacency values are %s" % (input.dtype, adj.values.dtype))
            fn = _GcnRaggedFunction if input.dtype == torch.float32 else _GcnB16RaggedFunction
            return fn.apply(input, adj.values, self.weight, self.bias, adj)
        fn = _GcnB16Function if input.dtype == torch.bfloat16 else _GcnFunction     # bf16 storage / fp32 accumulate (module.to(torch.bfloat16))
        extra = (not self.training,) if fn is _GcnB16Function else ()              # eval(): the repacked weight planes are kept across calls
        if input.dim() == 3 and input.shape[0] > _lib.MAX_BATCH:   # 16-bit grid dimension over the graphs; graphs are independent: run slices
            B = input.shape[0]
            return torch.cat([fn.apply(input[b0:b0 + _lib.MAX_BATCH], adj[b0:b0 + _lib.MAX_BATCH] if adj.dim() == 3 else adj, self.weight, self.bias, *extra)
                              for b0 in range(0, B, _lib.MAX_BATCH)], dim=0)
        if fn is _GcnB16Function and not torch.is_grad_enabled():
            # inference: nothing is recorded, so the autograd.Function machinery (~10 us per call, a third of this layer's host time at
            # cfg 3a) is skipped; the same forward body runs with a context that says "no gradients" and stores nothing
            return _dense_forward(_NO_GRAD_CTX, input, adj, self.weight, self.bias, *extra)[0]
        return fn.apply(input, adj, self.weight, self.bias, *extra)

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'
