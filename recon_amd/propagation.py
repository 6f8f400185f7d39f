"""GP-GNN propagation step.  The reference has no module for it: the block is inlined four times in
models/models.py (GPGNN :238-277, RECON_EAC :447-487, RECON_EAC_KGGAT :657-701, RECON :895-968).
This module offers the same arithmetic as functions with the reference's tensor conventions, running
in the gfx950 kernels of csrc/prop.hip:

    build_block_adjacency(T, identity, n)            models/models.py:240-259
    propagate(adj_list, h0, nonlinearity, head_indices, tail_indices)     :260-274
    make_start_embedding / get_head_indices / get_tail_indices            utils/embedding_utils.py:170-202
    make_start_entity_embeddings                     utils/context_utils.py:387-426
    build_adjecent_matrix                            utils/build_adjecent_matrix.py:6-17

No CPU path: the tensor functions require GPU tensors.
"""
import ctypes as C
import os
import itertools

import numpy as np
import torch

from . import _lib


# how this module's calls check dtypes: index tensors pass, and the message names the kernels the call runs
_ONE_DTYPE = dict(floats_only=True, wrong_dtype=(TypeError, "recon_amd: this call runs the %(want)s kernels, got a %(got)s tensor"))


def _float_dtype(*ts):
    """float32 or bfloat16: the one floating dtype of the call's tensors (the kernels exist for these two)."""
    dts = {t.dtype for t in ts if t is not None and t.is_floating_point()}
    if len(dts) != 1 or next(iter(dts)) not in (torch.float32, torch.bfloat16):
        raise TypeError("recon_amd: the propagation kernels take float32 or bfloat16 tensors of ONE dtype, got %s" % sorted(map(str, dts)))
    return next(iter(dts))


# ------------------------------------------------------------------------------- which kernel instance ran
_TRACE = None


class trace_instances:
    """`with trace_instances() as t: ...` — t collects (call, key) for every propagation launch of the block, `call` the C entry's name
    and `key` the kernel instance the library selects for exactly the arguments of that launch (include/recon_hip.h:
    recon_propagate_instance).  For tests: tests/test_prop_instances_gpu.py pins every row of its table to the instance it names.
    One module-wide list: not re-entrant across threads (launches of another thread inside the block are recorded too), inert when unused."""

    def __enter__(self):
        global _TRACE
        self.prev, _TRACE = _TRACE, []
        return _TRACE

    def __exit__(self, *exc):
        global _TRACE
        _TRACE = self.prev
        return False


def _launch(name, args, what=None):
    """One propagation entry of the library on the current stream of the caller's device (set by the caller's on_device block)."""
    L = _lib.lib()
    if _TRACE is not None:
        if name.startswith("recon_propagate_b16"):
            key = L.recon_propagate_b16_instance(C.byref(args.fwd if name.endswith("bwd") else args), int(name.endswith("bwd")))
        else:
            key = (L.recon_propagate_bwd_instance if name.endswith("bwd") else L.recon_propagate_instance)(C.byref(args))
        _TRACE.append((name, key))
    _lib.check(getattr(L, name)(C.byref(args), _lib.current_stream()), what or name)


# ------------------------------------------------------------------------------- host-side index builders
def _pairs(n):
    return [(i, j) for i in range(n) for j in range(n) if i != j]     # channel order, conversion_util.py:6-20


def make_start_embedding(n, d):
    """[n(n-1), 2dn, 1] float64 numpy array, as utils/embedding_utils.py:170-182 returns it."""
    v = np.zeros((n * (n - 1), 2 * d * n, 1), dtype=np.float64)
    for c, (i, j) in enumerate(_pairs(n)):
        v[c, 2 * d * i: 2 * d * i + d, 0] = 1.0
        v[c, 2 * d * j + d: 2 * d * (j + 1), 0] = 1.0
    return v


def get_head_indices(n, d, bs=50):
    """utils/embedding_utils.py:184-192 (nested lists of ranges there; an int64 array here)."""
    rows = np.asarray([list(range(2 * d * i, 2 * d * (i + 1))) for i, _ in _pairs(n)], dtype=np.int64)
    return np.tile(rows[None], (bs, 1, 1))


def get_tail_indices(n, d, bs=50):
    """utils/embedding_utils.py:194-202."""
    rows = np.asarray([list(range(2 * d * j, 2 * d * (j + 1))) for _, j in _pairs(n)], dtype=np.int64)
    return np.tile(rows[None], (bs, 1, 1))


def build_adjecent_matrix(n, size=72):
    """utils/build_adjecent_matrix.py:6-17 -> torch.FloatTensor [72,72] (row-normalised line graph)."""
    A = np.zeros((size, size), dtype=np.float32)
    V = list(itertools.permutations(range(n), 2))
    for i, x in enumerate(V):
        for j, y in enumerate(V):
            A[i, j] = 1.0 if (x[0] == y[1] or x[1] == y[0] or i == j) else 0.0
        s = A[i].sum()
        if s != 0:
            A[i] /= s
    return torch.from_numpy(A)


# ------------------------------------------------------------------------------- P1
class _BlockAdjacency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, T, identity, n):
        _lib.require_gpu(T, identity, dtype=torch.float32, **_ONE_DTYPE)
        T, identity = T.contiguous(), identity.contiguous()
        B = T.shape[0]
        dd = identity.shape[0]
        if T.numel() != B * n * (n - 1) * dd * dd:
            raise ValueError("T must hold B x n(n-1) transition matrices of %dx%d" % (dd, dd))
        A = torch.empty(B, n * dd, n * dd, dtype=torch.float32, device=T.device)
        with _lib.on_device(T.device):
            _lib.check(_lib.lib().recon_block_adjacency_fwd(T.data_ptr(), identity.data_ptr(), B, n, dd, A.data_ptr(),
                                                            _lib.current_stream()), "recon_block_adjacency_fwd")
        ctx.dims = (B, n, dd, tuple(T.shape))
        return A

    @staticmethod
    def backward(ctx, gA):
        B, n, dd, tshape = ctx.dims
        gA = gA.contiguous()
        gT = torch.empty(tshape, dtype=torch.float32, device=gA.device) if ctx.needs_input_grad[0] else None
        gI = torch.empty(dd, dd, dtype=torch.float32, device=gA.device) if ctx.needs_input_grad[1] else None
        L = _lib.lib()
        ws = (torch.empty(L.recon_block_adjacency_bwd_workspace_floats(B, n, dd), dtype=torch.float32, device=gA.device)
              if gI is not None else None)
        with _lib.on_device(gA.device):
            _lib.check(L.recon_block_adjacency_bwd(gA.data_ptr(), B, n, dd, _lib.ptr(gT), _lib.ptr(gI), _lib.ptr(ws),
                                                   _lib.current_stream()), "recon_block_adjacency_bwd")
        return gT, gI, None


class _BlockAdjacencyB16(torch.autograd.Function):
    """P1 on bfloat16 tensors (csrc/prop_b16.hip)."""

    @staticmethod
    def forward(ctx, T, identity, n):
        _lib.require_gpu(T, identity, dtype=torch.bfloat16, **_ONE_DTYPE)
        T, identity = T.contiguous(), identity.contiguous()
        B = T.shape[0]
        dd = identity.shape[0]
        if T.numel() != B * n * (n - 1) * dd * dd:
            raise ValueError("T must hold B x n(n-1) transition matrices of %dx%d" % (dd, dd))
        A = torch.empty(B, n * dd, n * dd, dtype=torch.bfloat16, device=T.device)
        with _lib.on_device(T.device):
            for b0 in range(0, B, _lib.MAX_BATCH):
                nb = min(B, b0 + _lib.MAX_BATCH) - b0
                _lib.check(_lib.lib().recon_block_adjacency_b16_fwd(T[b0:].data_ptr(), identity.data_ptr(), nb, n, dd, A[b0:].data_ptr(),
                                                                    _lib.current_stream()), "recon_block_adjacency_b16_fwd")
        ctx.dims = (B, n, dd, tuple(T.shape))
        return A

    @staticmethod
    def backward(ctx, gA):
        B, n, dd, tshape = ctx.dims
        gA = gA.contiguous()
        if B > _lib.MAX_BATCH:
            raise NotImplementedError("bfloat16 block adjacency backward: more than %d graphs per call" % _lib.MAX_BATCH)
        gT = torch.empty(tshape, dtype=torch.bfloat16, device=gA.device) if ctx.needs_input_grad[0] else None
        gI = torch.empty(dd, dd, dtype=torch.bfloat16, device=gA.device) if ctx.needs_input_grad[1] else None
        L = _lib.lib()
        ws = (torch.empty(L.recon_block_adjacency_b16_bwd_workspace_floats(dd), dtype=torch.float32, device=gA.device)
              if gI is not None else None)
        with _lib.on_device(gA.device):
            _lib.check(L.recon_block_adjacency_b16_bwd(gA.data_ptr(), B, n, dd, _lib.ptr(gT), _lib.ptr(gI), _lib.ptr(ws),
                                                       _lib.current_stream()), "recon_block_adjacency_b16_bwd")
        return gT, gI, None


def build_block_adjacency(T, identity, n):
    """models/models.py:240-259: T [B, n-1, n, (2d)^2] or [B, n(n-1), (2d)^2] (AFTER the non-linearity),
    identity [2d,2d] -> A [B, S, S], A[b, i*2d+r, j*2d+c] = T[b, e(i,j)].view(2d,2d)[r,c], identity on the
    diagonal blocks.  float32 or bfloat16 (both tensors alike)."""
    if _float_dtype(T, identity) == torch.bfloat16:
        return _BlockAdjacencyB16.apply(T, identity, n)
    return _BlockAdjacency.apply(T, identity, n)


# ------------------------------------------------------------------------------- P2
_STANDIN = 16        # a probe's non-null, 16-byte-aligned stand-in for a pointer the queries test but never follow


class _Call:
    """One propagation call, normalised once: the sizes, the strides, the contiguous tensors and the callers' shapes, for float32 and bfloat16,
    adjacency mode (`mats` = the L adjacencies [B,S,S] or [B,1,S,S]) and block mode (`identity` and `n` given: `mats` = the L transition
    tensors [B, n(n-1), (2d)^2] or [B, n-1, n, (2d)^2]).  Performs the shape checks, and writes the library's argument struct for a launch,
    for the `fwd` field of a backward and (probe) for a query ahead of the call — every field by name."""
    __slots__ = ("B", "Cn", "S", "L", "dd", "act", "h0_bs", "idx_bs", "b16", "dev", "h0", "head", "tail", "identity", "mats", "given", "h0_shape", "mat_shapes")

    def __init__(self, h0, act, head, tail, mats, identity=None, n=None):
        self.act, self.L, self.b16, self.dev, self.given = act, len(mats), h0.dtype == torch.bfloat16, h0.device, mats
        if identity is None:
            self.mats = mats = [a.contiguous().view(a.shape[0], a.shape[-2], a.shape[-1]) for a in mats]   # accepts [B,1,S,S]
            B, S = mats[0].shape[0], mats[0].shape[-1]
            h0 = h0.contiguous()
            Cn = h0.shape[1] if h0.dim() == 4 else h0.shape[0]
            dd = head.shape[-1]
        else:
            dd, B = identity.shape[0], mats[0].shape[0]
            S, Cn = n * dd, n * (n - 1)
            self.mats = [t.contiguous().view(B, Cn, dd * dd) for t in mats]
            identity, h0 = identity.contiguous(), h0.contiguous()
        self.B, self.Cn, self.S, self.dd = B, Cn, S, dd
        self.h0, self.identity = h0, identity
        self.h0_bs = Cn * S if h0.dim() == 4 else 0       # [B, C, S, 1] (RECON*: models/models.py:470), else [C, S, 1] shared (GPGNN: :260)
        self.head, self.tail = head.contiguous(), tail.contiguous()
        per_graph = head.dim() == 3 and head.shape[0] > 1   # the kernels then index head / tail by graph: rows for every graph, or one set shared
        self.idx_bs = Cn * dd if per_graph else 0
        if per_graph and head.shape[0] < B:
            raise ValueError("head/tail indices hold %d batch rows but the batch has %d" % (head.shape[0], B))

    def new(self, *shape):
        return torch.empty(shape, dtype=torch.bfloat16 if self.b16 else torch.float32, device=self.dev)

    def new_out(self):
        return self.new(self.B, self.Cn, self.L * self.dd)

    def new_states(self):
        return self.new(self.L, self.B, self.Cn, self.S)

    def args(self, out, hs=None, stats=None):
        """recon_prop_args / recon_prop_b16_args of this call (include/recon_hip.h).  A launch passes its buffers; a backward's `fwd` field
        passes grad_out as `out` (unused there, but the argument check wants it non-null).  The struct keeps the pointer array alive."""
        a = (_lib.PropB16Args if self.b16 else _lib.PropArgs)(
            B=self.B, C=self.Cn, S=self.S, L=self.L, dd=self.dd, act=_lib.ACT[self.act], h0=self.h0.data_ptr(), h0_batch_stride=self.h0_bs,
            head_idx=self.head.data_ptr(), tail_idx=self.tail.data_ptr(), idx_batch_stride=self.idx_bs, out=out.data_ptr(), h_saved=_lib.ptr(hs))
        if self.identity is None:
            a.adj = _lib.ptr_array(self.mats)
        else:
            a.trans, a.identity = _lib.ptr_array(self.mats), self.identity.data_ptr()
        if self.b16:
            a.zeros = _lib.zero_page(self.dev).data_ptr()
        else:
            a.stats = _lib.ptr(stats)
        return a

    @staticmethod
    def probe(b16, B, Cn, S, L, dd, h0=None, wide_blocks=False):
        """The struct of a call that does not exist yet, for the library's form and workspace queries: sizes, and h0's address and stride
        where the query looks at them.  wide_blocks: as block mode's wide-state forms see it — the queries test `trans`, `identity` and
        `split_ws` for null and never follow them (csrc/prop.hip: recon_propagate_ws_bytes, recon_propagate_bwd_chain_ws_floats), so
        stand-ins are set here, and nowhere else: `split_ws` where the library says that workspace exists."""
        p = (_lib.PropB16Args if b16 else _lib.PropArgs)(B=B, C=Cn, S=S, L=L, dd=dd, act=1)
        if h0 is not None:
            p.h0, p.h0_batch_stride = h0.data_ptr(), Cn * S if h0.dim() == 4 else 0
        if wide_blocks:
            p.trans, p.identity = (C.c_void_p * 1)(), _STANDIN
            p.split_ws_bytes = _lib.lib().recon_propagate_ws_bytes(C.byref(p))
            p.split_ws = _STANDIN if p.split_ws_bytes else None
        return p

    def save(self, ctx, *extra):
        """For the backward: the tensors through save_for_backward (`extra` first); on ctx only a tuple of the sizes and the callers' shapes."""
        ctx.save_for_backward(*extra, self.h0, self.head, self.tail, self.identity, *self.mats)
        ctx.sizes = (self.B, self.Cn, self.S, self.L, self.dd, self.act, self.h0_bs, self.idx_bs, self.b16, self.dev,
                     self.h0.shape, [m.shape for m in self.given], len(extra))

    @staticmethod
    def saved(ctx):
        """(the call save() saw, rebuilt from ctx.sizes and autograd's saved tensors; the `extra` tensors of save())."""
        nz, t = object.__new__(_Call), ctx.saved_tensors
        nz.B, nz.Cn, nz.S, nz.L, nz.dd, nz.act, nz.h0_bs, nz.idx_bs, nz.b16, nz.dev, nz.h0_shape, nz.mat_shapes, k = ctx.sizes
        nz.h0, nz.head, nz.tail, nz.identity = t[k:k + 4]
        nz.mats = list(t[k + 4:])
        return nz, t[:k]


def _split_workspace(args, dev):
    """Workspace of the wide-state two-term forward (include/recon_hip.h: recon_prop_args.split_ws); None where that form does not
    exist.  Sets the two fields of `args`; the caller keeps the returned tensor alive across the launch."""
    nbytes = _lib.lib().recon_propagate_ws_bytes(C.byref(args))
    if not nbytes:
        return None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args.split_ws, args.split_ws_bytes = ws.data_ptr(), nbytes
    return ws


def _chain_workspaces(nz, args):
    """The wide-state backward on the forward's two-term f16 kernels (csrc/prop_hl.hip: all hops in one launch), for GP-GNN's block-structured
    gather indices: sets fwd.split_ws, head_blk, tail_blk and chain_ws of `args` where that form exists.  Returns the tensors to keep alive
    across the launch, the chain workspace last (None: no chain form)."""
    blk = _index_blocks(nz.head, nz.tail, nz.dd, nz.S, align=16)
    if blk is None:
        return None, None
    fwd = args.fwd
    ws = _split_workspace(fwd, nz.dev)
    nch = _lib.lib().recon_propagate_bwd_chain_ws_floats(C.byref(fwd)) if ws is not None else 0
    if not nch:
        return ws, None
    chain = torch.empty(nch, dtype=torch.float32, device=nz.dev)
    args.head_blk, args.tail_blk, args.chain_ws = blk[0].data_ptr(), blk[1].data_ptr(), chain.data_ptr()
    return ws, chain


def _forward_f32(ctx, nz, what=None):
    need = any(ctx.needs_input_grad)
    out = nz.new_out()
    hs = nz.new_states() if need else None
    args = nz.args(out, hs)
    ws = _split_workspace(args, nz.dev)       # wide states (160 < S <= 512): A_l pre-split into half terms, slice by slice
    stats = None
    if need and _lib.lib().recon_propagate_form(C.byref(args)) & 1:
        # two-term f16 kernels: the forward records per graph the max magnitudes of the states and adjacencies, the backward takes its
        # per-tensor scales from them (include/recon_hip.h: recon_prop_args.stats)
        stats = nz.new(nz.B, 2 * nz.L + 1)
        args.stats = stats.data_ptr()
    with _lib.on_device(nz.dev):
        _launch("recon_propagate_fwd", args, what)
    if need:
        nz.save(ctx, hs, stats)
    return out


def _backward(ctx, gout, first, name, what, fill):
    """What the four backwards share.  grad_out contiguous and 16-byte aligned (a view at an odd offset is copied: the kernels read it in
    16-byte pieces); d loss / d A_l or d T_l for the inputs from position `first` on that want one; g_h [B, C, S]; the backward's struct
    with `fwd`, grad_out, g_h and g_adj | g_trans set.  fill(nz, args, stats) adds the workspaces and fields of its form and returns
    (g_identity or None, what must outlive the launch).  Then d loss / d h0 — g_h itself per graph, its sum over the graphs (bfloat16:
    summed in fp32, rounded once) where h0 is shared — and every gradient in its input's own shape.  Returns (g_h0, g_identity, the L
    gradients)."""
    nz, (hs, stats) = _Call.saved(ctx)
    gout = gout.contiguous()
    if gout.data_ptr() % 16:
        gout = gout.clone()
    g_mats = [nz.new(*m.shape) if ctx.needs_input_grad[first + l] else None for l, m in enumerate(nz.mats)]
    g_h = nz.new(nz.B, nz.Cn, nz.S)
    fwd = nz.args(gout, hs, stats)
    args = (_lib.PropB16BwdArgs if nz.b16 else _lib.PropBwdArgs)(fwd=fwd, grad_out=gout.data_ptr(), g_h=g_h.data_ptr())
    garr = _lib.ptr_array(g_mats)
    if nz.identity is None:
        args.g_adj = garr
    else:
        args.g_trans = garr
    g_identity, keep = fill(nz, args, stats)
    with _lib.on_device(nz.dev):
        _launch(name, args, what)
    g_h0 = None
    if ctx.needs_input_grad[0]:
        g_h0 = (g_h if nz.h0_bs else g_h.sum(0, dtype=torch.float32).to(torch.bfloat16) if nz.b16 else g_h.sum(0)).view(nz.h0_shape)
    return g_h0, g_identity, tuple(g.view(sh) if g is not None else None for g, sh in zip(g_mats, nz.mat_shapes))


class _Propagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h0, act, head, tail, *adjs):
        _lib.require_gpu(h0, head, tail, *adjs, dtype=torch.float32, **_ONE_DTYPE)
        return _forward_f32(ctx, _Call(h0, act, head, tail, adjs))

    @staticmethod
    def backward(ctx, gout):
        def fill(nz, args, stats):
            # wide states (the library sizes `wide_ws` for them alone): GP-GNN's block-structured gather indices let the chain of products run
            # on the forward's two-term f16 kernel (all hops in one launch); otherwise both products of a hop are batched fp32 GEMMs
            nws = _lib.lib().recon_propagate_bwd_ws_floats(C.byref(args.fwd))
            ws = chain = wide = None
            if nws and nz.dd == 16 and not nz.idx_bs and nz.h0.data_ptr() % 16 == 0 and all(a.data_ptr() % 16 == 0 for a in nz.mats):
                ws, chain = _chain_workspaces(nz, args)
            if nws and chain is None:
                wide = torch.empty(nws, dtype=torch.float32, device=nz.dev)
                args.wide_ws = wide.data_ptr()
            return None, (ws, chain, wide)
        g_h0, _, g_adjs = _backward(ctx, gout, 4, "recon_propagate_bwd", None, fill)
        return (g_h0, None, None, None) + g_adjs


_BLK_IDX = {}


def _index_blocks(head, tail, dd, S, align=8):
    """(head_blk, tail_blk) int32 [C] device tensors when the gather indices are blocks of dd consecutive columns — head[c, x] = head[c, 0] + x,
    likewise tail, every block inside [0, S], head and tail blocks of a channel distinct — shared by the batch; else None.  That is what
    utils/embedding_utils.py:184-202 builds; the bfloat16 backward then forms Y_l in its GEMM epilogues.  One host read per index tensor
    pair (cached on identity + version)."""
    key = (head.data_ptr(), head._version, tail.data_ptr(), tail._version, tuple(head.shape), int(dd), int(S), int(align))
    hit = _BLK_IDX.get(key)
    if hit is None:
        res = None
        if dd % 8 == 0 and (head.dim() == 2 or head.shape[0] == 1):
            h2, t2 = head.reshape(-1, dd), tail.reshape(-1, dd)
            ar = torch.arange(dd, device=head.device)
            ok = ((h2 == h2[:, :1] + ar).all() & (t2 == t2[:, :1] + ar).all() & (h2[:, 0] % align == 0).all() & (t2[:, 0] % align == 0).all()
                  & (h2[:, 0] >= 0).all() & (t2[:, 0] >= 0).all() & (h2[:, 0] + dd <= S).all() & (t2[:, 0] + dd <= S).all()
                  & ((h2[:, 0] - t2[:, 0]).abs() >= dd).all())
            if bool(ok):
                res = (h2[:, 0].to(torch.int32).contiguous(), t2[:, 0].to(torch.int32).contiguous())
        if len(_BLK_IDX) >= 16:
            _BLK_IDX.clear()
        hit = _BLK_IDX[key] = (res, head, tail)                         # pins the tensors while cached
    return hit[0]


def _fill_b16(nz, args):
    """Both bfloat16 backwards: the second [B, C, S] buffer the products alternate with, and the index blocks where the batch shares them."""
    ws = nz.new(nz.B, nz.Cn, nz.S)
    args.ws = ws.data_ptr()
    blk = _index_blocks(nz.head, nz.tail, nz.dd, nz.S) if nz.idx_bs == 0 else None
    if blk:
        args.head_blk, args.tail_blk = blk[0].data_ptr(), blk[1].data_ptr()
    return ws, blk


def _forward_b16(ctx, nz, want_states=False, what=None):
    """The bfloat16 forward (ctx None: inference outside autograd).  It stores the states H^1 .. H^L where the backward, the caller or the
    library's GEMM form (2: its products go through them) wants them."""
    need = ctx is not None and any(ctx.needs_input_grad)
    out = nz.new_out()
    args = nz.args(out)
    hs = nz.new_states() if need or want_states or _lib.lib().recon_propagate_b16_form(C.byref(args)) == 2 else None
    args.h_saved = _lib.ptr(hs)
    with _lib.on_device(nz.dev):
        _launch("recon_propagate_b16_fwd", args, what)
    if need:
        nz.save(ctx, hs, None)
    if want_states:                                                       # the states [L, B, C, S] as the forward stored them (no gradient)
        ctx.mark_non_differentiable(hs)
        return out, hs
    return out


class _PropagateB16(torch.autograd.Function):
    """models/models.py:260-274 on bfloat16 tensors (csrc/prop_b16.hip): bf16 storage, fp32 accumulation, every state rounded to bf16 once
    per hop, gradients in bf16."""

    @staticmethod
    def forward(ctx, h0, act, head, tail, want_states, *adjs):
        _lib.require_gpu(h0, head, tail, *adjs, dtype=torch.bfloat16, **_ONE_DTYPE)
        return _forward_b16(ctx, _Call(h0, act, head, tail, adjs), want_states)

    @staticmethod
    def backward(ctx, gout, *_unused):
        g_h0, _, g_adjs = _backward(ctx, gout, 5, "recon_propagate_b16_bwd", None, lambda nz, args, stats: (None, _fill_b16(nz, args)))
        return (g_h0, None, None, None, None) + g_adjs


def _propagate_b16(adj_list, h0, nonlinearity, head_indices, tail_indices, return_states=False):
    B, S = adj_list[0].shape[0], adj_list[0].shape[-1]
    Cn = h0.shape[1] if h0.dim() == 4 else h0.shape[0]
    probe = _Call.probe(True, B, Cn, S, len(adj_list), head_indices.shape[-1])
    aligned = all(a.data_ptr() % 16 == 0 for a in adj_list) and h0.data_ptr() % 16 == 0
    if not aligned or _lib.lib().recon_propagate_b16_form(C.byref(probe)) == 0:
        # shapes the bf16 kernels do not take (S % 8 != 0): bf16 storage around the float32 kernels
        out = _Propagate.apply(h0.float(), nonlinearity, head_indices, tail_indices, *[a.float() for a in adj_list])
        return out.to(torch.bfloat16)
    return _PropagateB16.apply(h0, nonlinearity, head_indices, tail_indices, bool(return_states), *adj_list)


def propagate(adj_list, h0, nonlinearity, head_indices, tail_indices, return_states=False):
    """models/models.py:260-274.  adj_list: L tensors [B,S,S] (or [B,1,S,S] as the reference views them);
    h0 [C,S,1] shared (GPGNN) or [B,C,S,1] per batch (RECON*); nonlinearity 'relu' | 'tanh' | 'linear'
    (model_params.json "non-linear1"); head/tail_indices int64 [C,2d] or [bs,C,2d] as the reference
    stores them.  Returns cat(relation_1..L, -1): [B, C, 2d*L].
    return_states (bfloat16 kernels, one launch's worth of graphs): also the states H^1 .. H^L [L, B, C, S] as the forward rounded and
    stored them — what its backward takes the activation's derivative from (the parity tests compare gradients on exactly these)."""
    if nonlinearity not in _lib.ACT:
        raise NotImplementedError(nonlinearity)
    B = adj_list[0].shape[0] if adj_list else 0
    if return_states:
        if _float_dtype(h0, *adj_list) != torch.bfloat16 or B > _lib.MAX_BATCH:
            raise NotImplementedError("return_states: bfloat16 tensors, at most %d graphs" % _lib.MAX_BATCH)
        res = _propagate_b16(adj_list, h0, nonlinearity, head_indices, tail_indices, return_states=True)
        return res if isinstance(res, tuple) else (res, None)          # None: the shape ran on the float32 kernels behind casts (no bf16 states)
    one = _propagate_b16 if _float_dtype(h0, *adj_list) == torch.bfloat16 else (lambda adjs, h, act, hi, ti: _Propagate.apply(h, act, hi, ti, *adjs))
    if B > _lib.MAX_BATCH:                    # the kernels index graphs with a 16-bit grid dimension; graphs are independent: run slices
        outs = []
        for b0 in range(0, B, _lib.MAX_BATCH):
            sl = slice(b0, min(B, b0 + _lib.MAX_BATCH))
            hs = h0[sl] if h0.dim() == 4 else h0
            hi = head_indices[sl] if head_indices.dim() == 3 and head_indices.shape[0] == B else head_indices
            ti = tail_indices[sl] if tail_indices.dim() == 3 and tail_indices.shape[0] == B else tail_indices
            outs.append(one([a[sl] for a in adj_list], hs, nonlinearity, hi, ti))
        return torch.cat(outs, dim=0)
    return one(adj_list, h0, nonlinearity, head_indices, tail_indices)


class _PropagateBlocks(torch.autograd.Function):
    """Block adjacency + propagation in one pass (models/models.py:240-274 as the reference inlines it): the kernels read
    A_l[b, i*2d+r, j*2d+c] = T_l[b, e(i,j), r, c] (identity on the diagonal) in place, so A_l is never written or read, and the
    backward writes d loss / d T_l in T's own layout and sums the diagonal blocks into d loss / d identity."""

    @staticmethod
    def forward(ctx, h0, identity, act, head, tail, n, *Ts):
        _lib.require_gpu(h0, identity, head, tail, *Ts, dtype=torch.float32, **_ONE_DTYPE)
        return _forward_f32(ctx, _Call(h0, act, head, tail, Ts, identity, n), "recon_propagate_fwd (block mode)")

    @staticmethod
    def backward(ctx, gout):
        def fill(nz, args, stats):
            g_I = nz.new(nz.dd, nz.dd) if ctx.needs_input_grad[1] else None
            args.g_identity = _lib.ptr(g_I)
            if stats is None:
                # the forward asked recon_propagate_form and took no stats: the two-term form of csrc/prop_h.hip does not exist for these
                # states, and block mode's other backward is the wide-state chain + d T products of csrc/prop_hl.hip (csrc/prop.hip: plan_bwd;
                # block-structured indices: propagate_blocks checked)
                return g_I, _chain_workspaces(nz, args)
            ws = nz.new(_lib.lib().recon_propagate_identity_ws_floats(nz.dd)) if g_I is not None else None
            args.identity_ws = _lib.ptr(ws)
            return g_I, ws
        g_h0, g_I, g_Ts = _backward(ctx, gout, 6, "recon_propagate_bwd", "recon_propagate_bwd (block mode)", fill)
        return (g_h0, g_I, None, None, None, None) + g_Ts


def _blocks_gate(B, n, dd, max_n=None):
    """What every block-mode form asks of the sizes: 2d = 16, 2 <= n (<= max_n), one launch's worth of graphs.  RECON_PROP_BLOCKS=0, read at
    every call, sends every call through the adjacency."""
    return (dd == 16 and n >= 2 and (max_n is None or n <= max_n) and 0 < B <= _lib.MAX_BATCH
            and os.environ.get("RECON_PROP_BLOCKS", "1") != "0")


def _blocks_wide_trainable(B, n, dd, h0, L, head, tail):
    """Wide states (10 < n <= 32) with gradients in float32: the forward reads the transition tensors in place (csrc/prop_hl.hip) and the
    backward's chain / d T products run on its mirror images — for GP-GNN's block-structured gather indices shared by the batch.  The
    library says whether: the split workspace and the chain workspace exist for exactly these shapes."""
    if head.dim() == 3 and head.shape[0] > 1:
        return False
    Cn, S = n * (n - 1), n * dd
    probe = _Call.probe(False, B, Cn, S, max(1, int(L)), dd, h0, wide_blocks=True)
    if not (probe.split_ws and _lib.lib().recon_propagate_bwd_chain_ws_floats(C.byref(probe)) > 0):
        return False
    return _index_blocks(head.contiguous(), tail.contiguous(), dd, S, align=16) is not None


def blocks_mode_available(B, n, dd, h0, need_grad=True, L=1, T_list=None):
    """Whether propagate_blocks() runs fused (two-term f16 kernels for the forward and, when gradients are wanted, for the backward:
    2d = 16, n <= 9; forward only — inference — for 10 <= n <= 32; B within one launch).  `L` (hops) and `T_list` (the transition tensors:
    16-byte alignment) make the probe exact: the wide form's LDS budget grows with the hop count."""
    if not _blocks_gate(B, n, dd, 32):
        return False
    if T_list is not None and any(t.data_ptr() % 16 for t in T_list):
        return False
    probe = _Call.probe(False, B, n * (n - 1), n * dd, max(1, int(L)), dd, h0)
    form = _lib.lib().recon_propagate_form(C.byref(probe))
    if form:            # the state fits a workgroup's LDS; bit 1: the backward's two-term form exists too
        return form == 3 or not need_grad
    # wide states: the forward-only form of csrc/prop_hl.hip reads the transition tensors in place too, where its split workspace exists
    return (not need_grad) and h0.data_ptr() % 16 == 0 and _lib.lib().recon_propagate_ws_bytes(C.byref(probe)) > 0


# csrc/prop_b16.hip, bwd_b16_check: `8ull * a->S * sizeof(float) > 64 * 1024` is unsupported (its row kernel keeps 8 rows of S floats in LDS).
# No query answers it without the call's pointers, so the host states it, here alone.
_B16_BWD_MAX_S = 64 * 1024 // (8 * 4)


def _blocks_b16_available(B, n, dd, h0, T_list, identity, need_grad):
    """Block mode on bfloat16 tensors.  Inference: the kernels with the state in LDS (forms 1 and 3), n <= 32, contiguous transition
    tensors.  With gradients: any form the bfloat16 kernels take (S = 16 n: always a multiple of 8), states the backward's row kernel holds."""
    if not _blocks_gate(B, n, dd, None if need_grad else 32):
        return False
    if h0.data_ptr() % 16 or identity.data_ptr() % 16 or any(T.data_ptr() % 16 or not (need_grad or T.is_contiguous()) for T in T_list):
        return False
    form = _lib.lib().recon_propagate_b16_form(C.byref(_Call.probe(True, B, n * (n - 1), n * dd, len(T_list), dd)))
    return (form != 0 and n * dd <= _B16_BWD_MAX_S) if need_grad else form in (1, 3)


def _propagate_blocks_b16(T_list, identity, n, h0, act, head, tail):
    """Inference: block adjacency + propagation in one launch on bfloat16 tensors; A_l is never written."""
    _lib.require_gpu(h0, identity, head, tail, *T_list, dtype=torch.bfloat16, **_ONE_DTYPE)
    return _forward_b16(None, _Call(h0, act, head, tail, T_list, identity, n), what="recon_propagate_b16_fwd (block mode)")


class _PropagateBlocksB16(torch.autograd.Function):
    """models/models.py:240-274 on bfloat16 tensors WITH gradients and without an adjacency: the forward reads the transition tensors in
    place (and saves the states), the backward's products read them in place again, write d T_l in T's layout and sum the diagonal
    blocks of every hop into d identity (fp32, fixed order, rounded once)."""

    @staticmethod
    def forward(ctx, h0, identity, act, head, tail, n, want_states, *Ts):
        _lib.require_gpu(h0, identity, head, tail, *Ts, dtype=torch.bfloat16, **_ONE_DTYPE)
        return _forward_b16(ctx, _Call(h0, act, head, tail, Ts, identity, n), want_states, "recon_propagate_b16_fwd (block mode)")

    @staticmethod
    def backward(ctx, gout, *_unused):
        def fill(nz, args, stats):
            g_I = diag = iws = None
            if ctx.needs_input_grad[1]:
                Lb = _lib.lib()
                g_I = nz.new(nz.dd, nz.dd)
                diag = nz.new(Lb.recon_propagate_b16_bwd_diag_elems(C.byref(args.fwd)))
                iws = torch.empty(Lb.recon_block_adjacency_b16_bwd_workspace_floats(nz.dd), dtype=torch.float32, device=nz.dev)
                args.g_identity, args.diag_ws, args.ident_ws = g_I.data_ptr(), diag.data_ptr(), iws.data_ptr()
            return g_I, (diag, iws, _fill_b16(nz, args))
        g_h0, g_I, g_Ts = _backward(ctx, gout, 7, "recon_propagate_b16_bwd", "recon_propagate_b16_bwd (block mode)", fill)
        return (g_h0, g_I, None, None, None, None, None) + g_Ts


def propagate_blocks(T_list, identity, n, h0, nonlinearity, head_indices, tail_indices, return_states=False):
    """models/models.py:240-274 in one call: T_list = L transition tensors [B, n(n-1), (2d)^2] (or [B, n-1, n, (2d)^2]) AFTER their
    non-linearity, identity [2d, 2d]; equivalent to
        propagate([build_block_adjacency(T, identity, n) for T in T_list], h0, nonlinearity, head_indices, tail_indices)
    and computed exactly like that wherever the fused kernels do not apply (2d != 16, n > 32, shapes the library has no in-place form for, batches above one launch)."""
    if nonlinearity not in _lib.ACT:
        raise NotImplementedError(nonlinearity)
    B, dd, L = T_list[0].shape[0], identity.shape[0], len(T_list)
    need_grad = torch.is_grad_enabled() and (identity.requires_grad or h0.requires_grad or any(T.requires_grad for T in T_list))
    if _float_dtype(h0, identity, *T_list) == torch.bfloat16:
        # bfloat16: the kernels read the transition tensors in place (csrc/prop_b16.hip, block mode) — inference through the fused forms,
        # training through _PropagateBlocksB16 (no adjacency is materialised in either direction); other shapes: block adjacency + propagate
        if _blocks_b16_available(B, n, dd, h0, T_list, identity, need_grad):
            if need_grad:
                return _PropagateBlocksB16.apply(h0, identity, nonlinearity, head_indices, tail_indices, n, bool(return_states), *T_list)
            return _propagate_blocks_b16(T_list, identity, n, h0, nonlinearity, head_indices, tail_indices)
        if return_states:
            raise NotImplementedError("return_states: the bfloat16 training form only")
        return propagate([build_block_adjacency(T, identity, n) for T in T_list], h0, nonlinearity, head_indices, tail_indices)
    if return_states:
        raise NotImplementedError("return_states: bfloat16 tensors only")
    ok = blocks_mode_available(B, n, dd, h0, need_grad, L=L, T_list=T_list)
    if not ok and need_grad:                # no state-in-LDS backward: the wide-state forms, where the library has them for these shapes
        ok = (blocks_mode_available(B, n, dd, h0, False, L=L, T_list=T_list) and identity.data_ptr() % 16 == 0 and
              _blocks_wide_trainable(B, n, dd, h0, L, head_indices, tail_indices))
    if not ok:
        return propagate([build_block_adjacency(T, identity, n) for T in T_list], h0, nonlinearity, head_indices, tail_indices)
    return _PropagateBlocks.apply(h0, identity, nonlinearity, head_indices, tail_indices, n, *T_list)


# ------------------------------------------------------------------------------- P4
def make_start_entity_embeddings(entity_embeddings, entity_pos_indices, unique_entities, embedding_dim,
                                 max_occurred_entity_in_batch_pos, start_embedding_template, max_num_nodes=9):
    """utils/context_utils.py:387-426, same argument list (unique_entities and the most-frequent-entity
    hint only steer a speed trick there and do not change the result).  Returns [B, C, 2dn, 1].
    Forward and backward are kernels; the gradient of `entity_embeddings` is a fixed-order segment sum (bitwise run-to-run)."""
    _lib.require_gpu(entity_embeddings, start_embedding_template, dtype=torch.float32, **_ONE_DTYPE)
    n, d = max_num_nodes, embedding_dim
    B, Cn = entity_pos_indices.shape[:2]
    S = 2 * d * n
    pos = entity_pos_indices.to(device=entity_embeddings.device, dtype=torch.int64).contiguous()
    return _StartEntity.apply(entity_embeddings, pos, start_embedding_template.contiguous().view(Cn, S), B, n, d)


class _StartEntity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ent, pos, templ, B, n, d):
        ent = ent.contiguous()
        Cn, S = n * (n - 1), 2 * d * n
        out = torch.empty(B, Cn, S, 1, dtype=torch.float32, device=ent.device)
        with _lib.on_device(ent.device):
            _lib.check(_lib.lib().recon_start_entity_embeddings(ent.data_ptr(), pos.data_ptr(), templ.data_ptr(), B, n, d,
                                                                out.data_ptr(), _lib.current_stream()),
                       "recon_start_entity_embeddings")
        ctx.save_for_backward(pos, templ)
        ctx.dims = (B, n, d, ent.shape[0])
        return out

    @staticmethod
    def backward(ctx, g):
        """Fixed summation order, no torch op: one kernel cuts the two d-wide pieces per (b, c) out of g * templ, the
        SpecialSpmmFinal walk (csrc/gat.hip: k_rowsum_walk / _fix over a destination-only CSR keyed on the entity ids) adds the rows of
        each entity in slot order.  The segment key — and with it the CSR, through prepare_graph's cache — is kept per position tensor."""
        from .gat_layers import _rowsum_keyed
        pos, templ = ctx.saved_tensors
        B, n, d, U = ctx.dims
        Cn = n * (n - 1)
        dev = g.device
        g = g.contiguous()
        if g.dtype != torch.float32:
            g = g.float()
        rows = torch.empty(2 * B * Cn, d, dtype=torch.float32, device=dev)
        ck = (pos.data_ptr(), pos._version, tuple(pos.shape), str(dev))
        hit = _P4_KEYS.get(ck)
        key = None if hit is not None else torch.empty(2, 2 * B * Cn, dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.lib().recon_start_entity_embeddings_bwd(g.data_ptr(), pos.data_ptr(), templ.data_ptr(), B, n, d, rows.data_ptr(),
                                                                    _lib.ptr(key), _lib.current_stream()), "recon_start_entity_embeddings_bwd")
        if hit is None:
            if len(_P4_KEYS) >= 4:
                _P4_KEYS.pop(next(iter(_P4_KEYS)))
            hit = _P4_KEYS[ck] = (key, pos)                               # `pos` pins data_ptr identity while cached
        return _rowsum_keyed(rows, hit[0], U), None, None, None, None, None


_P4_KEYS = {}
