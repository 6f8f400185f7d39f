"""The pair states' transition projections (models/models.py:185-192 tied, :240-249 untied; the same lines of RECON_EAC :395-402 / :450-459,
RECON_EAC_KGGAT :605-612 / :660-669 and RECON :843-850 / :898-907) as one device op:

    from recon_amd import pair_transitions
    Ts = pair_transitions(x, weights, biases, nonlinearity)        # tuple of L tensors [..., N1]
    Ts[l] = act(x W_l^T + b_l)

x [..., K] (read in place where `_lib.rows_in_place` allows), weights a sequence of L >= 1 tensors [N1, K] of one shape, biases a sequence
of L entries, each [N1] or None, nonlinearity a string as in model_params.json ("relu", "tanh", "linear", or any other name of
torch.nn.functional).  With fp32 GPU tensors, a nonlinearity in `_lib.ACT` and a shape `recon_pair_transitions_supported` takes, the
kernels of csrc/pair_trans.hip run: one launch forward, three backward (d_x; the weight and bias gradients over row groups; their sum in
group order), all fp32 on the fp32 MFMA, bitwise reproducible.  The outputs are the only saved activations: act' is taken from them and
g_T act'(T) is formed while an operand is staged.  The backward destroys nothing, so a second backward over a retained graph runs the
kernels again and gives the same bits.  Differentiable in x, every W_l and every b_l.  Otherwise — CPU tensors, another dtype, another
nonlinearity, a shape or an alignment the library refuses, a backward under create_graph — the call runs `_chain`, the op sequence the
models are without it.  DESIGN.md section 22.
"""
import torch
import torch.nn.functional as F

from . import _lib

WGRAD_MAX_ROW_GROUPS = 8          # kPtMaxGroups of csrc/pair_trans.hip: the weight-gradient pass cuts the M rows into min(8, ceil(M / 32)) groups


def _chain(x, weights, biases, nonlinearity):
    """The stock sequence (models/models.py:185-192, :240-249): per layer F.linear, then the named function of torch.nn.functional."""
    outs = []
    for W, b in zip(weights, biases):
        T = F.linear(x, W, b)
        if nonlinearity != "linear":
            T = getattr(F, nonlinearity)(T)
        outs.append(T)
    return tuple(outs)


def _rows(x, K):
    """x as the kernels read it: [M, K] rows at one 4-element-aligned stride from a 16-byte aligned base (a copy where the view is not)."""
    flat = x if x.dim() in (2, 3) else x.reshape(-1, K)
    flat, ld = _lib.rows_in_place(flat, K)
    if ld % 4 or flat.data_ptr() % 16:
        flat, ld = flat.contiguous(), K
    return flat, ld


class _PairTransitions(torch.autograd.Function):
    """csrc/pair_trans.hip: saves references to x, the weights and biases, and the outputs — nothing else."""

    @staticmethod
    def forward(ctx, nonlinearity, wants, L, x, *params):
        lib = _lib.lib()
        weights, biases = params[:L], params[L:]
        N1, K = weights[0].shape
        xd, ld = _rows(x.detach(), K)
        M = x.numel() // K
        w = [q.detach() for q in weights]
        b = [None if q is None else q.detach() for q in biases]
        dev = x.device
        outs = [torch.empty(x.shape[:-1] + (N1,), dtype=torch.float32, device=dev) for _ in range(L)]
        pw, pb, po = _lib.ptr_array(w), _lib.ptr_array(b), _lib.ptr_array(outs)
        with _lib.on_device(dev):
            _lib.check(lib.recon_pair_transitions_fwd(xd.data_ptr(), ld, pw, pb, M, K, N1, L, _lib.ACT[nonlinearity], po, _lib.current_stream()),
                       "recon_pair_transitions_fwd")
        ctx.set_materialize_grads(False)
        if wants:
            ctx.save_for_backward(x, *outs, *weights, *[q for q in biases if q is not None])
            ctx.nonlinearity, ctx.L, ctx.has_bias = nonlinearity, L, [q is not None for q in biases]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_outs):
        L = ctx.L
        x, saved = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        outs, weights, rest = saved[:L], saved[L:2 * L], iter(saved[2 * L:])
        biases = [next(rest) if h else None for h in ctx.has_bias]
        need = ctx.needs_input_grad[3:]
        if all(g is None for g in g_outs) or not any(need):
            return (None,) * (3 + 1 + 2 * L)
        if torch.is_grad_enabled():                                      # create_graph: the gradient itself must be differentiable
            gs = [torch.zeros_like(o) if g is None else g for g, o in zip(g_outs, outs)]
            inputs = (x,) + tuple(weights) + tuple(biases)
            live = [n and t is not None for n, t in zip(need, inputs)]
            grads = _lib.recompute_grads(lambda: _chain(x, weights, biases, ctx.nonlinearity), [t for t in inputs if t is not None],
                                         [n for n, t in zip(live, inputs) if t is not None], gs, True)
            grads = iter(grads)
            return (None,) * 3 + tuple(None if t is None else next(grads) for t in inputs)
        lib = _lib.lib()
        N1, K = weights[0].shape
        M = x.numel() // K
        xd, ld = _rows(x.detach(), K)
        dev = x.device
        g = [None if q is None else q.contiguous().to(torch.float32) for q in g_outs]
        g_x = torch.empty(x.shape, dtype=torch.float32, device=dev) if need[0] else None
        g_w = [torch.empty_like(q) if n else None for q, n in zip(weights, need[1:1 + L])]
        g_b = [torch.empty_like(q) if (n and q is not None) else None for q, n in zip(biases, need[1 + L:])]
        params = any(q is not None for q in g_w + g_b)
        ws = _lib.workspace(lib.recon_pair_transitions_workspace_bytes(M, K, N1, L, 1) if params else 0, dev)
        w = [q.detach() for q in weights]
        o = [q.detach() for q in outs]
        pw, po, pg, pgw, pgb = _lib.ptr_array(w), _lib.ptr_array(o), _lib.ptr_array(g), _lib.ptr_array(g_w), _lib.ptr_array(g_b)
        with _lib.on_device(dev):
            _lib.check(lib.recon_pair_transitions_bwd(xd.data_ptr(), ld, pw, po, pg, M, K, N1, L, _lib.ACT[ctx.nonlinearity], _lib.ptr(g_x), pgw, pgb,
                                                      ws.data_ptr(), ws.numel(), _lib.current_stream()), "recon_pair_transitions_bwd")
        return (None, None, None, g_x) + tuple(g_w) + tuple(g_b)


def _fused(x, weights, biases, nonlinearity):
    tensors = [x] + list(weights) + [b for b in biases if b is not None]
    if not x.is_cuda or nonlinearity not in _lib.ACT or any(t.dtype != torch.float32 for t in tensors):
        return False
    if any(not t.is_contiguous() or t.data_ptr() % 16 for t in weights) or any(not b.is_contiguous() for b in biases if b is not None):
        return False
    N1, K = weights[0].shape
    if K == 0 or not _lib.lib().recon_pair_transitions_supported(x.numel() // K, K, N1, len(weights)):
        return False
    _, ld = _rows(x, K)
    return ld < 2 ** 31


def pair_transitions(x, weights, biases, nonlinearity):
    """[..., K], L x [N1, K], L x ([N1] or None), name -> tuple of L tensors [..., N1]: act(x W_l^T + b_l), differentiable in x, every W_l and
    every b_l (models/models.py:185-192, :240-249).  M = 0 rows give empty outputs without a launch."""
    if not isinstance(nonlinearity, str) or not (nonlinearity == "linear" or callable(getattr(F, nonlinearity, None))):
        raise ValueError("pair_transitions: nonlinearity must be \"linear\" or the name of a function of torch.nn.functional, got %r" % (nonlinearity,))
    if not torch.is_tensor(x) or x.dim() < 1 or not x.is_floating_point():
        raise ValueError("pair_transitions: x must be a floating-point [..., K] tensor, got %s %s"
                         % (getattr(x, "dtype", type(x).__name__), tuple(getattr(x, "shape", ()))))
    weights, biases = list(weights), list(biases)
    L, K = len(weights), x.shape[-1]
    if L < 1 or len(biases) != L:
        raise ValueError("pair_transitions: needs L >= 1 weights and as many biases (None for none), got %d and %d" % (L, len(biases)))
    shapes = [tuple(getattr(W, "shape", ())) for W in weights]
    if any(not torch.is_tensor(W) or W.dim() != 2 or W.shape != weights[0].shape or W.shape[1] != K or W.dtype != x.dtype for W in weights):
        raise ValueError("pair_transitions: the weights must be L tensors [N1, K] = [N1, %d] of one shape and of x's dtype %s, got %s %s"
                         % (K, x.dtype, [getattr(W, "dtype", None) for W in weights], shapes))
    N1 = weights[0].shape[0]
    if any(b is not None and (not torch.is_tensor(b) or tuple(b.shape) != (N1,) or b.dtype != x.dtype) for b in biases):
        raise ValueError("pair_transitions: every bias must be None or [N1] = [%d] of x's dtype %s, got %s"
                         % (N1, x.dtype, [None if b is None else (getattr(b, "dtype", None), tuple(getattr(b, "shape", ()))) for b in biases]))
    if any(t.device != x.device for t in weights + [b for b in biases if b is not None]):
        raise ValueError("pair_transitions: the tensors must be on one device")
    if _fused(x, weights, biases, nonlinearity):
        # (inside the function grad mode is off and needs_input_grad ignores no_grad: whether a backward can follow is decided here)
        wants = torch.is_grad_enabled() and any(t.requires_grad for t in [x] + weights + [b for b in biases if b is not None])
        return _PairTransitions.apply(nonlinearity, wants, L, x, *weights, *biases)
    return _chain(x, weights, biases, nonlinearity)
