"""The relation classifier over its feature blocks (models/models.py:213, :234, :275 GPGNN and RECON_EAC; :693-697 RECON_EAC_KGGAT;
:954-966 RECON) as one device op:

    from recon_amd import relation_logits
    logits = relation_logits(blocks, weight, bias=None, scattered=None, positions=None)      # [..., N]
    logits = cat(blocks..., scatter(scattered, positions)) weight^T + bias

blocks: a sequence of 1 to 4 tensors [..., K_i] with one leading shape of M rows, read in place where `_lib.rows_in_place` allows.
scattered [Mnz, K_s] and positions [Mnz] (both or neither) stand for one more column block behind the others: its row positions[i] is
scattered[i], every other row is zero (the `zeros` + `index_put` of models/models.py:954-958).  positions is integer, STRICTLY INCREASING
and inside [0, M), which is how utils/context_utils.py:455-475 builds it; given as a list or a numpy array (or a CPU tensor) it is checked
here, a device tensor is trusted (no sync) and a position outside [0, M) is ignored by the kernels, never used as an address.  Mnz = 0
is an all-zero block.  weight [N, sum K_i + K_s], bias [N] or None.

With fp32 GPU tensors and a shape `recon_relation_logits_supported` takes, the kernels of csrc/rel_head.hip run: one launch forward, up to
three backward (the gradients of the blocks that want one, the scattered block's for its present rows alone; the weight and bias gradients
over row groups; their sum in group order), all fp32 on the fp32 MFMA, bitwise reproducible; neither the scattered block nor the
concatenation is ever written.  A block that does not require a gradient gets none and costs nothing.  The op saves references to its
inputs and nothing else, and its backward destroys nothing: a second backward over a retained graph runs the kernels again and gives the
same bits.  Otherwise — CPU tensors, another dtype, a shape the library refuses, a backward under create_graph — the call runs `_chain`,
the op sequence the models are without it.  DESIGN.md section 23.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

WGRAD_MAX_ROW_GROUPS = 8          # kRhMaxGroups of csrc/rel_head.hip: the weight-gradient pass cuts the M rows into min(8, ceil(M / 32)) groups
MAX_DENSE_BLOCKS = 4              # kRhMaxDense


def _chain(blocks, weight, bias=None, scattered=None, positions=None):
    """The stock sequence (models/models.py:693-697, :954-966): `zeros`, `index_put`, `cat`, `F.linear`."""
    parts = list(blocks)
    if scattered is not None:
        lead = parts[0].shape[:-1]
        block = torch.zeros(parts[0].numel() // parts[0].shape[-1], scattered.shape[-1], device=parts[0].device, dtype=parts[0].dtype)
        if scattered.shape[0] > 0:
            block = block.index_put((positions,), scattered)
        parts.append(block.view(lead + (scattered.shape[-1],)))
    return F.linear(torch.cat(parts, dim=-1) if len(parts) > 1 else parts[0], weight, bias)


def _rows(x, K):
    """x as the kernels read it: [M, K] rows at one stride (a copy where the view has none); the kernels need no alignment."""
    flat = x if x.dim() in (2, 3) else x.reshape(-1, K)
    return _lib.rows_in_place(flat, K)


def _c_array(ctype, values):
    return (ctype * len(values))(*values)


def _operands(blocks, scattered, positions):
    """The C arguments that describe the blocks: (kept tensors, pointer / stride / width arrays, scattered pointer, ld_s, K_s, positions
    pointer, Mnz)."""
    import ctypes as C
    rows = [_rows(b.detach(), b.shape[-1]) for b in blocks]
    keep = [r[0] for r in rows]
    if scattered is not None:
        s, ld_s = _rows(scattered.detach(), scattered.shape[-1])
        pos = positions if positions.dtype == torch.int64 and positions.is_contiguous() else positions.to(torch.int64).contiguous()
        keep += [s, pos]
        tail = (s.data_ptr(), ld_s, scattered.shape[-1], pos.data_ptr(), scattered.shape[0])
    else:
        tail = (None, 0, 0, None, 0)
    return (keep, _lib.ptr_array([r[0] for r in rows]), _c_array(C.c_int64, [r[1] for r in rows]),
            _c_array(C.c_int32, [b.shape[-1] for b in blocks])) + tail


class _RelationLogits(torch.autograd.Function):
    """csrc/rel_head.hip: saves references to its inputs (the blocks, the weight, the bias, scattered, positions) — nothing else."""

    @staticmethod
    def forward(ctx, wants, nb, *tensors):
        lib = _lib.lib()
        blocks, (weight, bias, scattered, positions) = tensors[:nb], tensors[nb:]
        N = weight.shape[0]
        M = blocks[0].numel() // blocks[0].shape[-1]
        dev = weight.device
        keep, pb, lds, widths, ps, ld_s, K_s, ppos, Mnz = _operands(blocks, scattered, positions)
        out = torch.empty(blocks[0].shape[:-1] + (N,), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(lib.recon_relation_logits_fwd(pb, lds, widths, nb, ps, ld_s, K_s, ppos, Mnz, weight.detach().data_ptr(),
                                                     None if bias is None else bias.detach().data_ptr(), M, N, out.data_ptr(),
                                                     _lib.current_stream()), "recon_relation_logits_fwd")
        del keep
        ctx.set_materialize_grads(False)
        if wants:
            ctx.save_for_backward(*[t for t in tensors if t is not None])
            ctx.nb, ctx.present = nb, [t is not None for t in tensors]
        return out

    @staticmethod
    def backward(ctx, g_out):
        nb = ctx.nb
        saved = iter(ctx.saved_tensors)
        tensors = [next(saved) if h else None for h in ctx.present]
        blocks, (weight, bias, scattered, positions) = tensors[:nb], tensors[nb:]
        need = list(ctx.needs_input_grad[2:])
        none = (None,) * (2 + len(tensors))
        if g_out is None or not any(need):
            return none
        if torch.is_grad_enabled():                                      # create_graph: the gradient itself must be differentiable
            inputs = [t for t in tensors[:nb + 3] if t is not None]
            live = [n for n, t in zip(need, tensors[:nb + 3]) if t is not None]
            grads = iter(_lib.recompute_grads(lambda: _chain(blocks, weight, bias, scattered, positions), inputs, live, g_out, True))
            return (None, None) + tuple(None if t is None else next(grads) for t in tensors[:nb + 3]) + (None,)
        lib = _lib.lib()
        N, Kt = weight.shape
        M = blocks[0].numel() // blocks[0].shape[-1]
        dev = weight.device
        keep, pb, lds, widths, ps, ld_s, K_s, ppos, Mnz = _operands(blocks, scattered, positions)
        g = g_out.to(torch.float32).contiguous()
        g_blocks = [torch.empty(b.shape, dtype=torch.float32, device=dev) if n else None for b, n in zip(blocks, need[:nb])]
        g_w = torch.empty_like(weight) if need[nb] else None
        g_b = torch.empty_like(bias) if (bias is not None and need[nb + 1]) else None
        # (an empty scattered block takes no part in the product: no gradient, as the stock lines give none)
        g_s = torch.empty(scattered.shape, dtype=torch.float32, device=dev) if (scattered is not None and need[nb + 2] and Mnz) else None
        params = g_w is not None or g_b is not None
        ws = _lib.workspace(lib.recon_relation_logits_workspace_bytes(M, nb, Kt, N, 1) if params else 0, dev)
        with _lib.on_device(dev):
            _lib.check(lib.recon_relation_logits_bwd(pb, lds, widths, nb, ps, ld_s, K_s, ppos, Mnz, weight.detach().data_ptr(), g.data_ptr(), M, N,
                                                     _lib.ptr_array(g_blocks), _lib.ptr(g_s), _lib.ptr(g_w), _lib.ptr(g_b), ws.data_ptr(), ws.numel(),
                                                     _lib.current_stream()), "recon_relation_logits_bwd")
        del keep
        return (None, None) + tuple(g_blocks) + (g_w, g_b, g_s, None)


def _fused(blocks, weight, bias, scattered, positions):
    tensors = list(blocks) + [weight] + [t for t in (bias, scattered) if t is not None]
    if not weight.is_cuda or any(t.dtype != torch.float32 for t in tensors):
        return False
    if not weight.is_contiguous() or (bias is not None and not bias.is_contiguous()):
        return False
    N, Kt = weight.shape
    M = blocks[0].numel() // blocks[0].shape[-1]
    return len(blocks) <= MAX_DENSE_BLOCKS and bool(_lib.lib().recon_relation_logits_supported(M, len(blocks), Kt, N))


def _shape(t):
    return tuple(getattr(t, "shape", ())) if torch.is_tensor(t) else type(t).__name__


def _host_positions(positions, M, Mnz, device):
    """A list, a numpy array or a CPU tensor, checked where the check is free: integer, [Mnz], strictly increasing, inside [0, M)."""
    p = positions.detach().numpy() if torch.is_tensor(positions) else np.asarray(positions)
    if p.size == 0:
        p = p.reshape(0).astype(np.int64)
    if p.ndim != 1 or not np.issubdtype(p.dtype, np.integer) or p.shape[0] != Mnz:
        raise ValueError("relation_logits: positions must be %d integers, one per row of scattered, got %s %s" % (Mnz, p.dtype, p.shape))
    p = p.astype(np.int64)
    if Mnz and (p[0] < 0 or p[-1] >= M or (np.diff(p) <= 0).any()):
        raise ValueError("relation_logits: positions must be strictly increasing and inside [0, M) = [0, %d), got %s%s"
                         % (M, p[:8].tolist(), " ..." if Mnz > 8 else ""))
    return positions.to(device) if torch.is_tensor(positions) else torch.from_numpy(p).to(device)


def relation_logits(blocks, weight, bias=None, scattered=None, positions=None):
    """1..4 x [..., K_i], [N, sum K_i + K_s], [N] or None, [Mnz, K_s] and [Mnz] or neither -> [..., N]: cat(blocks..., S) weight^T + bias
    with S zero but for its rows positions[i] = scattered[i] (models/models.py:693-697, :954-966), differentiable in every block that
    requires a gradient, in scattered, weight and bias.  M = 0 rows give an empty result without a launch."""
    blocks = [blocks] if torch.is_tensor(blocks) else list(blocks)
    shapes = [_shape(b) for b in blocks]
    if not 1 <= len(blocks) <= MAX_DENSE_BLOCKS or any(not torch.is_tensor(b) or b.dim() < 1 or not b.is_floating_point() or b.shape[-1] < 1
                                                       for b in blocks):
        raise ValueError("relation_logits: blocks must be 1 to %d floating-point tensors [..., K_i], K_i >= 1, got %s" % (MAX_DENSE_BLOCKS, shapes))
    x = blocks[0]
    if any(b.shape[:-1] != x.shape[:-1] or b.dtype != x.dtype for b in blocks):
        raise ValueError("relation_logits: the blocks must share one leading shape and one dtype, got %s %s" % ([b.dtype for b in blocks], shapes))
    M = x.numel() // x.shape[-1]
    if (scattered is None) != (positions is None):
        raise ValueError("relation_logits: scattered and positions are given together or not at all, got scattered %s and positions %s"
                         % (_shape(scattered), _shape(positions)))
    K_s = 0
    if scattered is not None:
        if not torch.is_tensor(scattered) or scattered.dim() != 2 or scattered.shape[1] < 1 or scattered.dtype != x.dtype:
            raise ValueError("relation_logits: scattered must be [Mnz, K_s], K_s >= 1, of the blocks' dtype %s, got %s %s"
                             % (x.dtype, getattr(scattered, "dtype", None), _shape(scattered)))
        Mnz, K_s = scattered.shape
        if torch.is_tensor(positions) and positions.is_cuda:
            if positions.dim() != 1 or positions.shape[0] != Mnz or positions.is_floating_point() or positions.dtype == torch.bool:
                raise ValueError("relation_logits: positions must be %d integers, one per row of scattered %s, got %s %s"
                                 % (Mnz, _shape(scattered), positions.dtype, _shape(positions)))
        else:
            positions = _host_positions(positions, M, Mnz, x.device)
    Kt = sum(b.shape[-1] for b in blocks) + K_s
    if not torch.is_tensor(weight) or weight.dim() != 2 or weight.shape[1] != Kt or weight.dtype != x.dtype:
        raise ValueError("relation_logits: weight must be [N, %d] (the blocks' widths %s%s added up) of the blocks' dtype %s, got %s %s"
                         % (Kt, [b.shape[-1] for b in blocks], " + %d scattered" % K_s if K_s else "", x.dtype, getattr(weight, "dtype", None),
                            _shape(weight)))
    N = weight.shape[0]
    if bias is not None and (not torch.is_tensor(bias) or tuple(bias.shape) != (N,) or bias.dtype != x.dtype):
        raise ValueError("relation_logits: bias must be None or [N] = [%d] of the blocks' dtype %s, got %s %s"
                         % (N, x.dtype, getattr(bias, "dtype", None), _shape(bias)))
    if any(t.device != x.device for t in blocks + [weight] + [t for t in (bias, scattered, positions) if t is not None]):
        raise ValueError("relation_logits: the tensors must be on one device")
    if _fused(blocks, weight, bias, scattered, positions):
        # (inside the function grad mode is off and needs_input_grad ignores no_grad: whether a backward can follow is decided here)
        wants = torch.is_grad_enabled() and any(t.requires_grad for t in blocks + [weight] + [t for t in (bias, scattered) if t is not None])
        return _RelationLogits.apply(wants, len(blocks), *blocks, weight, bias, scattered, positions)
    return _chain(blocks, weight, bias, scattered, positions)
