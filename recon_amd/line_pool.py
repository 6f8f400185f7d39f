"""The entity-level tail of the entity-context encoder (models/models.py:73-81: `conv1d_entity` over the line states, the line mask, the
max over the lines) as one device op:

    from recon_amd import entity_line_pool
    out = entity_line_pool(states, weight, bias, mask)                 # [U, E]
    out[u, e] = max over unmasked p of  bias[e] + sum_{j < k} sum_c weight[e, c, j] states[u, p + j, c]

states [U, Ln, C] (read in place where `_lib.rows_in_place` allows), weight [E, C, k] in nn.Conv1d's layout, bias [E], mask bool [U, P]
with P = Ln - k + 1 and True = padding position, any pattern.  An exact tie takes the lowest position; an entity without an unmasked
position gives -inf and a zero gradient (what `masked_fill` then `max` give; the reference writes -inf into `.data` in place and so
leaks such an entity's gradient to position 0); a NaN at an unmasked position gives NaN.

With fp32 GPU tensors and a shape `recon_line_pool_supported` takes, the kernels of csrc/line_pool.hip run: one launch forward, at most
two backward (every cell of d_states once plus the parameter gradients' slabs over entity groups; the slabs' sum in group order), fp32,
no atomics, bitwise reproducible.  Neither the [U, E, P] convolution output nor its masked copy is written: the op saves references to
its inputs and one position byte per output (255: none), which makes P <= 255 the kernels' limit.  Under no_grad, or when nothing
requires a gradient, the forward allocates the output alone.  An input that does not require a gradient gets none and costs nothing.
The backward destroys nothing: a second backward over a retained graph runs the kernels again and gives the same bits.  Otherwise —
CPU tensors, another dtype, a shape the library refuses, a backward under create_graph — the call runs `_chain`, the three lines
`EntityEmbedding.forward` is without it.  DESIGN.md section 24.
"""
import torch
import torch.nn.functional as F

from . import _lib

MAX_ENTITY_GROUPS = 256           # kLpMaxGroups of csrc/line_pool.hip: the backward cuts the U entities into groups of ceil(U / min(256, U))
NO_POSITION = 255                 # kLpNone: the position byte of an output without an unmasked position


def _chain(states, weight, bias, mask):
    """The stock lines (models/models.py:73-81): the convolution over the permuted states, `masked_fill`, `max`."""
    conv = F.conv1d(states.permute(0, 2, 1), weight, bias)
    conv = conv.masked_fill(mask.unsqueeze(1), -float('inf'))
    return conv.max(dim=2).values


class _LinePool(torch.autograd.Function):
    """csrc/line_pool.hip: saves references to its inputs and the position bytes — nothing else."""

    @staticmethod
    def forward(ctx, wants, states, weight, bias, mask):
        lib = _lib.lib()
        U, Ln, C = states.shape
        E, _, k = weight.shape
        dev = states.device
        rows, ld = _lib.rows_in_place(states.detach(), C)
        mask = mask.contiguous()
        out = torch.empty(U, E, dtype=torch.float32, device=dev)
        pos = torch.empty(U, E, dtype=torch.uint8, device=dev) if wants else None
        with _lib.on_device(dev):
            _lib.check(lib.recon_line_pool_fwd(rows.data_ptr(), ld, weight.detach().data_ptr(), bias.detach().data_ptr(), mask.data_ptr(), U, Ln, C,
                                               E, k, out.data_ptr(), _lib.ptr(pos), _lib.current_stream()), "recon_line_pool_fwd")
        del rows
        ctx.set_materialize_grads(False)
        if wants:
            ctx.save_for_backward(states, weight, bias, mask, pos)
        return out

    @staticmethod
    def backward(ctx, g_out):
        states, weight, bias, mask, pos = ctx.saved_tensors
        need = list(ctx.needs_input_grad[1:4])
        if g_out is None or not any(need):
            return (None,) * 5
        if torch.is_grad_enabled():                                      # create_graph: the gradient itself must be differentiable
            return (None,) + _lib.recompute_grads(lambda: _chain(states, weight, bias, mask), [states, weight, bias], need, g_out, True) + (None,)
        lib = _lib.lib()
        U, Ln, C = states.shape
        E, _, k = weight.shape
        dev = states.device
        rows, ld = _lib.rows_in_place(states.detach(), C)
        g = g_out.to(torch.float32).contiguous()
        g_s = torch.empty(U, Ln, C, dtype=torch.float32, device=dev) if need[0] else None
        g_w = torch.empty_like(weight) if need[1] else None
        g_b = torch.empty_like(bias) if need[2] else None
        params = g_w is not None or g_b is not None
        ws = _lib.workspace(lib.recon_line_pool_workspace_bytes(U, Ln, C, E, k) if params else 0, dev)
        with _lib.on_device(dev):
            _lib.check(lib.recon_line_pool_bwd(rows.data_ptr(), ld, weight.detach().data_ptr(), g.data_ptr(), pos.data_ptr(), U, Ln, C, E, k,
                                               _lib.ptr(g_s), _lib.ptr(g_w), _lib.ptr(g_b), ws.data_ptr(), ws.numel(), _lib.current_stream()),
                       "recon_line_pool_bwd")
        del rows
        return None, g_s, g_w, g_b, None


def _fused(states, weight, bias):
    if not states.is_cuda or any(t.dtype != torch.float32 for t in (states, weight, bias)):
        return False
    if not weight.is_contiguous() or not bias.is_contiguous():
        return False
    U, Ln, C = states.shape
    E, _, k = weight.shape
    return bool(_lib.lib().recon_line_pool_supported(U, Ln, C, E, k))


def _shape(t):
    return tuple(getattr(t, "shape", ())) if torch.is_tensor(t) else type(t).__name__


def entity_line_pool(states, weight, bias, mask):
    """[U, Ln, C], [E, C, k], [E], bool [U, Ln - k + 1] (True = padding position) -> [U, E]: the maximum over the unmasked positions of the
    convolution of the line states (models/models.py:73-81), differentiable in states, weight and bias.  U = 0 gives an empty [0, E]
    without a launch."""
    shapes = "states %s, weight %s, bias %s, mask %s" % (_shape(states), _shape(weight), _shape(bias), _shape(mask))
    if not all(torch.is_tensor(t) for t in (states, weight, bias, mask)):
        raise ValueError("entity_line_pool: states, weight, bias and mask must be tensors, got " + shapes)
    if states.dim() != 3 or weight.dim() != 3 or not states.is_floating_point() or states.shape[2] < 1 or weight.shape[0] < 1:
        raise ValueError("entity_line_pool: states must be floating-point [U, Ln, C] and weight [E, C, k], got " + shapes)
    U, Ln, C = states.shape
    E, Cw, k = weight.shape
    if Cw != C or not 1 <= k <= Ln:
        raise ValueError("entity_line_pool: weight must be [E, C, k] with C = %d channels of states and 1 <= k <= Ln = %d, got %s" % (C, Ln, shapes))
    if tuple(bias.shape) != (E,):
        raise ValueError("entity_line_pool: bias must be [E] = [%d], got %s" % (E, shapes))
    if weight.dtype != states.dtype or bias.dtype != states.dtype:
        raise ValueError("entity_line_pool: states, weight and bias must share one dtype, got %s, %s, %s" % (states.dtype, weight.dtype, bias.dtype))
    P = Ln - k + 1
    if mask.dtype != torch.bool or tuple(mask.shape) != (U, P):
        raise ValueError("entity_line_pool: mask must be bool [U, Ln - k + 1] = [%d, %d], got %s %s" % (U, P, mask.dtype, shapes))
    if any(t.device != states.device for t in (weight, bias, mask)):
        raise ValueError("entity_line_pool: the tensors must be on one device, got %s" % [str(t.device) for t in (states, weight, bias, mask)])
    if _fused(states, weight, bias):
        # (inside the function grad mode is off and needs_input_grad ignores no_grad: whether a backward can follow is decided here)
        wants = torch.is_grad_enabled() and any(t.requires_grad for t in (states, weight, bias))
        return _LinePool.apply(wants, states, weight, bias, mask)
    return _chain(states, weight, bias, mask)


# ------------------------------------------------------------------------------------------------------------- the ragged form
def _chain_ragged(states, lines, weight, bias):
    """The stock lines on the padded form: `lines.pad` to the longest entity (at least k lines), the positions' mask from the counts."""
    k = weight.shape[2]
    Ln = max(lines.n_max, k)
    return _chain(lines.pad(states, Ln), weight, bias, lines.to_mask(Ln, k))


class _LinePoolRagged(torch.autograd.Function):
    """csrc/line_pool.hip, the kernels instantiated for rows found through line_ptr: saves references to its inputs and the position bytes."""

    @staticmethod
    def forward(ctx, wants, lines, states, weight, bias):
        lib = _lib.lib()
        L, C = states.shape
        E, _, k = weight.shape
        dev = states.device
        rows, ld = _lib.rows_in_place(states.detach(), C)
        out = torch.empty(lines.U, E, dtype=torch.float32, device=dev)
        pos = torch.empty(lines.U, E, dtype=torch.uint8, device=dev) if wants else None
        with _lib.on_device(dev):
            _lib.check(lib.recon_line_pool_ragged_fwd(rows.data_ptr() or None, ld, weight.detach().data_ptr(), bias.detach().data_ptr(),
                                                      lines.line_ptr.data_ptr(), lines.U, L, lines.n_max, C, E, k, out.data_ptr(), _lib.ptr(pos),
                                                      _lib.current_stream()), "recon_line_pool_ragged_fwd")
        del rows
        ctx.set_materialize_grads(False)
        ctx.lines = lines
        if wants:
            ctx.save_for_backward(states, weight, bias, pos)
        return out

    @staticmethod
    def backward(ctx, g_out):
        states, weight, bias, pos = ctx.saved_tensors
        lines = ctx.lines
        need = list(ctx.needs_input_grad[2:5])
        if g_out is None or not any(need):
            return (None,) * 5
        if torch.is_grad_enabled():                                      # create_graph: the gradient itself must be differentiable
            return (None, None) + _lib.recompute_grads(lambda: _chain_ragged(states, lines, weight, bias), [states, weight, bias], need, g_out, True)
        lib = _lib.lib()
        L, C = states.shape
        E, _, k = weight.shape
        dev = states.device
        rows, ld = _lib.rows_in_place(states.detach(), C)
        g = g_out.to(torch.float32).contiguous()
        g_s = torch.empty(L, C, dtype=torch.float32, device=dev) if need[0] else None
        g_w = torch.empty_like(weight) if need[1] else None
        g_b = torch.empty_like(bias) if need[2] else None
        params = g_w is not None or g_b is not None
        ws = _lib.workspace(lib.recon_line_pool_ragged_workspace_bytes(lines.U, L, lines.n_max, C, E, k) if params else 0, dev)
        with _lib.on_device(dev):
            _lib.check(lib.recon_line_pool_ragged_bwd(rows.data_ptr() or None, ld, weight.detach().data_ptr(), g.data_ptr(), pos.data_ptr(),
                                                      lines.line_ptr.data_ptr(), lines.U, L, lines.n_max, C, E, k, _lib.ptr(g_s) or None,
                                                      _lib.ptr(g_w), _lib.ptr(g_b), ws.data_ptr(), ws.numel(), _lib.current_stream()),
                       "recon_line_pool_ragged_bwd")
        del rows
        return None, None, g_s, g_w, g_b


def _fused_ragged(states, lines, weight, bias):
    if not states.is_cuda or any(t.dtype != torch.float32 for t in (states, weight, bias)):
        return False
    if not weight.is_contiguous() or not bias.is_contiguous():
        return False
    E, C, k = weight.shape
    return bool(_lib.lib().recon_line_pool_ragged_supported(lines.U, lines.total, lines.n_max, C, E, k))


def entity_line_pool_ragged(states, lines, weight, bias):
    """[L, C], RaggedLines, [E, C, k], [E] -> [U, E]: `entity_line_pool` over the n_u - k + 1 windows of entity u's own rows
    states[line_ptr[u] : line_ptr[u + 1]], every one of them present — what the padded call gives with the positions p > n_u - k masked,
    without the padding lines' rows.  The lowest position wins an exact tie; an entity with n_u < k lines (none included) gives -inf and
    zero gradients.  states is read in place where its rows share one stride (a column view of a wider tensor).

    With fp32 GPU tensors and a shape `recon_line_pool_ragged_supported` takes (at most 255 windows per entity, C k <= 1024, E <= 64) the
    kernels of csrc/line_pool.hip run, instantiated for rows found through `lines.line_ptr`: one launch forward, at most two backward,
    every cell of d_states [L, C] written once, the parameter slabs summed over entity groups in group order, no atomics, bitwise
    reproducible, any number of backwards per forward; one position byte per output is the only saved intermediate.  Otherwise — CPU
    tensors, another dtype, an unsupported shape, a backward under create_graph — `lines.pad` and the stock lines.  DESIGN.md section 34."""
    from .ragged_lines import RaggedLines
    shapes = "states %s, lines %r, weight %s, bias %s" % (_shape(states), lines, _shape(weight), _shape(bias))
    if not all(torch.is_tensor(t) for t in (states, weight, bias)) or not isinstance(lines, RaggedLines):
        raise ValueError("entity_line_pool_ragged: states, weight and bias must be tensors and lines a RaggedLines, got " + shapes)
    if states.dim() != 2 or weight.dim() != 3 or not states.is_floating_point() or states.shape[1] < 1 or weight.shape[0] < 1 or weight.shape[2] < 1:
        raise ValueError("entity_line_pool_ragged: states must be floating-point [L, C] and weight [E, C, k], got " + shapes)
    L, C = states.shape
    E, Cw, k = weight.shape
    if Cw != C:
        raise ValueError("entity_line_pool_ragged: weight must be [E, C, k] with C = %d channels of states, got %s" % (C, shapes))
    if L != lines.total:
        raise ValueError("entity_line_pool_ragged: states must hold the batch's L = %d rows, got %s" % (lines.total, shapes))
    if tuple(bias.shape) != (E,):
        raise ValueError("entity_line_pool_ragged: bias must be [E] = [%d], got %s" % (E, shapes))
    if weight.dtype != states.dtype or bias.dtype != states.dtype:
        raise ValueError("entity_line_pool_ragged: states, weight and bias must share one dtype, got %s, %s, %s" % (states.dtype, weight.dtype, bias.dtype))
    if any(t.device != states.device for t in (weight, bias, lines.line_ptr)):
        raise ValueError("entity_line_pool_ragged: the tensors must be on one device, got %s"
                         % [str(t.device) for t in (states, lines.line_ptr, weight, bias)])
    if _fused_ragged(states, lines, weight, bias):
        wants = torch.is_grad_enabled() and any(t.requires_grad for t in (states, weight, bias))
        return _LinePoolRagged.apply(wants, lines, states, weight, bias)
    return _chain_ragged(states, lines, weight, bias)
