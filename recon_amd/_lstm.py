"""What `context_lstm.py` and `sentence_lstm.py` share: which LSTMs their kernels take, and the Python half of the saved-state contract of
csrc/lstm_common.h (5 H floats per direction, sequence and step, which a backward consumes)."""
import torch
from torch import nn

from . import _lib

_PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
           "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")


def _kernel_lstm(lstm):
    return (isinstance(lstm, nn.LSTM) and lstm.num_layers == 1 and lstm.bidirectional and lstm.batch_first and lstm.bias
            and lstm.proj_size == 0 and lstm.dropout == 0)


def _empty_states(lstm, lead, like):               # the result of an empty batch, without a launch
    dirs = 2 if lstm.bidirectional else 1
    return torch.empty(*lead, dirs * (lstm.proj_size or lstm.hidden_size), dtype=like.dtype, device=like.device)


def _recompute(ctx, rerun, inputs, need, g_out):
    """The gradients through the stock ops, or None: the kernels' backward may run and consumes the saved state.  create_graph (the gradient
    itself must be differentiable; MIOpen's RNN backward is not) or a second backward over a retained graph (the first consumed the saved
    state): recompute through the native ops, which differentiate twice and run a backward in eval mode too."""
    if torch.is_grad_enabled() or ctx.consumed:
        with torch.backends.cudnn.flags(enabled=False):
            return _lib.recompute_grads(rerun, inputs, need, g_out, torch.is_grad_enabled())
    ctx.consumed = True
    return None

