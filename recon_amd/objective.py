"""The stage-B objective between the logits and the optimiser (train.py:232, :309-324 and :395-404, test.py:274-291: the masked cross
entropy, `torch.max`, the softmax probability of the prediction and `evaluate_instance_based`, utils/evaluation_utils.py:17-59) as one
device op without a host read:

    from recon_amd import relation_objective, RelationMetrics
    res = relation_objective(logits, labels, ignore_index=0, empty_label=1, metrics=None)
    res.loss        # 0-d fp32, differentiable in logits: mean over the rows with label != ignore_index of logsumexp(row) - row[label]
    res.predicted   # [M] int64: argmax of every row (ignored rows too), the lowest index at a tie, a NaN counting as the maximum
    res.confidence  # [M] fp32: the softmax probability of `predicted`
    res.counts      # [4] int64 on the device: kept rows, n_pred, n_gold, n_ok
    res.f1          # 0-d fp64 on the device: the batch F1 of evaluate_instance_based(..., empty_label), in its double arithmetic

logits [M, n_out] floating point, read in place where `_lib.rows_in_place` allows; labels int64 with M elements in any shape.  A row is
kept when its label is not ignore_index; over the kept rows n_pred counts predicted != empty_label, n_gold counts label != empty_label and
n_ok counts predicted == label != empty_label.  Precision is n_ok / n_pred, recall n_ok / n_gold (0 where the denominator is 0), F1 is
2.0 * prec * rec / (prec + rec) (0 where prec + rec == 0): what the reference's two calls of `micro_avg_precision` give.  With every label
ignored the loss is NaN, its gradient zero, the counters and F1 zero, as the stock lines give.  labels=None is the test-time form:
`predicted` and `confidence`, everything else None.  M = 0 gives empty outputs and a NaN loss without a launch.

`RelationMetrics(device)` keeps an epoch's sums on the device: passed as `metrics=`, the launch that forms `res.f1` adds the counters, the
F1 (the reference's `f1 += add_f1`, the same bits over the same batches in the same order) and 1 to it.  `result()` is the only host read.

With fp32 GPU logits and a shape `recon_relation_objective_supported` takes, the kernels of csrc/objective.hip run: two launches forward
(a wavefront per row; one workgroup for the sums), one backward, no atomics, bitwise reproducible.  The op saves references to its inputs,
one float per row (the log-sum-exp less the row's maximum: the maximum is exact and the backward takes it from the row again, where adding
it in fp32 would cost every probability the maximum's rounding) and the counters it returns; under no_grad, or when logits needs no
gradient, it saves nothing.  The backward reads the incoming gradient and the number of kept rows on the device and destroys nothing: a
second backward over a retained graph gives the same bits.  A kept row whose label lies outside [0, n_out) makes the loss NaN, gets a zero gradient row, counts as gold and
matches nothing; the label is never used as an address (the stock op aborts the device context on such a label, and so does `_chain` on a
GPU; on the CPU it raises).  Otherwise (CPU tensors, another dtype, a shape the library refuses, a backward under create_graph) the call
runs `_chain`, the stock lines plus a tensor formulation of the counters.  DESIGN.md section 25.
"""
import collections

import torch
import torch.nn.functional as F

from . import _lib

RelationObjective = collections.namedtuple("RelationObjective", "loss predicted confidence counts f1")
MetricsResult = collections.namedtuple("MetricsResult", "kept n_pred n_gold n_ok f1_sum batches")


def micro_prf(counts):
    """(precision, recall, F1) as 0-d fp64 tensors from counts = [kept, n_pred, n_gold, n_ok], in evaluate_instance_based's arithmetic
    (utils/evaluation_utils.py:17-59); on the counters' device, no host read."""
    c = counts.to(torch.float64)
    zero = torch.zeros((), dtype=torch.float64, device=counts.device)
    prec = torch.where(c[1] > 0, c[3] / c[1], zero)
    rec = torch.where(c[2] > 0, c[3] / c[2], zero)
    f1 = torch.where(rec + prec > 0, 2.0 * prec * rec / (prec + rec), zero)
    return prec, rec, f1


class RelationMetrics:
    """An epoch's counters on the device: `counts` [4] int64 (kept, n_pred, n_gold, n_ok), `f1_sum` 0-d fp64 and `batches` 0-d int64, views
    of one 48-byte buffer.  `relation_objective(..., metrics=m)` adds a batch to it; `result()` is the only host read; `reset()` zeroes it
    on the device."""

    def __init__(self, device):
        self.buffer = torch.zeros(6, dtype=torch.int64, device=device)
        self.counts = self.buffer[:4]
        self.f1_sum = self.buffer[4:5].view(torch.float64)[0]
        self.batches = self.buffer[5]

    @property
    def device(self):
        return self.buffer.device

    def reset(self):
        self.buffer.zero_()

    def add(self, counts, f1):
        """One batch through tensor ops (the chain's form; the kernels add in their own launch)."""
        self.counts += counts
        self.f1_sum += f1
        self.batches += 1

    def result(self):
        """The sums as Python numbers: one copy to the host."""
        host = self.buffer.cpu()
        return MetricsResult(*host[:4].tolist(), host[4:5].view(torch.float64).item(), int(host[5]))


def _counters(predicted, labels, ignore_index, empty_label):
    kept = labels != ignore_index
    pred, gold = kept & (predicted != empty_label), kept & (labels != empty_label)
    return torch.stack([kept.sum(), pred.sum(), gold.sum(), (gold & (predicted == labels)).sum()])


def _chain(logits, labels, ignore_index=0, empty_label=1, metrics=None):
    """The stock lines (train.py:232, :309-324, test.py:274-291) and the counters of evaluate_instance_based as tensor ops."""
    predicted = torch.max(logits, dim=1)[1]
    confidence = torch.softmax(logits, dim=1, dtype=torch.float32).gather(1, predicted.unsqueeze(1)).squeeze(1)
    if labels is None:
        return RelationObjective(None, predicted, confidence, None, None)
    loss = F.cross_entropy(logits, labels, ignore_index=ignore_index).to(torch.float32)
    counts = _counters(predicted, labels, ignore_index, empty_label)
    f1 = micro_prf(counts)[2]
    if metrics is not None:
        metrics.add(counts, f1)
    return RelationObjective(loss, predicted, confidence, counts, f1)


class _Objective(torch.autograd.Function):
    """csrc/objective.hip: saves references to its inputs, the rows' log-sum-exp (less the maximum) and the counters — nothing else."""

    @staticmethod
    def forward(ctx, wants, logits, labels, ignore_index, empty_label, metrics):
        lib = _lib.lib()
        M, n = logits.shape
        dev = logits.device
        rows, ld = _lib.rows_in_place(logits.detach(), n)
        predicted = torch.empty(M, dtype=torch.int64, device=dev)
        confidence = torch.empty(M, dtype=torch.float32, device=dev)
        ctx.set_materialize_grads(False)
        if labels is None:
            with _lib.on_device(dev):
                _lib.check(lib.recon_relation_objective_fwd(rows.data_ptr(), ld, None, M, n, ignore_index, empty_label, None, predicted.data_ptr(),
                                                            confidence.data_ptr(), None, None, None, None, None, None, None, 0,
                                                            _lib.current_stream()), "recon_relation_objective_fwd")
            ctx.mark_non_differentiable(predicted, confidence)
            return predicted, confidence
        loss = torch.empty((), dtype=torch.float32, device=dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        f1 = torch.empty((), dtype=torch.float64, device=dev)
        lse = torch.empty(M, dtype=torch.float32, device=dev) if wants else None
        ws = _lib.workspace(lib.recon_relation_objective_workspace_bytes(M, n), dev)
        acc = (None, None, None) if metrics is None else (metrics.counts.data_ptr(), metrics.f1_sum.data_ptr(), metrics.batches.data_ptr())
        with _lib.on_device(dev):
            _lib.check(lib.recon_relation_objective_fwd(rows.data_ptr(), ld, labels.data_ptr(), M, n, ignore_index, empty_label, loss.data_ptr(),
                                                        predicted.data_ptr(), confidence.data_ptr(), _lib.ptr(lse), counts.data_ptr(),
                                                        f1.data_ptr(), acc[0], acc[1], acc[2], ws.data_ptr(), ws.numel(),
                                                        _lib.current_stream()), "recon_relation_objective_fwd")
        del rows
        ctx.mark_non_differentiable(predicted, confidence, counts, f1)
        if wants:
            ctx.save_for_backward(logits, labels, lse, counts)
            ctx.ignore_index = ignore_index
        return loss, predicted, confidence, counts, f1

    @staticmethod
    def backward(ctx, g_loss, *unused):
        if g_loss is None or not ctx.needs_input_grad[1]:
            return (None,) * 6
        logits, labels, lse, counts = ctx.saved_tensors
        if torch.is_grad_enabled():                                      # create_graph: the gradient itself must be differentiable
            rerun = lambda: F.cross_entropy(logits, labels, ignore_index=ctx.ignore_index)
            return (None,) + _lib.recompute_grads(rerun, [logits], [True], g_loss, True) + (None,) * 4
        lib = _lib.lib()
        M, n = logits.shape
        dev = logits.device
        rows, ld = _lib.rows_in_place(logits.detach(), n)
        g = g_loss.to(torch.float32).contiguous()
        g_logits = torch.empty(M, n, dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(lib.recon_relation_objective_bwd(rows.data_ptr(), ld, labels.data_ptr(), lse.data_ptr(), g.data_ptr(), counts.data_ptr(), M, n,
                                                        ctx.ignore_index, g_logits.data_ptr(), _lib.current_stream()),
                       "recon_relation_objective_bwd")
        del rows
        return None, g_logits, None, None, None, None


def _fused(logits):
    if not logits.is_cuda or logits.dtype != torch.float32:
        return False
    return bool(_lib.lib().recon_relation_objective_supported(logits.shape[0], logits.shape[1]))


def _shape(t):
    return tuple(getattr(t, "shape", ())) if torch.is_tensor(t) else type(t).__name__


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool) and -2 ** 63 <= v < 2 ** 63


def relation_objective(logits, labels=None, ignore_index=0, empty_label=1, metrics=None):
    """[M, n_out] logits and int64 labels with M elements (None: the test-time form) -> RelationObjective(loss, predicted, confidence,
    counts, f1): train.py:232 and :309-324 without a host read, differentiable in logits."""
    shapes = "logits %s, labels %s" % (_shape(logits), _shape(labels))
    if not torch.is_tensor(logits) or not (labels is None or torch.is_tensor(labels)):
        raise ValueError("relation_objective: logits and labels must be tensors (labels may be None), got " + shapes)
    if logits.dim() != 2 or not logits.is_floating_point() or logits.shape[1] < 1:
        raise ValueError("relation_objective: logits must be floating-point [M, n_out] with n_out >= 1, got " + shapes)
    if not _is_int(ignore_index) or not _is_int(empty_label):
        raise ValueError("relation_objective: ignore_index and empty_label must be integers, got %r and %r" % (ignore_index, empty_label))
    M = logits.shape[0]
    if labels is not None:
        if labels.dtype != torch.int64 or labels.numel() != M:
            raise ValueError("relation_objective: labels must be int64 with M = %d elements, got %s %s" % (M, labels.dtype, shapes))
        if labels.device != logits.device:
            raise ValueError("relation_objective: the tensors must be on one device, got %s" % [str(logits.device), str(labels.device)])
        labels = labels.reshape(-1).contiguous()
    if metrics is not None:
        if not isinstance(metrics, RelationMetrics):
            raise ValueError("relation_objective: metrics must be a RelationMetrics or None, got %s with %s" % (type(metrics).__name__, shapes))
        if labels is None:
            raise ValueError("relation_objective: metrics needs labels, got %s" % shapes)
        if metrics.device != logits.device:
            raise ValueError("relation_objective: metrics must be on the device of %s, got %s and %s" % (shapes, metrics.device, logits.device))
    if M == 0:                                                           # no launch of ours; the loss stays differentiable, as the stock line's
        predicted = torch.empty(0, dtype=torch.int64, device=logits.device)
        confidence = torch.empty(0, dtype=torch.float32, device=logits.device)
        if labels is None:
            return RelationObjective(None, predicted, confidence, None, None)
        counts = torch.zeros(4, dtype=torch.int64, device=logits.device)
        f1 = torch.zeros((), dtype=torch.float64, device=logits.device)
        if metrics is not None:
            metrics.add(counts, f1)
        return RelationObjective(logits.sum().to(torch.float32) * float("nan"), predicted, confidence, counts, f1)
    if _fused(logits):
        # (inside the function grad mode is off and needs_input_grad ignores no_grad: whether a backward can follow is decided here)
        wants = labels is not None and torch.is_grad_enabled() and logits.requires_grad
        out = _Objective.apply(wants, logits, labels, ignore_index, empty_label, metrics)
        return RelationObjective(None, out[0], out[1], None, None) if labels is None else RelationObjective(*out)
    return _chain(logits, labels, ignore_index, empty_label, metrics)
