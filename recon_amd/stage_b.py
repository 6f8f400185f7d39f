"""A stage-B epoch from device-resident data — DESIGN.md §28.

The reference's loop (train.py:240-330, :331-407, test.py:205-306) keeps the dataset that `graphs_to_indices` returns
(parsing/legacy_sp_models.py:276-333) on the host: per iteration four numpy fancy-index slices with `astype(int)`, four
`torch.from_numpy(...).cuda()` uploads from pageable memory and, in the test loop, two [M] copies back with `.tolist()`.  Here the
dataset is moved to the device once, in its compact dtypes (about 4 KB per sentence at the reference's widths), and an iteration's
inputs are cut from it by one launch:

    data = StageBData.from_indices(train_as_indices, surface_ids).to(device)     # surface_ids: of ContextTables.build; None for GPGNN
    metrics, rows = RelationMetrics(device), EpochRows.for_data(data)
    run_epoch(model, data, batch_size, order=order, batcher=batcher, optimizer=opt, metrics=metrics)      # one training epoch
    run_epoch(model, test_data, batch_size, batcher=test_batcher, metrics=metrics, rows=rows)             # a test pass
    pair, predicted, gold, confidence = rows.result()                             # what test.py:285-302 reads

    sl = data.take(order, start, count, index_dtype=torch.int64)                  # the slice alone: train.py:247-251, :261-262, :309

`StageBSlice` (batch row b is dataset row idx[b], idx = order[start:start + count], the identity without an order):
    sentence_input [count, T] and entity_markers [count, C, T] in index_dtype (int64, the reference's, or int32: `pair_sentence_states`
    and `nn.Embedding` take both); labels int64 [count C], row-major; num_entities int32 [count] (the dataset's own: the reference's
    validation loop passes the training set's by mistake, and no model reads it); entity_indices int64 [count, C, 2], sign-extended, and
    surface_ids int32 [count, C, 2], the dtypes `ContextBatcher.batch` takes (None where the dataset has none); rows int64 [count] = idx.

Two implementations of one result, as in `sampler.py` and `context_batch.py`: torch indexing (`_take_torch`, `_append_torch`), which is
the CPU path and the comparison, and the kernels of csrc/stage_b.hip (`_take_kernel`, `_append_kernel`) on the GPU; `_KERNELS = False`
forces the torch path.  A batch beyond `recon_stage_b_supported` goes to the torch path.

Host reads: none in `take` and `append`.  `run_epoch` validates an `order` once where it enters (one min/max read per epoch,
IndexError outside [0, N)); the kernel also clamps what it reads from `order` into [0, N), so that a value never becomes an address.
`EpochRows.result()` is one read of 16 bytes.  With a `ContextBatcher` the batcher's header read stays (one per iteration).  For a model with
`distinct_pair_sequences` set, `run_epoch` reads the batches' distinct-sequence totals once per epoch and the status word of
`pair_groups` once behind the loop.
"""
import collections
import contextlib

import numpy as np
import torch

from . import _lib, pair_groups
from .objective import relation_objective
from .sentence_conv import ids_prechecked

_KERNELS = True                 # False: the torch path on every device
_ARRAYS = ("sentences", "markers", "labels", "num_entities", "entity_indices", "surface_ids")

StageBSlice = collections.namedtuple("StageBSlice", "sentence_input entity_markers labels num_entities entity_indices surface_ids rows")
EpochRowsResult = collections.namedtuple("EpochRowsResult", "pair predicted gold confidence")


def _new(shape, dtype, device):
    """Every buffer the kernels write comes from here (the tests put guard rows around them)."""
    return torch.empty(shape, dtype=dtype, device=device)


def _compact(a, dtype, name, owner="StageBData"):
    """`a` (numpy array or tensor of integers) as a CPU tensor of the compact dtype; ValueError for a value the dtype cannot hold."""
    t = a.detach().cpu() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype == torch.bool or t.is_floating_point() or t.is_complex():
        raise TypeError("%s: %s must be an integer array, got %s" % (owner, name, t.dtype))
    c = t.to(dtype)
    if c.dtype != t.dtype and not torch.equal(c.to(t.dtype), t):
        raise ValueError("%s: %s holds a value that %s cannot hold" % (owner, name, dtype))
    return c.contiguous()


def _check_order(order, N):
    """One min/max read: IndexError for a value outside [0, N)."""
    if order.numel():
        lo, hi = torch.stack((order.min(), order.max())).tolist()
        if lo < 0 or hi >= N:
            raise IndexError("recon_amd: order holds a row outside [0, %d): min %d, max %d" % (N, lo, hi))


class StageBData:
    """What `graphs_to_indices` returns, on one device: sentences int32 [N, T], markers int8 [N, C, T], labels int16 [N, C], num_entities
    int32 [N] and, for the context models, entity_indices int32 [N, C, 2] (values -1 and up) and surface_ids int32 [N, C, 2] (of
    `ContextTables.build`); both None for GPGNN.  `kept_pairs` = (labels != 0).sum(), counted once on the host."""

    def __init__(self, arrays, kept_pairs):
        self.arrays, self.kept_pairs = dict(arrays), int(kept_pairs)
        for name in _ARRAYS:
            setattr(self, name, self.arrays.get(name))
        self.device = self.sentences.device
        self.N, self.C, self.T = self.markers.shape
        self._distinct_counts = None

    @classmethod
    def from_indices(cls, as_indices, surface_ids=None):
        """as_indices: the reference's tuple (sentences, markers, labels, entity counts[, entity_indices, surface forms, pairs]); the object
        array of surface forms and the pair list are ignored.  surface_ids [N, C, 2]: of `ContextTables.build`, with entity_indices.
        Shapes, dtypes and marker values (every one >= 0: an embedding row) are checked here, once, on the host."""
        if len(as_indices) < 4:
            raise ValueError("StageBData: as_indices must hold sentences, markers, labels and entity counts, got %d arrays" % len(as_indices))
        a = {"sentences": _compact(as_indices[0], torch.int32, "sentences"), "markers": _compact(as_indices[1], torch.int8, "markers"),
             "labels": _compact(as_indices[2], torch.int16, "labels"), "num_entities": _compact(as_indices[3], torch.int32, "num_entities")}
        if a["markers"].dim() != 3 or 0 in a["markers"].shape:
            raise ValueError("StageBData: markers must be a non-empty [N, C, T], got %s" % (tuple(a["markers"].shape),))
        N, C, T = a["markers"].shape
        has_ids = len(as_indices) > 4 and getattr(as_indices[4], "ndim", 0) == 3 and getattr(as_indices[4], "dtype", None) != object
        if has_ids:
            a["entity_indices"] = _compact(as_indices[4], torch.int32, "entity_indices")
        if surface_ids is not None:
            if not has_ids:
                raise ValueError("StageBData: surface_ids come with entity_indices (as_indices[4]), which this tuple does not have")
            a["surface_ids"] = _compact(surface_ids, torch.int32, "surface_ids")
        want = {"sentences": (N, T), "markers": (N, C, T), "labels": (N, C), "num_entities": (N,), "entity_indices": (N, C, 2), "surface_ids": (N, C, 2)}
        for name, t in a.items():
            if tuple(t.shape) != want[name]:
                raise ValueError("StageBData: %s must be %s beside markers %s, got %s" % (name, want[name], (N, C, T), tuple(t.shape)))
        if int(a["markers"].min()) < 0:
            raise ValueError("StageBData: markers holds a negative value (a marker is a row of the position embedding)")
        if "entity_indices" in a and int(a["entity_indices"].min()) < -1:
            raise ValueError("StageBData: entity_indices holds a value below -1")
        return cls(a, int((a["labels"] != 0).sum()))

    def to(self, device):
        device = torch.device(device)
        return StageBData({k: v.to(device) for k, v in self.arrays.items()}, self.kept_pairs)

    def distinct_counts(self):
        """int32 [N] on the data's device: every sentence's distinct marker rows (`pair_groups.distinct_counts` over the resident int8
        markers, in chunks), computed once and kept: what `run_epoch` sums per batch for a model with `distinct_pair_sequences`."""
        if self._distinct_counts is None:
            self._distinct_counts = pair_groups.distinct_counts(self.markers)
        return self._distinct_counts

    # ------------------------------------------------------------------------------------------------------------- take
    def take(self, order, start, count, index_dtype=torch.int64):
        """train.py:247-251 with the casts of :261-262 and :309 -> StageBSlice of the rows order[start:start + count] (order None: the rows
        start .. start + count - 1, as the validation and test loops take them, :333-337).  order: int64, one-dimensional, on the data's
        device; its values are the caller's to validate (`run_epoch` does) — on the GPU they are clamped into [0, N), on the CPU an
        outside one raises IndexError.  No host read."""
        if index_dtype not in (torch.int64, torch.int32):
            raise TypeError("index_dtype must be torch.int64 or torch.int32")
        if order is not None:
            if not torch.is_tensor(order) or order.dtype != torch.int64 or order.dim() != 1:
                raise TypeError("order must be a one-dimensional int64 tensor or None")
            if order.device != self.device:
                raise RuntimeError("recon_amd: order and the data must live on one device")
            order = order.contiguous()
        limit = self.N if order is None else order.numel()
        if not (isinstance(start, int) and isinstance(count, int)) or start < 0 or count < 0 or start + count > limit:
            raise IndexError("take: rows [%r, %r + %r) outside [0, %d)" % (start, start, count, limit))
        if count and _KERNELS and self.device.type == "cuda" and _lib.lib().recon_stage_b_supported(count, self.C, self.T):
            return self._take_kernel(order, start, count, index_dtype)
        return self._take_torch(order, start, count, index_dtype)

    def _take_kernel(self, order, start, count, index_dtype):
        dev, C, T = self.device, self.C, self.T
        ids, sid = self.entity_indices, self.surface_ids
        sl = StageBSlice(_new((count, T), index_dtype, dev), _new((count, C, T), index_dtype, dev), _new((count * C,), torch.int64, dev),
                         _new((count,), torch.int32, dev), None if ids is None else _new((count, C, 2), torch.int64, dev),
                         None if sid is None else _new((count, C, 2), torch.int32, dev), _new((count,), torch.int64, dev))
        with _lib.on_device(dev):
            _lib.check(_lib.lib().recon_stage_b_slice(
                self.sentences.data_ptr(), self.markers.data_ptr(), self.labels.data_ptr(), self.num_entities.data_ptr(), _lib.ptr(ids), _lib.ptr(sid),
                self.N, C, T, _lib.ptr(order), 0 if order is None else order.numel(), start, count, 8 if index_dtype == torch.int64 else 4,
                sl.sentence_input.data_ptr(), sl.entity_markers.data_ptr(), sl.labels.data_ptr(), sl.num_entities.data_ptr(),
                _lib.ptr(sl.entity_indices), _lib.ptr(sl.surface_ids), sl.rows.data_ptr(), _lib.current_stream()), "recon_stage_b_slice")
        return sl

    def _take_torch(self, order, start, count, index_dtype):
        if order is None:
            idx = torch.arange(start, start + count, dtype=torch.int64, device=self.device)
            cut = lambda t: t[start:start + count]
        else:
            idx = order[start:start + count]
            if idx.is_cuda:
                idx = idx.clamp(0, self.N - 1)                        # (as the kernel does: an outside value aborts the device context otherwise)
            else:
                _check_order(idx, self.N)
            cut = lambda t: t[idx]
        ids, sid = self.entity_indices, self.surface_ids
        return StageBSlice(cut(self.sentences).to(index_dtype), cut(self.markers).to(index_dtype), cut(self.labels).to(torch.int64).reshape(-1),
                           cut(self.num_entities).clone(), None if ids is None else cut(ids).to(torch.int64),
                           None if sid is None else cut(sid).clone(), idx.clone())


class EpochRows:
    """What test.py:285-302 reads, kept on the device for a whole pass: for every pair whose label is not ignored, in row order,
    `pair` (int64: sentence C + pair, what :301-302 index the test set and the pair list with), `predicted` and `gold` (int64) and
    `confidence` (fp32, the bits of `RelationObjective.confidence`).  `append` makes no host read; `result()` is the one read.

    An EpochRows belongs to ONE stream: an append starts where the one before it ended by reading a cursor that the earlier launch
    stored with a plain store, which only the order of launches on one stream makes safe."""

    def __init__(self, capacity, device):
        if not isinstance(capacity, int) or capacity < 0:
            raise ValueError("EpochRows: capacity must be an integer >= 0, got %r" % (capacity,))
        self.capacity, self.device = capacity, torch.device(device)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)                   # rows so far; 1 once a row found no room
        self.pair, self.predicted, self.gold = (_new((capacity,), torch.int64, self.device) for _ in range(3))
        self.confidence = _new((capacity,), torch.float32, self.device)

    @classmethod
    def for_data(cls, data):
        """Room for every pair of `data` whose label is not 0 (`kept_pairs`)."""
        return cls(data.kept_pairs, data.device)

    def reset(self):
        self.state.zero_()

    def append(self, res, sl, ignore_index=0):
        """res: the RelationObjective of the batch, sl: its StageBSlice.  Row m of the batch is pair sl.rows[m // C] C + m % C."""
        labels = sl.labels.reshape(-1)
        M = labels.numel()
        count = sl.rows.numel()
        if res.predicted.numel() != M or res.confidence.numel() != M or count == 0 or M % count:
            raise ValueError("EpochRows.append: %d labels, %d predictions, %d confidences and %d sentences do not belong together"
                             % (M, res.predicted.numel(), res.confidence.numel(), count))
        if labels.device != self.device or res.predicted.device != self.device:
            raise RuntimeError("recon_amd: the batch and the EpochRows must live on one device")
        if _KERNELS and self.device.type == "cuda" and res.confidence.dtype == torch.float32:
            return self._append_kernel(res, sl, labels, M // count, ignore_index)
        return self._append_torch(res, sl, labels, M // count, ignore_index)

    def _append_kernel(self, res, sl, labels, C, ignore_index):
        predicted, confidence, rows = res.predicted.contiguous(), res.confidence.contiguous(), sl.rows.contiguous()
        with _lib.on_device(self.device):
            _lib.check(_lib.lib().recon_stage_b_collect(labels.data_ptr(), predicted.data_ptr(), confidence.data_ptr(), rows.data_ptr(), labels.numel(), C,
                                                        ignore_index, self.state.data_ptr(), self.capacity, _lib.ptr(self.pair) or None,
                                                        _lib.ptr(self.predicted) or None, _lib.ptr(self.gold) or None,
                                                        _lib.ptr(self.confidence) or None, _lib.current_stream()), "recon_stage_b_collect")

    def _append_torch(self, res, sl, labels, C, ignore_index):
        """Boolean indexing: the CPU path (on a GPU it reads the count back)."""
        keep = labels != ignore_index
        m = torch.nonzero(keep).squeeze(1)
        at, k = int(self.state[0]), m.numel()
        room = max(0, min(k, self.capacity - at))
        m_in = m[:room]
        self.pair[at:at + room] = sl.rows[m_in // C] * C + m_in % C
        self.predicted[at:at + room] = res.predicted[m_in]
        self.gold[at:at + room] = labels[m_in]
        self.confidence[at:at + room] = res.confidence[m_in].to(torch.float32)
        self.state[0] = at + k
        if at + k > self.capacity:
            self.state[1] = 1

    def result(self):
        """-> EpochRowsResult(pair, predicted, gold, confidence), views trimmed to the rows appended since the last reset; the one host
        read.  OverflowError when more rows arrived than the capacity holds."""
        n, overflow = self.state.tolist()
        if overflow or n > self.capacity:
            raise OverflowError("EpochRows: %d rows arrived, the capacity is %d" % (n, self.capacity))
        return EpochRowsResult(self.pair[:n], self.predicted[:n], self.gold[:n], self.confidence[:n])


def run_epoch(model, data, batch_size, *, order=None, batcher=None, optimizer=None, metrics=None, rows=None, empty_label=1, index_dtype=torch.int64):
    """One pass over `data` in batches of `batch_size` (the tail is dropped, as train.py:244 and :332 do): per iteration `data.take`, with a
    `ContextBatcher` its `batch`, the model's forward and `relation_objective(..., ignore_index=0, empty_label=empty_label,
    metrics=metrics)`; with an optimizer (any torch.optim.Optimizer) `zero_grad()` in front and `loss.backward()` / `step()` behind, in the
    reference's order (train.py:245, :313-315), without one everything under `torch.no_grad()`; with `rows` (an EpochRows)
    `rows.append`.  order: int64 on the data's device, at least (N // batch_size) * batch_size long, validated here with one min/max read.
    The model's train / eval mode is the caller's.  Returns nothing: `metrics` and `rows` hold the results.

    Over a `PairData` (recon_amd/pair_data.py: the per-pair baselines LSTM, CNN and PCNN) the model is called as
    `model(*sl.model_args())`, there is no batcher (ValueError), and the ids are checked once, not once per forward: `data.check_model(model)`
    on the host in front, and the loop inside `sentence_conv.ids_prechecked()`, whose one read of the status word comes behind the loop.

    A model with `distinct_pair_sequences` set: the dataset's per-sentence distinct counts are computed once
    (`data.distinct_counts()`), the per-batch totals are read once per epoch, and every batch runs inside `pair_groups.known_total`, so
    that `PairGroups.from_markers` reads nothing; the status word is read once behind the loop (ValueError at a mismatch)."""
    if not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError("run_epoch: batch_size must be an integer >= 1, got %r" % (batch_size,))
    iterations = data.N // batch_size
    if order is not None:
        if not torch.is_tensor(order) or order.dtype != torch.int64 or order.dim() != 1:
            raise TypeError("order must be a one-dimensional int64 tensor or None")
        if order.numel() < iterations * batch_size:
            raise ValueError("run_epoch: order holds %d rows, %d iterations of %d need %d" % (order.numel(), iterations, batch_size, iterations * batch_size))
        _check_order(order, data.N)
    check_model = getattr(data, "check_model", None)                    # a PairData: one entity pair per row
    if check_model is not None:
        if batcher is not None:
            raise ValueError("run_epoch: a batcher belongs to the per-sentence layout of a StageBData, not to a PairData")
        check_model(model)
    elif batcher is not None and (data.entity_indices is None or data.surface_ids is None):
        raise ValueError("run_epoch: a batcher needs a dataset with entity_indices and surface_ids")
    totals = None
    if check_model is None and getattr(model, "distinct_pair_sequences", False) and iterations:
        # the batches' distinct sequences from the dataset's cached per-sentence counts: the epoch's one host read for `PairGroups`
        counts = data.distinct_counts()
        used = counts[:iterations * batch_size] if order is None else counts[order[:iterations * batch_size]]
        totals = used.view(iterations, batch_size).sum(1).tolist()
    outer = ids_prechecked() if check_model is not None else (pair_groups.known_total(None) if totals is not None else contextlib.nullcontext())
    with outer:
        for i in range(iterations):
            sl = data.take(order, i * batch_size, batch_size, index_dtype)
            with contextlib.nullcontext() if optimizer is not None else torch.no_grad(), \
                    pair_groups.known_total(int(totals[i])) if totals is not None else contextlib.nullcontext():
                if optimizer is not None:
                    optimizer.zero_grad()
                if hasattr(sl, "model_args"):
                    logits = model(*sl.model_args())
                else:
                    extra = batcher.batch(sl.entity_indices, sl.surface_ids, index_dtype).model_args() if batcher is not None else ()
                    logits = model(sl.sentence_input, sl.entity_markers, sl.num_entities, *extra)
                res = relation_objective(logits, sl.labels, ignore_index=0, empty_label=empty_label, metrics=metrics)
                if optimizer is not None:
                    res.loss.backward()
                    optimizer.step()
            if rows is not None:
                rows.append(res, sl)
