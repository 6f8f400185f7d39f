"""The per-pair baselines' datasets on one device — DESIGN.md §32.

LSTM, CNN and PCNN (recon_amd/baselines.py) read one entity pair per row, from the reference's per-pair preprocessing
(parsing/legacy_sp_models.py:67-97 `to_indices`, :503-565 `to_indices_with_relative_positions[_and_entity_pair]`, :567-603
`..._and_pcnn_mask_and_entity_pair`), and its loops slice those arrays on the host per iteration (train.py:247-249 with the casts of
:301-309, again :333-335, :387-393, and test.py).  Here the dataset is moved to the device once, in compact dtypes, and an iteration's
inputs are cut by one launch:

    data = PairData.from_indices(train_as_indices).to(device)
    metrics, rows = RelationMetrics(device), EpochRows.for_data(data)
    run_epoch(model, data, batch_size, order=order, optimizer=opt, metrics=metrics)           # one training epoch (recon_amd/stage_b.py)
    run_epoch(model, test_data, batch_size, metrics=metrics, rows=rows)                        # a test pass
    pair, predicted, gold, confidence = rows.result()                                          # pair: the dataset row (test.py:297-302)

    sl = data.take(order, start, count, index_dtype=torch.int64); model(*sl.model_args())      # the slice alone

The form is told from the arrays:
    marks      markers [N, T]                       LSTM     sentences int32 [N, T], markers int8 [N, T], labels int16 [N]
    positions  markers [N, 2, T]                    CNN      the same with markers int8 [N, 2, T]
    segments   and a floating as_indices[3] [N, 3, T]   PCNN     and segment_bits uint8 [N, T]: bit s of byte [n, t] is pcnn_mask[n, s, t]
The mask holds nothing but 0.0 and 1.0 (semanticgraph/graph_utils.py get_pcnn_mask; checked here), so its 12 bytes per token pack into one
without loss.

`PairSlice` (batch row b is dataset row idx[b], idx = order[start:start + count], the identity without an order): sentence_input
[count, T] and entity_markers [count, T] or [count, 2, T] in index_dtype, pcnn_mask fp32 [count, 3, T] or None, labels int64 [count],
rows int64 [count] = idx; `model_args()` is what the model's forward takes.

One deviation from the reference: the mask follows `order` like every other array.  The reference's shuffled training loop cuts
pcnn_mask from the UNSHUFFLED rows i bs:(i + 1) bs (train.py:304) beside shuffled sentences and positions, which pairs a row with another
row's segments; with order None (validation, test) the two agree.

Two implementations of one result, as in stage_b.py: torch indexing and bit unpacking (`_take_torch`: CPU tensors, a batch beyond
`recon_pair_slice_supported`, and the comparison) and k_sb_slice<5, true> of csrc/stage_b.hip (`_take_kernel`); `_KERNELS = False` forces
the torch path.  No host read in `take`.  `check_model` compares extrema recorded on the host at `from_indices`: no device read either.
"""
import collections

import numpy as np
import torch

from . import _lib
from .stage_b import _check_order, _compact

_KERNELS = True                 # False: the torch path on every device
_ARRAYS = ("sentences", "markers", "labels", "segment_bits")
FORMS = ("marks", "positions", "segments")


class PairSlice(collections.namedtuple("PairSlice", "sentence_input entity_markers pcnn_mask labels rows")):
    __slots__ = ()

    def model_args(self):
        """What the forward takes: (sentence_input, entity_markers), with PCNN's mask behind them where the dataset has one."""
        return self[:2] if self.pcnn_mask is None else self[:3]


def _new(shape, dtype, device):
    """Every buffer the kernel writes comes from here (the tests put guard cells around them)."""
    return torch.empty(shape, dtype=dtype, device=device)


def _pack_mask(mask, N, T):
    """pcnn_mask [N, 3, T] of exactly 0.0 / 1.0 -> uint8 [N, T], plane s in bit s."""
    m = mask.detach().cpu() if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask))
    if tuple(m.shape) != (N, 3, T):
        raise ValueError("PairData: pcnn_mask must be [N, 3, T] = %s beside the markers, got %s" % ((N, 3, T), tuple(m.shape)))
    if not bool(((m == 0.0) | (m == 1.0)).all()):
        raise ValueError("PairData: pcnn_mask holds a value other than 0.0 and 1.0 (one bit per segment and token cannot hold it)")
    b = m.to(torch.uint8)
    return (b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2)).contiguous()


def _extrema(t):
    return int(t.min()), int(t.max())


class PairData:
    """What a per-pair `graphs_to_indices` returns, on one device; see the module's text for the forms.  Recorded once on the host:
    `kept_pairs` = (labels != 0).sum(), `word_ids` = (min, max) of sentences and `marker_ids` = (min, max) of markers."""

    def __init__(self, arrays, kept_pairs, word_ids, marker_ids):
        self.arrays, self.kept_pairs, self.word_ids, self.marker_ids = dict(arrays), int(kept_pairs), tuple(word_ids), tuple(marker_ids)
        for name in _ARRAYS:
            setattr(self, name, self.arrays.get(name))
        self.device = self.sentences.device
        self.N, self.T = self.sentences.shape
        self.marker_rows = 1 if self.markers.dim() == 2 else 2
        self.form = "marks" if self.marker_rows == 1 else ("positions" if self.segment_bits is None else "segments")

    @classmethod
    def from_indices(cls, as_indices):
        """as_indices: the reference's list (sentences, markers, labels[, pcnn_mask][, entity pairs]); a trailing Python list (the entity
        pairs) is ignored.  Shapes, dtypes, marker values (every one >= 0: an embedding row) and the mask's values are checked here, once,
        on the host."""
        as_indices = list(as_indices)
        while as_indices and isinstance(as_indices[-1], (list, tuple)):
            as_indices.pop()
        if len(as_indices) < 3:
            raise ValueError("PairData: as_indices must hold sentences, markers and labels, got %d arrays" % len(as_indices))
        own = lambda i, dtype, name: _compact(as_indices[i], dtype, name, "PairData")
        a = {"sentences": own(0, torch.int32, "sentences"), "markers": own(1, torch.int8, "markers"), "labels": own(2, torch.int16, "labels")}
        if a["sentences"].dim() != 2 or 0 in a["sentences"].shape:
            raise ValueError("PairData: sentences must be a non-empty [N, T], got %s" % (tuple(a["sentences"].shape),))
        N, T = a["sentences"].shape
        if tuple(a["markers"].shape) not in ((N, T), (N, 2, T)):
            raise ValueError("PairData: markers must be %s or %s beside sentences %s, got %s" % ((N, T), (N, 2, T), (N, T), tuple(a["markers"].shape)))
        if tuple(a["labels"].shape) != (N,):
            raise ValueError("PairData: labels must be %s beside sentences %s, got %s" % ((N,), (N, T), tuple(a["labels"].shape)))
        if len(as_indices) > 3:
            mask = as_indices[3]
            if not (torch.is_tensor(mask) and mask.is_floating_point()) and getattr(getattr(mask, "dtype", None), "kind", "") != "f":
                raise TypeError("PairData: as_indices[3] must be the floating pcnn_mask, got %s" % (getattr(mask, "dtype", type(mask).__name__),))
            if a["markers"].dim() != 3:
                raise ValueError("PairData: a pcnn_mask comes with the relative positions [N, 2, T], the markers here are %s" % (tuple(a["markers"].shape),))
            a["segment_bits"] = _pack_mask(mask, N, T)
        marker_ids = _extrema(a["markers"])
        if marker_ids[0] < 0:
            raise ValueError("PairData: markers holds a negative value (a marker is a row of a position embedding)")
        return cls(a, int((a["labels"] != 0).sum()), _extrema(a["sentences"]), marker_ids)

    def to(self, device):
        device = torch.device(device)
        return PairData({k: v.to(device) for k, v in self.arrays.items()}, self.kept_pairs, self.word_ids, self.marker_ids)

    def check_model(self, model):
        """ValueError when an id of the dataset is no row of the model's table: sentences against `word_embedding`, markers against
        `pos_embedding` (marks) or `pos_embedding_0` / `pos_embedding_1` (positions, segments).  Host values only: no device read."""
        tables = ("pos_embedding",) if self.form == "marks" else ("pos_embedding_0", "pos_embedding_1")
        for array, (lo, hi), names in (("sentences", self.word_ids, ("word_embedding",)), ("markers", self.marker_ids, tables)):
            for name in names:
                table = getattr(model, name, None)
                if table is None:
                    raise ValueError("PairData: a %s dataset needs a model with %s, %s has none" % (self.form, name, type(model).__name__))
                if lo < 0 or hi >= table.num_embeddings:
                    raise ValueError("PairData: %s holds ids %d..%d, %s has the rows [0, %d)" % (array, lo, hi, name, table.num_embeddings))

    # ------------------------------------------------------------------------------------------------------------- take
    def take(self, order, start, count, index_dtype=torch.int64):
        """train.py:247-249 with the casts of :301-309 -> PairSlice of the rows order[start:start + count] (order None: the rows start .. start + count - 1, as the
        validation and test loops take them).  The arguments and errors are `StageBData.take`'s: order int64, one-dimensional, on the
        data's device, its values the caller's to validate (`run_epoch` does) — on the GPU they are clamped into [0, N), on the CPU an
        outside one raises IndexError.  The mask follows `order` too (the reference's train.py:304 does not: see the module's text).
        No host read."""
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
        if count and _KERNELS and self.device.type == "cuda" and _lib.lib().recon_pair_slice_supported(count, self.marker_rows, self.T):
            return self._take_kernel(order, start, count, index_dtype)
        return self._take_torch(order, start, count, index_dtype)

    def _take_kernel(self, order, start, count, index_dtype):
        dev, T, bits = self.device, self.T, self.segment_bits
        sl = PairSlice(_new((count, T), index_dtype, dev), _new((count, T) if self.marker_rows == 1 else (count, 2, T), index_dtype, dev),
                       None if bits is None else _new((count, 3, T), torch.float32, dev), _new((count,), torch.int64, dev),
                       _new((count,), torch.int64, dev))
        with _lib.on_device(dev):
            _lib.check(_lib.lib().recon_pair_slice(
                self.sentences.data_ptr(), self.markers.data_ptr(), self.labels.data_ptr(), _lib.ptr(bits), self.N, self.marker_rows, T,
                _lib.ptr(order), 0 if order is None else order.numel(), start, count, 8 if index_dtype == torch.int64 else 4,
                sl.sentence_input.data_ptr(), sl.entity_markers.data_ptr(), _lib.ptr(sl.pcnn_mask), sl.labels.data_ptr(), sl.rows.data_ptr(),
                _lib.current_stream()), "recon_pair_slice")
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
        mask = None
        if self.segment_bits is not None:
            bits = cut(self.segment_bits)
            mask = torch.stack([(bits >> s) & 1 for s in range(3)], dim=1).to(torch.float32)
        return PairSlice(cut(self.sentences).to(index_dtype), cut(self.markers).to(index_dtype), mask, cut(self.labels).to(torch.int64), idx.clone())
