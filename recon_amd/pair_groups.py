"""The distinct (sentence, pair markers) sequences of a stage-B batch — DESIGN.md §35.

`to_indices_with_real_entities_and_entity_nums_with_vertex_padding` (parsing/legacy_sp_models.py:294-326) fills a marker row only for the
pairs a sentence has; every other one of the C pair slots keeps an all-zero row, and `GPGNN.encode` (models/models.py:160-184) copies the
sentence once per slot.  Without dropout the slots of a sentence whose marker rows are equal are bit-identical LSTM inputs.  `PairGroups`
names them — what `RaggedAdjacency` is for graphs and `RaggedLines` for context lines:

    groups = PairGroups.from_markers(sentence, markers)                            # one host read of 4 bytes (S_d)
    states = pair_sentence_states(rnn, sentence, markers, word_table, pos_table, groups=groups)       # S_d sequences, [B, C, 2H] out
    states = groups.expand(rows)                                                   # [S_d, F] -> [B, C, F], differentiable

Grouping rule: two pair slots of the SAME sentence share a sequence exactly when their marker rows are equal element by element (row
equality, not "all zero"); slots of different sentences never share.  The representative of a group is its lowest c; the distinct
sequences are numbered in (b, lowest c) order.

Fields: `seq_pair` int32 [S_d] (the flat pair index b C + c of each sequence's representative), `pair_seq` int32 [B C] (the sequence of
every pair), `seq_ptr` int32 [B + 1], the host ints `B`, `C`, `total` (= S_d) and, from `from_markers`, the compact copies the encoder
reads: `sentence_d` [S_d, T] and `markers_d` [S_d, 1, T], the representatives' rows in the sentence's index dtype.

Two implementations of one result, as in `context_batch.py` and `stage_b.py`: the kernels of csrc/pair_groups.hip on the GPU (C <= 256,
B <= 8192 per call) and torch primitives (`_maps_torch`: the first-true argmax of the [B, C, C] row-equality matrix, then a cumulative
sum) for CPU tensors and anything above those limits; `_KERNELS = False` forces the torch path.

Host reads: `from_markers(total=None)` reads S_d (4 bytes).  With `total=` given it reads the status word instead, and inside
`known_total(n)` it reads nothing: the word is read once where the outermost context ends.
"""
import contextlib
import threading

import torch

from . import _lib

_KERNELS = True                 # False: the torch path on every device
MAX_C, MAX_B = 256, 8192        # kPgMaxC, kPgMaxB of csrc/pair_groups.hip
_MARKER_DTYPES = (torch.int64, torch.int32, torch.int8)
_INDEX_DTYPES = (torch.int64, torch.int32)


def _new(shape, dtype, device):
    """Every buffer the kernels write comes from here (the tests put guard rows around them)."""
    return torch.empty(shape, dtype=dtype, device=device)


def _mismatch(total):
    return ValueError("PairGroups: the batch's distinct sequences are not the %s given as total" % (total,))


# ------------------------------------------------------------------------------------------------------------- known_total
_KNOWN = threading.local()
_STATUS = {}


def _status(dev, stream):
    """One zeroed int32 per device and stream: k_pg_scan sets it to 1 at a total other than the scanned one; reset after it was seen."""
    s = _STATUS.get((dev, stream))
    if s is None:
        with torch.cuda.device(dev):
            s = _STATUS[(dev, stream)] = torch.zeros(1, dtype=torch.int32, device=dev)
    return s


@contextlib.contextmanager
def known_total(n):
    """Inside, `PairGroups.from_markers(..., total=None)` takes total = n and reads nothing from the device (`run_epoch` enters it per
    batch, with the batch's total from the dataset's cached per-sentence counts).  n None: no total is given, only the reading is
    deferred.  Thread-local; a context inside another overrides n and leaves the reading to the outermost one: where that one ends, the
    status word of every (device, stream) used inside is read once, and a mismatch raises ValueError there.  When an exception leaves
    the context, set words are cleared and the exception goes on."""
    if n is not None and (not isinstance(n, int) or isinstance(n, bool) or n < 0):
        raise ValueError("known_total: n must be an integer >= 0 or None, got %r" % (n,))
    outer = getattr(_KNOWN, "state", None)
    if outer is not None:
        before = outer["n"]
        outer["n"] = n
        try:
            yield
        finally:
            outer["n"] = before
        return
    state = _KNOWN.state = {"n": n, "used": {}, "bad": []}
    try:
        yield
    except BaseException:
        _KNOWN.state = None
        _read_words(state)
        raise
    _KNOWN.state = None
    bad = _read_words(state)
    if bad:
        raise _mismatch(bad[0])


def _read_words(state):
    bad = list(state["bad"])
    for status, stream, total in state["used"].values():
        with torch.cuda.stream(stream):
            if int(status):
                status.zero_()
                bad.append(total)
    return bad


def _report(dev, status, flag, total):
    """A mismatch found (`flag`: a host bool on the CPU path, None when the device's status word holds it): inside known_total it is
    kept for the context's end, outside it raises now (on the GPU: the one 4-byte read of a call with `total=`)."""
    state = getattr(_KNOWN, "state", None)
    if status is None:
        if flag:
            if state is None:
                raise _mismatch(total)
            state["bad"].append(total)
        return
    if state is not None:
        key = (dev, _lib.current_stream())
        if key not in state["used"]:
            state["used"][key] = (status, torch.cuda.current_stream(dev), total)
    elif int(status):
        status.zero_()
        raise _mismatch(total)


# ------------------------------------------------------------------------------------------------------------- the torch path
def _first_torch(markers):
    """[B, C] int64: the lowest c' whose row equals slot c's (the first True of the row-equality matrix; argmax returns the first maximum)."""
    B, C, T = markers.shape
    first = torch.empty(B, C, dtype=torch.int64, device=markers.device)
    step = max(1, (1 << 24) // max(1, C * C * T))                          # the [b, C, C, T] comparison in slabs of at most 2^24 cells
    for b0 in range(0, B, step):
        m = markers[b0:b0 + step]
        eq = (m[:, :, None, :] == m[:, None, :, :]).all(dim=3)
        first[b0:b0 + step] = eq.to(torch.uint8).argmax(dim=2)
    return first


def _maps_torch(markers):
    """(first [B, C], is_rep [B, C] bool, pair_seq int64 [B C], seq_ptr int64 [B + 1]) without a host read."""
    B, C, _ = markers.shape
    first = _first_torch(markers)
    is_rep = first == torch.arange(C, device=markers.device)[None, :]
    counts = is_rep.sum(1)
    seq_ptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    rank = is_rep.to(torch.int64).cumsum(1) - 1                            # of a representative: its group's number inside the sentence
    pair_seq = (seq_ptr[:B, None] + rank.gather(1, first)).reshape(-1)
    return first, is_rep, pair_seq, seq_ptr


def distinct_counts(markers, chunk=MAX_B):
    """int32 [N] on markers' device: every sentence's distinct marker rows; markers [N, C, T] of any of the three dtypes (the resident int8
    of a `StageBData` in place).  `k_pg_local` in chunks of at most `chunk` sentences where the kernels take the shape, torch otherwise.
    No host read."""
    _check_markers(markers, "distinct_counts")
    N, C, T = markers.shape
    if N == 0:
        return torch.zeros(0, dtype=torch.int32, device=markers.device)
    chunk = max(1, min(int(chunk), MAX_B))
    if _KERNELS and markers.is_cuda and _lib.lib().recon_pair_groups_supported(min(N, chunk), C, T):
        L = _lib.lib()
        m = markers.contiguous()
        counts = _new((N,), torch.int32, m.device)
        scratch = _new((2, min(N, chunk) * C), torch.int32, m.device)
        with _lib.on_device(m.device):
            for n0 in range(0, N, chunk):
                n = min(chunk, N - n0)
                _lib.check(L.recon_pair_groups_local(m[n0:n0 + n].data_ptr(), m.element_size(), n, C, T, scratch[0].data_ptr(), scratch[1].data_ptr(),
                                                     counts[n0:n0 + n].data_ptr(), _lib.current_stream()), "recon_pair_groups_local")
        return counts
    first = _first_torch(markers)
    return (first == torch.arange(C, device=markers.device)[None, :]).sum(1).to(torch.int32)


def _check_markers(markers, who):
    if not torch.is_tensor(markers) or markers.dim() != 3 or markers.dtype not in _MARKER_DTYPES:
        raise ValueError("%s: markers must be an int64, int32 or int8 [B, C, T] tensor, got %s %s"
                         % (who, getattr(markers, "dtype", None), tuple(getattr(markers, "shape", ()))))
    if markers.shape[1] < 1 or markers.shape[2] < 1:
        raise ValueError("%s: markers needs C >= 1 and T >= 1, got %s" % (who, tuple(markers.shape)))


# ------------------------------------------------------------------------------------------------------------- expand
class _Expand(torch.autograd.Function):
    """k_pg_expand / k_pg_reduce: saves the two maps, nothing of size B C F."""

    @staticmethod
    def forward(ctx, rows, groups):
        B, C, S_d, F = groups.B, groups.C, groups.total, rows.shape[1]
        r = rows.detach().contiguous()
        out = _new((B * C, F), torch.float32, r.device)
        with _lib.on_device(r.device):
            _lib.check(_lib.lib().recon_pair_groups_expand(r.data_ptr(), groups.pair_seq.data_ptr(), B * C, S_d, F, out.data_ptr(), _lib.current_stream()),
                       "recon_pair_groups_expand")
        ctx.groups = groups
        return out.view(B, C, F)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        gr = ctx.groups
        B, C, S_d, F = gr.B, gr.C, gr.total, g_out.shape[2]
        g = g_out.reshape(B * C, F).contiguous().to(torch.float32)
        g_rows = _new((S_d, F), torch.float32, g.device)
        with _lib.on_device(g.device):
            _lib.check(_lib.lib().recon_pair_groups_reduce(g.data_ptr(), gr.pair_seq.data_ptr(), gr.seq_pair.data_ptr(), B, C, S_d, F, g_rows.data_ptr(),
                                                           _lib.current_stream()), "recon_pair_groups_reduce")
        return g_rows, None


_EXPAND_MAX_CELLS = (1 << 31) - 4096


class PairGroups:
    __slots__ = ("seq_pair", "pair_seq", "seq_ptr", "B", "C", "total", "sentence_d", "markers_d", "_source")

    def __init__(self, seq_pair, pair_seq, seq_ptr, B, C, total, sentence_d=None, markers_d=None):
        """The three maps (int32, on one device) and the sizes, which are the caller's word: nothing is read back.  `from_markers` and
        `identity` derive them."""
        B, C, total = int(B), int(C), int(total)
        if B < 0 or C < 1 or not (B <= total <= B * C):
            raise ValueError("PairGroups: need B >= 0, C >= 1 and B <= total <= B C, got B %d, C %d, total %d" % (B, C, total))
        for name, t, n in (("seq_pair", seq_pair, total), ("pair_seq", pair_seq, B * C), ("seq_ptr", seq_ptr, B + 1)):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n or t.device != pair_seq.device or not t.is_contiguous():
                raise ValueError("PairGroups: %s must be a contiguous int32 [%d] tensor on the maps' device" % (name, n))
        if (sentence_d is None) != (markers_d is None):
            raise ValueError("PairGroups: the compact copies come together")
        if sentence_d is not None and not (sentence_d.dim() == 2 and sentence_d.shape[0] == total and sentence_d.dtype in _INDEX_DTYPES
                                           and tuple(markers_d.shape) == (total, 1, sentence_d.shape[1]) and markers_d.dtype == sentence_d.dtype
                                           and sentence_d.device == markers_d.device == pair_seq.device):
            raise ValueError("PairGroups: the compact copies must be [total, T] and [total, 1, T] of one index dtype on the maps' device")
        self.seq_pair, self.pair_seq, self.seq_ptr, self.B, self.C, self.total = seq_pair, pair_seq, seq_ptr, B, C, total
        self.sentence_d, self.markers_d, self._source = sentence_d, markers_d, None

    # ------------------------------------------------------------------------------------------------------------- builders
    @classmethod
    def identity(cls, B, C, device=None):
        """Every pair its own sequence (S_d = B C): the dense call written as groups."""
        B, C = int(B), int(C)
        p = torch.arange(B * C, dtype=torch.int32, device=device)
        return cls(p, p.clone(), torch.arange(B + 1, dtype=torch.int32, device=device) * C, B, C, B * C)

    @classmethod
    def from_markers(cls, sentence, markers, total=None):
        """sentence int64 or int32 [B, T], markers int64, int32 or int8 [B, C, T] on one device -> the groups with their compact copies in
        sentence's dtype.  total: the caller's S_d, else the value of an enclosing `known_total`, else read from the device (4 bytes).  A
        total other than the batch's raises ValueError: at once outside `known_total` (on the GPU that is the call's one read), where the
        outermost context ends inside."""
        _check_markers(markers, "PairGroups.from_markers")
        B, C, T = markers.shape
        if not torch.is_tensor(sentence) or sentence.dtype not in _INDEX_DTYPES or tuple(sentence.shape) != (B, T):
            raise ValueError("PairGroups.from_markers: sentence must be an int64 or int32 [B, T] = [%d, %d] tensor, got %s %s"
                             % (B, T, getattr(sentence, "dtype", None), tuple(getattr(sentence, "shape", ()))))
        if sentence.device != markers.device:
            raise ValueError("PairGroups.from_markers: sentence and markers must be on one device")
        if B * C >= 2 ** 31:
            raise ValueError("PairGroups.from_markers: 2^31 pairs or more")
        state = getattr(_KNOWN, "state", None)
        if total is None and state is not None:
            total = state["n"]
        if total is not None:
            if not isinstance(total, int) or isinstance(total, bool):
                raise ValueError("PairGroups.from_markers: total must be an integer or None, got %r" % (total,))
            if not (B <= total <= B * C):
                raise ValueError("PairGroups.from_markers: total = %d outside [B, B C] = [%d, %d]" % (total, B, B * C))
        if B == 0:
            z = torch.zeros(0, dtype=torch.int32, device=markers.device)
            g = cls(z, z.clone(), torch.zeros(1, dtype=torch.int32, device=markers.device), 0, C, 0, sentence.new_zeros((0, T)),
                    sentence.new_zeros((0, 1, T)))
        elif _KERNELS and markers.is_cuda and _lib.lib().recon_pair_groups_supported(B, C, T):
            g = cls._from_markers_kernel(sentence, markers, total)
        else:
            g = cls._from_markers_torch(sentence, markers, total)
        g._source = _source_key(sentence, markers)
        return g

    @classmethod
    def _from_markers_kernel(cls, sentence, markers, total):
        L = _lib.lib()
        B, C, T = markers.shape
        dev = markers.device
        s, m = sentence.contiguous(), markers.contiguous()
        ws = _lib.workspace(L.recon_pair_groups_workspace_bytes(B, C, T), dev)
        pair_seq, seq_ptr = _new((B * C,), torch.int32, dev), _new((B + 1,), torch.int32, dev)
        status = None
        with _lib.on_device(dev):
            if total is None:
                _lib.check(L.recon_pair_groups_build(None, s.element_size(), m.data_ptr(), m.element_size(), B, C, T, -1, None, pair_seq.data_ptr(),
                                                     seq_ptr.data_ptr(), None, None, None, ws.data_ptr(), ws.numel(), _lib.current_stream()),
                           "recon_pair_groups_build")
                total = int(seq_ptr[B])                                           # the one host read
            else:
                status = _status(dev, _lib.current_stream())
            seq_pair = _new((total,), torch.int32, dev)
            sentence_d, markers_d = _new((total, T), s.dtype, dev), _new((total, 1, T), s.dtype, dev)
            own = status if status is not None else _status(dev, _lib.current_stream())
            _lib.check(L.recon_pair_groups_build(s.data_ptr(), s.element_size(), m.data_ptr(), m.element_size(), B, C, T, total, seq_pair.data_ptr(),
                                                 pair_seq.data_ptr(), seq_ptr.data_ptr(), sentence_d.data_ptr(), markers_d.data_ptr(), own.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _lib.current_stream()), "recon_pair_groups_build")
        if status is not None:
            _report(dev, status, None, total)
        return cls(seq_pair, pair_seq, seq_ptr, B, C, total, sentence_d, markers_d)

    @classmethod
    def _from_markers_torch(cls, sentence, markers, total):
        B, C, T = markers.shape
        dev = markers.device
        first, is_rep, pair_seq, seq_ptr = _maps_torch(markers)
        flags = is_rep.reshape(-1)
        given = total
        if total is None:
            total = int(seq_ptr[B])                                               # (on a GPU: the one host read)
        # the representatives' flat indices ascending, without nonzero's host read: a stable sort brings them to the front
        seq_pair = torch.sort((~flags).to(torch.uint8), stable=True).indices[:total]
        if given is not None:
            if dev.type == "cuda":
                status = _status(dev, _lib.current_stream())
                status.logical_or_(seq_ptr[B:] != total)
                seq_pair = torch.where(torch.arange(total, device=dev) < seq_ptr[B], seq_pair, torch.zeros_like(seq_pair))
                pair_seq = pair_seq.clamp(max=max(total - 1, 0))
                _report(dev, status, None, total)
            else:
                wrong = int(seq_ptr[B]) != total
                if wrong:
                    seq_pair = torch.where(torch.arange(total) < seq_ptr[B], seq_pair, torch.zeros_like(seq_pair))
                    pair_seq = pair_seq.clamp(max=max(total - 1, 0))
                _report(dev, None, wrong, total)
        sentence_d = sentence[seq_pair // C].contiguous()
        markers_d = markers.reshape(B * C, T)[seq_pair].to(sentence.dtype).reshape(total, 1, T).contiguous()
        return cls(seq_pair.to(torch.int32), pair_seq.to(torch.int32), seq_ptr.to(torch.int32), B, C, total, sentence_d, markers_d)

    # ------------------------------------------------------------------------------------------------------------- use
    def compact(self, sentence, markers):
        """(sentence_d [S_d, T], markers_d [S_d, 1, T]): the representatives' rows.  The copies `from_markers` wrote where `sentence` and
        `markers` are the tensors it read (same storage, shape, dtype and version), a gather by `seq_pair` otherwise (`identity`,
        hand-built groups)."""
        B, C = self.B, self.C
        if markers.dim() != 3 or markers.shape[0] != B or markers.shape[1] != C or tuple(sentence.shape) != (B, markers.shape[2]):
            raise ValueError("PairGroups: the groups are over [%d, %d] pairs, got sentence %s and markers %s"
                             % (B, C, tuple(sentence.shape), tuple(markers.shape)))
        if markers.device != self.pair_seq.device or sentence.device != self.pair_seq.device:
            raise ValueError("PairGroups: the groups and the ids must be on one device")
        if self.sentence_d is not None and self._source == _source_key(sentence, markers):
            return self.sentence_d, self.markers_d
        p = self.seq_pair.to(torch.int64)
        T = markers.shape[2]
        return sentence[p // C].contiguous(), markers.reshape(B * C, T)[p].to(sentence.dtype).reshape(self.total, 1, T).contiguous()

    def expand(self, rows):
        """[S_d, F] -> [B, C, F]: pair (b, c) takes row pair_seq[b C + c]; differentiable (the gradient of a row is the sum of its pairs'
        gradients in c order).  fp32 on the GPU: k_pg_expand / k_pg_reduce; otherwise `index_select`."""
        if not torch.is_tensor(rows) or rows.dim() != 2 or rows.shape[0] != self.total:
            raise ValueError("PairGroups.expand: rows must be [S_d, F] = [%d, F], got %s" % (self.total, tuple(getattr(rows, "shape", ()))))
        if rows.device != self.pair_seq.device:
            raise ValueError("PairGroups.expand: rows and the groups must be on one device")
        F = rows.shape[1]
        if (_KERNELS and rows.is_cuda and rows.dtype == torch.float32 and F >= 1 and self.B * self.C > 0
                and self.B * self.C * F < _EXPAND_MAX_CELLS):
            return _Expand.apply(rows, self)
        return rows.index_select(0, self.pair_seq.to(torch.int64)).view(self.B, self.C, F)

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device)
        return PairGroups(mv(self.seq_pair), mv(self.pair_seq), mv(self.seq_ptr), self.B, self.C, self.total, mv(self.sentence_d), mv(self.markers_d))

    def __repr__(self):
        return "PairGroups(B=%d, C=%d, total=%d, device=%s)" % (self.B, self.C, self.total, self.pair_seq.device)


def _source_key(sentence, markers):
    return tuple((t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype, t._version) for t in (sentence, markers))
