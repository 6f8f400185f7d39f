"""The distinct word forms of a stage-B entity-context batch — DESIGN.md §36.

`get_char_indices` (utils/context_utils.py:265-283) lays every word slot of a context line out as [cfs - 1 pads][max_char_len ids]
[cfs - 1 pads], and the char-CNN (models/models.py:57-61) computes the feature of a slot from that window of `cfs - 1 + word_span` ids
alone (word_span = max_char_len + cfs - 1), wherever the slot stands.  Most slots of a batch hold the same few windows: every slot behind a
line's last token is all PAD, "instance of" and "also known as" open most lines.  `WordForms` names the distinct windows — what
`RaggedLines` is for padding lines and `PairGroups` for repeated pair sequences:

    forms = WordForms.from_chars(chars, word_span, cfs)                 # or ContextBatcher.batch(..., word_forms=True).context_chars
    feat = word_form_features(forms, emb_weight, conv_weight, conv_bias, keep=keep)          # S_d windows through the char-CNN, [rows, T, Fo] out
    feat = forms.expand(rows_f)                                          # [S_d, F] -> [rows, T, F], differentiable

Fields: `chars` int64 or int32 [S_d, cfs - 1 + word_span], one `W = 1` row of `char_word_features` per form; `slot_form` int32
[rows T], the form of every word slot, row-major; the occurrence lists `form_ptr` int32 [S_d + 1] and `form_slots` int32 [rows T] (the
slots of form 0, then of form 1, ..., ascending inside a form); and the host ints `rows`, `T`, `total` (= S_d), `word_span`, `cfs`.

Numbering: `from_chars` numbers the forms as `torch.unique(dim=0)` sorts them (lexicographically); the batcher numbers them by ascending
table form id.  Both are valid: nothing but the replay of a recorded dropout draw depends on the numbering.

Dropout: `keep` is drawn for [S_d, cfs - 1 + word_span, C], so every occurrence of a form in the batch shares one draw — another
distribution than the dense block's, where every slot draws its own.  That is why the forms are an opt-in.

Two implementations of `expand`, as in `pair_groups.py`: fp32 on the GPU the forward is `recon_pair_groups_expand` (a row gather by
slot_form) and the backward csrc/word_forms.hip (pieces of `piece()` slots, added in piece order: no atomics, bitwise reproducible);
other dtypes, CPU tensors and `_KERNELS = False` run `index_select` and autograd.
"""
import torch

from . import _lib
from .char_features import char_word_features

_KERNELS = True                 # False: index_select on every device
_INDEX_DTYPES = (torch.int64, torch.int32)
_MAX_CELLS = (1 << 31) - 4096   # kPgMaxCells / kWfMaxCells: flat indices are int32


def _new(shape, dtype, device):
    """Every buffer the kernels write comes from here (the tests put guard rows around them)."""
    return torch.empty(shape, dtype=dtype, device=device)


def piece():
    """kWfPiece of csrc/word_forms.hip: the slots per piece of `expand`'s backward."""
    return int(_lib.lib().recon_word_forms_piece())


def occurrence_lists(slot_form, total):
    """(form_ptr int32 [total + 1], form_slots int32 [n_slots]) of slot_form int32 [n_slots] with values in [0, total): the stable
    grouping, from a stable sort and a `searchsorted` of the sorted ids.  No host read."""
    dev = slot_form.device
    if slot_form.numel() == 0:
        return torch.zeros(total + 1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    ordered, form_slots = torch.sort(slot_form, stable=True)
    form_ptr = torch.searchsorted(ordered, torch.arange(total + 1, dtype=slot_form.dtype, device=dev))
    return form_ptr.to(torch.int32), form_slots.to(torch.int32)


class _Expand(torch.autograd.Function):
    """k_pg_expand forward, k_wf_pieces / k_wf_combine backward: saves the forms, nothing of size rows T F."""

    @staticmethod
    def forward(ctx, rows_f, forms):
        n, S_d, F = forms.rows * forms.T, forms.total, rows_f.shape[1]
        r = rows_f.detach().contiguous()
        out = _new((n, F), torch.float32, r.device)
        with _lib.on_device(r.device):
            _lib.check(_lib.lib().recon_pair_groups_expand(r.data_ptr(), forms.slot_form.data_ptr(), n, S_d, F, out.data_ptr(), _lib.current_stream()),
                       "recon_pair_groups_expand")
        ctx.forms = forms
        return out.view(forms.rows, forms.T, F)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        fm = ctx.forms
        n, S_d, F = fm.rows * fm.T, fm.total, g_out.shape[2]
        g = g_out.reshape(n, F).contiguous().to(torch.float32)
        L = _lib.lib()
        g_rows = _new((S_d, F), torch.float32, g.device)
        ws = _lib.workspace(L.recon_word_forms_reduce_workspace_bytes(n, S_d, F), g.device)
        with _lib.on_device(g.device):
            _lib.check(L.recon_word_forms_reduce(g.data_ptr(), fm.form_ptr.data_ptr(), fm.form_slots.data_ptr(), n, S_d, F, g_rows.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _lib.current_stream()), "recon_word_forms_reduce")
        return g_rows, None


class WordForms:
    __slots__ = ("chars", "slot_form", "form_ptr", "form_slots", "rows", "T", "total", "word_span", "cfs")

    def __init__(self, chars, slot_form, form_ptr, form_slots, rows, T, total, word_span, cfs):
        """The four tensors (on one device) and the sizes, which are the caller's word: nothing is read back.  `from_chars` and
        `ContextBatcher.batch(..., word_forms=True)` derive them."""
        rows, T, total, word_span, cfs = int(rows), int(T), int(total), int(word_span), int(cfs)
        if rows < 0 or T < 0 or total < 0 or word_span < 1 or cfs < 1 or (rows * T > 0 and total < 1):
            raise ValueError("WordForms: need rows, T, total >= 0, word_span, cfs >= 1 and a form where there is a slot, got rows %d, T %d, total %d, "
                             "word_span %d, cfs %d" % (rows, T, total, word_span, cfs))
        if rows * T >= 2 ** 31:
            raise ValueError("WordForms: 2^31 word slots or more")
        if not torch.is_tensor(chars) or chars.dtype not in _INDEX_DTYPES or tuple(chars.shape) != (total, cfs - 1 + word_span):
            raise ValueError("WordForms: chars must be an int64 or int32 [total, cfs - 1 + word_span] = [%d, %d] tensor, got %s %s"
                             % (total, cfs - 1 + word_span, getattr(chars, "dtype", None), tuple(getattr(chars, "shape", ()))))
        for name, t, n in (("slot_form", slot_form, rows * T), ("form_ptr", form_ptr, total + 1), ("form_slots", form_slots, rows * T)):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
                raise ValueError("WordForms: %s must be a contiguous int32 [%d] tensor" % (name, n))
            if t.device != chars.device:
                raise ValueError("WordForms: %s and chars must be on one device" % name)
        self.chars, self.slot_form, self.form_ptr, self.form_slots = chars, slot_form, form_ptr, form_slots
        self.rows, self.T, self.total, self.word_span, self.cfs = rows, T, total, word_span, cfs

    # ------------------------------------------------------------------------------------------------------------- builders
    @classmethod
    def from_slot_form(cls, chars, slot_form, rows, T, word_span, cfs):
        """The forms' windows and every slot's form given: the occurrence lists are derived (`occurrence_lists`)."""
        if not torch.is_tensor(slot_form) or slot_form.dtype != torch.int32 or slot_form.dim() != 1:
            raise ValueError("WordForms: slot_form must be a contiguous int32 [%d] tensor" % (int(rows) * int(T)))
        form_ptr, form_slots = occurrence_lists(slot_form, int(chars.shape[0]))
        return cls(chars, slot_form, form_ptr, form_slots, rows, T, chars.shape[0], word_span, cfs)

    @classmethod
    def from_chars(cls, chars, word_span, cfs):
        """chars int64 or int32 [rows, cfs - 1 + T word_span] (or [U, P, .]: rows = U P), the dense block of get_char_indices -> the forms,
        numbered as `torch.unique(dim=0)` sorts the windows.  From torch primitives; reads S_d back once on a GPU."""
        word_span, cfs = int(word_span), int(cfs)
        if not torch.is_tensor(chars) or chars.dtype not in _INDEX_DTYPES or chars.dim() not in (2, 3):
            raise ValueError("WordForms.from_chars: chars must be an int64 or int32 [rows, Lc] or [U, P, Lc] tensor, got %s %s"
                             % (getattr(chars, "dtype", None), tuple(getattr(chars, "shape", ()))))
        if word_span < 1 or cfs < 1:
            raise ValueError("WordForms.from_chars: word_span and cfs must be at least 1, got %d and %d" % (word_span, cfs))
        chars = chars.reshape(-1, chars.shape[-1])
        rows, Lc = chars.shape
        T = (Lc - (cfs - 1)) // word_span
        if T < 0 or Lc != cfs - 1 + T * word_span:
            raise ValueError("WordForms.from_chars: chars has %d columns, expected cfs - 1 + T * word_span with cfs = %d, word_span = %d" % (Lc, cfs, word_span))
        Wf = cfs - 1 + word_span
        if rows * T == 0:
            z = torch.zeros(0, dtype=torch.int32, device=chars.device)
            return cls(chars.new_zeros((0, Wf)), z, torch.zeros(1, dtype=torch.int32, device=chars.device), z.clone(), rows, T, 0, word_span, cfs)
        windows = chars.unfold(1, Wf, word_span).reshape(rows * T, Wf)              # window t of a row: columns [t word_span, t word_span + Wf)
        uniq, inverse = torch.unique(windows, dim=0, return_inverse=True)
        return cls.from_slot_form(uniq.contiguous(), inverse.to(torch.int32).contiguous(), rows, T, word_span, cfs)

    # ------------------------------------------------------------------------------------------------------------- use
    @property
    def n_slots(self):
        return self.rows * self.T

    @property
    def device(self):
        return self.chars.device

    def dense(self):
        """The [rows, cfs - 1 + T word_span] block the forms stand for (every slot's window written back; overlapping pad columns agree)."""
        lead = self.cfs - 1
        if self.n_slots == 0:
            raise ValueError("WordForms.dense: a batch without a word slot does not say what its pad id is")
        w = self.chars[self.slot_form.to(torch.int64)].view(self.rows, self.T, lead + self.word_span)
        return torch.cat((w[:, 0, :lead], w[:, :, lead:].reshape(self.rows, self.T * self.word_span)), dim=1)

    def expand(self, rows_f):
        """[S_d, F] -> [rows, T, F]: slot (r, t) takes row slot_form[r T + t]; differentiable (the gradient of a form's row is the sum of
        its slots' gradient rows in `form_slots` order, cut into pieces of `piece()` slots).  fp32 on the GPU: the kernels; otherwise
        `index_select`."""
        if not torch.is_tensor(rows_f) or rows_f.dim() != 2 or rows_f.shape[0] != self.total:
            raise ValueError("WordForms.expand: rows must be [S_d, F] = [%d, F], got %s" % (self.total, tuple(getattr(rows_f, "shape", ()))))
        if rows_f.device != self.slot_form.device:
            raise ValueError("WordForms.expand: rows and the forms must be on one device")
        F, n = rows_f.shape[1], self.n_slots
        if (_KERNELS and rows_f.is_cuda and rows_f.dtype == torch.float32 and F >= 1 and n > 0
                and _lib.lib().recon_word_forms_reduce_workspace_bytes(n, self.total, F) > 0):
            return _Expand.apply(rows_f, self)
        return rows_f.index_select(0, self.slot_form.to(torch.int64)).view(self.rows, self.T, F)

    def to(self, device):
        return WordForms(self.chars.to(device), self.slot_form.to(device), self.form_ptr.to(device), self.form_slots.to(device), self.rows, self.T,
                         self.total, self.word_span, self.cfs)

    def __repr__(self):
        return "WordForms(rows=%d, T=%d, total=%d, word_span=%d, cfs=%d, device=%s)" % (self.rows, self.T, self.total, self.word_span, self.cfs,
                                                                                       self.chars.device)


def word_form_features(forms, emb_weight, conv_weight, conv_bias, keep=None, padding_idx=0):
    """`char_word_features` over the S_d distinct windows of `forms`, copied to their slots: [rows, T, Fo], differentiable in the three
    parameters; `forms.expand(char_word_features(forms.chars, ..., forms.word_span, keep=keep)[:, 0, :])`.  keep: None, fp32 factors or a
    `PackedKeep` drawn for [S_d, cfs - 1 + word_span, C]: every occurrence of a form shares its draw (see the module's docstring).
    Without keep, and in the table form of the kernels, the values are bit for bit those of the dense call."""
    if not isinstance(forms, WordForms):
        raise ValueError("word_form_features: forms must be a WordForms, got %s" % type(forms).__name__)
    if conv_weight.dim() != 3 or conv_weight.shape[2] != forms.cfs:
        raise ValueError("word_form_features: the forms were cut for cfs = %d, conv_weight is %s" % (forms.cfs, tuple(conv_weight.shape)))
    feat = char_word_features(forms.chars, emb_weight, conv_weight, conv_bias, forms.word_span, keep=keep, padding_idx=padding_idx)
    return forms.expand(feat[:, 0, :])
