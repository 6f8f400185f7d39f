"""Shared by tests/test_word_forms_cpu.py and tests/test_word_forms_gpu.py: what a `WordForms` has to satisfy against the
dense char block it stands for, hand-built forms with chosen segment lengths, and `restate_expand` — `WordForms.expand` and its backward
written once more as plain float32 loops from the definitions in recon_amd/word_forms.py's docstring and include/recon_hip.h, sharing no
code with the package.  `wrong=` makes it wrong in one named way, so that the tests can show the checks catch each.  Not a test module
and not a conftest."""
import numpy as np
import torch

from op_checks import band_failures

WRONG = ("dropped_last_piece", "form_ptr_off_by_one", "slot_form_transposed", "form_zero_skipped", "gather_by_form_slots")


def windows_of(dense, word_span, cfs):
    """[rows, cfs - 1 + T word_span] (numpy) -> [rows T, cfs - 1 + word_span]: the window of every word slot, row-major."""
    dense = np.asarray(dense).reshape(-1, np.asarray(dense).shape[-1])
    rows, Lc = dense.shape
    T = (Lc - (cfs - 1)) // word_span
    assert Lc == cfs - 1 + T * word_span
    return np.stack([dense[:, t * word_span:t * word_span + cfs - 1 + word_span] for t in range(T)], axis=1).reshape(rows * T, -1) if T else \
        np.zeros((0, cfs - 1 + word_span), dense.dtype)


def forms_failures(forms, dense, index_dtype=None):
    """The named properties a `WordForms` misses against the dense block `dense` (numpy [rows, Lc] or [U, P, Lc]); [] when all hold."""
    bad = []
    chars, slot_form = forms.chars.cpu().numpy(), forms.slot_form.cpu().numpy()
    form_ptr, form_slots = forms.form_ptr.cpu().numpy(), forms.form_slots.cpu().numpy()
    want = windows_of(dense, forms.word_span, forms.cfs)
    n = forms.rows * forms.T
    if index_dtype is not None and forms.chars.dtype != index_dtype:
        bad.append("dtype")
    if want.shape[0] != n or slot_form.shape != (n,) or chars.shape != (forms.total, forms.cfs - 1 + forms.word_span):
        return bad + ["shape"]
    if n and (slot_form.min() < 0 or slot_form.max() >= forms.total):
        return bad + ["slot_form out of range"]
    if not np.array_equal(chars[slot_form].astype(np.int64), want.astype(np.int64)):
        bad.append("windows")
    if len({row.tobytes() for row in chars}) != forms.total:
        bad.append("two equal rows")
    if len({row.tobytes() for row in want.astype(np.int64)}) != forms.total:
        bad.append("total")
    order = np.argsort(slot_form, kind="stable")
    counts = np.bincount(slot_form, minlength=forms.total) if n else np.zeros(forms.total, np.int64)
    if not np.array_equal(form_slots, order) or not np.array_equal(form_ptr, np.concatenate(([0], np.cumsum(counts)))):
        bad.append("occurrence lists")
    if forms.n_slots and not np.array_equal(forms.dense().cpu().numpy().astype(np.int64), np.asarray(dense).reshape(forms.rows, -1).astype(np.int64)):
        bad.append("dense()")
    return bad


def hand_forms(lengths, rng, device, T=None, word_span=12, cfs=3, shuffle=True):
    """A `WordForms` whose form f has lengths[f] slots (0 allowed), the slots dealt out in a random order (shuffle) or form by form; rows T
    = sum(lengths) with T a divisor of it (default: the whole batch as one row).  The windows are distinct rows of small ids."""
    from recon_amd import WordForms
    n, S_d = int(sum(lengths)), len(lengths)
    T = n if T is None else T
    assert T == 0 or n % T == 0
    slot_form = np.repeat(np.arange(S_d), lengths).astype(np.int32)
    if shuffle:
        slot_form = slot_form[rng.permutation(n)]
    chars = np.zeros((S_d, cfs - 1 + word_span), np.int64)
    chars[:, cfs - 1] = np.arange(S_d) % 7 + 1
    chars[:, cfs] = np.arange(S_d) // 7 % 7 + 1
    chars[:, cfs + 1] = np.arange(S_d) // 49 + 1
    order = np.argsort(slot_form, kind="stable").astype(np.int32)
    ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return WordForms(t(chars), t(slot_form), t(ptr), t(order), n // T if T else 0, T, S_d, word_span, cfs)


def layout_inputs(rows, T, max_char, cfs, C, Fo, V, seed=0, lexicon=12):
    """A dense char block in get_char_indices' layout — [cfs - 1 pads] then per word slot [max_char ids][cfs - 1 pads] — whose lines hold
    0 .. T words drawn from `lexicon` spellings (so the windows repeat), and parameters as tests/test_char_features_cpu.py's `inputs`
    draws them (row 0 of E, the pad char's, is zero).  CPU tensors: chars [rows, cfs - 1 + T span], E, Wc, b, span, g_out."""
    g = torch.Generator().manual_seed(9000 * seed + rows + T + max_char + cfs + C + Fo + V)
    span = max_char + cfs - 1
    lens = torch.randint(1, max_char + 1, (lexicon,), generator=g)
    words = torch.randint(1, V, (lexicon, max_char), generator=g) * (torch.arange(max_char)[None, :] < lens[:, None])
    chars = torch.zeros(rows, cfs - 1 + T * span, dtype=torch.int64)
    n_words = torch.randint(0, T + 1, (rows,), generator=g)
    pick = torch.randint(0, lexicon, (rows, T), generator=g)
    for r in range(rows):
        for t in range(int(n_words[r])):
            chars[r, cfs - 1 + t * span:cfs - 1 + t * span + max_char] = words[pick[r, t]]
    E = torch.randn(V, C, generator=g)
    E[0] = 0
    Wc = torch.randn(Fo, C, cfs, generator=g) * (2.0 / (C * cfs + Fo * cfs)) ** 0.5
    b = 0.1 * torch.randn(Fo, generator=g)
    return chars, E, Wc, b, span, torch.randn(rows, T, Fo, generator=g)


def restate_expand(rows_f, g_out, forms, piece, wrong=None):
    """(out [rows, T, F], g_rows [S_d, F]) in float32 by plain loops: out[slot] = rows_f[slot_form[slot]]; g_rows[f] = the sum over f's
    pieces, in piece order, of each piece's slots' gradient rows added in list order from zero."""
    rows_f, g = np.asarray(rows_f, np.float32), np.asarray(g_out, np.float32).reshape(-1, np.asarray(g_out).shape[-1])
    slot_form, ptr, slots = forms.slot_form.cpu().numpy(), forms.form_ptr.cpu().numpy(), forms.form_slots.cpu().numpy()
    n, F = forms.rows * forms.T, rows_f.shape[1]
    which = slot_form
    if wrong == "slot_form_transposed":
        which = np.ascontiguousarray(slot_form.reshape(forms.T, forms.rows).T).reshape(-1)       # read as [T, rows]
    if wrong == "gather_by_form_slots":
        which = np.minimum(slots, forms.total - 1)
    out = rows_f[which].reshape(forms.rows, forms.T, F)
    g_rows = np.zeros((forms.total, F), np.float32)
    for f in range(forms.total):
        if wrong == "form_zero_skipped" and f == 0:
            continue
        a, b = int(ptr[f]), int(ptr[f + 1])
        if wrong == "form_ptr_off_by_one":
            a, b = min(a + 1, n), min(b + 1, n)
        starts = list(range(a, b, piece))
        if wrong == "dropped_last_piece" and len(starts) > 1:
            starts = starts[:-1]
        total = np.zeros(F, np.float32)
        for s0 in starts:
            acc = np.zeros(F, np.float32)
            for s in slots[s0:min(s0 + piece, b)]:
                acc = acc + g[s]
            total = total + acc
        g_rows[f] = total
    return out, g_rows


def expand_failures(out, g_rows, rows_f, g_out, forms, label):
    """`out` and `g_rows` (torch or numpy, float32) against float64 inside op_checks' band, the chain being `index_select` and its autograd
    backward in float32 on the CPU; the forward has to be the gather's exact values."""
    idx = forms.slot_form.cpu().to(torch.int64)
    r64 = torch.from_numpy(np.asarray(rows_f, np.float64)).requires_grad_(True)
    g64 = torch.from_numpy(np.asarray(g_out, np.float64)).reshape(forms.rows, forms.T, -1)
    ref = r64.index_select(0, idx).view(forms.rows, forms.T, -1)
    ref.backward(g64)
    r32 = r64.detach().float().requires_grad_(True)
    chain = r32.index_select(0, idx).view(forms.rows, forms.T, -1)
    chain.backward(g64.float())
    as_t = lambda a: a.detach().cpu() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))
    out, g_rows = as_t(out), as_t(g_rows)
    bad = []
    if out.shape != chain.shape or not torch.equal(out, chain.detach()):
        bad.append(("out", "not the gather's values"))
    if forms.total and forms.n_slots:
        bad += band_failures(("g_rows",), (g_rows,), (r32.grad,), (r64.grad,), label)
    elif forms.total and bool((g_rows != 0).any()):
        bad.append(("g_rows", "not zero"))
    return bad
