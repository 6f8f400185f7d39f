"""`WordForms` on the host: the form tables of `ContextTables.build` on a hand-written dataset, the `from_chars` round trip,
the batcher's torch path on the fixture recorded from the reference's own functions, `word_form_features` and `EntityEmbedding` on CPU
tensors against the dense call, every rejection, the C ABI's entries, and the guard of the checks themselves: a float32 restatement of
`expand` and its backward passes them, five wrong restatements are reported."""
import numpy as np
import pytest
import torch

from context_batch_checks import TOKENIZERS, as_numpy, build, expected, fixture, random_batch, random_dataset, to_device
from op_checks import entries_declared_and_bound
from test_char_features_cpu import inputs_word_by_word
from word_forms_checks import WRONG, expand_failures, forms_failures, hand_forms, restate_expand, windows_of

PIECE = 512          # kWfPiece of csrc/word_forms.hip; test_word_forms_gpu.py holds the library to it


def hand_dataset():
    """Two entities and ALL_ZERO; 'abcdefghijXYZ' and 'abcdefghijKLM' agree in their first 10 characters, both are longer than 10."""
    e2i = {"ALL_ZERO": -1, "A": 0, "B": 1, "_UNKNOWN": 2}
    ctx = {"A": {"desc": "abcdefghijXYZ ab abcdefghijKLM", "instances": [{"label": "ab cd"}], "aliases": ["cd"]},
           "B": {"desc": "cd ab zz", "instances": [], "aliases": []}}
    chars = {"<PAD>": 0, "<UNK>": 1}
    for c in "abcdefghijklmnopqrstuvwxyzAKLMXYZ_":
        chars[c] = len(chars)
    vocab = {"_UNKNOWN": 1, "ALL_ZERO": 2, "instance": 3, "of": 4, "also": 5, "known": 6, "as": 7, "ab": 8}
    return {"entity2idx": e2i, "context_wikidata": ctx, "word2idx": vocab, "char2idx": chars, "conv_filter_size": 3}


def test_the_form_tables_of_a_hand_written_dataset():
    from recon_amd import ContextTables
    ds = hand_dataset()
    sf = np.empty((1, 1, 2), dtype=object)
    sf[0, 0, 0], sf[0, 0, 1] = ["ab"], ["abcdefghijXYZ", "q"]
    tables, _ = ContextTables.build(ds["entity2idx"], ds["context_wikidata"], ds["word2idx"], ds["char2idx"], 3, sf, **TOKENIZERS)
    a, c2i = tables.arrays, ds["char2idx"]
    # tokens in interning order: A's lines, B's lines, then the surface forms
    tokens = ["abcdefghijXYZ", "ab", "abcdefghijKLM", "instance", "of", "cd", "also", "known", "as", "zz", "ALL_ZERO", "q"]
    assert tables.dims["V"] == len(tokens)
    row = lambda w: [c2i.get(c, 1) for c in w[:10]] + [0] * (10 - len(w[:10]))
    assert a["tok_chars"].tolist() == [row(w) for w in tokens]
    want_forms = [[0] * 10]
    want_tok = []
    for w in tokens:
        if row(w) not in want_forms:
            want_forms.append(row(w))
        want_tok.append(want_forms.index(row(w)))
    assert a["form_chars"].tolist() == want_forms and a["tok_form"].tolist() == want_tok
    assert want_tok[0] == want_tok[2] == 1 and tables.dims["NFm"] == len(tokens)            # one form for the two long tokens; form 0 on top
    assert a["tok_form"].dtype == a["form_chars"].dtype == torch.int32
    moved = tables.to("cpu")
    assert moved.dims["NFm"] == tables.dims["NFm"] and torch.equal(moved.arrays["tok_form"], a["tok_form"])
    # tables from before the forms carry none: they are derived where the tables are made
    older = ContextTables({k: v for k, v in a.items() if k not in ("tok_form", "form_chars")}, {k: v for k, v in tables.dims.items() if k != "NFm"}, None)
    assert torch.equal(older.arrays["tok_form"], a["tok_form"]) and torch.equal(older.arrays["form_chars"], a["form_chars"])


@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32))
def test_from_chars_round_trip(index_dtype):
    from recon_amd import WordForms
    chars = inputs_word_by_word(7, 3, 4, 3, 5, 6, 9, seed=3)[0].to(index_dtype)
    forms = WordForms.from_chars(chars, 6, 3)
    assert (forms.rows, forms.T, forms.word_span, forms.cfs) == (7, 3, 6, 3) and forms.chars.dtype == index_dtype
    assert forms_failures(forms, chars.numpy(), index_dtype) == []
    assert torch.equal(forms.dense(), chars)
    uniq = np.unique(windows_of(chars.numpy(), 6, 3), axis=0)                   # torch.unique's numbering is numpy's: lexicographic
    assert np.array_equal(forms.chars.numpy(), uniq)
    three = WordForms.from_chars(chars.view(7, 1, -1), 6, 3)
    assert three.rows == 7 and torch.equal(three.slot_form, forms.slot_form)
    empty = WordForms.from_chars(chars[:0], 6, 3)
    assert (empty.rows, empty.total, empty.n_slots) == (0, 0, 0) and empty.expand(torch.zeros(0, 4)).shape == (0, 3, 4)
    no_slots = WordForms.from_chars(chars[:, :2], 6, 3)
    assert (no_slots.rows, no_slots.T, no_slots.total) == (7, 0, 0)


@pytest.mark.parametrize("layout", ("wikidata", "nyt"))
def test_the_torch_path_on_the_fixture(layout):
    from recon_amd import ContextBatcher, RaggedLines, WordForms
    ds, g = fixture()
    all_sf = np.concatenate([sf for _, sf in ds["batches"]], axis=0)
    tables, surface_ids = build(ds, layout, all_sf, None)
    batcher = ContextBatcher(tables)
    for b, (ids, _) in enumerate(ds["batches"]):
        args = to_device(ids, surface_ids[3 * b:3 * b + 3], "cpu")
        want = expected(g, layout, b, None)
        for index_dtype in (torch.int64, torch.int32):
            got = batcher.batch(*args, index_dtype=index_dtype, word_forms=True)
            assert isinstance(got.context_chars, WordForms) and forms_failures(got.context_chars, want["chars"], index_dtype) == []
            assert got.context_chars.rows == want["chars"].shape[0] * want["chars"].shape[1]
            assert np.array_equal(got.context_words.numpy(), want["words"]) and np.array_equal(got.context_mask.numpy(), want["mask"])
            ragged = batcher.batch(*args, index_dtype=index_dtype, ragged_lines=True, word_forms=True)
            dense = batcher.batch(*args, index_dtype=index_dtype, ragged_lines=True)
            assert isinstance(ragged.context_mask, RaggedLines) and ragged.context_chars.rows == ragged.context_mask.total
            assert forms_failures(ragged.context_chars, dense.context_chars.numpy(), index_dtype) == []
            assert torch.equal(ragged.context_words, dense.context_words)
    # the constructor's defaults are what batch falls back to, and an argument overrides them
    both = ContextBatcher(tables, ragged_lines=True, word_forms=True)
    assert isinstance(both.batch(*args).context_chars, WordForms) and isinstance(both.batch(*args).context_mask, RaggedLines)
    assert torch.is_tensor(both.batch(*args, word_forms=False).context_chars) and torch.is_tensor(both.batch(*args, ragged_lines=False).context_mask)
    assert torch.is_tensor(batcher.batch(*args).context_chars)


def test_the_torch_path_numbers_by_ascending_table_form():
    from recon_amd import ContextBatcher
    rng = np.random.default_rng(3)
    ds = random_dataset(rng, 30, 3, max_lines=7)
    ids, sf = random_batch(rng, ds, 3, 6)
    tables, surface_ids = build(ds, "wikidata", sf, None)
    forms = ContextBatcher(tables, word_forms=True).batch(*to_device(ids, surface_ids, "cpu")).context_chars
    table_rows = [tuple(r) for r in tables.arrays["form_chars"].tolist()]
    ranks = [table_rows.index(tuple(r)) for r in forms.chars[:, 2:12].tolist()]
    assert ranks == sorted(ranks) and len(set(ranks)) == forms.total and ranks[0] == 0          # form 0: some slot is empty
    assert bool((forms.chars[:, :2] == 0).all()) and bool((forms.chars[:, 12:] == 0).all())


def test_cpu_tensors_give_the_dense_values():
    from recon_amd import WordForms, char_word_features, word_form_features
    chars, E, Wc, b, span = inputs_word_by_word(9, 4, 4, 3, 5, 6, 9, seed=5)
    forms = WordForms.from_chars(chars, span, 3)
    G = torch.randn(9, 4, 6)
    res = []
    for fn in (lambda *p: word_form_features(forms, *p), lambda *p: char_word_features(chars, *p, span)):
        p = [t.clone().requires_grad_(True) for t in (E, Wc, b)]
        y = fn(*p)
        (y * G).sum().backward()
        res.append([y.detach()] + [t.grad for t in p])
    assert torch.equal(res[0][0], res[1][0])
    for a, c in zip(res[0][1:], res[1][1:]):
        assert torch.allclose(a, c, rtol=1e-5, atol=1e-6)                       # the same sums in another order
    keep = torch.nn.functional.dropout(torch.ones(forms.total, forms.chars.shape[1], 5), 0.5, True)
    dense_keep = torch.ones(9, chars.shape[1], 5)
    shared = word_form_features(forms, E, Wc, b, keep=keep)
    assert shared.shape == (9, 4, 6)
    same = forms.slot_form.view(9, 4)
    first = {int(f): (r, t) for (r, t), f in reversed(list(np.ndenumerate(same.numpy())))}
    for (r, t), f in np.ndenumerate(same.numpy()):                              # every occurrence of a form shares its draw
        assert torch.equal(shared[r, t], shared[first[int(f)]])
    assert not torch.equal(shared, char_word_features(chars, E, Wc, b, span, keep=dense_keep))


def test_entity_embedding_takes_the_forms_on_the_cpu():
    import torch.nn as nn
    from recon_amd import RaggedLines, WordForms
    from recon_amd.gpgnn import EntityEmbedding
    torch.manual_seed(0)
    m = EntityEmbedding(3 + 5, 3, 1, 1, 0.5, 2, 2, 1, nn.Embedding(7, 5, padding_idx=0), 3, 4, list(range(8)), 3).eval()
    words = torch.randint(0, 7, (2, 3, 4))
    chars = torch.randint(0, 8, (2, 3, 1 + 4 * 5))
    mask = torch.tensor([[False, False, True], [False, True, True]])
    forms = WordForms.from_chars(chars, 5, 2)
    with torch.no_grad():
        assert torch.equal(m(words, forms, mask), m(words, chars, mask))
        live = ~mask
        lines = RaggedLines.from_mask(mask)
        assert torch.equal(m(words[live], WordForms.from_chars(chars[live], 5, 2), lines), m(words[live], chars[live], lines))
    with pytest.raises(ValueError):
        m(words, WordForms.from_chars(chars[:1], 5, 2), mask)
    with pytest.raises(ValueError):
        m(words[live], forms, lines)
    with pytest.raises(ValueError):
        m(words, WordForms.from_chars(chars[:, :, :1 + 2 * 10], 10, 2), mask)


def test_rejections():
    from recon_amd import WordForms, word_form_features
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    chars = torch.zeros(2, 14, dtype=torch.int64)
    ok = dict(chars=chars, slot_form=i32(0, 1, 1), form_ptr=i32(0, 1, 3), form_slots=i32(0, 1, 2), rows=3, T=1, total=2, word_span=12, cfs=3)
    WordForms(**ok)
    for change in (dict(chars=chars[:, :13]), dict(chars=chars.float()), dict(chars=chars[:1]), dict(slot_form=i32(0, 1)), dict(slot_form=i32(0, 1, 1).long()),
                   dict(form_ptr=i32(0, 3)), dict(form_slots=i32(0, 1, 2, 3)), dict(rows=-1), dict(T=2), dict(word_span=0), dict(cfs=0),
                   dict(total=3), dict(slot_form=i32(0, 9, 1, 9, 1, 9)[::2]), dict(form_ptr=[0, 1, 3])):
        with pytest.raises(ValueError):
            WordForms(**dict(ok, **change))
    with pytest.raises(ValueError):
        WordForms(chars[:0], i32(0), i32(0), i32(0), 1, 1, 0, 12, 3)                         # a slot and no form
    for bad in ((chars.float(), 12, 3), (chars[0], 12, 3), (chars, 11, 3), (chars, 0, 3), (chars, 12, 0), ("chars", 12, 3)):
        with pytest.raises(ValueError):
            WordForms.from_chars(*bad)
    forms = WordForms(**ok)
    for rows in (torch.zeros(3, 4), torch.zeros(2), "rows"):
        with pytest.raises(ValueError):
            forms.expand(rows)
    if torch.cuda.is_available():
        with pytest.raises(ValueError):
            forms.expand(torch.zeros(2, 4, device="cuda"))
    E, Wc, b = torch.zeros(5, 4), torch.zeros(6, 4, 3), torch.zeros(6)
    with pytest.raises(ValueError):
        word_form_features(chars, E, Wc, b)
    with pytest.raises(ValueError):
        word_form_features(forms, E, torch.zeros(6, 4, 2), b)
    with pytest.raises(ValueError):
        word_form_features(forms, E, Wc, b, keep=torch.ones(3, 14, 4))                       # drawn for the slots, not for the forms
    assert word_form_features(forms, E, Wc, b, keep=torch.ones(2, 14, 4)).shape == (3, 1, 6)


def test_entries_are_declared_bound_and_cite_the_reference():
    entries_declared_and_bound(("recon_word_forms_piece", "recon_word_forms_reduce_workspace_bytes", "recon_word_forms_reduce"), "models/models.py:57-61")
    entries_declared_and_bound(("recon_ctx_batch_forms_scratch_bytes", "recon_ctx_batch_forms_count", "recon_ctx_batch_fill_forms"),
                               "utils/context_utils.py:265-283")


# ------------------------------------------------------------------------------------------------------------- the guard of the checks
def _guard_case():
    rng = np.random.default_rng(17)
    forms = hand_forms([3 * PIECE + 5, 1, 0, PIECE + 1, 7], rng, "cpu", T=2)
    rows_f = rng.standard_normal((forms.total, 5)).astype(np.float32)
    g_out = rng.standard_normal((forms.rows, forms.T, 5)).astype(np.float32)
    return forms, rows_f, g_out


def test_the_float32_restatement_passes_the_checks():
    forms, rows_f, g_out = _guard_case()
    out, g_rows = restate_expand(rows_f, g_out, forms, PIECE)
    assert expand_failures(out, g_rows, rows_f, g_out, forms, "restated") == []
    assert not g_rows[2].any()                                                                # the form without a slot
    # the package's second implementation (index_select and autograd) passes them too
    r = torch.from_numpy(rows_f).requires_grad_(True)
    y = forms.expand(r)
    y.backward(torch.from_numpy(g_out))
    assert expand_failures(y, r.grad, rows_f, g_out, forms, "index_select") == []


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_restatement_is_reported(wrong):
    forms, rows_f, g_out = _guard_case()
    out, g_rows = restate_expand(rows_f, g_out, forms, PIECE, wrong=wrong)
    bad = expand_failures(out, g_rows, rows_f, g_out, forms, wrong)
    assert bad and bad[0][0] == ("out" if wrong in ("slot_form_transposed", "gather_by_form_slots") else "g_rows"), bad
