"""`WordForms` on the GPU: the batcher's kernels (k_cb_forms_mark, k_cb_forms_scan, k_cb_forms_fill of csrc/ctx_batch.hip)
against the dense block of the same call and against the torch path, exactly; `WordForms.expand` and its backward (k_wf_pieces,
k_wf_combine of csrc/word_forms.hip) on hand-built forms whose segments stand on both sides of the piece length, through the Python entry
and through the C ABI inside NaN-filled guards, against float64 inside `op_checks`' band; `word_form_features` against the float64 dense
chain; and `EntityEmbedding`, `RECON` and `RECON_EAC` fed the forms against the same models fed the dense block."""
import warnings

import numpy as np
import pytest
import torch

from conftest import load_golden
from context_batch_checks import build, fixture, random_batch, random_dataset, to_device
from op_checks import band_failures, calls_of, close, dev, eac_fixture, peak_bytes, same, state_dict_of
from test_word_forms_cpu import PIECE, hand_dataset
from word_forms_checks import expand_failures, forms_failures, hand_forms, layout_inputs

pytestmark = pytest.mark.gpu
PARAMS = ("emb_weight", "conv_weight", "conv_bias")
GUARD = 37


def test_the_piece_length_is_the_one_the_host_tests_restate():
    from recon_amd import word_forms
    assert word_forms.piece() == PIECE


# ------------------------------------------------------------------------------------------------------------- the batcher
def _paths(monkeypatch):
    from recon_amd.context_batch import ContextBatcher
    return calls_of(monkeypatch, ContextBatcher, "_batch_kernels"), calls_of(monkeypatch, ContextBatcher, "_batch_torch")


def _torch_path(batcher, *args, **kw):
    from recon_amd import context_batch
    prev, context_batch._KERNELS = context_batch._KERNELS, False
    try:
        return batcher.batch(*args, **kw)
    finally:
        context_batch._KERNELS = prev


def _fields(batch):
    """Everything of a forms batch as a flat list of tensors and ints, for exact comparison."""
    from recon_amd import RaggedLines
    f, m = batch.context_chars, batch.context_mask
    mask = [m.line_ptr, m.U, m.total, m.n_max] if isinstance(m, RaggedLines) else [m]
    return [f.chars, f.slot_form, f.form_ptr, f.form_slots, f.rows, f.T, f.total, f.word_span, f.cfs, batch.context_words, batch.unique_entities,
            batch.entities_position, batch.max_occurred_entity_in_batch_pos, batch.gat_entity_embeddings, batch.nonzero_gat_entity_embeddings,
            batch.nonzero_entity_pos] + mask


def _equal(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if torch.is_tensor(x):
            assert torch.is_tensor(y) and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), i
        else:
            assert x == y, (i, x, y)


def _agree(batcher, args, monkeypatch, want_kernels=True):
    """word_forms=True, padded and ragged, both index dtypes: the forms rebuild the dense block of the same call with word_forms=False, no
    two rows are equal, total is the number of distinct windows, the lists are the stable grouping; everything else of the batch is the
    dense call's; and the torch path gives the same forms in the same numbering.  -> the last (ragged, int32) batch."""
    from recon_amd import WordForms
    for ragged in (False, True):
        for index_dtype in (torch.int64, torch.int32):
            kernels, stock = _paths(monkeypatch)
            got = batcher.batch(*args, index_dtype=index_dtype, ragged_lines=ragged, word_forms=True)
            assert (len(kernels), len(stock)) == ((1, 0) if want_kernels else (0, 1))
            dense = batcher.batch(*args, index_dtype=index_dtype, ragged_lines=ragged)
            forms = got.context_chars
            assert isinstance(forms, WordForms) and forms.chars.is_cuda
            assert forms_failures(forms, dense.context_chars.cpu().numpy(), index_dtype) == [], (ragged, index_dtype)
            assert forms.rows * forms.T == dense.context_words.numel() and got.context_words.shape == dense.context_words.shape
            dense.context_chars = forms
            _equal(_fields(got), _fields(dense))
            _equal(_fields(got), _fields(_torch_path(batcher, *args, index_dtype=index_dtype, ragged_lines=ragged, word_forms=True)))
    return got


@pytest.mark.parametrize("layout", ("wikidata", "nyt"))
def test_fixture_through_the_kernels(layout, monkeypatch):
    from recon_amd import ContextBatcher
    ds, g = fixture()
    all_sf = np.concatenate([sf for _, sf in ds["batches"]], axis=0)
    tables, surface_ids = build(ds, layout, all_sf, "selected")
    batcher = ContextBatcher(tables.to(dev()))
    for b, (ids, _) in enumerate(ds["batches"]):
        got = _agree(batcher, to_device(ids, surface_ids[3 * b:3 * b + 3], dev()), monkeypatch)
        want = g["%s.b%d.chars" % (layout, b)]                               # the reference's own char block
        padded = batcher.batch(*to_device(ids, surface_ids[3 * b:3 * b + 3], dev()), word_forms=True).context_chars
        assert forms_failures(padded, want, torch.int64) == [] and got.context_chars.total == padded.total


# (entities, lines at most, B, C, share of padding pairs, one-token surface forms, mode)
SMALL = {"B1_C1": (9, 5, 1, 1, 0.0, False, "selected"), "all_ALL_ZERO": (9, 5, 2, 6, 1.0, False, "selected"), "no_empty_slot": (9, 0, 2, 3, 0.3, True, None),
         "G_all": (30, 31, 3, 6, 0.0, False, "all")}


@pytest.mark.parametrize("case", sorted(SMALL))
def test_small_shapes(case, monkeypatch):
    from recon_amd import ContextBatcher
    n_ent, lines, B, Cn, pad, one_token, mode = SMALL[case]
    rng = np.random.default_rng(sorted(SMALL).index(case))
    ds = random_dataset(rng, n_ent, 3, max_lines=lines)
    ids, sf = random_batch(rng, ds, B, Cn, pad_share=pad, one_token=one_token)
    tables, surface_ids = build(ds, "wikidata", sf, mode)
    got = _agree(ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev()), monkeypatch)
    forms = got.context_chars
    if case == "B1_C1":
        assert ids.shape == (1, 1, 2)
    if case == "all_ALL_ZERO":                                                 # one entity, one line, one token
        assert got.unique_entities.tolist() == [-1] and (forms.rows, forms.T, forms.total) == (1, 1, 1)
    elif case == "no_empty_slot":                                                # every line is T_b = 1 token long: form 0 is absent
        assert forms.T == 1 and not bool((forms.chars == 0).all(dim=1).any())
    else:
        assert bool((forms.chars[0] == 0).all())                              # form 0 is the lowest table form: the batch's form 0


def test_the_references_batch_and_beyond_the_kernels_limit(monkeypatch):
    from recon_amd import ContextBatcher
    from recon_amd.context_batch import MAX_IDS
    rng = np.random.default_rng(7)
    ds = random_dataset(rng, 600, 100)
    # 7200 ids, the reference's; 8320 = 65 x 64 x 2, the torch path.  (A batch holds 2 B C ids, so the 8 193 one above the kernels' 8 192 cannot
    # occur; 8320 is the batch tests/test_context_batch_gpu.py stands above the limit with.)
    for B, Cn, in_kernels in ((50, 72, True), (MAX_IDS // 128 + 1, 64, False)):
        ids, sf = random_batch(rng, ds, B, Cn)
        tables, surface_ids = build(ds, "wikidata", sf, "selected")
        batcher, args = ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev())
        if in_kernels:
            got = _agree(batcher, args, monkeypatch)
        else:
            assert ids.size > 8192
            kernels, stock = _paths(monkeypatch)
            got = batcher.batch(*args, word_forms=True)
            assert not kernels and len(stock) == 1
            assert forms_failures(got.context_chars, batcher.batch(*args).context_chars.cpu().numpy(), torch.int64) == []
        assert got.context_chars.T == 32 and got.context_chars.total < got.context_chars.n_slots // 50


def test_random_batches_kernels_against_the_torch_path(monkeypatch):
    from recon_amd import ContextBatcher
    rng = np.random.default_rng(98)
    for trial in range(8):
        B, Cn = int(rng.choice([1, 3, 7, 20])), int(rng.choice([2, 6, 12]))
        layout = ("wikidata", "nyt")[trial % 2]
        ds = random_dataset(rng, int(rng.choice([5, 40, 200])), 3, max_lines=int(rng.choice([0, 7, 31])), layout=layout)
        ids, sf = random_batch(rng, ds, B, Cn, pad_share=float(rng.choice([0.0, 0.3])))
        tables, surface_ids = build(ds, layout, sf, (None, "all", "selected")[trial % 3])
        _agree(ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev()), monkeypatch)


def test_two_tokens_equal_in_their_first_ten_characters_share_a_form(monkeypatch):
    from recon_amd import ContextBatcher, ContextTables
    from context_batch_checks import TOKENIZERS
    ds = hand_dataset()
    sf = np.empty((1, 2, 2), dtype=object)
    sf[0, 0, 0], sf[0, 0, 1], sf[0, 1, 0], sf[0, 1, 1] = ["ab"], ["abcdefghijXYZ", "q"], ["abcdefghijKLM"], ["zz"]
    ids = np.array([[[0, 1], [1, 0]]], dtype=np.int64)
    tables, surface_ids = ContextTables.build(ds["entity2idx"], ds["context_wikidata"], ds["word2idx"], ds["char2idx"], 3, sf, **TOKENIZERS)
    got = _agree(ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev()), monkeypatch)
    forms, c2i = got.context_chars, ds["char2idx"]
    long_row = [c2i[c] for c in "abcdefghij"]
    rows = forms.chars[:, 2:12].tolist()
    assert rows.count(long_row) == 1                                          # three spellings, one form
    f = rows.index(long_row)
    assert int((forms.slot_form == f).sum()) == 3                             # B's last surface form and A's description twice


@pytest.mark.parametrize("ragged", (False, True))
@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32))
def test_every_cell_is_written_and_nothing_outside(ragged, index_dtype, monkeypatch):
    """Every buffer of a call lies inside sentinel-filled memory behind a guard of 37 elements and in front of another: the guards stay,
    and the outputs equal an unguarded call's, so no cell kept its sentinel."""
    from recon_amd import ContextBatcher, context_batch
    rng = np.random.default_rng(21)
    ds = random_dataset(rng, 200, 3)
    ids, sf = random_batch(rng, ds, 5, 6)
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    batcher, args = ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev())
    ref = _fields(batcher.batch(*args, index_dtype=index_dtype, ragged_lines=ragged, word_forms=True))
    sentinel = {torch.int64: -7777, torch.int32: -7777, torch.float32: 12345.678, torch.bool: 0x5A}
    held = []

    def guarded(shape, dtype, device):
        n = int(np.prod(shape))
        raw = torch.uint8 if dtype == torch.bool else dtype
        flat = torch.full((n + 2 * GUARD,), sentinel[dtype], dtype=raw, device=device)
        held.append((flat, n, dtype))
        inner = flat[GUARD:GUARD + n]
        return (inner.view(torch.bool) if dtype == torch.bool else inner).view(shape)
    monkeypatch.setattr(context_batch, "_new", guarded)
    got = batcher.batch(*args, index_dtype=index_dtype, ragged_lines=ragged, word_forms=True)
    assert len(held) >= 10
    for flat, n, dtype in held:
        s = torch.full((GUARD,), sentinel[dtype], dtype=flat.dtype, device=flat.device)
        assert torch.equal(flat[:GUARD], s) and torch.equal(flat[GUARD + n:], s), (dtype, n)
    _equal(_fields(got), ref)
    _equal(_fields(batcher.batch(*args, index_dtype=index_dtype, ragged_lines=ragged, word_forms=True)), ref)        # two calls, bit for bit


@pytest.mark.parametrize("ragged", (False, True))
def test_a_call_makes_one_host_read(ragged):
    from recon_amd import ContextBatcher
    rng = np.random.default_rng(22)
    ds = random_dataset(rng, 60, 3)
    ids, sf = random_batch(rng, ds, 5, 6)
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    batcher, args = ContextBatcher(tables.to(dev()), ragged_lines=ragged), to_device(ids, surface_ids, dev())
    counts = {}
    for forms in (False, True):
        batcher.batch(*args, word_forms=forms)                                # warm-up: library load, allocator
        torch.cuda.synchronize()
        prev = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                batcher.batch(*args, word_forms=forms)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
        counts[forms] = sum("synchroniz" in str(w.message).lower() for w in seen)
    assert counts == {False: 1, True: 1}, counts


def test_bad_ids_raise_from_the_header(monkeypatch):
    from recon_amd import ContextBatcher
    ds, g = fixture()
    ids, sf = ds["batches"][0]
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    batcher = ContextBatcher(tables.to(dev()), word_forms=True)
    ok = to_device(ids, surface_ids, dev())
    for value in (tables.dims["Ne"], -2, 2 ** 40, tables.dims["Ne"] - 2):
        bad = ok[0].clone()
        bad[2, 1, 0] = value
        with pytest.raises(IndexError):
            batcher.batch(bad, ok[1])
    for value in (tables.dims["S"], -1):
        bad = ok[1].clone()
        bad[0, 3, 1] = value
        with pytest.raises(IndexError):
            batcher.batch(ok[0], bad)
    torch.cuda.synchronize()
    _agree(ContextBatcher(tables.to(dev())), ok, monkeypatch)


# ------------------------------------------------------------------------------------------------------------- expand
LENGTHS = {"around_the_piece": [1, PIECE - 1, PIECE, PIECE + 1, 3 * PIECE + 5, 0], "one_form": [PIECE + 3], "identity": [1] * 77, "no_slot_last": [5, 0, 0]}
_EXPAND = {}


def expand_case(name, F):
    if (name, F) not in _EXPAND:
        rng = np.random.default_rng(100 * sorted(LENGTHS).index(name) + F)
        forms = hand_forms(LENGTHS[name], rng, "cpu", T=1 if name == "identity" else None, shuffle=name != "identity")
        _EXPAND[name, F] = (forms, rng.standard_normal((forms.total, F)).astype(np.float32),
                            rng.standard_normal((forms.rows, forms.T, F)).astype(np.float32))
    return _EXPAND[name, F]


def _python_entry(forms, rows_f, g_out, backwards=1):
    r = torch.from_numpy(rows_f).to(dev()).requires_grad_(True)
    out = forms.expand(r)
    grads = [torch.autograd.grad(out, r, torch.from_numpy(g_out).to(dev()), retain_graph=True)[0] for _ in range(backwards)]
    return out.detach(), grads


@pytest.mark.parametrize("F", (1, 3, 50, 64, 65))
@pytest.mark.parametrize("name", sorted(LENGTHS))
def test_expand_and_its_backward(name, F, monkeypatch):
    from recon_amd import word_forms
    forms_cpu, rows_f, g_out = expand_case(name, F)
    forms = forms_cpu.to(dev())
    ran = calls_of(monkeypatch, word_forms._Expand, "apply")
    held = []

    def guarded(shape, dtype, device):
        n = int(np.prod(shape))
        flat = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=device)
        held.append((flat, n))
        return flat[GUARD:GUARD + n].view(shape)
    monkeypatch.setattr(word_forms, "_new", guarded)
    out, grads = _python_entry(forms, rows_f, g_out, backwards=2)
    assert len(ran) == 1 and len(held) == 3
    for flat, n in held:
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[GUARD + n:]).all()) and not bool(torch.isnan(flat[GUARD:GUARD + n]).any())
    assert torch.equal(grads[0], grads[1])                                     # any number of backwards follow one forward
    bad = expand_failures(out, grads[0], rows_f, g_out, forms_cpu, "expand %s F %d" % (name, F))
    assert not bad, bad
    if name == "identity":
        assert torch.equal(out.view(-1, F), torch.from_numpy(rows_f).to(dev())) and torch.equal(grads[0], torch.from_numpy(g_out).to(dev()).view(-1, F))
    again, grads_again = _python_entry(forms, rows_f, g_out)
    same([out, grads[0]], [again, grads_again[0]])                             # twice, bit for bit
    # CPU tensors and _KERNELS = False: the second implementation, the same values inside the same band
    monkeypatch.setattr(word_forms, "_KERNELS", False)
    out2, grads2 = _python_entry(forms, rows_f, g_out)
    assert len(ran) == 2 and torch.equal(out2, out)
    assert not expand_failures(out2, grads2[0], rows_f, g_out, forms_cpu, "index_select %s F %d" % (name, F))


@pytest.mark.parametrize("F", (1, 3, 50, 64, 65))
@pytest.mark.parametrize("name", sorted(LENGTHS))
def test_expand_through_the_c_abi(name, F):
    from recon_amd import _lib
    forms_cpu, rows_f, g_out = expand_case(name, F)
    forms, L, nan = forms_cpu.to(dev()), _lib.lib(), float("nan")
    n, S_d = forms.n_slots, forms.total
    r, g = torch.from_numpy(rows_f).to(dev()), torch.from_numpy(g_out).to(dev()).reshape(n, F).contiguous()
    results = []
    for _ in range(2):
        held = []

        def guarded(count, dtype, fill):
            flat = torch.full((count + 2 * GUARD,), fill, dtype=dtype, device=dev())
            held.append((flat, count))
            return flat[GUARD:GUARD + count]
        out, g_rows = guarded(n * F, torch.float32, nan), guarded(S_d * F, torch.float32, nan)
        nbytes = L.recon_word_forms_reduce_workspace_bytes(n, S_d, F)
        assert nbytes == ((n // PIECE + S_d + 1) * F * 4 + 15) // 16 * 16
        ws = guarded(nbytes // 4, torch.float32, nan)
        st = _lib.current_stream()
        _lib.check(L.recon_pair_groups_expand(r.data_ptr(), forms.slot_form.data_ptr(), n, S_d, F, out.data_ptr(), st), "recon_pair_groups_expand")
        _lib.check(L.recon_word_forms_reduce(g.data_ptr(), forms.form_ptr.data_ptr(), forms.form_slots.data_ptr(), n, S_d, F, g_rows.data_ptr(),
                                             ws.data_ptr(), nbytes, st), "recon_word_forms_reduce")
        torch.cuda.synchronize()
        for flat, count in held:
            assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[GUARD + count:]).all())
        assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(g_rows).any())
        results.append([out.view(forms.rows, forms.T, F).clone(), g_rows.view(S_d, F).clone()])
    same(*results)
    bad = expand_failures(results[0][0], results[0][1], rows_f, g_out, forms_cpu, "expand %s F %d (C ABI)" % (name, F))
    assert not bad, bad
    py_out, py_grads = _python_entry(forms, rows_f, g_out)
    same(results[0], [py_out, py_grads[0]])                                    # the Python entry runs the same kernels
    # refusals, before any launch
    assert L.recon_word_forms_reduce(g.data_ptr(), forms.form_ptr.data_ptr(), forms.form_slots.data_ptr(), n, S_d, 0, g_rows.data_ptr(), ws.data_ptr(), nbytes,
                                     st) == -1
    assert L.recon_word_forms_reduce(g.data_ptr(), forms.form_ptr.data_ptr(), forms.form_slots.data_ptr(), n, S_d, F, g_rows.data_ptr(), ws.data_ptr(),
                                     nbytes - 16, st) == -4
    assert L.recon_word_forms_reduce(g.data_ptr(), None, forms.form_slots.data_ptr(), n, S_d, F, g_rows.data_ptr(), ws.data_ptr(), nbytes, st) == -1
    assert L.recon_word_forms_reduce_workspace_bytes(2 ** 31, 1, 1) == 0 and L.recon_word_forms_reduce(g.data_ptr(), forms.form_ptr.data_ptr(),
                                                                                                        forms.form_slots.data_ptr(), 2 ** 31, S_d, F, g_rows.data_ptr(),
                                                                                                        ws.data_ptr(), nbytes, st) == -2


# ------------------------------------------------------------------------------------------------------------- the op
#          rows T  max_char cfs C   Fo  V
OP_CASES = [(1, 1, 10, 3, 50, 50, 90), (3, 5, 10, 3, 50, 50, 90), (40, 32, 10, 3, 50, 50, 90), (24, 5, 4, 2, 3, 7, 8)]
_OP = {}


def op_case(shape):
    """Inputs in the reference's layout, tie-masked g_out, the forms and the float64 oracle of the dense chain, computed once."""
    from recon_amd import WordForms
    from test_char_features_cpu import stock
    from test_char_features_gpu import near_ties
    if shape not in _OP:
        chars, E, Wc, b, span, g_out = layout_inputs(*shape)
        g_out = g_out.masked_fill(near_ties(chars, E, Wc, b, span), 0.0)
        p = [t.double().requires_grad_(True) for t in (E, Wc, b)]
        ref = stock(chars, *p, span)
        ref.backward(g_out.double())
        _OP[shape] = (chars, E, Wc, b, span, g_out, WordForms.from_chars(chars, span, shape[3]), [ref.detach()] + [t.grad for t in p])
    return _OP[shape]


def _run(fn, E, Wc, b, g_out):
    p = [t.to(dev()).requires_grad_(True) for t in (E, Wc, b)]
    out = fn(*p)
    out.backward(g_out.to(dev()))
    return [out.detach()] + [t.grad for t in p]


@pytest.mark.parametrize("shape", OP_CASES, ids=lambda s: "x".join(map(str, s)))
def test_op_value_and_gradients(shape, monkeypatch):
    from recon_amd import char_features, char_word_features, word_form_features, word_forms
    from recon_amd.char_features import _chain
    chars, E, Wc, b, span, g_out, forms_cpu, ref = op_case(shape)
    forms, dchars = forms_cpu.to(dev()), chars.to(dev())
    table = calls_of(monkeypatch, char_features._CharWordFeatures, "apply")
    op = _run(lambda *p: word_form_features(forms, *p), E, Wc, b, g_out)
    assert len(table) == 1                                                     # the table form takes every one of these shapes
    chain = _run(lambda *p: _chain(dchars, *p, span), E, Wc, b, g_out)
    bad = band_failures(("out",) + PARAMS, op, chain, ref, "word_form_features %s" % (shape,))
    assert not bad, bad
    dense = _run(lambda *p: char_word_features(dchars, *p, span), E, Wc, b, g_out)
    assert torch.equal(op[0], dense[0])                                        # the table form: the dense call's bits
    assert torch.count_nonzero(op[1][0]) == 0                                  # the padding row's gradient
    same(op, _run(lambda *p: word_form_features(forms, *p), E, Wc, b, g_out))  # twice, bit for bit
    # CPU tensors and _KERNELS = False give the same values
    monkeypatch.setattr(word_forms, "_KERNELS", False)
    second = _run(lambda *p: word_form_features(forms, *p), E, Wc, b, g_out)
    assert torch.equal(second[0], op[0]) and not band_failures(PARAMS, second[1:], chain[1:], ref[1:], "index_select %s" % (shape,))
    p = [t.clone().requires_grad_(True) for t in (E, Wc, b)]
    on_cpu = word_form_features(forms_cpu, *p)
    on_cpu.backward(g_out)
    assert not band_failures(("out",) + PARAMS, [on_cpu.detach()] + [t.grad for t in p], chain, ref, "cpu %s" % (shape,))


@pytest.mark.parametrize("shape", OP_CASES[1:], ids=lambda s: "x".join(map(str, s)))
def test_op_masked_form_replays_the_forms_bits(shape, monkeypatch):
    """Bits drawn for the S_d forms; the dense block's `PackedKeep` carries each word's form's bits at that word's own positions (the pad
    columns two windows share carry the later word's: the pad char's embedding row is zero, so they do not matter).  The forms call equals
    the float64 dense chain under those factors inside the band."""
    from recon_amd import _lib, char_features, word_form_features
    from recon_amd.char_features import PackedKeep, _chain, draw_keep_bits, keep_threshold
    from test_char_masked_gpu import f32, near_ties_masked, oracle
    chars, E, Wc, b, span, g_out, forms_cpu, _ = op_case(shape)
    rows, T, cfs, C = shape[0], shape[1], shape[3], shape[4]
    Wf, scale = cfs - 1 + span, f32(1.0 / (1.0 - 0.3))
    bits = draw_keep_bits(forms_cpu.total, Wf, C, keep_threshold(0.3), 1234, 8, "cpu")
    dense_bits = torch.zeros(rows, chars.shape[1], bits.shape[2], dtype=torch.int32)
    slot_form = forms_cpu.slot_form.view(rows, T).long()
    for t in range(T):
        dense_bits[:, t * span:t * span + Wf] = bits[slot_form[:, t]]
    keep = PackedKeep(dense_bits, scale, C).factors()
    assert bool((E[0] == 0).all())
    g_out = g_out.masked_fill(near_ties_masked(chars, E, Wc, b, span, keep), 0.0)
    ref = oracle(chars, E, Wc, b, span, keep, g_out)
    forms, dchars = forms_cpu.to(dev()), chars.to(dev())
    masked = calls_of(monkeypatch, char_features._CharWordFeaturesMasked, "apply")
    op = _run(lambda *p: word_form_features(forms, *p, keep=PackedKeep(bits.to(dev()), scale, C)), E, Wc, b, g_out)
    runs = int(_lib.lib().recon_char_masked_supported(forms.total, 1, span, cfs, shape[6], C, shape[5]))
    assert len(masked) == runs
    chain = _run(lambda *p: _chain(dchars, *p, span, keep.to(dev())), E, Wc, b, g_out)
    bad = band_failures(("out",) + PARAMS, op, chain, ref, "word_form_features masked %s" % (shape,))
    assert not bad, bad
    # the fp32 factors of the same bits (the op chain over the S_d windows) inside the same band
    fkeep = PackedKeep(bits, scale, C).factors().to(dev())
    op2 = _run(lambda *p: word_form_features(forms, *p, keep=fkeep), E, Wc, b, g_out)
    assert len(masked) == runs and not band_failures(("out",) + PARAMS, op2, chain, ref, "word_form_features factors %s" % (shape,))


def test_training_step_allocates_nothing_of_the_dense_bits_size():
    """Forward and backward with packed dropout at rows = 130, T = 32, C = 50, Fo = 4: the dense call's `PackedKeep` alone is
    rows Lc ceil(C / 32) int32; the forms call, its draw included, stays below that at its peak."""
    from recon_amd import WordForms, word_form_features
    from recon_amd.char_features import draw_packed_keep
    shape = (130, 32, 10, 3, 50, 4, 90)
    chars, E, Wc, b, span, _ = layout_inputs(*shape)
    forms = WordForms.from_chars(chars.to(dev()), span, 3)
    p = [t.to(dev()).requires_grad_(True) for t in (E, Wc, b)]
    dense_bits = 130 * chars.shape[1] * 2 * 4

    def step():
        keep = draw_packed_keep(forms.total, forms.chars.shape[1], 50, 0.5, dev())
        out = word_form_features(forms, *p, keep=keep)
        out.sum().backward()
        return out.detach()
    peak, out = peak_bytes(step)
    print("word_form_features training step: peak %d bytes, the dense bits alone %d bytes, S_d %d of %d slots" % (peak, dense_bits, forms.total, forms.n_slots))
    assert out.shape == (130, 32, 4) and 0 < peak < dense_bits, (peak, dense_bits)


# ------------------------------------------------------------------------------------------------------------- the models
def test_entity_embedding_reproduces_the_char_features_fixture(monkeypatch):
    from recon_amd import WordForms, word_forms
    from test_char_features_cpu import fixture_model
    g = load_golden("char_features1_eval")
    m = fixture_model(g)
    ran = calls_of(monkeypatch, word_forms._Expand, "apply")
    m.train().to(dev())                      # MIOpen's LSTM backward needs training mode; the fixture has p = 0: no factors drawn
    t = lambda k: torch.from_numpy(g[k]).to(dev())
    forms = WordForms.from_chars(t("chars"), int(g["word_span"]), m.conv1d.kernel_size[0])
    out = m(t("words"), forms, t("mask"))
    assert len(ran) == 1
    close(out, g["out"], atol=1e-4, what="char_features1_eval out")
    (out * t("G").float()).sum().backward()
    for k in ("char_embeddings.embeddings.weight", "conv1d.weight", "conv1d.bias"):
        close(dict(m.named_parameters())[k].grad, g["g." + k], atol=1e-4, rel_to_max=1e-4, what="char_features1_eval grad " + k)


def test_recon_eac_reproduces_its_fixture(monkeypatch):
    from recon_amd import WordForms, word_forms
    from tests.test_host_cpu import EAC_P
    m, g, _, name = eac_fixture()
    m.train().to(dev())
    ran = calls_of(monkeypatch, word_forms._Expand, "apply")
    t = lambda k: torch.from_numpy(g[k]).to(dev())
    forms = WordForms.from_chars(t("ctx_chars"), EAC_P["max_char_len"] + EAC_P["conv_filter_size"] - 1, EAC_P["conv_filter_size"])
    out = m(t("sent"), t("mark"), None, None, None, t("ctx_words"), forms, t("ctx_mask"), t("pos"), int(g["max_occ"]))
    assert len(ran) == 1
    close(out, g["out"], atol=1e-4, what=name + " logits")
    (out * torch.from_numpy(g["G"]).to(dev())).sum().backward()
    seen = 0
    for k, v in m.named_parameters():
        if "g." + k in g:
            close(v.grad, g["g." + k], atol=1e-4, rel_to_max=1e-4, what=name + " grad " + k)
            seen += 1
    assert seen == sum(k.startswith("g.") for k in g)


@pytest.mark.parametrize("which", ("recon1_untied", "eac1_untied"))
def test_run_epoch_with_the_switch_off_and_on(which, monkeypatch):
    """N = 7 in batches of 3, dropout 0.  Evaluation: the logits of every batch bit for bit, the counters and the result rows equal, with
    word_forms off and on, padded and ragged.  Then one training epoch (two Adam steps) per setting: every parameter within
    `op_checks.close`'s defaults of the dense run of the same line form."""
    from recon_amd import ContextBatcher, EpochRows, RelationMetrics, StageBData, run_epoch, stage_b, word_forms
    from recon_amd.optim import Adam
    from stage_b_checks import permutation
    from test_ragged_lines_gpu import _eac
    from test_stage_b_gpu import _recon
    make, as_indices, surface_ids, batcher = _recon(False) if which == "recon1_untied" else _eac()
    data = StageBData.from_indices(as_indices, surface_ids).to(dev())
    order = torch.from_numpy(permutation(7, 3)).to(dev())
    logits, real = [], stage_b.relation_objective

    def recorded(*a, **k):
        logits[-1].append(a[0].detach().clone())
        return real(*a, **k)
    monkeypatch.setattr(stage_b, "relation_objective", recorded)
    ran = calls_of(monkeypatch, word_forms._Expand, "apply")
    results = {}
    for ragged in (False, True):
        for forms in (False, True):
            b = ContextBatcher(batcher.tables, ragged_lines=ragged, word_forms=forms)
            m = make().eval()
            test, rows = RelationMetrics(dev()), EpochRows.for_data(data)
            logits.append([])
            run_epoch(m, data, 3, batcher=b, metrics=test, rows=rows)
            evaluated = (logits[-1], test.result(), rows.result())
            m.train()
            logits.append([])
            run_epoch(m, data, 3, order=order, batcher=b, optimizer=Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-2, weight_decay=1e-4,
                                                                         max_grad_norm=0.25), metrics=RelationMetrics(dev()))
            results[ragged, forms] = evaluated + (m,)
    assert len(ran) == 2 * 2 * 2                                              # two settings with the forms, two batches, evaluation and training
    fresh = list(make().parameters())
    for ragged in (False, True):
        (la, ta, ra, ma), (lb, tb, rb, mb) = results[ragged, False], results[ragged, True]
        assert len(la) == len(lb) == 2
        same(la, lb)                                                           # bit for bit
        assert ta == tb and ta.batches == 2
        for f in ("pair", "predicted", "gold", "confidence"):
            assert torch.equal(getattr(ra, f), getattr(rb, f)), f
        changed = 0
        for (k, p), q, f in zip(ma.named_parameters(), mb.parameters(), fresh):
            close(q, p, what=k)
            changed += int(p.requires_grad and not torch.equal(p, f))
        assert changed > 0
