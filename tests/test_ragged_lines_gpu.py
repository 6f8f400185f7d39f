"""Ragged stage-B batches on the GPU: `entity_line_pool_ragged` through the Python entry and through the C ABI
(csrc/line_pool.hip instantiated for rows found through line_ptr), `ContextBatcher.batch(..., ragged_lines=True)` through k_cb_scan and
k_cb_fill (csrc/ctx_batch.hip), `EntityEmbedding.forward` with a RaggedLines, and RECON / RECON_EAC under `run_epoch` fed either form.

The pool's cases, inputs, float64 reference and comparison are those of tests/ragged_lines_checks.py, guarded on the CPU by
tests/test_ragged_lines_cpu.py; the band is `op_checks.bound` of the stock fp32 chain's own error on the padded form, measured here on
the GPU.  The batcher's outputs are compared exactly: nothing is computed.  The figures measured on an MI355X are in DESIGN.md
section 34."""
import numpy as np
import pytest
import torch

from context_batch_checks import as_numpy, build, differences, expected, fixture, random_batch, random_dataset, to_device
from conftest import load_golden
from op_checks import band_failures, calls_of, close, dev, entries_declared_and_bound, peak_bytes, same, state_dict_of
from ragged_lines_checks import (CASES, CITES, ENCODER_COUNTS, ENTRIES, FILL_CITES, FILL_ENTRY, NONE, REFUSED, case, encoder, encoder_inputs, failures,
                                 run, tie_case)
from test_ragged_lines_cpu import ragged_differences, ragged_numpy

pytestmark = pytest.mark.gpu
GUARD = 48                                                               # elements around every buffer of an ABI run (48 bytes keep 16-byte alignment)


def lines_of(counts):
    from recon_amd import RaggedLines
    return RaggedLines.from_counts(counts, dev())


def kernels_ran(monkeypatch):
    from recon_amd import line_pool
    return calls_of(monkeypatch, line_pool._LinePoolRagged, "apply")


def op_fn(lines):
    from recon_amd import entity_line_pool_ragged
    return lambda s, w, b: entity_line_pool_ragged(s, lines, w, b)


def chain_fn(lines):
    from recon_amd.line_pool import _chain_ragged
    return lambda s, w, b: _chain_ragged(s, lines, w, b)


# ------------------------------------------------------------------------------------------------------------- the pool, Python entry
@pytest.mark.parametrize("name", sorted(CASES))
def test_pool_value_and_gradients(name, monkeypatch):
    from recon_amd import _lib
    c = case(name)
    counts = c["counts"]
    assert _lib.lib().recon_line_pool_ragged_supported(len(counts), sum(counts), max(counts), c["C"], c["E"], c["k"])
    lines = lines_of(counts)
    calls = kernels_ran(monkeypatch)
    fused = run(op_fn(lines), c, dev())
    assert len(calls) == 1, "the kernels take this case: the op must not run the chain"
    chain = run(chain_fn(lines), c, dev())
    print("entity_line_pool_ragged %s: %d of %d cells near a tie" % (name, int(c["ties"].sum()), c["ties"].numel()))
    bad = failures(fused, chain, c["ref"], name)
    assert not bad, bad
    same(fused, run(op_fn(lines), c, dev()))                             # two runs, bit for bit


def test_pool_refused_shape_runs_the_stock_lines(monkeypatch):
    from recon_amd import _lib
    c = case("refused")
    counts, C, E, k = REFUSED
    assert not _lib.lib().recon_line_pool_ragged_supported(len(counts), sum(counts), max(counts), C, E, k)
    lines = lines_of(counts)
    calls = kernels_ran(monkeypatch)
    got = run(op_fn(lines), c, dev())
    assert not calls
    bad = failures(got, run(chain_fn(lines), c, dev()), c["ref"], "refused")
    assert not bad, bad


def test_pool_equals_the_padded_kernels_bit_for_bit(monkeypatch):
    """An entity's sums do not depend on the chunk sizes: the ragged instance gives the bits of the padded instance under the mask of the
    same counts (the value, d_states and d_bias; d_weight's slabs group the same entities, and its bits agree too)."""
    from recon_amd import entity_line_pool
    for name in ("fixture_widths", "two_per_group", "position_chunks"):
        c = case(name)
        counts, k = c["counts"], c["k"]
        lines = lines_of(counts)
        Ln = max(max(counts), k)
        ragged = run(op_fn(lines), c, dev())
        padded = run(lambda s, w, b: entity_line_pool(lines.pad(s, Ln), w, b, lines.to_mask(Ln, k)), c, dev())
        same(ragged, padded)


def test_pool_exact_tie_takes_the_lowest_position(monkeypatch):
    c = tie_case()                                                       # small integers: every sum exact in fp32, in any order
    calls = kernels_ran(monkeypatch)
    got = run(op_fn(lines_of(c["counts"])), c, dev())
    assert len(calls) == 1
    for a, r in zip(got, c["ref"]):
        assert torch.equal(a.cpu().double(), r)


def test_pool_no_line_at_all(monkeypatch):
    from recon_amd import entity_line_pool_ragged
    calls = kernels_ran(monkeypatch)
    c = case("empty_entities")
    weight, bias = c["weight"].to(dev()).requires_grad_(True), c["bias"].to(dev()).requires_grad_(True)
    states = torch.zeros(0, c["C"], device=dev(), requires_grad=True)
    out = entity_line_pool_ragged(states, lines_of([0, 0, 0]), weight, bias)
    assert len(calls) == 1 and out.shape == (3, c["E"]) and (out == -float('inf')).all()
    grads = torch.autograd.grad(entity_line_pool_ragged(states, lines_of([0, 0, 0]), weight, bias), [states, weight, bias],
                                torch.ones(3, c["E"], device=dev()))
    assert grads[0].shape == (0, c["C"]) and torch.count_nonzero(grads[1]) == 0 and torch.count_nonzero(grads[2]) == 0
    empty = entity_line_pool_ragged(states, lines_of([]), weight, bias)
    assert empty.shape == (0, c["E"]) and empty.is_cuda


def test_pool_strided_column_view_gives_the_contiguous_copys_bits(monkeypatch):
    from recon_amd import _lib
    calls = kernels_ran(monkeypatch)
    strides, real = [], _lib.rows_in_place
    monkeypatch.setattr(_lib, "rows_in_place", lambda *a, **k: (lambda r: strides.append(r[1]) or r)(real(*a, **k)))
    for name in ("fixture_widths", "empty_entities", "two_per_group"):
        c = case(name)
        L, C = c["states"].shape
        lines = lines_of(c["counts"])

        def view(leaf):
            wide = torch.full((L, C + 7), 99.0, device=dev())
            wide[:, 3:3 + C] = leaf
            return wide[:, 3:3 + C]
        del strides[:]
        got = run(op_fn(lines), c, dev(), states_of=view)
        assert strides == [C + 7, C + 7]                                 # read in place, forward and backward
        same(got, run(op_fn(lines), c, dev()))
    assert len(calls) == 6


def test_pool_second_backward_and_no_grad(monkeypatch):
    from recon_amd import entity_line_pool_ragged
    c = case("fixture_widths")
    lines = lines_of(c["counts"])
    leaves = [c[n].to(dev()).requires_grad_(True) for n in ("states", "weight", "bias")]
    out = entity_line_pool_ragged(leaves[0], lines, leaves[1], leaves[2])
    kept = out.clone()
    g = c["g_out"].to(dev())
    first = torch.autograd.grad(out, leaves, g, retain_graph=True)
    second = torch.autograd.grad(out, leaves, g, retain_graph=True)
    same(first, second)
    same([kept], [out])                                                 # the backward destroys nothing
    with torch.no_grad():
        plain = entity_line_pool_ragged(leaves[0], lines, leaves[1], leaves[2])
    assert plain.grad_fn is None
    same([plain], [out.detach()])
    U, E = out.shape
    peak, res = peak_bytes(lambda: entity_line_pool_ragged(leaves[0], lines, leaves[1], leaves[2]))
    assert res.grad_fn is not None and peak == (U * E * 4 + 511) // 512 * 512 + (U * E + 511) // 512 * 512      # the output and one byte per output


# ------------------------------------------------------------------------------------------------------------- the pool, C ABI
def _guarded(n, dtype, fill, held):
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev())
    held.append((flat, n))
    return flat[GUARD:GUARD + n]


def _intact(held):
    for flat, n in held:
        for part in (flat[:GUARD], flat[GUARD + n:]):
            assert bool(torch.isnan(part).all()) if flat.is_floating_point() else bool((part == 0x5A).all()), (flat.dtype, n)


def abi_run(c):
    """One forward and one backward through the C ABI, every output inside NaN-filled (bytes: 0x5A-filled) memory: the guards stay, and
    no output cell keeps its fill.  -> ([out, d_states, d_weight, d_bias], positions)."""
    from recon_amd import _lib
    lib, nan = _lib.lib(), float('nan')
    counts, C, E, k = c["counts"], c["C"], c["E"], c["k"]
    U, L, n_max = len(counts), sum(counts), max(counts)
    lines = lines_of(counts)
    states, weight, bias, g_out = (c[n].to(dev()).contiguous() for n in ("states", "weight", "bias", "g_out"))
    held = []
    out, pos = _guarded(U * E, torch.float32, nan, held), _guarded(U * E, torch.uint8, 0x5A, held)
    st = _lib.current_stream()
    _lib.check(lib.recon_line_pool_ragged_fwd(states.data_ptr(), C, weight.data_ptr(), bias.data_ptr(), lines.line_ptr.data_ptr(), U, L, n_max, C, E, k,
                                              out.data_ptr(), pos.data_ptr(), st), "recon_line_pool_ragged_fwd")
    nbytes = lib.recon_line_pool_ragged_workspace_bytes(U, L, n_max, C, E, k)
    assert nbytes > 0 and nbytes % 16 == 0
    g_s, g_w, g_b = _guarded(L * C, torch.float32, nan, held), _guarded(E * C * k, torch.float32, nan, held), _guarded(E, torch.float32, nan, held)
    ws = _guarded(nbytes, torch.uint8, 0x5A, held)
    assert ws.data_ptr() % 16 == 0
    _lib.check(lib.recon_line_pool_ragged_bwd(states.data_ptr(), C, weight.data_ptr(), g_out.data_ptr(), pos.data_ptr(), lines.line_ptr.data_ptr(), U, L,
                                              n_max, C, E, k, g_s.data_ptr(), g_w.data_ptr(), g_b.data_ptr(), ws.data_ptr(), nbytes, st),
               "recon_line_pool_ragged_bwd")
    torch.cuda.synchronize()
    _intact(held)
    for t in (out, g_s, g_w, g_b):
        assert not torch.isnan(t).any()                                  # every cell was written
    return [out.view(U, E).clone(), g_s.view(L, C).clone(), g_w.view(E, C, k).clone(), g_b.clone()], pos.view(U, E).clone()


@pytest.mark.parametrize("name", sorted(CASES))
def test_pool_through_the_c_abi(name):
    c = case(name)
    lines = lines_of(c["counts"])
    got, pos = abi_run(c)
    again, pos_again = abi_run(c)
    same(got + [pos], again + [pos_again])                               # twice, bit for bit
    bad = failures(got, run(chain_fn(lines), c, dev()), c["ref"], name + " (C ABI)")
    assert not bad, bad
    windows = torch.tensor([max(n - c["k"] + 1, 0) for n in c["counts"]], device=dev())
    assert bool(((pos == NONE) == (windows == 0)[:, None]).all()) and bool((pos[windows > 0] < windows[windows > 0][:, None]).all())
    same(got, run(op_fn(lines), c, dev()))                               # the Python entry runs the same kernels


def test_pool_c_abi_refuses_the_shape_past_the_position_byte():
    from recon_amd import _lib
    counts, C, E, k = REFUSED
    c = case("refused")
    lines = lines_of(counts)
    out = torch.full((E,), 7.0, device=dev())
    states, weight, bias = (c[n].to(dev()) for n in ("states", "weight", "bias"))
    rc = _lib.lib().recon_line_pool_ragged_fwd(states.data_ptr(), C, weight.data_ptr(), bias.data_ptr(), lines.line_ptr.data_ptr(), 1, 256, 256, C, E, k,
                                               out.data_ptr(), None, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == -2 and bool((out == 7.0).all())                         # nothing is written


def test_the_entries_are_declared_bound_and_cite_the_reference():
    entries_declared_and_bound(ENTRIES, CITES)
    entries_declared_and_bound(FILL_ENTRY, FILL_CITES)


# ------------------------------------------------------------------------------------------------------------- the batcher
MODES = (None, "all", "selected")
SENTINEL = {torch.int64: -7777, torch.int32: -7777, torch.float32: 12345.678, torch.bool: 0x5A}


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


def _agree(batcher, args, monkeypatch, index_dtype=torch.int64):
    """The ragged batch of the kernels against the padded batch of the torch path (the rows under ~mask, line_ptr, the sizes, every other
    field) and against the ragged batch of the torch path, exactly."""
    kernels, stock = _paths(monkeypatch)
    got = batcher.batch(*args, index_dtype=index_dtype, ragged_lines=True)
    assert (len(kernels), len(stock)) == (1, 0)
    np_dtype = np.int32 if index_dtype == torch.int32 else np.int64
    assert got.context_words.dtype == index_dtype and got.context_chars.dtype == index_dtype
    assert got.context_words.shape[0] == got.context_chars.shape[0] == got.context_mask.total
    padded = as_numpy(_torch_path(batcher, *args, index_dtype=index_dtype))
    assert ragged_differences(ragged_numpy(got), padded, np_dtype) == []
    ref, ref_lines = ragged_numpy(_torch_path(batcher, *args, index_dtype=index_dtype, ragged_lines=True))
    mine, lines = ragged_numpy(got)
    assert differences(dict(mine, mask=None), dict(ref, mask=None), index_dtype=np_dtype) == []
    assert torch.equal(lines.line_ptr.cpu(), ref_lines.line_ptr.cpu()) and (lines.U, lines.total, lines.n_max) == (ref_lines.U, ref_lines.total, ref_lines.n_max)
    return got


@pytest.mark.parametrize("layout", ("wikidata", "nyt"))
def test_fixture_through_the_kernels(layout, monkeypatch):
    from recon_amd import ContextBatcher, RaggedLines
    ds, g = fixture()
    all_sf = np.concatenate([sf for _, sf in ds["batches"]], axis=0)
    for mode in MODES:
        tables, surface_ids = build(ds, layout, all_sf, mode)
        batcher = ContextBatcher(tables.to(dev()))
        kernels, stock = _paths(monkeypatch)
        for b, (ids, _) in enumerate(ds["batches"]):
            args = to_device(ids, surface_ids[3 * b:3 * b + 3], dev())
            if mode == "all" and bool(g["b%d.gat_all_keyerror" % b]):
                with pytest.raises(KeyError):
                    batcher.batch(*args, ragged_lines=True)
                continue
            for index_dtype, np_dtype in ((torch.int64, np.int64), (torch.int32, np.int32)):
                batch = batcher.batch(*args, index_dtype=index_dtype, ragged_lines=True)
                assert isinstance(batch.context_mask, RaggedLines) and batch.model_args()[4] is batch.context_mask
                assert ragged_differences(ragged_numpy(batch), expected(g, layout, b, mode), np_dtype) == [], (layout, mode, b)
            # the padded call on the same ids returns what it returned: the header's seventh word is invisible to it
            assert differences(as_numpy(batcher.batch(*args)), expected(g, layout, b, mode)) == [], (layout, mode, b)
        assert len(kernels) == 3 * len(ds["batches"]) - 2 * (mode == "all") and not stock


def test_the_smallest_batch(monkeypatch):
    """One pair, both ids -1: one entity (ALL_ZERO), one line (its surface form)."""
    from recon_amd import ContextBatcher
    rng = np.random.default_rng(3)
    ds = random_dataset(rng, 4, 2, max_lines=3)
    ids = -np.ones((1, 1, 2), dtype=np.int64)
    sf = np.empty((1, 1, 2), dtype=object)
    sf[0, 0, 0] = sf[0, 0, 1] = ["ALL_ZERO"]
    for mode in MODES:
        tables, surface_ids = build(ds, "wikidata", sf, mode)
        for index_dtype in (torch.int64, torch.int32):
            got = _agree(ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev()), monkeypatch, index_dtype)
            assert got.context_mask.line_ptr.tolist() == [0, 1] and got.context_words.shape == (1, 1) and got.unique_entities.tolist() == [-1]


@pytest.fixture(scope="module")
def big():
    """One dataset at the reference's scale: 600 entities with up to 31 lines, G = 100."""
    rng = np.random.default_rng(7)
    return random_dataset(rng, 600, 100), rng


def test_the_references_batch(big, monkeypatch):
    from recon_amd import ContextBatcher
    ds, rng = big
    ids, sf = random_batch(rng, ds, 50, 72)
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    got = _agree(ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev()), monkeypatch)
    lines = got.context_mask
    assert got.context_chars.shape[1] == 386 and lines.U > 100 and lines.n_max == 32 and lines.U < lines.total < lines.U * 32


def test_random_batches_kernels_against_the_torch_path(monkeypatch):
    from recon_amd import ContextBatcher
    rng = np.random.default_rng(199)
    for trial in range(12):
        B, Cn, G = int(rng.choice([1, 3, 7, 20])), int(rng.choice([2, 6, 12])), int(rng.choice([1, 3, 100]))
        mode = MODES[trial % 3]
        layout = ("wikidata", "nyt")[trial % 2]
        ds = random_dataset(rng, int(rng.choice([5, 40, 200])), G, max_lines=int(rng.choice([0, 7, 31])), layout=layout)
        ids, sf = random_batch(rng, ds, B, Cn, pad_share=float(rng.choice([0.0, 0.3])))
        tables, surface_ids = build(ds, layout, sf, mode)
        _agree(ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev()), monkeypatch, (torch.int64, torch.int32)[trial % 2])


def test_a_full_hash_table_scans_8193_entities(monkeypatch):
    """MAX_IDS distinct ids: U = 8193, nine entities per thread of the scan."""
    from recon_amd import ContextBatcher
    from recon_amd.context_batch import MAX_IDS
    rng = np.random.default_rng(11)
    ds = random_dataset(rng, MAX_IDS + 8, 1, max_lines=2)
    ids, sf = random_batch(rng, ds, MAX_IDS // 128, 64, distinct=True, one_token=True)
    tables, surface_ids = build(ds, "wikidata", sf, None)
    got = _agree(ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev()), monkeypatch, torch.int32)
    assert got.context_mask.U == MAX_IDS + 1


@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32), ids=("int64", "int32"))
def test_every_cell_is_written_and_nothing_behind_row_L(big, index_dtype, monkeypatch):
    """Every buffer of a call lies inside sentinel-filled memory, behind a guard of 37 elements (so no base is 16-byte aligned) and in
    front of another: the guards stay — nothing is written behind row L — and the outputs equal the torch path's, so no cell kept its
    sentinel.  Twice, bit for bit."""
    from recon_amd import ContextBatcher, context_batch
    ds, rng = big
    ids, sf = random_batch(rng, ds, 5, 6)
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    batcher, args = ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev())
    np_dtype = np.int32 if index_dtype == torch.int32 else np.int64
    padded = as_numpy(_torch_path(batcher, *args, index_dtype=index_dtype))
    held, guard = [], 37

    def guarded(shape, dtype, device):
        n = int(np.prod(shape))
        raw = torch.uint8 if dtype == torch.bool else dtype
        flat = torch.full((n + 2 * guard,), SENTINEL[dtype], dtype=raw, device=device)
        held.append((flat, n, dtype))
        inner = flat[guard:guard + n]
        return (inner.view(torch.bool) if dtype == torch.bool else inner).view(shape)
    monkeypatch.setattr(context_batch, "_new", guarded)
    kernels, stock = _paths(monkeypatch)
    got = batcher.batch(*args, index_dtype=index_dtype, ragged_lines=True)
    again = batcher.batch(*args, index_dtype=index_dtype, ragged_lines=True)
    assert len(kernels) == 2 and not stock and len(held) >= 20
    for flat, n, dtype in held:
        sentinel = torch.full((guard,), SENTINEL[dtype], dtype=flat.dtype, device=flat.device)
        assert torch.equal(flat[:guard], sentinel) and torch.equal(flat[guard + n:], sentinel), (dtype, n)
    assert got.context_chars.data_ptr() % 16 != 0
    assert ragged_differences(ragged_numpy(got), padded, np_dtype) == []
    a, b = ragged_numpy(got), ragged_numpy(again)
    assert differences(dict(a[0], mask=None), dict(b[0], mask=None), index_dtype=np_dtype) == [] and torch.equal(a[1].line_ptr, b[1].line_ptr)
    row_ent = [flat[guard:guard + n] for flat, n, dtype in held if dtype == torch.int32 and n == got.context_mask.total][-1]
    u = torch.searchsorted(got.context_mask.line_ptr[1:].long().contiguous(), torch.arange(got.context_mask.total, device=dev()), right=True)
    assert index_dtype == torch.int32 or torch.equal(row_ent.long(), u)                    # the scan's row-to-entity map


# ------------------------------------------------------------------------------------------------------------- the encoder
def _encoder_reference(counts, words, chars, g_out, keep, monkeypatch):
    """[out, parameter gradients...] of the stock chain on the padded form: in float64 on the CPU (CPU tensors run the stock ops) and in
    float32 on the GPU with every fused op switched off; and the parameters' names."""
    from recon_amd import RaggedLines, char_features, context_lstm
    P = max(counts)
    res = []
    with monkeypatch.context() as mp:
        mp.setattr(char_features, "_runs", lambda *a, **k: False)
        mp.setattr(context_lstm, "_fused", lambda *a, **k: False)
        for dtype, device in ((torch.float64, torch.device("cpu")), (torch.float32, dev())):
            lines = RaggedLines.from_counts(counts, device)
            m = encoder(p=0.0 if keep is None else 0.5).to(dtype).to(device)
            m.fused_line_pool = False
            m.train(keep is not None)
            m.lstm.train()                                               # (the vendor LSTM has a backward in training mode only; no dropout inside it)
            if keep is not None:
                padded_keep = lines.pad(keep.to(device=device, dtype=dtype), P).reshape((-1,) + tuple(keep.shape[1:]))
                m.char_embeddings.draw_keep = lambda *a, padded_keep=padded_keep: padded_keep
            out = m(lines.pad(words.to(device), P), lines.pad(chars.to(device), P), lines.to_mask(P))
            finite = torch.isfinite(out.detach())
            (out.masked_fill(~finite, 0.0) * g_out.to(device=device, dtype=dtype)).sum().backward()
            named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
            res.append([out.detach().masked_fill(~finite, 0.0).cpu()] + [p.grad.cpu() for _, p in named])
    return res[0], res[1], ["out"] + [n for n, _ in named], finite.cpu()


def _encoder_case(L, monkeypatch, keep_p=None):
    from recon_amd import char_features, context_lstm, line_pool
    counts = ENCODER_COUNTS[L]
    lines = lines_of(counts)
    words, chars = encoder_inputs(counts)
    g_out = torch.randn(len(counts), 2, generator=torch.Generator().manual_seed(L))
    keep = None
    if keep_p is not None:                                               # recorded factors for the L rows: 0 or 1 / (1 - p)
        keep = (torch.rand(L, chars.shape[1], 3, generator=torch.Generator().manual_seed(7 + L)) >= keep_p).float() / (1 - keep_p)
    ref, chain, names, finite = _encoder_reference(counts, words, chars, g_out, keep, monkeypatch)
    m = encoder(p=0.0 if keep is None else keep_p).to(dev())
    m.train(keep is not None)
    if keep is not None:
        on_dev = keep.to(dev())
        m.char_embeddings.draw_keep = lambda *a: on_dev
    ran = [calls_of(monkeypatch, f, "apply") for f in (char_features._CharWordFeatures, context_lstm._ContextLineStates, line_pool._LinePoolRagged)]
    out = m(words.to(dev()), chars.to(dev()), lines)
    assert [len(r) for r in ran] == [0 if keep is not None else 1, 1, 1]      # the kernels ran, not the chains (recorded factors: the char op chain)
    assert torch.equal(torch.isfinite(out.detach()).cpu(), finite)
    (out.masked_fill(~finite.to(dev()), 0.0) * g_out.to(dev())).sum().backward()
    got = [out.detach().masked_fill(~finite.to(dev()), 0.0)] + [p.grad for _, p in m.named_parameters() if p.requires_grad]
    bad = band_failures(names, got, chain, ref, "EntityEmbedding ragged L = %d%s" % (L, "" if keep is None else " training"))
    assert not bad, bad


@pytest.mark.parametrize("L", sorted(ENCODER_COUNTS))
def test_encoder_eval_against_the_float64_stock_chain_on_the_padded_form(L, monkeypatch):
    _encoder_case(L, monkeypatch)


def test_encoder_training_with_replayed_dropout_factors(monkeypatch):
    _encoder_case(17, monkeypatch, keep_p=0.5)


def test_encoder_peak_memory_is_below_the_padded_calls():
    """A quarter of the lines present (one 32-line entity, so P_b = 32): forward + backward of the ragged call peaks strictly below the
    padded call's on the same entities."""
    counts = [32] + [6] * 9 + [7] * 6
    assert sum(counts) * 4 == len(counts) * 32
    lines = lines_of(counts)
    words, chars = (t.to(dev()) for t in encoder_inputs(counts, tokens=8))
    m = encoder().to(dev()).eval()
    padded = (lines.pad(words, 32), lines.pad(chars, 32), lines.to_mask(32))

    def step(*args):
        m.zero_grad(set_to_none=True)
        m(*args).sum().backward()
    ragged_peak, _ = peak_bytes(lambda: step(words, chars, lines))
    padded_peak, _ = peak_bytes(lambda: step(*padded))
    print("EntityEmbedding forward + backward peak: ragged %d bytes, padded %d bytes" % (ragged_peak, padded_peak))
    assert 0 < ragged_peak < padded_peak


# ------------------------------------------------------------------------------------------------------------- whole models
class _RaggedBatcher:
    """`run_epoch` calls batcher.batch(ids, surface_ids, index_dtype): the same batcher with ragged_lines=True."""

    def __init__(self, batcher):
        self.batcher = batcher

    def batch(self, entity_indices, surface_ids, index_dtype=torch.int64):
        return self.batcher.batch(entity_indices, surface_ids, index_dtype, ragged_lines=True)


def _eac():
    from recon_amd import ContextBatcher
    from recon_amd.gpgnn import RECON_EAC
    from stage_b_checks import dataset
    from tests.test_host_cpu import EAC_P
    g = load_golden("eac1_untied")
    p = dict(EAC_P, entity_conv_filter_size=1, batch_size=3)

    def make():
        torch.manual_seed(0)
        m = RECON_EAC(dict(p), g["emb"], 4, 3, list(range(int(g["n_chars"]))))
        own = m.state_dict()
        m.load_state_dict({k: v for k, v in state_dict_of(g).items() if k in own and own[k].shape == v.shape}, strict=False)
        return m.to(dev())
    rng = np.random.default_rng(6)
    ds = random_dataset(rng, 9, 3, max_lines=5, n_words=g["emb"].shape[0], n_chars=int(g["n_chars"]), conv_filter_size=EAC_P["conv_filter_size"])
    ids, sf = random_batch(rng, ds, 7, 6, pad_share=0.3)
    tables, surface_ids = build(ds, "wikidata", sf, None, max_char_len=EAC_P["max_char_len"])
    base, _ = dataset(7, 3, 4, seed=33, entity_arrays=False, n_words=g["emb"].shape[0], n_out=3)
    labels = np.where(ids[:, :, 0] == -1, 0, np.maximum(base[2], 1)).astype(np.int16)
    return make, (base[0], base[1], labels, base[3], ids.astype(np.int32), sf, None), surface_ids, ContextBatcher(tables.to(dev()))


@pytest.mark.parametrize("which", ("recon1_untied", "eac1_untied"))
def test_run_epoch_ragged_against_padded(which, monkeypatch):
    """N = 7 in batches of 3, dropout 0: two training iterations under Adam, then an evaluation pass with rows, once with the batcher's
    padded form and once with ragged_lines=True.  Losses and every parameter agree within `op_checks.close`'s defaults (the project's 1e-4
    parity bound; not bitwise: the weight-gradient slabs of the char-CNN and the line LSTM group other rows); counters, predictions and
    result rows are equal."""
    from recon_amd import EpochRows, RelationMetrics, StageBData, line_pool, run_epoch, stage_b
    from recon_amd.optim import Adam
    from stage_b_checks import permutation
    from test_stage_b_gpu import _recon
    make, as_indices, surface_ids, batcher = _recon(False) if which == "recon1_untied" else _eac()
    data = StageBData.from_indices(as_indices, surface_ids).to(dev())
    order = torch.from_numpy(permutation(7, 3)).to(dev())
    adam = lambda m: Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-2, weight_decay=1e-4, max_grad_norm=0.25)
    losses, real = [], stage_b.relation_objective

    def recorded(*a, **k):
        res = real(*a, **k)
        losses[-1].append(res.loss.detach().clone())
        return res
    monkeypatch.setattr(stage_b, "relation_objective", recorded)
    ragged_pool, padded_pool = calls_of(monkeypatch, line_pool._LinePoolRagged, "apply"), calls_of(monkeypatch, line_pool._LinePool, "apply")
    results = []
    for b in (batcher, _RaggedBatcher(batcher)):
        m = make().train()
        train, test, rows = RelationMetrics(dev()), RelationMetrics(dev()), EpochRows.for_data(data)
        losses.append([])
        run_epoch(m, data, 3, order=order, batcher=b, optimizer=adam(m), metrics=train)
        m.eval()
        run_epoch(m, data, 3, batcher=b, metrics=test, rows=rows)
        results.append((m, train.result(), test.result(), rows.result()))
    assert (len(padded_pool), len(ragged_pool)) == (4, 4) and len(losses[0]) == len(losses[1]) == 4
    (ma, train_a, test_a, rows_a), (mb, train_b, test_b, rows_b) = results
    for x, y in zip(losses[0], losses[1]):
        close(y.reshape(1), x.reshape(1), what="loss")
    changed = 0
    for (k, p), q, fresh in zip(ma.named_parameters(), mb.parameters(), make().parameters()):
        close(q, p, what=k)
        changed += int(p.requires_grad and not torch.equal(p, fresh))
    assert changed > 0                                                  # the two iterations trained something
    assert train_a[:4] == train_b[:4] and train_a.batches == train_b.batches == 2 and train_a.kept > 0
    assert abs(train_a.f1_sum - train_b.f1_sum) <= 1e-4 and abs(test_a.f1_sum - test_b.f1_sum) <= 1e-4
    assert test_a[:4] == test_b[:4] and test_a.batches == 2
    assert rows_a.pair.numel() == test_a.kept > 0
    for f in ("pair", "predicted", "gold"):
        assert torch.equal(getattr(rows_a, f), getattr(rows_b, f)), f
    close(rows_b.confidence, rows_a.confidence, what="confidence")
