"""recon_amd/pair_data.py through csrc/stage_b.hip (k_sb_slice<5, true>): `take` at the shapes of tests/pair_data_checks.py, through the
Python entry and through the C ABI, against the torch path on the same device and the numpy restatement, every output inside
sentinel-filled memory behind a guard of 37 elements, two runs bit for bit; the clamp and the rejections of the ABI; `EpochRows` fed with
PairSlices; a whole `run_epoch` over the fixtures' CNN, PCNN and LSTM against the hand-written loop; and `ids_prechecked()`.  Everything
is compared exactly: every value is selected or copied."""
import numpy as np
import pytest
import torch

from op_checks import calls_of, dev
from pair_data_checks import (FORMS, MODEL_FORMS, SHAPES, assert_epochs_equal, epoch_pair, extent, restate_take, shape_dataset, shape_order,
                              slice_differences)
from stage_b_checks import Outputs, batch_outputs, join_rows, restate_collect, row_differences

pytestmark = pytest.mark.gpu
SENTINEL = {torch.int64: -7777, torch.int32: -7777, torch.float32: 12345.678}
GUARD = 37
NP = {torch.int64: np.int64, torch.int32: np.int32}


def _guarded(monkeypatch, modules):
    """Every buffer of the modules' `_new` inside sentinel-filled memory, a guard of 37 elements in front (so no base is 16-byte aligned)
    and another behind; returns the list of (flat, n, dtype), the allocator and the check that the guards are intact."""
    held = []

    def guarded(shape, dtype, device):
        n = int(np.prod(shape))
        flat = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=device)
        held.append((flat, n, dtype))
        return flat[GUARD:GUARD + n].view(shape)
    for module in modules:
        monkeypatch.setattr(module, "_new", guarded)

    def intact():
        for flat, n, dtype in held:
            sentinel = torch.full((GUARD,), SENTINEL[dtype], dtype=dtype, device=flat.device)
            assert torch.equal(flat[:GUARD], sentinel) and torch.equal(flat[GUARD + n:], sentinel), (dtype, n)
    return held, guarded, intact


def _torch_path(fn):
    from recon_amd import pair_data
    prev, pair_data._KERNELS = pair_data._KERNELS, False
    try:
        return fn()
    finally:
        pair_data._KERNELS = prev


@pytest.fixture(scope="module")
def datasets():
    """One dataset per shape and form, on the host and on the device, shared by the cases and left unchanged."""
    from recon_amd import PairData
    out = {}
    for i, shape in enumerate(sorted(SHAPES)):
        for form in FORMS:
            as_indices = shape_dataset(shape, form, seed=i)
            out[shape, form] = (as_indices, PairData.from_indices(as_indices).to(dev()))
    return out


def _orders(shape):
    (count, _), (N, start) = SHAPES[shape], extent(shape)
    assert start > 0 and start + count <= N
    return (None, shape_order(shape))


def _check_take(datasets, shape, form, index_dtype, monkeypatch, kernels):
    from recon_amd import PairData, pair_data
    (count, T), (N, start) = SHAPES[shape], extent(shape)
    as_indices, data = datasets[shape, form]
    for order in _orders(shape):
        order_d = None if order is None else torch.from_numpy(order).to(dev())
        ref = _torch_path(lambda: data.take(order_d, start, count, index_dtype))
        with monkeypatch.context() as mp:
            held, _, intact = _guarded(mp, (pair_data,))
            kernel, stock = calls_of(mp, PairData, "_take_kernel"), calls_of(mp, PairData, "_take_torch")
            got = data.take(order_d, start, count, index_dtype)
            again = data.take(order_d, start, count, index_dtype)
            assert (len(kernel), len(stock)) == ((2, 0) if kernels else (0, 2))
            if kernels:
                assert len(held) == 2 * (5 if form == "segments" else 4)
                intact()
                assert got.entity_markers.data_ptr() % 16 != 0 and got.rows.data_ptr() % 16 != 0
        assert got.sentence_input.dtype == index_dtype and got.entity_markers.shape == ((count, T) if form == "marks" else (count, 2, T))
        assert (got.pcnn_mask is None) == (form != "segments")
        assert slice_differences(got, ref) == []                        # the outputs equal the torch path's: no cell kept its sentinel
        assert slice_differences(got, restate_take(as_indices, order, start, count, NP[index_dtype])) == []
        assert slice_differences(got, again) == []                      # two runs, bit for bit


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32))
def test_take_through_the_kernel(datasets, shape, form, index_dtype, monkeypatch):
    _check_take(datasets, shape, form, index_dtype, monkeypatch, kernels=True)


@pytest.mark.parametrize("form", FORMS)
def test_take_on_the_torch_path_when_the_kernels_are_off(datasets, form, monkeypatch):
    """`_KERNELS = False`: the same checks pass, and no kernel ran."""
    from recon_amd import pair_data
    monkeypatch.setattr(pair_data, "_KERNELS", False)
    for shape in sorted(SHAPES):
        for index_dtype in (torch.int64, torch.int32):
            _check_take(datasets, shape, form, index_dtype, monkeypatch, kernels=False)


def _abi_take(L, data, order_d, start, count, index_dtype, new, N=None):
    """recon_pair_slice itself, its outputs from `new` -> (status, dict over the slice's fields)."""
    from recon_amd import _lib
    T, two = data.T, data.marker_rows == 2
    out = {"sentence_input": new((count, T), index_dtype, dev()), "entity_markers": new((count, 2, T) if two else (count, T), index_dtype, dev()),
           "pcnn_mask": None if data.segment_bits is None else new((count, 3, T), torch.float32, dev()),
           "labels": new((count,), torch.int64, dev()), "rows": new((count,), torch.int64, dev())}
    status = L.recon_pair_slice(data.sentences.data_ptr(), data.markers.data_ptr(), data.labels.data_ptr(), _lib.ptr(data.segment_bits),
                                data.N if N is None else N, data.marker_rows, T, _lib.ptr(order_d), 0 if order_d is None else order_d.numel(), start,
                                count, 8 if index_dtype == torch.int64 else 4, out["sentence_input"].data_ptr(), out["entity_markers"].data_ptr(),
                                _lib.ptr(out["pcnn_mask"]), out["labels"].data_ptr(), out["rows"].data_ptr(), _lib.current_stream())
    torch.cuda.synchronize()
    return status, {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32))
def test_take_through_the_c_abi(datasets, shape, form, index_dtype, monkeypatch):
    from recon_amd import _lib, pair_data
    L = _lib.lib()
    (count, T), (N, start) = SHAPES[shape], extent(shape)
    as_indices, data = datasets[shape, form]
    assert L.recon_pair_slice_supported(count, data.marker_rows, T) == 1
    for order in _orders(shape):
        order_d = None if order is None else torch.from_numpy(order).to(dev())
        held, new, intact = _guarded(monkeypatch, (pair_data,))
        status, got = _abi_take(L, data, order_d, start, count, index_dtype, new)
        assert status == 0 and len(held) == (5 if form == "segments" else 4)
        intact()
        assert slice_differences(got, restate_take(as_indices, order, start, count, NP[index_dtype])) == []
        assert slice_differences(got, _abi_take(L, data, order_d, start, count, index_dtype, new)[1]) == []
        intact()


@pytest.mark.parametrize("form", FORMS)
def test_the_abi_clamps_what_it_reads_from_an_order(datasets, form, monkeypatch):
    """-5 reads row 0 and N + 3 reads row N - 1: a value of `order` never becomes an address (the Python entry validates it first)."""
    from recon_amd import _lib, pair_data
    as_indices, data = datasets["unaligned", form]
    N = data.N
    order = np.asarray([2, -5, N + 3, 1, N - 1, 0], dtype=np.int64)
    held, new, intact = _guarded(monkeypatch, (pair_data,))
    status, got = _abi_take(_lib.lib(), data, torch.from_numpy(order).to(dev()), 1, 4, torch.int64, new)
    assert status == 0
    intact()
    assert slice_differences(got, restate_take(as_indices, np.clip(order, 0, N - 1), 1, 4)) == []
    assert got["rows"].tolist() == [0, N - 1, 1, N - 1]


def test_status_codes_before_any_launch():
    from recon_amd import _lib
    L = _lib.lib()
    ok = L.recon_pair_slice_supported
    assert ok(50, 1, 36) and ok(50, 2, 36) and ok(1, 1, 1)
    assert not ok(0, 2, 36) and not ok(50, 0, 36) and not ok(50, 3, 36) and not ok(50, 2, 0) and not ok(-1, 2, 36)
    assert 19884069 * 3 * 36 < 2 ** 31 - 4096 <= 19884070 * 3 * 36 and ok(19884069, 2, 36) and not ok(19884070, 2, 36)
    assert ok(19884069, 1, 36) and not ok(19884070, 1, 36)             # one bound for every form: the mask's 3 count T cells
    assert ok(1, 2, (2 ** 31 - 4096) // 3 - 1) and not ok(1, 2, (2 ** 31 - 4096) // 3 + 1)
    fake = 16                                                          # never dereferenced: every call below returns before a launch

    def cut(sent=fake, bits=fake, mask=fake, N=173, R=2, T=36, order=None, order_len=0, start=0, count=50, nbytes=8, out=fake, labels=fake, rows=fake):
        return L.recon_pair_slice(sent, fake, fake, bits, N, R, T, order, order_len, start, count, nbytes, out, fake, mask, labels, rows, None)
    assert cut(sent=None) == -1 and cut(out=None) == -1 and cut(labels=None) == -1 and cut(rows=None) == -1
    assert cut(bits=None) == -1 and cut(mask=None) == -1              # the bits and the mask: both or neither
    assert cut(count=0) == -1 and cut(count=-2) == -1 and cut(start=-1) == -1 and cut(N=0) == -1 and cut(T=0) == -1
    assert cut(R=0) == -1 and cut(R=3) == -1 and cut(nbytes=2) == -1 and cut(out=20) == -1 and cut(mask=18) == -1 and cut(rows=20) == -1
    assert cut(start=124) == -1 and cut(order=fake, order_len=49) == -1 and cut(order=fake, order_len=173, start=124) == -1   # rows outside the array
    assert cut(N=2 ** 25, count=19884070) == -2 and cut(N=2 ** 40, count=19884070, order=fake, order_len=2 ** 25) == -2     # the size over the limit
    torch.cuda.synchronize()                                           # nothing was launched: nothing can have faulted


# ------------------------------------------------------------------------------------------------------------- the result rows
def _pair_slice(labels, rows):
    from recon_amd import PairSlice
    return PairSlice(None, None, None, torch.from_numpy(labels).to(dev()), torch.from_numpy(rows).to(dev()))


@pytest.mark.parametrize("M", (1, 1023, 1024, 1025))
def test_epoch_rows_take_a_pair_slice(M, monkeypatch):
    """One pair per row: `pair` = rows[m].  The collector's chunk of 1024 from both sides."""
    from recon_amd import EpochRows, stage_b
    labels, predicted, confidence, _ = batch_outputs(M, 5, 0.5, seed=M, C=1)
    rows = np.random.default_rng(M).permutation(M + 9)[:M].astype(np.int64)
    want = restate_collect(labels, predicted, confidence, rows, 1)
    held, _, intact = _guarded(monkeypatch, (stage_b,))
    kernel = calls_of(monkeypatch, EpochRows, "_append_kernel")
    r = EpochRows(M, dev())
    r.append(Outputs(predicted, confidence, dev()), _pair_slice(labels, rows))
    assert len(kernel) == 1 and len(held) == 4
    got = r.result()
    intact()
    assert row_differences(got, want) == [] and np.array_equal(got.pair.cpu().numpy(), rows[labels != 0])


def test_epoch_rows_at_the_capacity_and_one_past_it(monkeypatch):
    from recon_amd import EpochRows, stage_b
    batches = []
    for i, M in enumerate((1025, 50, 7)):
        labels, predicted, confidence, _ = batch_outputs(M, 4, 0.4, seed=20 + i, C=1)
        batches.append((labels, predicted, confidence, np.arange(100 * i, 100 * i + M, dtype=np.int64)))
    parts = [restate_collect(*b, 1) for b in batches]
    total = sum(len(p["pair"]) for p in parts)
    held, _, intact = _guarded(monkeypatch, (stage_b,))
    exact, short = EpochRows(total, dev()), EpochRows(total - 1, dev())
    for labels, predicted, confidence, rows in batches:
        for r in (exact, short):
            r.append(Outputs(predicted, confidence, dev()), _pair_slice(labels, rows))
    assert row_differences(exact.result(), join_rows(parts)) == []      # the capacity met exactly
    with pytest.raises(OverflowError, match=r"%d rows.*%d" % (total, total - 1)):
        short.result()                                                  # exceeded by one
    intact()                                                            # nothing was written at or beyond the capacity
    assert np.array_equal(short.pair.cpu().numpy(), join_rows(parts)["pair"][:total - 1])


# ------------------------------------------------------------------------------------------------------------- a whole epoch
def _adam(m):
    from recon_amd.optim import Adam
    return Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-2, weight_decay=1e-4, max_grad_norm=0.25)


@pytest.mark.parametrize("name", sorted(MODEL_FORMS))
@pytest.mark.parametrize("dropout", (False, True))
def test_run_epoch_against_the_hand_written_loop(name, dropout, monkeypatch):
    """N = 10 in batches of 3 with the fused ops on: three training iterations under recon_amd.optim.Adam(max_grad_norm=0.25), then a test
    pass with rows.  Both loops run the same deterministic ops on the same values in the same order."""
    from recon_amd import PairData, sentence_conv
    from recon_amd.sentence_conv import _SentenceConvPool
    kernel = calls_of(monkeypatch, PairData, "_take_kernel")
    fused = calls_of(monkeypatch, _SentenceConvPool, "apply")
    entered = calls_of(monkeypatch, sentence_conv, "_read_words")
    assert_epochs_equal(*epoch_pair(name, dev(), _adam, dropout=dropout))
    assert len(kernel) == 6 and len(entered) == 2                       # run_epoch's two passes; one read of the status words behind each
    assert len(fused) == (0 if name == "lstm_baseline1" else 12)        # both loops went through the fused sentence convolution


# ------------------------------------------------------------------------------------------------------------- the id check
def test_ids_prechecked_reads_the_word_where_the_context_ends(monkeypatch):
    """Inside the context a word id equal to V reads row 0 and does not raise; leaving raises and clears the word; a plain forward with
    valid ids then passes.  The kernels are built for this input: an outside id is never used as an address."""
    from recon_amd import _lib, sentence_conv, sentence_conv_pool
    from recon_amd.sentence_conv import _SentenceConvPool, ids_prechecked
    g = torch.Generator().manual_seed(3)
    B, T, V, Dw, P, Dp, E = 2, 5, 6, 4, 11, 2, 3
    r = lambda *shape: torch.randn(*shape, generator=g).to(dev())
    word_table, p0, p1, w, b = r(V, Dw), r(P, Dp), r(P, Dp), [r(E, Dw + 2 * Dp, 3)], [r(E)]
    sentence = torch.randint(1, V, (B, T), generator=g).to(dev())
    positions = torch.randint(0, P, (B, 2, T), generator=g).to(dev())
    outside, row0 = sentence.clone(), sentence.clone()
    outside[1, 2], row0[1, 2] = V, 0
    fused = calls_of(monkeypatch, _SentenceConvPool, "apply")
    run = lambda s: sentence_conv_pool(s, positions, word_table, p0, p1, w, b, activation="tanh")
    want = run(row0)
    with pytest.raises(ValueError, match=r"outside \[0, 6\)"):
        with ids_prechecked():
            got = run(outside)                                          # does not raise here
            again = run(sentence)                                       # nor does a later forward clear what the first one set
            assert torch.equal(got, want) and len(fused) == 3
    word = sentence_conv._status(dev(), _lib.current_stream())
    assert int(word) == 0                                               # cleared on the way out
    assert torch.equal(run(sentence), again)                            # the next plain forward passes
    with ids_prechecked():
        run(sentence)                                                   # valid ids: leaving raises nothing
    with pytest.raises(ValueError, match=r"outside \[0, 6\)"):
        run(outside)                                                    # outside the context nothing changed: the forward itself raises
    assert int(word) == 0 and len(fused) == 6
