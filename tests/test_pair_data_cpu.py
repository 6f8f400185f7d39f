"""recon_amd/pair_data.py on CPU tensors (the torch path): the fixture written from the reference's per-pair preprocessing and random
datasets through `PairData.take` against the plain-numpy restatement of tests/pair_data_checks.py, the wrong restatements each caught,
every rejection of `from_indices` and `check_model`, `EpochRows` at one pair per row, `run_epoch` over the fixtures' CNN, PCNN and LSTM
against the hand-written loop, and the new entries' declarations.  Everything is compared exactly: every value is selected or copied."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from op_checks import entries_declared_and_bound
from pair_data_checks import (FORMS, MODEL_FORMS, SHAPES, WRONG_TAKE, assert_epochs_equal, dataset, epoch_pair, extent, model_dataset, restate_take,
                              shape_dataset, shape_order, slice_differences)
from stage_b_checks import Outputs, join_rows, permutation, restate_collect, row_differences

CPU = torch.device("cpu")
NP = {torch.int64: np.int64, torch.int32: np.int32}


def _fixture(form):
    g = load_golden("pair_data1")
    a = [g[form + "_sentences"], g[form + "_markers"], g[form + "_labels"]]
    return a + ([g["segments_mask"]] if form == "segments" else []) + ([[("Q1", "Q2")] * len(a[2])] if form != "marks" else [])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("permuted", (False, True))
@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32))
def test_the_reference_arrays_through_take(form, permuted, index_dtype):
    """The arrays the reference's own preprocessing wrote, cut by numpy indexing with the reference's casts."""
    from recon_amd import PairData, PairSlice
    as_indices = _fixture(form)
    assert [a.dtype for a in as_indices[:3]] == [np.int32, np.int8, np.int16] and as_indices[0].shape == (10, 8)
    data = PairData.from_indices(as_indices)
    assert (data.N, data.T, data.form, data.device, data.kept_pairs) == (10, 8, form, CPU, int((as_indices[2] != 0).sum()))
    assert [data.arrays[k].dtype for k in ("sentences", "markers", "labels")] == [torch.int32, torch.int8, torch.int16]
    assert data.word_ids == (int(as_indices[0].min()), int(as_indices[0].max())) and data.marker_ids == (int(as_indices[1].min()), int(as_indices[1].max()))
    if form == "segments":
        m = as_indices[3]
        assert data.segment_bits.dtype == torch.uint8 and int(data.segment_bits.max()) < 8
        assert np.array_equal(data.segment_bits.numpy(), (m[:, 0] + 2 * m[:, 1] + 4 * m[:, 2]).astype(np.uint8))
        assert len(set(data.segment_bits.reshape(-1).tolist())) >= 5                    # overlapping planes and empty tails
    order = permutation(10, 5) if permuted else None
    for start, count in ((0, 10), (3, 4), (9, 1)):
        got = data.take(None if order is None else torch.from_numpy(order), start, count, index_dtype)
        assert isinstance(got, PairSlice) and len(got.model_args()) == (3 if form == "segments" else 2)
        assert got.sentence_input.dtype == got.entity_markers.dtype == index_dtype and got.labels.dtype == got.rows.dtype == torch.int64
        assert slice_differences(got, restate_take(as_indices, order, start, count, NP[index_dtype])) == []
    moved = data.to("cpu")
    assert (moved.kept_pairs, moved.word_ids, moved.marker_ids, moved.form) == (data.kept_pairs, data.word_ids, data.marker_ids, form)
    assert data.take(None, 0, 0).sentence_input.shape == (0, 8)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("form", FORMS)
def test_take_equals_the_restatement(shape, form):
    from recon_amd import PairData
    (count, T), (N, start) = SHAPES[shape], extent(shape)
    as_indices = shape_dataset(shape, form, seed=sorted(SHAPES).index(shape))
    data = PairData.from_indices(as_indices)
    for order in (None, shape_order(shape)):
        for index_dtype in (torch.int64, torch.int32):
            got = data.take(None if order is None else torch.from_numpy(order), start, count, index_dtype)
            assert got.entity_markers.shape == ((count, T) if form == "marks" else (count, 2, T))
            assert slice_differences(got, restate_take(as_indices, order, start, count, NP[index_dtype])) == []
    order = shape_order(shape)
    assert len(set(order.tolist())) < N and 0 in order[start:start + count] and (count < 2 or N - 1 in order[start:start + count])


def test_the_mask_bytes_cover_every_pattern():
    as_indices = shape_dataset("reference", "segments", seed=0)
    m = as_indices[3]
    bits = (m[:, 0] + 2 * m[:, 1] + 4 * m[:, 2]).astype(int)
    assert set(bits.reshape(-1).tolist()) == set(range(8)) and (bits[[0, 100]] == 0).all() and (bits[[172, 149]] == 7).all()


@pytest.mark.parametrize("wrong", WRONG_TAKE)
def test_a_wrong_slice_is_caught(wrong):
    from recon_amd import PairData
    as_indices = dataset(11, 5, "segments", seed=1)
    order, start, count = permutation(11, 3), 3, 3
    got = PairData.from_indices(as_indices).take(torch.from_numpy(order), start, count)
    assert slice_differences(got, restate_take(as_indices, order, start, count)) == []
    assert slice_differences(got, restate_take(as_indices, order, start, count, wrong=wrong)) != []


def test_from_indices_checks_its_arrays():
    from recon_amd import PairData
    as_indices = dataset(5, 4, "segments", seed=6)

    def changed(i, value):
        bad = list(as_indices)
        bad[i] = value
        return bad
    mask = as_indices[3].copy()
    mask[2, 1, 3] = 0.5
    with pytest.raises(ValueError, match="pcnn_mask"):
        PairData.from_indices(changed(3, mask))
    markers = as_indices[1].copy()
    markers[2, 1, 3] = -1
    with pytest.raises(ValueError, match="negative"):
        PairData.from_indices(changed(1, markers))
    with pytest.raises(ValueError, match="sentences"):
        PairData.from_indices(changed(0, as_indices[0].astype(np.int64) + 2 ** 31))     # a word id beyond int32
    with pytest.raises(ValueError, match="labels"):
        PairData.from_indices(changed(2, as_indices[2][:4]))
    with pytest.raises(ValueError, match="markers"):
        PairData.from_indices(changed(1, as_indices[1][:, :, :3]))
    with pytest.raises(ValueError, match="pcnn_mask"):
        PairData.from_indices(changed(3, as_indices[3][:, :2]))
    with pytest.raises(ValueError, match="pcnn_mask"):
        PairData.from_indices(dataset(5, 4, "marks", seed=6) + [as_indices[3]])          # a mask beside [N, T] markers
    with pytest.raises(ValueError, match="got 2 arrays"):
        PairData.from_indices(as_indices[:2] + [as_indices[4]])                          # fewer than three arrays: the pair list does not count
    with pytest.raises(TypeError):
        PairData.from_indices(changed(0, as_indices[0].astype(np.float32)))
    with pytest.raises(TypeError):
        PairData.from_indices(changed(3, as_indices[3].astype(np.int32)))
    wide = PairData.from_indices([a.astype(np.int64) for a in as_indices[:3]] + [as_indices[3].astype(np.float64)])   # wider types that fit
    assert wide.markers.dtype == torch.int8 and wide.form == "segments" and torch.equal(wide.segment_bits, PairData.from_indices(as_indices).segment_bits)


def test_take_argument_errors():
    from recon_amd import PairData
    data = PairData.from_indices(dataset(7, 5, "positions", seed=8))
    for value in (7, -1, 2 ** 40):
        order = torch.arange(7)
        order[4] = value
        with pytest.raises(IndexError):
            data.take(order, 3, 3)
    with pytest.raises(IndexError):
        data.take(None, 5, 3)
    with pytest.raises(TypeError):
        data.take(torch.arange(7, dtype=torch.int32), 0, 3)
    with pytest.raises(TypeError):
        data.take(None, 0, 3, torch.int16)


@pytest.mark.parametrize("name", sorted(MODEL_FORMS))
def test_check_model_names_the_array(name):
    from recon_amd import PairData
    from sentence_conv_checks import baseline_fixture
    model = baseline_fixture(name)[0]
    as_indices = model_dataset(name)
    PairData.from_indices(as_indices).check_model(model)                                 # 11 words, 4 marks or 19 positions: every id has its row
    words = as_indices[0].copy()
    words[3, 2] = 11
    with pytest.raises(ValueError, match=r"sentences .*word_embedding.*\[0, 11\)"):
        PairData.from_indices([words] + as_indices[1:]).check_model(model)
    markers = as_indices[1].copy()
    markers.reshape(-1)[5] = 4 if name == "lstm_baseline1" else 19
    with pytest.raises(ValueError, match=r"markers .*pos_embedding"):
        PairData.from_indices([as_indices[0], markers] + as_indices[2:]).check_model(model)
    other = baseline_fixture("cnn1" if name == "lstm_baseline1" else "lstm_baseline1")[0]
    with pytest.raises(ValueError, match="pos_embedding"):
        PairData.from_indices(as_indices).check_model(other)                             # another form's model


def test_run_epoch_refuses_a_batcher_and_checks_the_model():
    from recon_amd import PairData, run_epoch
    from sentence_conv_checks import baseline_fixture
    model = baseline_fixture("cnn1")[0]
    as_indices = model_dataset("cnn1")
    with pytest.raises(ValueError, match="batcher"):
        run_epoch(model, PairData.from_indices(as_indices), 3, batcher=object())
    words = as_indices[0].copy()
    words[9, 0] = 11                                                                     # in the dropped tail: still the dataset's
    with pytest.raises(ValueError, match="sentences"):
        run_epoch(model, PairData.from_indices([words] + as_indices[1:]), 3)


def test_epoch_rows_at_one_pair_per_row():
    """`pair` is the dataset row: what test.py:297-302 index the entity pairs with."""
    from recon_amd import EpochRows, PairData
    as_indices = dataset(23, 4, "positions", seed=12, kept_share=0.6)
    data = PairData.from_indices(as_indices)
    order = permutation(23, 9)
    rows, parts = EpochRows.for_data(data), []
    assert rows.capacity == data.kept_pairs == int((as_indices[2] != 0).sum())
    rng = np.random.default_rng(0)
    for start, count in ((0, 9), (9, 5), (14, 9)):
        sl = data.take(torch.from_numpy(order), start, count)
        predicted, confidence = rng.integers(0, 7, count).astype(np.int64), rng.random(count).astype(np.float32)
        rows.append(Outputs(predicted, confidence, CPU), sl)
        parts.append(restate_collect(as_indices[2][order[start:start + count]].astype(np.int64), predicted, confidence, order[start:start + count], 1))
    got = rows.result()
    assert got.pair.numel() == data.kept_pairs and row_differences(got, join_rows(parts)) == []
    assert np.array_equal(got.pair.numpy(), order[as_indices[2][order] != 0])


@pytest.mark.parametrize("name", sorted(MODEL_FORMS))
def test_run_epoch_against_the_hand_written_loop(name):
    """The stock fallbacks on the CPU: three Adam steps and a test pass, both loops the same ops on the same values in the same order."""
    adam = lambda m: torch.optim.Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-2, weight_decay=1e-4)
    assert_epochs_equal(*epoch_pair(name, CPU, adam))


def test_entries_are_declared_and_bound():
    entries_declared_and_bound(("recon_pair_slice",), "train.py:247-249")
    entries_declared_and_bound(("recon_pair_slice_supported",), "recon_pair_slice")
