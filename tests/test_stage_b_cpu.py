"""recon_amd/stage_b.py on CPU tensors (the torch path): `take`, `EpochRows` and `run_epoch` against the plain-numpy restatements of
tests/stage_b_checks.py, the wrong restatements each caught, and the new entries' declarations and status codes.  Everything is compared
exactly: every value is selected or copied."""
import copy

import numpy as np
import pytest
import torch

from op_checks import entries_declared_and_bound
from stage_b_checks import (SHAPES, WRONG_COLLECT, WRONG_TAKE, Outputs, Rows, batch_outputs, dataset, join_rows, permutation, restate_collect,
                            restate_take, row_differences, slice_differences)

CPU = torch.device("cpu")


def _order(N, permuted, seed=3):
    return permutation(N, seed) if permuted else None


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("permuted", (False, True))
@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32))
def test_take_equals_the_restatement(shape, permuted, index_dtype):
    from recon_amd import StageBData, StageBSlice
    N, n, T, count, start = SHAPES[shape]
    as_indices, surface_ids = dataset(N, n, T, seed=sorted(SHAPES).index(shape))
    data = StageBData.from_indices(as_indices, surface_ids)
    assert (data.N, data.C, data.T) == (N, n * (n - 1), T) and data.kept_pairs == int((as_indices[2] != 0).sum())
    assert [data.arrays[k].dtype for k in ("sentences", "markers", "labels", "num_entities", "entity_indices", "surface_ids")] == \
        [torch.int32, torch.int8, torch.int16, torch.int32, torch.int32, torch.int32]
    order = _order(N, permuted)
    got = data.take(None if order is None else torch.from_numpy(order), start, count, index_dtype)
    assert isinstance(got, StageBSlice)
    want = restate_take(as_indices, surface_ids, order, start, count, np.int32 if index_dtype == torch.int32 else np.int64)
    assert slice_differences(got, want) == []
    assert got.labels.shape == (count * n * (n - 1),) and got.entity_indices.dtype == torch.int64 and got.surface_ids.dtype == torch.int32


def test_take_without_the_entity_arrays():
    from recon_amd import StageBData
    N, n, T, count, start = SHAPES["last_batch"]
    as_indices, _ = dataset(N, n, T, seed=9, entity_arrays=False)
    data = StageBData.from_indices(as_indices)
    order = _order(N, True)
    got = data.take(torch.from_numpy(order), start, count)
    assert got.entity_indices is None and got.surface_ids is None
    assert slice_differences(got, restate_take(as_indices, None, order, start, count)) == []
    assert data.take(None, 0, 0).sentence_input.shape == (0, T)


@pytest.mark.parametrize("wrong", WRONG_TAKE)
def test_a_wrong_slice_is_caught(wrong):
    from recon_amd import StageBData
    N, n, T, count, start = SHAPES["last_batch"]
    as_indices, surface_ids = dataset(N, n, T, seed=1)
    order = _order(N, True)
    got = StageBData.from_indices(as_indices, surface_ids).take(torch.from_numpy(order), start, count)
    assert slice_differences(got, restate_take(as_indices, surface_ids, order, start, count)) == []
    assert slice_differences(got, restate_take(as_indices, surface_ids, order, start, count, wrong=wrong)) != []


def _append(rows_obj, labels, predicted, confidence, rows, device=CPU):
    rows_obj.append(Outputs(predicted, confidence, device), Rows(labels, rows, device))


@pytest.mark.parametrize("wrong", WRONG_COLLECT)
def test_a_wrong_collector_is_caught(wrong):
    from recon_amd import EpochRows
    labels, predicted, confidence, rows = batch_outputs(24, 3, 0.5, seed=2, C=6)
    assert 1 < int((labels != 0).sum()) < 24
    r = EpochRows(24, CPU)
    _append(r, labels, predicted, confidence, rows)
    assert row_differences(r.result(), restate_collect(labels, predicted, confidence, rows, 6)) == []
    assert row_differences(r.result(), restate_collect(labels, predicted, confidence, rows, 6, wrong=wrong)) != []


def test_epoch_rows_appends_reset_and_capacity():
    from recon_amd import EpochRows
    batches = [batch_outputs(M, 4, 0.5, seed=10 + i, C=C) for i, (M, C) in enumerate(((12, 6), (18, 6), (6, 6)))]
    parts = [restate_collect(*b, 6) for b in batches]
    total = sum(len(p["pair"]) for p in parts)
    r = EpochRows(total + 3, CPU)
    for b in batches:
        _append(r, *b)
    got = r.result()
    assert got.pair.dtype == torch.int64 and got.confidence.dtype == torch.float32
    assert row_differences(got, join_rows(parts)) == []
    r.reset()
    assert r.result().pair.numel() == 0
    _append(r, *batches[1])
    assert row_differences(r.result(), parts[1]) == []
    exact = EpochRows(total, CPU)                                       # the capacity met exactly
    for b in batches:
        _append(exact, *b)
    assert row_differences(exact.result(), join_rows(parts)) == []
    short = EpochRows(total - 1, CPU)                                   # exceeded by one
    for b in batches:
        _append(short, *b)
    with pytest.raises(OverflowError, match=r"%d rows.*%d" % (total, total - 1)):
        short.result()
    assert np.array_equal(short.pair.numpy(), join_rows(parts)["pair"][:total - 1])
    short.reset()
    _append(short, *batches[2])
    assert row_differences(short.result(), parts[2]) == []


def test_for_data_sizes_to_the_kept_pairs():
    from recon_amd import EpochRows, StageBData
    as_indices, surface_ids = dataset(7, 3, 5, seed=4)
    data = StageBData.from_indices(as_indices, surface_ids)
    assert EpochRows.for_data(data).capacity == int((as_indices[2] != 0).sum())


def test_from_indices_checks_its_arrays():
    from recon_amd import StageBData
    as_indices, surface_ids = dataset(5, 3, 4, seed=6)
    bad = list(as_indices)
    bad[1] = as_indices[1].copy()
    bad[1][2, 1, 3] = -1
    with pytest.raises(ValueError):
        StageBData.from_indices(tuple(bad), surface_ids)
    bad = list(as_indices)
    bad[2] = as_indices[2][:4]
    with pytest.raises(ValueError):
        StageBData.from_indices(tuple(bad), surface_ids)
    bad = list(as_indices)
    bad[0] = as_indices[0].astype(np.float32)
    with pytest.raises(TypeError):
        StageBData.from_indices(tuple(bad), surface_ids)
    bad = list(as_indices)
    bad[0] = as_indices[0].astype(np.int64) + 2 ** 40
    with pytest.raises(ValueError):
        StageBData.from_indices(tuple(bad), surface_ids)
    with pytest.raises(ValueError):
        StageBData.from_indices(as_indices[:4], surface_ids)
    wide = StageBData.from_indices(tuple(a.astype(np.int64) for a in as_indices[:5]), surface_ids.astype(np.int64))   # wider integers that fit
    assert wide.markers.dtype == torch.int8 and torch.equal(wide.entity_indices, torch.from_numpy(as_indices[4]))


class Stub(torch.nn.Module):
    """Three inputs -> [count C, n_out] logits through two small trainable tables."""

    def __init__(self, n_words, n_out):
        super().__init__()
        torch.manual_seed(0)
        self.words, self.marks = torch.nn.Embedding(n_words, n_out), torch.nn.Embedding(4, n_out)
        self.seen = []

    def forward(self, sentence_input, entity_markers, num_entities):
        self.seen.append(tuple(sentence_input.shape))
        x = self.words(sentence_input).mean(dim=1)[:, None, :] + self.marks(entity_markers).sum(dim=2) + num_entities[:, None, None].float() * 0.01
        return x.reshape(-1, x.shape[-1])


@pytest.mark.parametrize("permuted", (False, True))
def test_run_epoch_against_the_loop_written_out(permuted):
    from recon_amd import EpochRows, RelationMetrics, StageBData, relation_objective, run_epoch
    N, n, T, bs, n_out = 7, 3, 5, 3, 4
    as_indices, _ = dataset(N, n, T, seed=8, entity_arrays=False, n_words=20, n_out=n_out)
    order = _order(N, permuted)
    indices = np.arange(N) if order is None else order
    a, b = Stub(20, n_out), None
    b = copy.deepcopy(a)
    b.seen = []
    # ---- the loop of train.py:244-325 and test.py:285-302, written out
    opt_b, m_b, parts = torch.optim.SGD(b.parameters(), lr=0.1), RelationMetrics(CPU), []
    for i in range(int(N / bs)):
        rows = indices[i * bs:(i + 1) * bs]
        opt_b.zero_grad()
        out = b(torch.from_numpy(as_indices[0][rows].astype(int)), torch.from_numpy(as_indices[1][rows].astype(int)), torch.from_numpy(as_indices[3][rows]))
        labels = as_indices[2][rows]
        res = relation_objective(out, torch.from_numpy(labels.astype(int)).view(-1), ignore_index=0, empty_label=1, metrics=m_b)
        res.loss.backward()
        opt_b.step()
        parts.append(restate_collect(labels.reshape(-1), res.predicted.numpy(), res.confidence.detach().numpy(), rows, n * (n - 1)))
    # ---- run_epoch
    data = StageBData.from_indices(as_indices)
    m_a, rows_a = RelationMetrics(CPU), EpochRows.for_data(data)
    assert run_epoch(a, data, bs, order=None if order is None else torch.from_numpy(order), optimizer=torch.optim.SGD(a.parameters(), lr=0.1),
                     metrics=m_a, rows=rows_a) is None
    assert a.seen == b.seen == [(bs, T)] * 2                            # the tail of one sentence is dropped
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k
    assert m_a.result() == m_b.result() and m_a.result().batches == 2
    assert row_differences(rows_a.result(), join_rows(parts)) == []
    # ---- without an optimizer: no_grad, nothing trained
    before = [p.clone() for p in a.parameters()]
    run_epoch(a, data, bs, metrics=m_a)
    assert all(torch.equal(p, q) and p.grad is not None for p, q in zip(a.parameters(), before)) and m_a.result().batches == 4


def test_an_order_outside_the_dataset_raises():
    from recon_amd import StageBData, run_epoch
    as_indices, _ = dataset(7, 3, 5, seed=8, entity_arrays=False, n_words=20)
    data, model = StageBData.from_indices(as_indices), Stub(20, 4)
    for value in (7, -1, 2 ** 40):
        order = torch.arange(7)
        order[4] = value
        with pytest.raises(IndexError):
            run_epoch(model, data, 3, order=order)
        with pytest.raises(IndexError):
            data.take(order, 3, 3)
    assert model.seen == []
    with pytest.raises(ValueError):
        run_epoch(model, data, 3, order=torch.arange(5))                # shorter than the two batches
    with pytest.raises(IndexError):
        data.take(None, 5, 3)
    with pytest.raises(TypeError):
        data.take(torch.arange(7, dtype=torch.int32), 0, 3)


def test_entries_are_declared_and_bound():
    entries_declared_and_bound(("recon_stage_b_supported", "recon_stage_b_slice"), "train.py:247-251")
    entries_declared_and_bound(("recon_stage_b_collect",), "test.py:285-292")


def test_status_codes_before_any_launch():
    from recon_amd import _lib
    L = _lib.lib()
    ok = L.recon_stage_b_supported
    assert ok(50, 72, 36) and ok(1, 2, 1) and ok(1, 1, 1)
    assert not ok(0, 72, 36) and not ok(50, 0, 36) and not ok(50, 72, 0) and not ok(-1, 72, 36)
    assert ok(2 ** 17, 2 ** 7, 2 ** 6) and not ok(2 ** 18, 2 ** 7, 2 ** 6)                # 2^30 marker cells; 2^31
    assert 828502 * 72 * 36 < 2 ** 31 - 4096 <= 828503 * 72 * 36 and ok(828502, 72, 36) and not ok(828503, 72, 36)
    assert ok(1, 2 ** 30 - 2049, 1) and not ok(1, 2 ** 30 - 2048, 1)                       # T = 1: the id pairs, 2 C cells a sentence, are the widest
    fake = 16                                                          # never dereferenced: every call below returns before a launch

    def cut(sent=fake, ids=fake, ids_out=fake, sid=fake, sid_out=fake, N=64, C=72, T=36, order=None, order_len=0, start=0, count=50, nbytes=8, out=fake,
            rows=fake):
        return L.recon_stage_b_slice(sent, fake, fake, fake, ids, sid, N, C, T, order, order_len, start, count, nbytes, out, fake, fake, fake, ids_out,
                                     sid_out, rows, None)
    assert cut(sent=None) == -1 and cut(out=None) == -1 and cut(rows=None) == -1 and cut(ids=None) == -1 and cut(sid_out=None) == -1
    assert cut(count=0) == -1 and cut(count=-2) == -1 and cut(start=-1) == -1 and cut(N=0) == -1 and cut(C=0) == -1 and cut(T=0) == -1
    assert cut(nbytes=2) == -1 and cut(out=20) == -1                   # 20: not a multiple of 8
    assert cut(start=15) == -1 and cut(order=fake, order_len=49) == -1 and cut(order=fake, order_len=64, start=15) == -1     # rows outside the array
    assert cut(N=2 ** 20, count=2 ** 20) == -2 and cut(N=2 ** 20, count=828503) == -2                # the size over the limit
    assert cut(N=2 ** 40, count=828503, order=fake, order_len=2 ** 20) == -2

    def collect(labels=fake, state=fake, M=3600, C=72, capacity=100, out=fake, conf=fake):
        return L.recon_stage_b_collect(labels, fake, conf, fake, M, C, 0, state, capacity, out, fake, fake, fake, None)
    assert collect(labels=None) == -1 and collect(state=None) == -1 and collect(conf=None) == -1 and collect(out=None) == -1
    assert collect(M=0) == -1 and collect(C=0) == -1 and collect(M=3601) == -1 and collect(capacity=-1) == -1
