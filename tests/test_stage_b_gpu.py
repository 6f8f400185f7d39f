"""recon_amd/stage_b.py through csrc/stage_b.hip (k_sb_slice, k_sb_collect): `take` at the shapes of tests/stage_b_checks.py against the
torch path on the same device and the numpy restatement, every output inside sentinel-filled memory behind a guard of 37 elements, two
runs bit for bit; the collector at the chunk size from both sides, over several appends, at the capacity and one past it; and a whole
`run_epoch` over the fixtures' GPGNN and RECON against the hand-written loop of INTEGRATION.md.  Everything is compared exactly: every
value is selected or copied."""
import numpy as np
import pytest
import torch

from context_batch_checks import build, random_batch, random_dataset
from conftest import load_golden
from op_checks import calls_of, dev, state_dict_of
from stage_b_checks import (SHAPES, Outputs, Rows, batch_outputs, dataset, join_rows, permutation, restate_collect, restate_take, row_differences,
                            slice_differences)

pytestmark = pytest.mark.gpu
SENTINEL = {torch.int64: -7777, torch.int32: -7777, torch.float32: 12345.678}
GUARD = 37


def _guarded(monkeypatch):
    """Every buffer of stage_b._new inside sentinel-filled memory, a guard of 37 elements in front (so no base is 16-byte aligned) and
    another behind; returns the list of (flat, n, dtype) and the check that the guards are intact."""
    from recon_amd import stage_b
    held = []

    def guarded(shape, dtype, device):
        n = int(np.prod(shape))
        flat = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=device)
        held.append((flat, n, dtype))
        return flat[GUARD:GUARD + n].view(shape)
    monkeypatch.setattr(stage_b, "_new", guarded)

    def intact():
        for flat, n, dtype in held:
            sentinel = torch.full((GUARD,), SENTINEL[dtype], dtype=dtype, device=flat.device)
            assert torch.equal(flat[:GUARD], sentinel) and torch.equal(flat[GUARD + n:], sentinel), (dtype, n)
    return held, intact


def _torch_path(fn):
    from recon_amd import stage_b
    prev, stage_b._KERNELS = stage_b._KERNELS, False
    try:
        return fn()
    finally:
        stage_b._KERNELS = prev


@pytest.fixture(scope="module")
def datasets():
    """One dataset per shape, on the host and on the device, shared by the cases."""
    from recon_amd import StageBData
    out = {}
    for i, shape in enumerate(sorted(SHAPES)):
        N, n, T, _, _ = SHAPES[shape]
        as_indices, surface_ids = dataset(N, n, T, seed=i)
        out[shape] = (as_indices, surface_ids, StageBData.from_indices(as_indices, surface_ids).to(dev()))
    return out


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("permuted", (False, True))
@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32))
def test_take_through_the_kernel(datasets, shape, permuted, index_dtype, monkeypatch):
    from recon_amd import StageBData
    N, n, T, count, start = SHAPES[shape]
    as_indices, surface_ids, data = datasets[shape]
    order = permutation(N, 3) if permuted else None
    order_d = None if order is None else torch.from_numpy(order).to(dev())
    ref = _torch_path(lambda: data.take(order_d, start, count, index_dtype))
    held, intact = _guarded(monkeypatch)
    kernel, stock = calls_of(monkeypatch, StageBData, "_take_kernel"), calls_of(monkeypatch, StageBData, "_take_torch")
    got = data.take(order_d, start, count, index_dtype)
    assert (len(kernel), len(stock)) == (1, 0) and len(held) == 7
    intact()
    assert got.entity_markers.data_ptr() % 16 != 0
    assert got.sentence_input.dtype == index_dtype and got.entity_markers.shape == (count, n * (n - 1), T)
    assert slice_differences(got, ref) == []                            # the outputs equal the torch path's: no cell kept its sentinel
    assert slice_differences(got, restate_take(as_indices, surface_ids, order, start, count, np.int32 if index_dtype == torch.int32 else np.int64)) == []
    assert slice_differences(got, data.take(order_d, start, count, index_dtype)) == []       # two runs, bit for bit
    intact()


def test_take_without_the_entity_arrays(monkeypatch):
    from recon_amd import StageBData
    N, n, T, count, start = SHAPES["last_batch"]
    as_indices, _ = dataset(N, n, T, seed=9, entity_arrays=False)
    data = StageBData.from_indices(as_indices).to(dev())
    order = permutation(N, 3)
    held, intact = _guarded(monkeypatch)
    kernel = calls_of(monkeypatch, StageBData, "_take_kernel")
    got = data.take(torch.from_numpy(order).to(dev()), start, count)
    assert len(kernel) == 1 and len(held) == 5 and got.entity_indices is None and got.surface_ids is None
    intact()
    assert slice_differences(got, restate_take(as_indices, None, order, start, count)) == []


def _append(r, labels, predicted, confidence, rows):
    r.append(Outputs(predicted, confidence, dev()), Rows(labels, rows, dev()))


# M with a C that divides it: one row, one wave's start, the chunk of 1 024 from both sides, the reference's 50 x 72
COLLECT = {1: 1, 2: 2, 1023: 3, 1024: 2, 1025: 5, 3600: 72}


@pytest.mark.parametrize("M", sorted(COLLECT))
@pytest.mark.parametrize("kept_share", (0.0, 1.0, 0.1))
def test_collect_through_the_kernel(M, kept_share, monkeypatch):
    from recon_amd import EpochRows
    C = COLLECT[M]
    b = batch_outputs(M, 5, kept_share, seed=M, C=C)
    want = restate_collect(*b, C)
    if kept_share in (0.0, 1.0):
        assert len(want["pair"]) == int(kept_share) * M
    held, intact = _guarded(monkeypatch)
    kernel, stock = calls_of(monkeypatch, EpochRows, "_append_kernel"), calls_of(monkeypatch, EpochRows, "_append_torch")
    r = EpochRows(M, dev())
    _append(r, *b)
    assert (len(kernel), len(stock)) == (1, 0) and len(held) == 4
    got = r.result()
    intact()
    assert row_differences(got, want) == []
    ref = _torch_path(lambda: EpochRows(M, dev()))
    _torch_path(lambda: _append(ref, *b))
    assert row_differences(got, ref.result()) == []


def test_collect_appends_reset_and_capacity(monkeypatch):
    from recon_amd import EpochRows
    batches = [batch_outputs(M, 4, 0.4, seed=20 + i, C=C) for i, (M, C) in enumerate(((1025, 5), (3600, 72), (12, 6)))]
    parts = [restate_collect(*b, C) for b, C in zip(batches, (5, 72, 6))]
    total = sum(len(p["pair"]) for p in parts)
    assert total > 1024
    held, intact = _guarded(monkeypatch)
    r, exact, short = EpochRows(total + 100, dev()), EpochRows(total, dev()), EpochRows(total - 1, dev())
    for b in batches:
        for rows in (r, exact, short):
            _append(rows, *b)
    assert row_differences(r.result(), join_rows(parts)) == []          # three appends in a row
    assert row_differences(exact.result(), join_rows(parts)) == []      # the capacity met exactly
    with pytest.raises(OverflowError, match=r"%d rows.*%d" % (total, total - 1)):
        short.result()                                                  # exceeded by one
    intact()                                                            # nothing was written at or beyond the capacity
    assert np.array_equal(short.pair.cpu().numpy(), join_rows(parts)["pair"][:total - 1])
    assert np.array_equal(short.confidence.cpu().numpy(), join_rows(parts)["confidence"][:total - 1])
    for rows in (r, short):
        rows.reset()
        _append(rows, *batches[2])
        assert row_differences(rows.result(), parts[2]) == []
    intact()


# ------------------------------------------------------------------------------------------------------------- a whole epoch
def _gpgnn(dropout):
    from recon_amd.gpgnn import GPGNN
    g = load_golden("gpgnn1_untied")
    n = int(g["n"])
    p = {"max_num_nodes": n, "embedding_dim": int(g["d"]), "layer_number": int(g["L"]), "projection_style": str(g["style"]), "non-linear1": "relu",
         "non-linear": "tanh", "dropout1": 0.5 if dropout else 0.0, "position_emb": 3, "units1": 4, "rnn1_layers": 1, "bidirectional": 1, "batch_size": 3}

    def make():
        torch.manual_seed(0)
        m = GPGNN(dict(p), g["emb"], max_sent_len=4, n_out=3)
        m.load_state_dict(state_dict_of(g), strict=False)
        m.packed_word_dropout = dropout
        return m.to(dev())
    as_indices, _ = dataset(7, n, 4, seed=31, entity_arrays=False, n_words=g["emb"].shape[0], n_out=3)
    return make, as_indices, None, None


def _recon(dropout):
    from recon_amd import ContextBatcher
    from recon_amd.gpgnn import RECON
    from tests.test_host_cpu import KGGAT_P, recon_constructor_tables
    g = load_golden("recon1_untied")
    p = dict(KGGAT_P, entity_conv_filter_size=1, batch_size=3)
    if dropout:
        p.update(dropout1=0.5, drop_out_rate_ent=0.5)

    def make():
        torch.manual_seed(0)
        m = RECON(dict(p), g["emb"], 4, 3, list(range(int(g["n_chars"]))), *recon_constructor_tables(g))
        own = m.state_dict()
        m.load_state_dict({k: v for k, v in state_dict_of(g).items() if k in own and own[k].shape == v.shape}, strict=False)
        m.packed_word_dropout = dropout
        m.entity_embedding_module.packed_char_dropout = dropout
        return m.to(dev())
    rng = np.random.default_rng(5)
    ds = random_dataset(rng, 9, 3, max_lines=5, n_words=g["emb"].shape[0], n_chars=int(g["n_chars"]), conv_filter_size=KGGAT_P["conv_filter_size"])
    ids, sf = random_batch(rng, ds, 7, 6, pad_share=0.3)
    tables, surface_ids = build(ds, "wikidata", sf, "selected", max_char_len=KGGAT_P["max_char_len"])
    base, _ = dataset(7, 3, 4, seed=32, entity_arrays=False, n_words=g["emb"].shape[0], n_out=3)
    labels = np.where(ids[:, :, 0] == -1, 0, np.maximum(base[2], 1)).astype(np.int16)                  # a padding pair has no label
    as_indices = (base[0], base[1], labels, base[3], ids.astype(np.int32), sf, None)
    return make, as_indices, surface_ids, ContextBatcher(tables.to(dev()))


def _hand_written(model, as_indices, surface_ids, batcher, bs, indices, opt, metrics, collect):
    """The loops of INTEGRATION.md as they stood: host slices, uploads, `batcher.batch`, `relation_objective`; with `collect` the
    `.cpu()[rows]` lines of the test loop and the indices of test.py:299-302."""
    from recon_amd import relation_objective
    N, C = as_indices[0].shape[0], as_indices[1].shape[1]
    if batcher is not None:
        entity_indices_d = torch.from_numpy(as_indices[4].astype(np.int64)).to(dev())
        surface_ids_d = torch.from_numpy(surface_ids).to(dev())
    for i in range(int(N / bs)):
        at = indices[i * bs:(i + 1) * bs]
        sentence_input = torch.from_numpy(as_indices[0][at].astype(int)).to(dev())
        entity_markers = torch.from_numpy(as_indices[1][at].astype(int)).to(dev())
        labels = as_indices[2][at]
        extra = ()
        if opt is not None:
            opt.zero_grad()
        if batcher is not None:
            rows = torch.from_numpy(at).to(dev())
            extra = batcher.batch(entity_indices_d[rows], surface_ids_d[rows]).model_args()
        output = model(sentence_input, entity_markers, as_indices[3][at], *extra)
        res = relation_objective(output, torch.from_numpy(labels.astype(int)).to(dev()), ignore_index=0, empty_label=1, metrics=metrics)
        if opt is not None:
            res.loss.backward()
            opt.step()
        if collect is not None:
            rows = (torch.from_numpy(labels.reshape(-1).astype(int)) != 0).nonzero().squeeze(1)
            pred, conf = res.predicted.cpu()[rows].tolist(), res.confidence.cpu()[rows].tolist()
            start_idx = i * bs
            collect.append({"pair": np.asarray([(start_idx + int(m) // C) * C + int(m) % C for m in rows], dtype=np.int64),
                            "predicted": np.asarray(pred, dtype=np.int64), "gold": labels.reshape(-1).astype(np.int64)[rows.numpy()],
                            "confidence": np.asarray(conf, dtype=np.float32)})


@pytest.mark.parametrize("dropout", (False, True))
@pytest.mark.parametrize("which", ("gpgnn1_untied", "recon1_untied"))
def test_run_epoch_against_the_hand_written_loop(which, dropout, monkeypatch):
    """N = 7 in batches of 3: two training iterations under recon_amd.optim.Adam(max_grad_norm=0.25), then an evaluation pass with rows.
    Both loops run the same deterministic ops on the same values in the same order: every parameter, counter and row is equal.  With
    `dropout` the packed word (and, in RECON, char) dropout is on, in train mode, under one torch.manual_seed for both loops."""
    from recon_amd import EpochRows, RelationMetrics, StageBData, run_epoch
    from recon_amd.optim import Adam
    make, as_indices, surface_ids, batcher = (_gpgnn if which == "gpgnn1_untied" else _recon)(dropout)
    bs, order = 3, permutation(7, 3)
    data = StageBData.from_indices(as_indices, surface_ids).to(dev())
    adam = lambda m: Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-2, weight_decay=1e-4, max_grad_norm=0.25)
    # ---- the hand-written loops
    b = make().train()
    train_b, test_b, parts = RelationMetrics(dev()), RelationMetrics(dev()), []
    torch.manual_seed(77)
    _hand_written(b, as_indices, surface_ids, batcher, bs, order, adam(b), train_b, None)
    b.eval()
    with torch.no_grad():
        _hand_written(b, as_indices, surface_ids, batcher, bs, np.arange(7), None, test_b, parts)
    # ---- run_epoch
    a = make().train()
    train_a, test_a, rows_a = RelationMetrics(dev()), RelationMetrics(dev()), EpochRows.for_data(data)
    kernel = calls_of(monkeypatch, StageBData, "_take_kernel")
    torch.manual_seed(77)
    run_epoch(a, data, bs, order=torch.from_numpy(order).to(dev()), batcher=batcher, optimizer=adam(a), metrics=train_a)
    a.eval()
    run_epoch(a, data, bs, batcher=batcher, metrics=test_a, rows=rows_a)
    assert len(kernel) == 4
    changed = 0
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k
    for k, p in make().named_parameters():
        changed += int(p.requires_grad and not torch.equal(p, dict(a.named_parameters())[k]))
    assert changed > 0                                                  # the two iterations trained something
    assert train_a.result() == train_b.result() and train_a.result().batches == 2 and train_a.result().kept > 0
    assert test_a.result() == test_b.result() and test_a.result().batches == 2
    got = rows_a.result()
    assert got.pair.numel() == test_a.result().kept > 0
    assert row_differences(got, join_rows(parts)) == []
