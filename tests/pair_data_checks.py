"""Shared by tests/test_pair_data_cpu.py, tests/test_pair_data_gpu.py and tools/pair_epoch_bench.py: synthetic per-pair datasets in the
forms parsing/legacy_sp_models.py:67-97 and :503-603 return, the shapes, the slice written once more in plain numpy from the reference's
lines — `restate_take` from train.py:247-249 with the casts of :301-309 — sharing no code with the package, and the hand-written loop
that `run_epoch` is compared with.  `wrong=` makes the restatement wrong in one named way, so that the tests can show the checks catch
each.  Everything is selection and copying: every comparison is exact.  Not a test module and not a conftest."""
import numpy as np
import torch

from stage_b_checks import _differences, permutation

FORMS = ("marks", "positions", "segments")
# (count, T): the smallest shapes at which the slice can go wrong
SHAPES = {"one_cell": (1, 1),               # every output shorter than one vector
          "straddle": (3, 3),               # rows straddle 16-byte vectors at 4 and 8 bytes, 3 T odd
          "unaligned": (7, 5),              # nothing aligned
          "mask_1020": (20, 17),            # the mask's 1020 floats: below a 256-thread block's 1024 cells
          "mask_1044": (29, 12),            # and 1044, above
          "ids_510": (15, 34),              # 510 int64 cells: below a block's 512
          "ids_513": (19, 27),              # and 513, above
          "reference": (50, 36)}            # the reference's batch, the last full one of N = 173
SLICE_FIELDS = ("sentence_input", "entity_markers", "pcnn_mask", "labels", "rows")
WRONG_TAKE = ("permutation_ignored", "start_off_by_one_batch", "mask_not_permuted", "mask_planes_swapped", "mask_token_major")


def extent(shape):
    """(N, start) of a shape: the reference's batch is cut as the last full batch of 173 rows, the others from the middle of 2 count + 3."""
    count, _ = SHAPES[shape]
    return (173, 100) if shape == "reference" else (2 * count + 3, count + 1)


def dataset(N, T, form, seed, n_words=1000, n_out=7, kept_share=0.7, zero_rows=(), one_rows=()):
    """The list a per-pair `graphs_to_indices` returns, in its dtypes: sentences int32 [N, T], markers int8 [N, T] (marks: 0..3) or
    [N, 2, T] (0..2 T), labels int16 [N] (0 with probability 1 - kept_share) and, for `segments`, pcnn_mask float32 [N, 3, T] whose bytes
    run over all eight 3-bit patterns, all-zero in `zero_rows` and in row 0, all-one in `one_rows` and in row N - 1; and the pair list."""
    rng = np.random.default_rng(seed)
    sentences = rng.integers(0, n_words, (N, T)).astype(np.int32)
    markers = (rng.integers(0, 4, (N, T)) if form == "marks" else rng.integers(0, 2 * T + 1, (N, 2, T))).astype(np.int8)
    labels = (rng.integers(1, max(n_out, 2), N) * (rng.random(N) < kept_share)).astype(np.int16)
    pairs = [("Q%d" % i, "Q%d" % (i + 1)) for i in range(N)]
    if form != "segments":
        return [sentences, markers, labels, pairs] if form == "positions" else [sentences, markers, labels]
    bits = rng.integers(0, 8, (N, T))
    bits[[0] + list(zero_rows)] = 0
    bits[[N - 1] + list(one_rows)] = 7
    mask = np.stack([(bits >> s) & 1 for s in range(3)], axis=1).astype(np.float32)
    return [sentences, markers, labels, mask, pairs]


def shape_dataset(shape, form, seed):
    count, T = SHAPES[shape]
    N, start = extent(shape)
    return dataset(N, T, form, seed, zero_rows=(start,), one_rows=(start + count - 1,))


def shape_order(shape, seed=3):
    """A permutation of the rows changed so that it repeats a row and the slice [start, start + count) holds row 0 and, from two rows on,
    row N - 1."""
    count, _ = SHAPES[shape]
    N, start = extent(shape)
    order = permutation(N, seed)
    order[0] = order[1]
    order[start] = 0
    if count >= 2:
        order[start + count - 1] = N - 1
    if count >= 3:
        order[start + 1] = 0
    return order


# ------------------------------------------------------------------------------------------------------------- the restatement
def restate_take(as_indices, order, start, count, index_dtype=np.int64, wrong=None):
    """train.py:247-249 with the casts of :301-309 -> a dict over SLICE_FIELDS (numpy; pcnn_mask None where the list has none).  The mask
    follows the order (the package's stated deviation); `mask_not_permuted` is the reference's :304."""
    N = as_indices[0].shape[0]
    indices = np.arange(N) if (order is None or wrong == "permutation_ignored") else np.asarray(order)
    if wrong == "start_off_by_one_batch":
        indices = np.roll(indices, -count)
    rows = indices[start:start + count]
    out = {"sentence_input": as_indices[0][rows].astype(int).astype(index_dtype), "entity_markers": as_indices[1][rows].astype(int).astype(index_dtype),
           "pcnn_mask": None, "labels": as_indices[2][rows].astype(int).reshape(-1).astype(np.int64), "rows": rows.astype(np.int64)}
    if len(as_indices) > 3 and not isinstance(as_indices[3], list):
        mask = np.array(as_indices[3][start:start + count] if wrong == "mask_not_permuted" else as_indices[3][rows]).astype(np.float32)
        if wrong == "mask_planes_swapped":
            mask = mask[:, ::-1]
        if wrong == "mask_token_major":
            mask = mask.transpose(0, 2, 1).reshape(mask.shape)
        out["pcnn_mask"] = np.ascontiguousarray(mask)
    return out


def slice_differences(got, want):
    """The SLICE_FIELDS in which two slices (PairSlice or restatement) differ in shape, dtype or any bit."""
    return _differences(SLICE_FIELDS, got, want)


# ------------------------------------------------------------------------------------------------------------- a whole epoch
MODEL_FORMS = {"lstm_baseline1": "marks", "cnn1": "positions", "pcnn1": "segments"}


def model_dataset(name, N=10, seed=41):
    """Rows for the fixtures' models (tests/sentence_conv_checks.py baseline_fixture: 11 words, T = 9, 19 positions, 7 labels)."""
    return dataset(N, 9, MODEL_FORMS[name], seed, n_words=11, n_out=7)


def hand_written(model, as_indices, bs, indices, opt, metrics, collect, device):
    """The loop of train.py:244-315 for a per-pair model as it stood: host slices, `astype(int)`, uploads, `relation_objective`; the mask
    cut with the same rows as the sentences (the stated deviation from :304); with `collect` the `.cpu()[rows]` lines of the test loop
    and the indices of test.py:297-302, one pair per row."""
    from recon_amd import relation_objective
    N = as_indices[0].shape[0]
    has_mask = len(as_indices) > 3 and not isinstance(as_indices[3], list)
    for i in range(int(N / bs)):
        at = indices[i * bs:(i + 1) * bs]
        args = [torch.from_numpy(as_indices[0][at].astype(int)).to(device), torch.from_numpy(as_indices[1][at].astype(int)).to(device)]
        if has_mask:
            args.append(torch.from_numpy(np.array(as_indices[3][at])).float().to(device))
        labels = as_indices[2][at]
        if opt is not None:
            opt.zero_grad()
        output = model(*args)
        res = relation_objective(output, torch.from_numpy(labels.astype(int)).view(-1).to(device), ignore_index=0, empty_label=1, metrics=metrics)
        if opt is not None:
            res.loss.backward()
            opt.step()
        if collect is not None:
            kept = (torch.from_numpy(labels.reshape(-1).astype(int)) != 0).nonzero().squeeze(1)
            pred, conf = res.predicted.cpu()[kept].tolist(), res.confidence.cpu()[kept].tolist()
            collect.append({"pair": np.asarray([int(at[int(m)]) for m in kept], dtype=np.int64), "predicted": np.asarray(pred, dtype=np.int64),
                            "gold": labels.reshape(-1).astype(np.int64)[kept.numpy()], "confidence": np.asarray(conf, dtype=np.float32)})


def epoch_pair(name, device, make_adam, dropout=False, index_dtype=torch.int64):
    """Three training iterations (N = 10 in batches of 3, a permuted order) and a test pass with rows, once by the hand-written loop and
    once by `run_epoch` over a PairData -> (model, train metrics, test metrics, rows) of each, and the untrained model.  With `dropout`
    every dropout is 0.5 and the packed word dropout is on, in train mode, under one torch.manual_seed for both loops."""
    from recon_amd import EpochRows, PairData, RelationMetrics, run_epoch
    from sentence_conv_checks import baseline_fixture
    from stage_b_checks import join_rows
    as_indices = model_dataset(name)
    bs, order = 3, permutation(10, 3)

    def make():
        m = baseline_fixture(name, device)[0]
        if dropout:
            for mod in m.modules():
                if isinstance(mod, torch.nn.Dropout):
                    mod.p = 0.5
            m.packed_word_dropout = True
        return m
    b = make().train()
    train_b, test_b, parts = RelationMetrics(device), RelationMetrics(device), []
    torch.manual_seed(77)
    hand_written(b, as_indices, bs, order, make_adam(b), train_b, None, device)
    b.eval()
    with torch.no_grad():
        hand_written(b, as_indices, bs, np.arange(10), None, test_b, parts, device)
    data = PairData.from_indices(as_indices).to(device)
    a = make().train()
    train_a, test_a, rows_a = RelationMetrics(device), RelationMetrics(device), EpochRows.for_data(data)
    torch.manual_seed(77)
    run_epoch(a, data, bs, order=torch.from_numpy(order).to(device), optimizer=make_adam(a), metrics=train_a, index_dtype=index_dtype)
    a.eval()
    run_epoch(a, data, bs, metrics=test_a, rows=rows_a, index_dtype=index_dtype)
    return (a, train_a, test_a, rows_a.result()), (b, train_b, test_b, join_rows(parts)), make()


def assert_epochs_equal(ours, theirs, fresh):
    """Every parameter, every counter and every result row is equal, and the three steps trained something."""
    from stage_b_checks import row_differences
    (a, train_a, test_a, rows_a), (b, train_b, test_b, rows_b) = ours, theirs
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k
    trained = dict(a.named_parameters())
    assert sum(int(p.requires_grad and not torch.equal(p, trained[k])) for k, p in fresh.named_parameters()) > 0
    assert train_a.result() == train_b.result() and train_a.result().batches == 3 and train_a.result().kept > 0
    assert test_a.result() == test_b.result() and test_a.result().batches == 3
    assert rows_a.pair.numel() == test_a.result().kept > 0
    assert row_differences(rows_a, rows_b) == []
