"""Shared by tests/test_stage_b_cpu.py, tests/test_stage_b_gpu.py and tools/stage_b_iter_bench.py: synthetic stage-B datasets in the form
`graphs_to_indices` returns, the shapes, and the two ends of an iteration written once more in plain numpy from the reference's lines —
`restate_take` from train.py:247-251 with the casts of :261-262 and :309, `restate_collect` from test.py:285-292 with the indices of
:300-302 — sharing no code with the package.  `wrong=` makes either wrong in one named way, so that the tests can show the checks
catch each.  Not a test module and not a conftest."""
import numpy as np
import torch

# (N, n -> C = n (n - 1), T, count, start)
SHAPES = {"smallest": (1, 2, 1, 1, 0),
          "unaligned": (3, 3, 5, 2, 1),           # marker rows of 30 bytes: nothing is 16-byte aligned
          "last_batch": (7, 3, 5, 3, 4),          # the last full batch
          "reference": (64, 9, 36, 50, 14)}       # the reference's widths
SLICE_FIELDS = ("sentence_input", "entity_markers", "labels", "num_entities", "entity_indices", "surface_ids", "rows")
ROW_FIELDS = ("pair", "predicted", "gold", "confidence")
WRONG_TAKE = ("permutation_ignored", "labels_column_major", "zero_extended", "start_off_by_one_batch")
WRONG_COLLECT = ("keeps_ignored", "unstable")


def dataset(N, n, T, seed, entity_arrays=True, n_words=1000, n_out=3, n_entities=50, n_surfaces=90, kept_share=0.5):
    """(as_indices, surface_ids): the tuple of parsing/legacy_sp_models.py:276-333 in its dtypes — sentences int32 [N, T], markers int8
    [N, C, T], labels int16 [N, C] (0 = no pair: about 1 - kept_share of them), entity counts int32 [N], entity_indices int32 [N, C, 2]
    with (-1, -1) where the label is 0, an object array of surface forms, a pair list — and int32 surface ids as `ContextTables.build`
    returns them.  Without entity_arrays the tuple ends behind the counts and surface_ids is None."""
    rng = np.random.default_rng(seed)
    C = n * (n - 1)
    sentences = rng.integers(0, n_words, (N, T)).astype(np.int32)
    markers = rng.integers(0, 4, (N, C, T)).astype(np.int8)
    labels = (rng.integers(1, max(n_out, 2), (N, C)) * (rng.random((N, C)) < kept_share)).astype(np.int16)
    counts = rng.integers(2, n + 1, N).astype(np.int32)
    if not entity_arrays:
        return (sentences, markers, labels, counts), None
    present = (labels != 0)[:, :, None]
    entity_indices = np.where(present, rng.integers(0, n_entities, (N, C, 2)), -1).astype(np.int32)
    surface_ids = np.where(present, rng.integers(1, n_surfaces, (N, C, 2)), 0).astype(np.int32)
    forms = np.empty((N, C, 2), dtype=object)
    for i in range(N):
        for j in range(C):
            for k in range(2):
                forms[i, j, k] = ["sf%d" % surface_ids[i, j, k]]
    pairs = [[("Q%d" % a, "Q%d" % b) for a, b in entity_indices[i]] for i in range(N)]
    return (sentences, markers, labels, counts, entity_indices, forms, pairs), surface_ids


def permutation(N, seed):
    return np.random.default_rng(seed).permutation(N).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------- the restatements
def restate_take(as_indices, surface_ids, order, start, count, index_dtype=np.int64, wrong=None):
    """train.py:247-251, :261-262, :309 -> a dict over SLICE_FIELDS (numpy; None where the tuple has no such array)."""
    N = as_indices[0].shape[0]
    indices = np.arange(N) if (order is None or wrong == "permutation_ignored") else np.asarray(order)
    if wrong == "start_off_by_one_batch":
        indices = np.roll(indices, -count)
    rows = indices[start:start + count]
    labels = as_indices[2][rows]
    labels = (labels.T if wrong == "labels_column_major" else labels).astype(int).reshape(-1)
    out = {"sentence_input": as_indices[0][rows].astype(int).astype(index_dtype), "entity_markers": as_indices[1][rows].astype(int).astype(index_dtype),
           "labels": labels.astype(np.int64), "num_entities": as_indices[3][rows].astype(np.int32), "entity_indices": None, "surface_ids": None,
           "rows": rows.astype(np.int64)}
    if len(as_indices) > 4:
        ids = as_indices[4][rows]
        out["entity_indices"] = (ids.astype(np.uint32) if wrong == "zero_extended" else ids).astype(np.int64)
    if surface_ids is not None:
        out["surface_ids"] = surface_ids[rows].astype(np.int32)
    return out


def restate_collect(labels, predicted, confidence, rows, C, ignore_index=0, wrong=None):
    """test.py:285-292 and the indices of :300-302 for one batch -> a dict over ROW_FIELDS: the rows with a label other than
    ignore_index, in row order; `pair` = the dataset's sentence C + the pair within it."""
    kept = [m for m in range(len(labels)) if labels[m] != ignore_index or wrong == "keeps_ignored"]
    if wrong == "unstable":
        kept = kept[::-1]
    return {"pair": np.asarray([int(rows[m // C]) * C + m % C for m in kept], dtype=np.int64),
            "predicted": np.asarray([predicted[m] for m in kept], dtype=np.int64), "gold": np.asarray([labels[m] for m in kept], dtype=np.int64),
            "confidence": np.asarray([confidence[m] for m in kept], dtype=np.float32)}


def join_rows(parts):
    return {f: np.concatenate([p[f] for p in parts]) for f in ROW_FIELDS}


# ------------------------------------------------------------------------------------------------------------- the comparison
def _as_numpy(fields, obj):
    if isinstance(obj, dict):
        return obj
    return {f: None if getattr(obj, f) is None else getattr(obj, f).detach().cpu().numpy() for f in fields}


def _differences(fields, got, want):
    got, want = _as_numpy(fields, got), _as_numpy(fields, want)
    bad = []
    for f in fields:
        a, b = got[f], want[f]
        if (a is None) != (b is None):
            bad.append(f)
        elif a is not None and (a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes()):
            bad.append(f)
    return bad


def slice_differences(got, want):
    """The SLICE_FIELDS in which two slices (StageBSlice or restatement) differ in shape, dtype or any value."""
    return _differences(SLICE_FIELDS, got, want)


def row_differences(got, want):
    """The ROW_FIELDS in which two results (EpochRowsResult or restatement) differ in shape, dtype or any bit."""
    return _differences(ROW_FIELDS, got, want)


def batch_outputs(M, n_out, kept_share, seed, C):
    """labels int64 [M] (0 with probability 1 - kept_share), predicted int64 [M], confidence fp32 [M] and rows int64 [M / C], as numpy."""
    rng = np.random.default_rng(seed)
    labels = (rng.integers(1, n_out, M) * (rng.random(M) < kept_share)).astype(np.int64)
    predicted = rng.integers(0, n_out, M).astype(np.int64)
    confidence = rng.random(M).astype(np.float32)
    rows = rng.permutation(M // C + 5)[:M // C].astype(np.int64)
    return labels, predicted, confidence, rows


class Outputs:
    """Stands in for a RelationObjective where only `predicted` and `confidence` are read."""

    def __init__(self, predicted, confidence, device):
        self.predicted, self.confidence = torch.from_numpy(predicted).to(device), torch.from_numpy(confidence).to(device)


class Rows:
    """Stands in for a StageBSlice where only `labels` and `rows` are read."""

    def __init__(self, labels, rows, device):
        self.labels, self.rows = torch.from_numpy(labels).to(device), torch.from_numpy(rows).to(device)
