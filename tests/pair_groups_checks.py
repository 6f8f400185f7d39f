"""What tests/test_pair_groups_cpu.py and tests/test_pair_groups_gpu.py share: the marker cases, a plain-loop
restatement of the grouping rule with its five wrong variants, the comparison that has to report them, and the float64 reference of the
op — the DENSE stock chain, every pair encoded on its own.  Not a test module and not a conftest."""
import copy

import numpy as np
import torch

N_NODES = 9                                    # the reference's graph: C = 72 pair slots
VARIANTS = ("across_sentences", "highest_c", "zero_only", "ptr_off_by_one", "short_rows")


# ------------------------------------------------------------------------------------------------------------- the restatement
def restate(markers, variant=None):
    """The grouping in plain loops over a numpy [B, C, T] array -> dict(seq_pair, pair_seq, seq_ptr, total).  Two slots of one sentence
    share a sequence exactly when their rows are equal element by element; the representative is the lowest c; sequences are numbered
    in (b, lowest c) order.  `variant`: one of VARIANTS, a wrong reading of the rule (the checks must report each)."""
    m = np.asarray(markers)
    B, C, T = m.shape
    cut = T - 1 if variant == "short_rows" else T

    def equal(b0, c0, b1, c1):
        if variant == "zero_only" and (m[b0, c0].any() or m[b1, c1].any()):
            return b0 == b1 and c0 == c1
        return all(m[b0, c0, t] == m[b1, c1, t] for t in range(cut))
    rep = {}                                                       # (b, c) -> its representative's (b, c)
    for b in range(B):
        for c in range(C):
            if variant == "across_sentences":
                candidates = [(bb, cc) for bb in range(b + 1) for cc in range(C) if (bb, cc) < (b, c)]
            else:
                candidates = [(b, cc) for cc in range(c)]
            rep[b, c] = next((q for q in candidates if rep[q] == q and equal(q[0], q[1], b, c)), (b, c))
    if variant == "highest_c":
        last = {}
        for k, q in rep.items():
            last[q] = max(last.get(q, k), k)
        rep = {k: last[q] for k, q in rep.items()}
    reps = sorted(set(rep.values()))
    number = {q: j for j, q in enumerate(reps)}
    seq_pair = np.array([b * C + c for b, c in reps], dtype=np.int64)
    pair_seq = np.array([number[rep[b, c]] for b in range(B) for c in range(C)], dtype=np.int64)
    seq_ptr = np.zeros(B + 1, dtype=np.int64)
    for b, _ in reps:
        seq_ptr[b + 1:] += 1
    if variant == "ptr_off_by_one":
        seq_ptr[1:] += 1
    return {"seq_pair": seq_pair, "pair_seq": pair_seq, "seq_ptr": seq_ptr, "total": len(reps)}


def differences(got, want):
    """The names of the fields of `got` (a PairGroups or a restate() dict) that are not `want`'s (a restate() dict), exactly."""
    field = lambda g, k: g[k] if isinstance(g, dict) else getattr(g, k)
    bad = []
    for k in ("seq_pair", "pair_seq", "seq_ptr"):
        a = field(got, k)
        a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
        if a.shape != want[k].shape or not np.array_equal(a.astype(np.int64), want[k]):
            bad.append(k)
    if int(field(got, "total")) != want["total"]:
        bad.append("total")
    return bad


def compact_differences(groups, sentence, markers, want):
    """The compact copies against the representatives' rows: names of the ones that differ."""
    C = markers.shape[1]
    p = torch.from_numpy(want["seq_pair"])
    bad = []
    if groups.sentence_d.dtype != sentence.dtype or not torch.equal(groups.sentence_d.cpu(), sentence.cpu()[p // C]):
        bad.append("sentence_d")
    rows = markers.cpu().reshape(-1, markers.shape[2])[p].to(sentence.dtype).unsqueeze(1)
    if groups.markers_d.dtype != sentence.dtype or tuple(groups.markers_d.shape) != tuple(rows.shape) or not torch.equal(groups.markers_d.cpu(), rows):
        bad.append("markers_d")
    return bad


# ------------------------------------------------------------------------------------------------------------- the cases
def slot_of(i, j, n=N_NODES):
    """The pair slot of the ordered pair (i, j), i != j, in a graph padded to n nodes."""
    return i * (n - 1) + (j if j < i else j - 1)


def entity_markers(B, k, T, n=N_NODES, seed=0):
    """[B, n (n - 1), T] int64 as the preprocessing writes it for sentences of k entities: the k (k - 1) present pairs' slots hold a row
    of get_entity_indexed_vector's values (0 padding behind the sentence's end, 1 outside, 2 the left entity's tokens, 3 the right
    one's), every other slot stays all zero.  k may be a sequence of B counts."""
    rng = np.random.default_rng(seed)
    ks = [k] * B if isinstance(k, int) else list(k)
    m = np.zeros((B, n * (n - 1), T), dtype=np.int64)
    for b in range(B):
        kb = ks[b]
        assert 2 * kb <= T
        length = int(rng.integers(2 * kb, T + 1))
        for i in range(kb):
            for j in range(kb):
                if i != j:
                    row = np.ones(length, dtype=np.int64)
                    row[2 * i], row[2 * j + 1] = 2, 3              # (length >= 2 k: the 2 k positions are distinct)
                    m[b, slot_of(i, j, n), :length] = row
    return m


def _sentences(B, T, seed):
    return torch.from_numpy(np.random.default_rng(seed + 77).integers(0, 11, (B, T)).astype(np.int64))


def tile_case(S_d):
    """B sentences of C = 6 whose distinct rows add up to S_d: sentence b has 1 + (b % 3) distinct rows, the last one trimmed."""
    rows, counts = 0, []
    while rows < S_d:
        counts.append(min(1 + len(counts) % 3, S_d - rows))
        rows += counts[-1]
    m = np.zeros((len(counts), 6, 3), dtype=np.int64)
    for b, n in enumerate(counts):
        for r in range(1, n):
            m[b, 2 * r - 1, r % 3] = r                   # slots 1, 3: a distinct non-zero row each; the others stay zero
    return m


def wide_case(S_d):
    """T = 2, C = 2: sentences with two distinct rows, the last one with one when S_d is odd."""
    B = (S_d + 1) // 2
    m = np.zeros((B, 2, 2), dtype=np.int64)
    m[:, 1, 0] = 1
    if S_d % 2:
        m[-1, 1, 0] = 0
    return m


def _c_case(C, T=3):
    m = np.zeros((2, C, T), dtype=np.int64)
    m[0, C // 3, 0] = 2
    m[0, C - 1, 0] = 2                                   # equal to slot C / 3, far apart
    m[1, :, 1] = np.arange(C) % 5                        # five groups, interleaved
    return m


def marker_cases():
    """name -> int64 numpy [B, C, T]; every case small enough to take seconds (the two B ~ 8192 ones and C = 256 / 257 stay below a MB)."""
    cases = {}
    cases["equal_rows"] = np.array([[[1], [1]]], dtype=np.int64)
    cases["different_rows"] = np.array([[[1], [2]]], dtype=np.int64)
    m = np.zeros((2, 6, 5), dtype=np.int64)
    m[1] = 1 + np.arange(30).reshape(6, 5) % 3
    m[1, :, 0] = np.arange(6)                            # sentence 1: all distinct
    cases["zero_and_distinct"] = m
    m = np.zeros((1, 7, 4), dtype=np.int64)
    m[0, 0] = m[0, 5] = [1, 2, 3, 1]                     # equal non-zero rows that are not neighbours, a zero group between them
    cases["far_equal_nonzero"] = m
    m = np.ones((2, 4, 6), dtype=np.int64)
    m[:, 2, -1] = 3                                      # differ only in the last element
    cases["last_element"] = m
    m = np.ones((2, 4, 6), dtype=np.int64)
    m[:, 1, 0] = 2                                       # differ only in the first element
    m[:, 3, 0] = 2
    cases["first_element"] = m
    cases["T1"] = np.array([[[0], [1], [0], [2], [1]], [[3], [3], [3], [3], [3]]], dtype=np.int64)
    m = np.zeros((3, 5, 37), dtype=np.int64)
    m[:, 1, 36] = 1
    m[:, 3, 35] = 1
    m[1, 4, 36] = 1                                      # equal to slot 1
    cases["T37"] = m
    cases["C72_k2"] = entity_markers(3, 2, 12, seed=1)
    cases["C72_k3"] = entity_markers(3, 3, 12, seed=2)
    cases["C72_k9"] = entity_markers(2, 9, 20, seed=3)
    cases["C256"] = _c_case(256)
    cases["C257"] = _c_case(257)
    for S_d in (15, 16, 17, 33):
        cases["tile_%d" % S_d] = tile_case(S_d)
    cases["wide_2048"] = wide_case(2048)
    cases["wide_2049"] = wide_case(2049)
    cases["B8192"] = wide_case(2 * 8192 - 1)
    cases["B8193"] = wide_case(2 * 8193 - 1)
    return cases


_CASES = {}


def case(name):
    """(sentence int64 [B, T], markers int64 [B, C, T], the restatement's dict), built once and left unchanged."""
    if name not in _CASES:
        m = marker_cases()[name]
        _CASES[name] = (_sentences(m.shape[0], m.shape[2], len(name)), torch.from_numpy(m), restate(m))
    return _CASES[name]


CASE_NAMES = tuple(marker_cases())
KERNEL_REFUSES = ("C257", "B8193")                     # above the kernels' limits: the torch path is taken
EXPECTED_TOTAL = {"equal_rows": 1, "different_rows": 2, "zero_and_distinct": 7, "C72_k2": 3 * 3, "C72_k3": 3 * 7, "C72_k9": 2 * 72, "tile_15": 15,
                  "tile_16": 16, "tile_17": 17, "tile_33": 33, "wide_2048": 2048, "wide_2049": 2049, "B8192": 2 * 8192 - 1, "B8193": 2 * 8193 - 1}


# ------------------------------------------------------------------------------------------------------------- the op's reference
def dense_reference(rnn, sentence, markers, word_table, pos_table, g_out, pair_factors=None):
    """float64, the dense stock chain (models/models.py:160-184): every pair encoded on its own.  pair_factors: [B, C, T, Dw] dropout
    factors, pair (b, c) holding row pair_seq[b, c] of the draw.  -> [out, d_pos_table, the eight parameter gradients]."""
    from test_sent_lstm_cpu import stock
    r64 = copy.deepcopy(rnn).double()
    pt = pos_table.double().requires_grad_(True)
    ref = stock(r64, sentence, markers, word_table.double(), pt, None if pair_factors is None else pair_factors.double())
    ref.backward(g_out.double())
    return [ref.detach(), pt.grad] + [p.grad for p in r64.parameters()]


def op_inputs(markers, Dw, P, H, seed=0):
    """The sent_lstm tests' draws (weights uniform in +-1 / sqrt(H), tables N(0, 1) with a non-zero padding row) over a case's markers,
    clamped into the position table's rows."""
    from test_sent_lstm_cpu import VP, VW
    B, C, T = markers.shape
    g = torch.Generator().manual_seed(1000 * seed + B + C + T + Dw + P + H)
    torch.manual_seed(1000 * seed + B + 7 * T + C + Dw + P + H)
    rnn = torch.nn.LSTM(Dw + P, H, 1, batch_first=True, bidirectional=True)
    sentence = torch.randint(0, VW, (B, T), generator=g)
    word_table = torch.randn(VW, Dw, generator=g)
    pos_table = torch.randn(VP, P, generator=g)
    g_out = torch.randn(B, C, 2 * H, generator=g)
    return rnn, sentence, markers.clamp(0, VP - 1), word_table, pos_table, g_out
