"""Shared by tests/test_ragged_lines_cpu.py, tests/test_ragged_lines_gpu.py and tools/ragged_lines_bench.py: the ragged line pool's cases,
inputs, float64 reference, comparison and guard restatements, and the encoder's small model.  Not a test module and not a conftest.

A case is (counts, C, E, k): entity u owns counts[u] consecutive rows of states [L, C].  Inputs: states and g_out ~ N(0, 1), weight and
bias uniform in +-1 / sqrt(C k), from a torch.Generator whose seed is mixed with the case.  The padded form of a case has
Ln = max(max(counts), k) lines per entity, zero rows behind an entity's own, and the positions p > n_u - k masked — built here by plain
loops (`pad_rows`, `mask_of`), sharing no code with recon_amd.RaggedLines.

Reference: the stock lines (models/models.py:73-81) in float64 on the padded form, the gradient of the states taken back through the
padding.  Band: `op_checks.bound` of the stock fp32 chain's own error, by `op_checks.band_failures`, for the value and the three
gradients.  An entity with fewer than k lines gives -inf: `failures` first requires the -inf pattern of the reference exactly and then
compares with the -inf cells set to 0 on every side (-inf has no relative error).

Near ties: as tests/test_line_pool_cpu.py does, g_out is zeroed in every cell (u, e) where in float64 the best and the second-best
position are closer than 1e-5, and at most MAX_TIE_SHARE of a case's cells may be such — asserted on the CPU from the float64 reference
alone.

Guard: `restate` is the ragged pool in float32 in the kernels' order (per cell one sum over j then c, the bias last, the lowest maximal
position; d_weight and d_bias summed upwards inside an entity group, the groups in order).  `wrong=` makes it wrong in one named way."""
import math

import torch
import torch.nn.functional as F

from op_checks import band_failures
from test_line_pool_cpu import MAX_TIE_SHARE, NONE, groups_of  # noqa: F401

NAMES = ("out", "d_states", "d_weight", "d_bias")
CITES = "models/models.py:73-81"
ENTRIES = ["recon_line_pool_ragged_supported", "recon_line_pool_ragged_workspace_bytes", "recon_line_pool_ragged_fwd", "recon_line_pool_ragged_bwd"]
FILL_ENTRY, FILL_CITES = ["recon_ctx_batch_fill_ragged"], "utils/context_utils.py:365-385"

# (counts, C, E, k).  csrc/line_pool.hip: 1024 cells per position chunk, 12288 staged floats, a staged weight up to 8192 floats, 1024 slab
# cells per pass of the backward, entity groups of ceil(U / min(256, U)).
CASES = {
    "smallest": ([1], 4, 1, 1),
    "empty_entities": ([0, 3, 1, 0], 5, 3, 1),
    "fixture_widths": ([5, 1, 32, 2], 6, 2, 2),                          # (C, E, k) of the fixtures (test_line_pool_cpu.FIXTURE)
    "shorter_than_the_filter": ([1, 2, 3], 5, 3, 2),
    "byte_limit_k1": ([255], 8, 4, 1),                                   # 255 windows: the position byte's limit
    "byte_limit_k2": ([256], 8, 4, 2),
    "two_per_group": ([1 + i % 4 for i in range(257)], 3, 2, 2),         # 129 groups of two entities, the last of one
    "position_chunks": ([32, 7], 5, 64, 1),                              # 1024 / 64 = 16 positions per chunk: two chunks, then one
    "reduction_chunks": ([3, 40], 1024, 8, 1),                           # 12288 / (8 + 40) - 1 = 255 < 1024: five reduction chunks
    "weight_in_place": ([3, 9, 0, 4], 260, 33, 1),                       # 33 x 260 > 8192 floats: the backward reads the weight where it lies
}
REFUSED = ([256], 8, 4, 1)                                               # 256 windows: recon_line_pool_ragged_supported says no
WRONG = ("offset by one row", "the last line dropped", "the padding line included", "an entity shorter than the filter gives 0",
         "the highest position on a tie")


def line_ptr_of(counts):
    ptr = [0]
    for n in counts:
        ptr.append(ptr[-1] + n)
    return ptr


def pad_rows(counts, rows, P):
    """[L, ...] -> [U, P, ...], zero rows behind an entity's own; plain loops; differentiable."""
    ptr = line_ptr_of(counts)
    blocks = []
    for u, n in enumerate(counts):
        own = rows[ptr[u]:ptr[u] + n]
        blocks.append(torch.cat([own, rows.new_zeros((P - n,) + tuple(rows.shape[1:]))], dim=0))
    return torch.stack(blocks) if blocks else rows.new_zeros((0, P) + tuple(rows.shape[1:]))


def mask_of(counts, P, k=1):
    """bool [U, P - k + 1], True where the window of k lines from line p runs past the entity's own lines."""
    return torch.tensor([[p + k > n for p in range(P - k + 1)] for n in counts], dtype=torch.bool).reshape(len(counts), P - k + 1)


def inputs(counts, C, E, k, seed=0):
    g = torch.Generator().manual_seed(100003 * seed + 7919 * len(counts) + 131 * sum(counts) + 17 * C + 29 * E + 31 * k)
    L, U = sum(counts), len(counts)
    s = 1.0 / math.sqrt(C * k)
    states = torch.randn(L, C, generator=g)
    weight = (torch.rand(E, C, k, generator=g) * 2 - 1) * s
    bias = (torch.rand(E, generator=g) * 2 - 1) * s
    g_out = torch.randn(U, E, generator=g)
    return states, weight, bias, g_out


def stock_padded(counts, states, weight, bias):
    """models/models.py:73-81 on the padded form; any floating dtype."""
    k = weight.shape[2]
    Ln = max(max(counts), k)
    conv = F.conv1d(pad_rows(counts, states, Ln).permute(0, 2, 1), weight, bias)
    conv = conv.masked_fill(mask_of(counts, Ln, k).to(states.device).unsqueeze(1), -float('inf'))
    return conv.max(dim=2).values


def near_ties(counts, states, weight, bias, margin=1e-5):
    k = weight.shape[2]
    Ln = max(max(counts), k)
    conv = F.conv1d(pad_rows(counts, states.double(), Ln).permute(0, 2, 1), weight.double(), bias.double())
    conv = conv.masked_fill(mask_of(counts, Ln, k).unsqueeze(1), -float('inf'))
    if conv.shape[2] < 2:
        return torch.zeros(conv.shape[:2], dtype=torch.bool)
    top = conv.topk(2, dim=2).values
    return (top[..., 0] - top[..., 1]) < margin                          # (inf - inf = nan: no tie)


def reference(counts, states, weight, bias, g_out):
    p = [t.double().requires_grad_(True) for t in (states, weight, bias)]
    out = stock_padded(counts, *p)
    g = g_out.double().masked_fill(torch.isinf(out.detach()), 0.0)       # (no gradient flows into -inf; keeps 0 x inf out of the sums)
    (out.masked_fill(torch.isinf(out.detach()), 0.0) * g).sum().backward()
    return [out.detach()] + [t.grad if t.grad is not None else torch.zeros_like(t) for t in p]


_CASES = {}


def case(name):
    """Inputs, the tie-masked g_out and the float64 reference of a case, computed once and left unchanged."""
    if name not in _CASES:
        counts, C, E, k = REFUSED if name == "refused" else CASES[name]
        states, weight, bias, g_out = inputs(counts, C, E, k)
        ties = near_ties(counts, states, weight, bias)
        g_out = g_out.masked_fill(ties, 0.0)
        _CASES[name] = dict(counts=list(counts), C=C, E=E, k=k, states=states, weight=weight, bias=bias, g_out=g_out, ties=ties,
                            ref=reference(counts, states, weight, bias, g_out))
    return _CASES[name]


def run(fn, c, device="cpu", states_of=None):
    """[out, d_states, d_weight, d_bias] of fn(states, weight, bias) on `device` with the case's g_out; states_of: another view of the
    same values (its gradient is then the leaf's)."""
    states, weight, bias = (c[n].clone().to(device).requires_grad_(True) for n in ("states", "weight", "bias"))
    out = fn(states if states_of is None else states_of(states), weight, bias)
    g = c["g_out"].to(device)
    finite = torch.isfinite(out.detach())
    (out.masked_fill(~finite, 0.0) * g.masked_fill(~finite, 0.0)).sum().backward()
    zeros = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return [out.detach(), zeros(states), zeros(weight), zeros(bias)]


def failures(got, chain, ref, label=""):
    """The outputs of `got` outside the band, as `band_failures` reports them; ("out", "-inf pattern") first where got's -inf cells are
    not the reference's."""
    inf = torch.isinf(ref[0]) & (ref[0] < 0)
    g0 = got[0].detach().cpu()
    if g0.shape != ref[0].shape or not torch.equal(torch.isinf(g0) & (g0 < 0), inf):
        print("entity_line_pool_ragged %s out: the -inf cells differ" % label)
        return [("out", "-inf pattern")]
    cut = lambda r: [r[0].detach().cpu().masked_fill(inf, 0.0)] + list(r[1:])
    return band_failures(NAMES, cut(got), cut(chain), cut(ref), "entity_line_pool_ragged " + label)


# ------------------------------------------------------------------------------------------------------------- the guard
def restate(counts, states, weight, bias, g_out, wrong=None):
    """[out, d_states, d_weight, d_bias] in the inputs' dtype, by loops in the kernels' order; `wrong`: one of WRONG."""
    E, C, k = weight.shape
    U, L = len(counts), states.shape[0]
    ptr = line_ptr_of(counts)
    if wrong == "offset by one row":
        ptr = [min(p + 1, L) for p in ptr]
    out = torch.full((U, E), -float('inf'), dtype=states.dtype)
    pos = [[NONE] * E for _ in range(U)]
    d_states = torch.zeros_like(states)
    G, per = groups_of(U) if U else (0, 1)
    slabs_w = [torch.zeros_like(weight) for _ in range(G)]
    slabs_b = [torch.zeros_like(bias) for _ in range(G)]
    for u, n in enumerate(counts):
        rows = states[ptr[u]:min(ptr[u] + n, L)]
        n = rows.shape[0]
        if wrong == "the last line dropped":
            rows, n = rows[:max(n - 1, 0)], max(n - 1, 0)
        if wrong == "the padding line included":
            rows, n = torch.cat([rows, rows.new_zeros(1, C)]), n + 1
        P = n - k + 1
        if P < 1:
            if wrong == "an entity shorter than the filter gives 0":
                out[u] = 0.0
            continue
        X = rows.unfold(0, k, 1)                                         # [P, C, k]
        acc = torch.zeros(P, E, dtype=states.dtype)
        for j in range(k):
            for c in range(C):
                acc = acc + X[:, c, j][:, None] * weight[:, c, j][None, :]
        vals = acc + bias
        best = vals.max(dim=0).values
        for e in range(E):
            hits = (vals[:, e] == best[e]).nonzero().flatten().tolist()
            pos[u][e] = hits[-1] if wrong == "the highest position on a tie" else hits[0]
        out[u] = best
        for e in range(E):
            p, g = pos[u][e], g_out[u, e].to(states.dtype)
            for j in range(k):
                if ptr[u] + p + j < L:                                   # (a wrong restatement may reach behind the last row)
                    d_states[ptr[u] + p + j] += g * weight[e, :, j]
            slabs_w[u // per][e] += g * rows[p:p + k].t()
            slabs_b[u // per][e] += g
    d_w, d_b = torch.zeros_like(weight), torch.zeros_like(bias)
    for z in range(G):
        d_w, d_b = d_w + slabs_w[z], d_b + slabs_b[z]
    return [out, d_states, d_w, d_b]


def applies(wrong, c):
    """Where a wrong restatement must show (by the case's shape alone)."""
    counts, k, E = c["counts"], c["k"], c["E"]
    return {"offset by one row": any(n == k for n in counts),           # (an entity of exactly k lines gets another window, or none)
            "the last line dropped": any(n == k for n in counts),       # (an entity of exactly k lines loses its only window: -inf)
            # (an entity one line short of the filter then has a window: a finite value where -inf belongs)
            "the padding line included": any(n == k - 1 for n in counts),
            "an entity shorter than the filter gives 0": any(n < k for n in counts),
            "the highest position on a tie": False}[wrong]               # (needs an exact tie: `tie_case`)


def tie_case():
    """Small integers for values (every sum exact in fp32 in any order); entity 0's lines 2, 3 are copies of its lines 0, 1 and entity 2's
    line 1 a copy of its line 0: their first and last positions tie exactly."""
    counts, C, E, k = [4, 1, 2, 0], 6, 2, 1
    g = torch.Generator().manual_seed(11)
    states = torch.randint(-3, 4, (sum(counts), C), generator=g).float()
    states[2:4] = states[0:2]
    states[6] = states[5]
    weight = torch.randint(-2, 3, (E, C, k), generator=g).float()
    bias = torch.randint(-2, 3, (E,), generator=g).float()
    g_out = torch.randint(1, 4, (len(counts), E), generator=g).float()
    ref = restate(counts, states.double(), weight.double(), bias.double(), g_out)
    return dict(counts=counts, C=C, E=E, k=k, states=states, weight=weight, bias=bias, g_out=g_out, ref=ref)


# ------------------------------------------------------------------------------------------------------------- the encoder
def encoder(ecfs=1, p=0.0, seed=0):
    """recon_amd's EntityEmbedding at the widths of the eac1_untied fixture (7 words of 5, 8 chars of 3, 3 char features, hidden 3, entity
    vectors of 2, char filter 2, words of 4 chars) with the reference's own entity_conv_filter_size = 1, seeded."""
    from torch import nn
    from recon_amd.gpgnn import EntityEmbedding
    torch.manual_seed(seed)
    m = EntityEmbedding(3 + 5, 3, 1, 1, p, 2, 2, ecfs, nn.Embedding(7, 5, padding_idx=0), 3, 4, list(range(8)), 3)
    m.word_embeddings.weight.requires_grad_(False)                      # the models' word table is frozen
    return m


ENCODER_COUNTS = {1: [1], 15: [4, 0, 8, 3], 16: [16], 17: [9, 8], 33: [1, 32]}     # L: either side of the line LSTM's 16-sequence tile


def encoder_inputs(counts, seed=0, tokens=3):
    """words [L, 3] and chars [L, 1 + 3 * 5] of the ragged form, ids drawn per case."""
    g = torch.Generator().manual_seed(977 * seed + sum(counts) + 13 * len(counts))
    L = sum(counts)
    return torch.randint(0, 7, (L, tokens), generator=g), torch.randint(0, 8, (L, 1 + tokens * 5), generator=g)
