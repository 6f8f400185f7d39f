"""recon_amd.relation_logits without a GPU: the import, `_chain` against the literal stock lines of the three models (bit for bit on CPU
tensors), every argument error, the shape and workspace queries of the C ABI, the header / `_lib.SYMBOLS` check of the four entries,
`GPGNN.classify` on the CPU, and the guard of the band tests/test_relation_head_gpu.py holds the kernels to.

The shapes, the input generator, the fp64 reference and the comparison live here and are imported by the GPU file.  A shape is
(M, dense widths, (K_s, Mnz) or None, N).  Inputs: block entries, scattered entries and g_out ~ N(0, 1), weight and bias uniform in
+-1 / sqrt(Kt), from a torch.Generator whose seed is mixed with the shape; positions a sorted random subset of [0, M) of the requested size
that holds 0 and M - 1 when Mnz >= 2.  Band: `op_checks.bound` of the stock fp32 chain's error on the same inputs, applied by
`op_checks.band_failures` to the value and to every gradient.  The op is linear: nothing is masked and nothing is left out of a comparison.

Guard: an fp32 CPU restatement of the algebra passes the band at every shape (e_chain is then its own error), and four wrong restatements
fail it wherever they apply: the scattered rows one row late; no bias; d_scattered taken at rows i instead of positions[i]; a block's
weight columns offset by one."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from op_checks import band_failures, entries_declared_and_bound

G_WGRAD = 8                                     # the weight-gradient pass's row groups (relation_head.WGRAD_MAX_ROW_GROUPS, asserted below)
GROUP_ROWS = 32                                 # a group holds at least this many rows: G = min(G_WGRAD, ceil(M / 32))
FIXTURE = (24, (12, 6), (3, 7), 3)              # the fixtures' widths: nothing aligned, all tails
ONE_BLOCK = (17, (20,), None, 5)                # one block, one partial tile
KGGAT = (65, (48, 40), None, 33)                # the KGGAT form, one row past a tile, N tail
REF_WIDTHS = (131, (48, 400), (353, 97), 353)   # reference widths, three row tiles, the odd block and the odd weight stride
FOUR_BLOCKS = (257, (13, 7, 4, 9), (5, 257), 70)    # four blocks, every row present, one row past 8 x 32 (the row-group rule)
REF_BATCH = (360, (48, 400), (353, 251), 353)   # the reference's own batch, B = 5
EMPTY_SCATTER = (200, (48,), (8, 0), 6)         # an empty scattered block
SHAPES = [FIXTURE, ONE_BLOCK, KGGAT, REF_WIDTHS, FOUR_BLOCKS, REF_BATCH, EMPTY_SCATTER]
CITES = "models/models.py:213, :234, :275, :693-697, :954-966"
ENTRIES = ["recon_relation_logits_supported", "recon_relation_logits_workspace_bytes", "recon_relation_logits_fwd", "recon_relation_logits_bwd"]


def shape_id(s):
    return "%d-%s-%s-%d" % (s[0], "x".join(map(str, s[1])), "none" if s[2] is None else "%dat%d" % s[2], s[3])


def width(shape):
    return sum(shape[1]) + (shape[2][0] if shape[2] else 0)


def names(shape):
    return ["out"] + ["d_block_%d" % i for i in range(len(shape[1]))] + ["d_scattered", "d_W", "d_b"]


def inputs(shape, seed=0, positions=None):
    """blocks, weight, bias, scattered, positions (both None without a scattered block) and g_out, fp32 on the CPU.  `positions`: the rows to
    use in place of the random subset."""
    M, widths, sc, N = shape
    Kt = width(shape)
    g = torch.Generator().manual_seed(100003 * seed + 7919 * M + 131 * sum((i + 2) * k for i, k in enumerate(widths)) + 17 * N
                                      + (29 * sc[0] + 31 * sc[1] if sc else 0))
    blocks = [torch.randn(M, K, generator=g) for K in widths]
    s = 1.0 / math.sqrt(Kt)
    W = (torch.rand(N, Kt, generator=g) * 2 - 1) * s
    b = (torch.rand(N, generator=g) * 2 - 1) * s
    g_out = torch.randn(M, N, generator=g)
    scattered = pos = None
    if sc:
        K_s, Mnz = sc
        if positions is not None:
            pos = torch.as_tensor(positions, dtype=torch.int64)
            assert pos.shape == (Mnz,)
        elif Mnz >= 2:
            inner = torch.randperm(M - 2, generator=g)[:Mnz - 2] + 1
            pos = torch.cat([torch.tensor([0, M - 1]), inner]).sort().values
        else:
            pos = torch.randperm(M, generator=g)[:Mnz].sort().values
        scattered = torch.randn(Mnz, K_s, generator=g)
    return blocks, W, b, scattered, pos, g_out


def chain_fn(blocks, W, b, scattered, pos):
    from recon_amd.relation_head import _chain
    return _chain(blocks, W, b, scattered, pos)


_CASES = {}


def case(shape, positions=None):
    """Inputs and the fp64 oracle [out, d_block_i..., d_scattered, d_W, d_b] of `_chain` at a shape, computed once and left unchanged."""
    key = (shape, None if positions is None else tuple(positions))
    if key not in _CASES:
        blocks, W, b, scattered, pos, g_out = inputs(shape, positions=positions)
        leaves = [t.double().requires_grad_(True) for t in blocks + [W, b] + ([scattered] if scattered is not None else [])]
        nb = len(blocks)
        out = chain_fn(leaves[:nb], leaves[nb], leaves[nb + 1], leaves[nb + 2] if scattered is not None else None, pos)
        out.backward(g_out.double())
        d_s = leaves[nb + 2].grad if scattered is not None else None
        ref = [out.detach()] + [t.grad for t in leaves[:nb]] + [d_s, leaves[nb].grad, leaves[nb + 1].grad]
        _CASES[key] = dict(shape=shape, blocks=blocks, W=W, b=b, scattered=scattered, pos=pos, g_out=g_out, ref=ref)
    return _CASES[key]


def run(fn, c, device="cpu", needs=None, block_of=None, scattered_of=None, pos_of=None):
    """[out, d_block_i..., d_scattered, d_W, d_b] of fn(blocks, W, b, scattered, positions) on `device`, with the case's g_out.  needs: which
    blocks require a gradient (default all); block_of / scattered_of: another view of the same values."""
    nb = len(c["blocks"])
    needs = [True] * nb if needs is None else needs
    blocks = [t.to(device) for t in c["blocks"]]
    blocks = [(t if block_of is None else block_of(t)).requires_grad_(n) for t, n in zip(blocks, needs)]
    W, b = c["W"].to(device).requires_grad_(True), c["b"].to(device).requires_grad_(True)
    scattered = pos = None
    if c["scattered"] is not None:
        scattered = c["scattered"].to(device)
        scattered = (scattered if scattered_of is None else scattered_of(scattered)).requires_grad_(True)
        pos = c["pos"].to(device) if pos_of is None else pos_of(c["pos"])
    out = fn(blocks, W, b, scattered, pos)
    out.backward(c["g_out"].to(device))
    return [out.detach()] + [t.grad for t in blocks] + [None if scattered is None else scattered.grad, W.grad, b.grad]


def failures(got, chain, ref, shape, label=""):
    return band_failures(names(shape), got, chain, ref, "relation_logits " + label)


def groups_of(M):
    G = max(1, min(G_WGRAD, -(-M // GROUP_ROWS)))
    per = -(-M // G)
    return -(-M // per), per


# ------------------------------------------------------------------------------------------------------------- the op on the CPU
def test_import():
    from recon_amd import relation_logits
    from recon_amd.relation_head import relation_logits as same
    assert relation_logits is same


def test_chain_is_the_stock_lines_of_the_three_models():
    from recon_amd import relation_logits

    def gpgnn(blocks, W, b, scattered, pos):                             # models/models.py:213, :234, :275
        return F.linear(blocks[0], W, b)

    def kggat(blocks, W, b, scattered, pos):                             # :693-697
        both = torch.cat([blocks[0], blocks[1]], dim=-1)
        return F.linear(both, W, b)

    def recon(blocks, W, b, scattered, pos):                             # :954-966
        relation, gat = blocks
        scores = torch.zeros(relation.shape[0], scattered.shape[1], device=relation.device, dtype=relation.dtype)
        if scattered.shape[0] > 0:
            scores = scores.index_put((pos,), scattered)
        return F.linear(torch.cat([relation, gat, scores], dim=-1), W, b)
    empty = (40, (48, 400), (5, 0), 7)
    for literal, shape in ((gpgnn, ONE_BLOCK), (kggat, KGGAT), (recon, REF_WIDTHS), (recon, empty)):
        c = case(shape)
        want = run(literal, c)
        for fn in (chain_fn, relation_logits):                          # CPU tensors: the op runs the chain
            got = run(fn, c)
            assert len(got) == len(want) == len(shape[1]) + 4
            for u, v in zip(got, want):
                assert (u is None) == (v is None) and (u is None or torch.equal(u, v))
    # a leading shape of two dimensions, no bias, positions as a list
    c = case(FIXTURE)
    b3 = [t.reshape(4, 6, -1) for t in c["blocks"]]
    out = relation_logits(b3, c["W"], None, c["scattered"], c["pos"].tolist())
    assert out.shape == (4, 6, 3)
    assert torch.equal(out.reshape(24, 3), recon(c["blocks"], c["W"], None, c["scattered"], c["pos"]))
    assert torch.equal(relation_logits(c["blocks"][0], c["W"][:, :12]), F.linear(c["blocks"][0], c["W"][:, :12]))     # a lone tensor is one block


def test_argument_errors():
    from recon_amd import relation_logits
    blocks, W, b, scattered, pos, _ = inputs(FIXTURE)
    M = FIXTURE[0]
    late = pos.tolist()
    late[-1] = M
    twice = pos.tolist()
    twice[2] = twice[1]
    bad = [lambda: relation_logits(blocks, W[:, :-1], b, scattered, pos),                     # widths that do not add up to the weight's
           lambda: relation_logits(blocks, W, b),                                             # ... without the scattered block
           lambda: relation_logits(blocks, W, b, scattered, twice),                           # not strictly increasing
           lambda: relation_logits(blocks, W, b, scattered, pos.flip(0).tolist()),
           lambda: relation_logits(blocks, W, b, scattered, np.asarray(twice)),
           lambda: relation_logits(blocks, W, b, scattered, None),                            # one of the pair missing
           lambda: relation_logits(blocks, W, b, None, pos),
           lambda: relation_logits(blocks, W, b, scattered, late),                            # a position >= M
           lambda: relation_logits(blocks, W, b, scattered, [-1] + pos.tolist()[1:]),
           lambda: relation_logits(blocks, W, b, scattered, pos[:-1]),                        # not one per row
           lambda: relation_logits(blocks, W, b, scattered, pos.float()),
           lambda: relation_logits([], W, b),
           lambda: relation_logits(blocks * 3, W, b),                                         # more than four dense blocks
           lambda: relation_logits([blocks[0], blocks[1][:5]], W, b, scattered, pos),         # not one leading shape
           lambda: relation_logits([blocks[0], blocks[1].double()], W, b, scattered, pos),
           lambda: relation_logits([blocks[0].numpy()], W, b),
           lambda: relation_logits(blocks, W, b[:2], scattered, pos),
           lambda: relation_logits(blocks, W.double(), b, scattered, pos),
           lambda: relation_logits(blocks, W, b, scattered[0], pos)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError, match="relation_logits"):
            f()
            pytest.fail("case %d raised nothing" % i)
    with pytest.raises(ValueError, match=r"\[N, 21\].*\[12, 6\].*\(3, 20\)"):                  # the shapes are in the text
        relation_logits(blocks, W[:, :-1], b, scattered, pos)
    with pytest.raises(ValueError, match=r"\[0, 24\)"):
        relation_logits(blocks, W, b, scattered, late)


def test_shape_queries_and_row_split_are_the_librarys():
    from recon_amd import _lib, relation_head
    L = _lib.lib()
    assert relation_head.WGRAD_MAX_ROW_GROUPS == G_WGRAD
    ok = L.recon_relation_logits_supported
    assert all(ok(s[0], len(s[1]), width(s), s[3]) for s in SHAPES)
    assert ok(2 ** 24, 4, 2048, 1024) and ok(0, 1, 1, 1) and ok(3600, 2, 801, 353) and ok(7, 3, 1001, 1023)
    assert not ok(2 ** 24 + 1, 2, 801, 353) and not ok(5, 0, 8, 1) and not ok(5, 5, 8, 1) and not ok(5, 1, 0, 1) and not ok(5, 1, 2049, 1)
    assert not ok(5, 1, 8, 0) and not ok(5, 1, 8, 1025) and not ok(-1, 1, 8, 1)
    ws = L.recon_relation_logits_workspace_bytes
    for nb, Kt, N in ((2, 801, 353), (1, 20, 5), (3, 21, 3)):
        slab = N * (Kt + 1) * 4
        for M in (1, 31, 32, 33, 64, 65, 255, 256, 257, 360, 3600, 2 ** 24):
            G, per = groups_of(M)
            assert ws(M, nb, Kt, N, 1) == -(-G * slab // 16) * 16, (M, G)
            assert ws(M, nb, Kt, N, 0) <= 8 * M + 4 * N * (Kt + 3)
    assert ws(3600, 2, 801, 353, 1) == 8 * 353 * 802 * 4 == ws(360, 2, 801, 353, 1)           # whatever B is
    assert groups_of(257) == (8, 33) and groups_of(3600) == (8, 450) and groups_of(17) == (1, 17) and groups_of(65) == (3, 22)
    assert ws(0, 2, 801, 353, 1) == 0 and ws(5, 5, 8, 1, 1) == 0


def test_the_four_entries_are_declared_bound_and_cite_the_reference():
    entries_declared_and_bound(ENTRIES, CITES)


# ------------------------------------------------------------------------------------------------------------- the model's method
def _gpgnn(n_in):
    from recon_amd.gpgnn import GPGNN
    torch.manual_seed(5)
    p = {"max_num_nodes": 3, "embedding_dim": 2, "layer_number": 2, "projection_style": "untie", "non-linear1": "relu", "non-linear": "tanh",
         "dropout1": 0.5, "position_emb": 3, "units1": 4, "rnn1_layers": 1, "bidirectional": 1, "batch_size": 2}
    m = GPGNN(p, np.random.RandomState(0).randn(9, 5).astype("float32"), max_sent_len=4, n_out=3)
    m.linear3 = nn.Linear(n_in, 3)
    m.W_ent2rel = torch.zeros(3, 2, 2)
    return m


@pytest.mark.parametrize("fused", [False, True])
def test_classify_gives_todays_tensors_on_the_cpu(fused):
    from recon_amd.gpgnn import GPGNN
    assert isinstance(GPGNN.fused_classifier, bool)
    g = torch.Generator().manual_seed(3)
    relation, gat, scores, pos = torch.randn(12, 8, generator=g), torch.randn(12, 6, generator=g), torch.randn(4, 3, generator=g), torch.tensor([0, 3, 4, 11])
    m = _gpgnn(8)
    m.fused_classifier = fused
    assert torch.equal(m.classify(relation), m.linear3(relation))
    m = _gpgnn(14)
    m.fused_classifier = fused
    assert torch.equal(m.classify(relation, gat), m.linear3(torch.cat([relation, gat], dim=-1)))
    m = _gpgnn(17)
    m.fused_classifier = fused
    block = torch.zeros(12, 3).index_put((pos,), scores)
    want = m.linear3(torch.cat([relation, gat, block], dim=-1))
    called = []
    assert torch.equal(m.classify(relation, gat, lambda: called.append(1) or scores, pos), want) and called == [1]
    assert torch.equal(m.classify(relation, gat, scores, pos), want)
    none = m.linear3(torch.cat([relation, gat, torch.zeros(12, 3)], dim=-1))
    assert torch.equal(m.classify(relation, gat, lambda: pytest.fail("no position: no scores"), pos[:0]), none)

    class Twice(nn.Module):                                              # a replaced classifier still works: the stock calls
        def __init__(self, lin):
            super().__init__()
            self.lin = lin

        def forward(self, v):
            return 2 * self.lin(v)
    m.linear3 = Twice(m.linear3)
    assert torch.equal(m.classify(relation, gat, scores, pos), 2 * want)


# ------------------------------------------------------------------------------------------------------------- the band's guard
WRONG = ("scattered rows one row late", "no bias", "d_scattered at rows i", "a block's weight columns offset by one")


def restated(c, wrong=None):
    """The op's algebra in fp32 torch on the CPU, block by block (torch's own summation order inside a product; d_b by row groups as the
    kernels cut them)."""
    shape, blocks, W, b, scattered, pos, g = c["shape"], c["blocks"], c["W"], c["b"], c["scattered"], c["pos"], c["g_out"]
    M, widths = shape[0], shape[1]
    cols, cb = [], 0
    for K in widths:
        cols.append((cb, cb + K))
        cb += K
    Kt = W.shape[1]
    shifted = len(widths) - 1                                           # the block whose columns the fourth wrong form misplaces

    def w_of(i):
        lo, hi = cols[i]
        if wrong == "a block's weight columns offset by one" and i == shifted:
            if lo > 0:
                return W[:, lo - 1:hi - 1]
            return W[:, lo + 1:hi + 1] if hi + 1 <= Kt else torch.roll(W[:, lo:hi], 1, dims=1)
        return W[:, lo:hi]
    out = torch.zeros(M, W.shape[0])
    for i, x in enumerate(blocks):
        out = out + x @ w_of(i).t()
    d_blocks = [g @ w_of(i) for i in range(len(blocks))]
    d_W = [g.t() @ x for x in blocks]
    d_s = None
    if scattered is not None:
        Ws = W[:, cb:]
        rows = (pos + 1) % M if wrong == "scattered rows one row late" else pos
        part = torch.zeros_like(out)
        part[rows] = scattered @ Ws.t()
        out = out + part
        if pos.shape[0]:                                                # (an empty block takes no part: no gradient, as in the stock lines)
            d_s = (g[:pos.shape[0]] if wrong == "d_scattered at rows i" else g[pos]) @ Ws
        d_W.append(g[pos].t() @ scattered)
    if wrong != "no bias":
        out = out + b
    G, per = groups_of(M)
    d_b = torch.zeros(W.shape[0])
    for z in range(G):
        d_b = d_b + g[z * per:(z + 1) * per].sum(0)
    return [out] + d_blocks + [d_s, torch.cat(d_W, dim=1), d_b]


def applies(wrong, shape):
    sc = shape[2]
    return {"scattered rows one row late": bool(sc) and sc[1] > 0, "d_scattered at rows i": bool(sc) and 0 < sc[1] < shape[0]}.get(wrong, True)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fp32_restatement_passes_the_band_and_wrong_ones_fail(shape):
    c = case(shape)
    good = restated(c)
    assert not failures(good, good, c["ref"], shape, "%s stand-in" % shape_id(shape))
    for wrong in WRONG:
        if applies(wrong, shape):
            assert failures(restated(c, wrong), good, c["ref"], shape, "%s %s" % (shape_id(shape), wrong)), \
                "%s stays inside the band at %s" % (wrong, shape_id(shape))


def test_every_wrong_restatement_applies_somewhere_and_positions_are_as_promised():
    for wrong in WRONG:
        assert sum(applies(wrong, s) for s in SHAPES) >= 3, wrong
    for shape in SHAPES:
        if shape[2]:
            pos, (K_s, Mnz) = case(shape)["pos"], shape[2]
            assert pos.shape == (Mnz,) and pos.dtype == torch.int64 and (pos[1:] > pos[:-1]).all()
            assert Mnz < 2 or (pos[0] == 0 and pos[-1] == shape[0] - 1)
    a, b = inputs(FIXTURE), inputs((24, (12, 6), (3, 8), 3))
    assert not torch.equal(a[0][0], b[0][0])                            # the seed is mixed with the shape
