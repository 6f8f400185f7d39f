"""recon_amd.entity_line_pool without a GPU: the import, CPU tensors against the stock lines of models/models.py:73-81 bit for bit, every
argument error, the empty batch, the fully masked entity, the exact tie, the shape and workspace queries of the C ABI, the header /
`_lib.SYMBOLS` check of the four entries, the switch in `EntityEmbedding.forward`, and the guard of the band
tests/test_line_pool_gpu.py holds the kernels to.

The shapes, the input generator, the stock lines, the near-tie rule, the fp64 reference and the comparison live here and are imported by
the GPU file.  A shape is (U, Ln, C, E, k).  Inputs: states and g_out ~ N(0, 1), weight and bias uniform in +-1 / sqrt(C k), a suffix mask
with 1..P valid positions per entity (P = Ln - k + 1), from a torch.Generator whose seed is mixed with the shape.  Band:
`op_checks.bound` of the stock fp32 chain's error on the same inputs, applied by `op_checks.band_failures` to the value and to the three
gradients.

The maximum is a discrete choice: where the two best unmasked positions of an output are closer than fp32 rounding, fp32 may pick another
position than fp64 and the gradients then differ discretely, which is not an error.  As tests/test_char_features_gpu.py does, g_out is
zeroed in every cell (u, e) where in fp64 the best and the second-best unmasked positions are closer than 1e-5, and at most 1 % of a
shape's cells may be such (asserted here; with these inputs none is).

Guard: an fp32 CPU restatement of the op's definition (unfold, one product, the lowest maximal unmasked position, the three sums) passes
the band at every shape, and five wrong restatements fail it wherever they apply: the mask ignored; the bias dropped; the filter taps
reversed; the maximum over Ln instead of P positions (the states padded with zero lines); and, on a constructed exact tie, the gradient
sent to the last maximal position."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import load_golden
from op_checks import band_failures, entries_declared_and_bound

G_CAP = 256                                     # the backward's entity groups (line_pool.MAX_ENTITY_GROUPS, asserted below)
NONE = 255                                      # the position byte of an output without an unmasked position
SMALLEST = (1, 1, 1, 1, 1)
FIXTURE = (3, 4, 6, 2, 2)                       # the fixtures' own widths
K_IS_LN = (4, 5, 3, 2, 5)                       # k = Ln: one position
SMALL_ODD = (5, 7, 5, 3, 3)
UNALIGNED = (9, 33, 37, 17, 4)                  # nothing aligned; 33 x 17 cells: three cells per thread
REF_WIDTHS = (17, 32, 100, 8, 1)                # the reference's widths
BYTE_LIMIT = (6, 255, 8, 4, 1)                  # P at the position byte's limit
LONG_THIN = (1029, 3, 4, 5, 2)                  # 206 entity groups: 205 of 5 entities, the last of 4
# where the kernels take another path (csrc/line_pool.hip: 1024 cells per position chunk, 12288 staged floats, a staged weight up to 8192
# floats, 16 entities per chunk of the backward, 1024 slab cells per pass)
POSITION_CHUNKS = (3, 70, 5, 17, 2)             # 69 x 17 cells: two position chunks (60 + 9), the weight staged once
REDUCTION_CHUNKS = (3, 31, 260, 33, 1)          # 260 = 191 + 69: two reduction chunks; 33 x 260 > 8192: the backward reads the weight in place
BOTH_CHUNKS = (2, 40, 130, 33, 2)               # two position chunks (31 + 8) of two reduction chunks each
ENTITY_CHUNKS = (4400, 2, 3, 2, 1)              # 245 groups of 18 entities (the last of 8): 16 + 2 through the backward's LDS
SHAPES = [SMALLEST, FIXTURE, K_IS_LN, SMALL_ODD, UNALIGNED, REF_WIDTHS, BYTE_LIMIT, LONG_THIN, POSITION_CHUNKS, REDUCTION_CHUNKS, BOTH_CHUNKS,
          ENTITY_CHUNKS]
NAMES = ("out", "d_states", "d_weight", "d_bias")
CITES = "models/models.py:73-81"
ENTRIES = ["recon_line_pool_supported", "recon_line_pool_workspace_bytes", "recon_line_pool_fwd", "recon_line_pool_bwd"]
MAX_TIE_SHARE = 0.01


def shape_id(s):
    return "x".join(map(str, s))


def inputs(U, Ln, C, E, k, seed=0):
    """states, weight, bias, mask, g_out: fp32 (and bool) on the CPU."""
    g = torch.Generator().manual_seed(100003 * seed + 7919 * U + 131 * Ln + 17 * C + 29 * E + 31 * k)
    P = Ln - k + 1
    states = torch.randn(U, Ln, C, generator=g)
    s = 1.0 / math.sqrt(C * k)
    weight = (torch.rand(E, C, k, generator=g) * 2 - 1) * s
    bias = (torch.rand(E, generator=g) * 2 - 1) * s
    valid = torch.randint(1, P + 1, (U,), generator=g)
    mask = torch.arange(P)[None, :] >= valid[:, None]
    g_out = torch.randn(U, E, generator=g)
    return states, weight, bias, mask, g_out


def stock(states, weight, bias, mask):
    """models/models.py:73-81 as recon_amd/gpgnn.py runs them without the op; any floating dtype."""
    conv = F.conv1d(states.permute(0, 2, 1), weight, bias)
    conv = conv.masked_fill(mask.unsqueeze(1), -float('inf'))
    return conv.max(dim=2).values


def near_ties(states, weight, bias, mask, margin=1e-5):
    """bool [U, E]: in fp64 the best and the second-best unmasked positions are closer than `margin`."""
    conv = F.conv1d(states.double().permute(0, 2, 1), weight.double(), bias.double()).masked_fill(mask.unsqueeze(1), -float('inf'))
    if conv.shape[2] < 2:
        return torch.zeros(conv.shape[:2], dtype=torch.bool)
    top = conv.topk(2, dim=2).values
    return (top[..., 0] - top[..., 1]) < margin                          # (inf - inf = nan: a fully masked entity has no tie)


_CASES = {}


def case(shape):
    """Inputs, the tie-masked g_out and the fp64 oracle [out, d_states, d_weight, d_bias] of `stock` at a shape, computed once and left
    unchanged."""
    if shape not in _CASES:
        states, weight, bias, mask, g_out = inputs(*shape)
        ties = near_ties(states, weight, bias, mask)
        g_out = g_out.masked_fill(ties, 0.0)
        _CASES[shape] = dict(shape=shape, states=states, weight=weight, bias=bias, mask=mask, g_out=g_out, ties=ties,
                             ref=reference(stock, states, weight, bias, mask, g_out))
    return _CASES[shape]


def reference(fn, states, weight, bias, mask, g_out):
    p = [t.double().requires_grad_(True) for t in (states, weight, bias)]
    out = fn(*p, mask)
    out.backward(g_out.double())
    return [out.detach()] + [t.grad for t in p]


def run(fn, c, device="cpu", needs=(True, True, True), states_of=None, mask=None):
    """[out, d_states, d_weight, d_bias] of fn(states, weight, bias, mask) on `device` with the case's g_out.  needs: which of the three
    inputs require a gradient; states_of: another view of the same values; mask: another mask."""
    states, weight, bias = (c[k].clone().to(device) for k in ("states", "weight", "bias"))      # (fresh leaves: the case stays unchanged)
    states = (states if states_of is None else states_of(states)).requires_grad_(needs[0])
    weight, bias = weight.requires_grad_(needs[1]), bias.requires_grad_(needs[2])
    out = fn(states, weight, bias, (c["mask"] if mask is None else mask).to(device))
    out.backward(c["g_out"].to(device))
    return [out.detach(), states.grad, weight.grad, bias.grad]


def failures(got, chain, ref, label=""):
    return band_failures(NAMES, got, chain, ref, "entity_line_pool " + label)


def groups_of(U):
    per = -(-U // min(G_CAP, U))
    return -(-U // per), per


def definition(states, weight, bias, mask, g_out, wrong=None):
    """[out, d_states, d_weight, d_bias, positions] by the op's definition, in the inputs' dtype, independent of `stock`: every (position,
    channel) sum from the unfolded states, the LOWEST maximal unmasked position, the gradients through that position alone."""
    U, Ln, C = states.shape
    E, _, k = weight.shape
    if wrong == "the mask ignored":
        mask = torch.zeros_like(mask)
    if wrong == "the filter taps reversed":
        weight = weight.flip(2)
    if wrong == "the maximum over Ln positions":
        states = torch.cat([states, states.new_zeros(U, k - 1, C)], dim=1)
        mask = torch.cat([mask, mask.new_zeros(U, k - 1)], dim=1)
    P = states.shape[1] - k + 1
    X = states.unfold(1, k, 1)                                           # [U, P, C, k]
    vals = torch.einsum("upcj,ecj->upe", X, weight)
    if wrong != "the bias dropped":
        vals = vals + bias
    vals = vals.masked_fill(mask.unsqueeze(2), -float('inf'))
    out = vals.max(dim=1).values
    hit = (vals == out.unsqueeze(1)) & ~mask.unsqueeze(2)
    at = torch.arange(P).view(1, P, 1).expand(U, P, E)
    if wrong == "the gradient to the last maximal position":
        pos = torch.where(hit, at, torch.full_like(at, -1)).max(dim=1).values
        pos = torch.where(pos < 0, torch.full_like(pos, NONE), pos)
    else:
        pos = torch.where(hit, at, torch.full_like(at, NONE)).min(dim=1).values
    gv = (at == pos.unsqueeze(1)).to(states.dtype) * g_out.to(states.dtype).unsqueeze(1)      # [U, P, E]: g_out at the winning position
    d_X = torch.einsum("upe,ecj->upcj", gv, weight)
    d_states = torch.zeros_like(states)
    for j in range(k):
        d_states[:, j:j + P] += d_X[..., j]
    d_weight = torch.einsum("upe,upcj->ecj", gv, X)
    if wrong == "the filter taps reversed":
        d_weight = d_weight.flip(2)
    return [out, d_states[:, :Ln], d_weight, gv.sum((0, 1)), pos]


# ------------------------------------------------------------------------------------------------------------- the op on the CPU
def test_import():
    from recon_amd import entity_line_pool
    from recon_amd.line_pool import entity_line_pool as same
    assert entity_line_pool is same


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_cpu_tensors_run_the_stock_lines_bit_for_bit(shape):
    from recon_amd import entity_line_pool
    from recon_amd.line_pool import _chain
    c = case(shape)
    want = run(stock, c)
    for fn in (_chain, entity_line_pool):
        got = run(fn, c)
        assert got[0].shape == (shape[0], shape[3])
        for a, b in zip(got, want):
            assert torch.equal(a, b)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_near_ties_are_rare_and_fp32_picks_fp64s_position(shape):
    c = case(shape)
    share = c["ties"].float().mean().item()
    print("entity_line_pool %s: %d of %d cells near a tie" % (shape_id(shape), int(c["ties"].sum()), c["ties"].numel()))
    assert share <= MAX_TIE_SHARE, share
    args = (c["states"], c["weight"], c["bias"], c["mask"], c["g_out"])
    p32 = definition(*args)[4]
    p64 = definition(*[t.double() if t.is_floating_point() else t for t in args])[4]
    assert torch.equal(p32[~c["ties"]], p64[~c["ties"]])
    assert (p64 != NONE).all()                                           # every entity has a valid position
    valid = (~c["mask"]).sum(1)
    assert valid.min() >= 1 and (shape[0] < 4 or shape[1] - shape[4] < 1 or valid.max() > valid.min())
    assert torch.equal(c["mask"], torch.arange(c["mask"].shape[1])[None, :] >= valid[:, None])      # a suffix


def test_the_seed_is_mixed_with_the_shape():
    assert not torch.equal(inputs(3, 4, 6, 2, 2)[0][:, :3], inputs(3, 5, 6, 2, 2)[0][:, :3])
    assert torch.equal(inputs(3, 4, 6, 2, 2)[0], inputs(3, 4, 6, 2, 2)[0])


def test_argument_errors():
    from recon_amd import entity_line_pool
    s, w, b, m, _ = inputs(*FIXTURE)
    bad = [lambda: entity_line_pool(s[0], w, b, m),                       # not [U, Ln, C]
           lambda: entity_line_pool(s, w[0], b, m),
           lambda: entity_line_pool(s, w[:, :5], b, m),                   # C of the states and of the filters differ
           lambda: entity_line_pool(s[:, :1], w, b, m[:, :0]),            # k > Ln
           lambda: entity_line_pool(s, w, b[:1], m),
           lambda: entity_line_pool(s, w, b.view(1, 2), m),
           lambda: entity_line_pool(s, w.double(), b, m),
           lambda: entity_line_pool(s, w, b.double(), m),
           lambda: entity_line_pool(s.long(), w, b, m),
           lambda: entity_line_pool(s, w, b, m.float()),                  # not bool
           lambda: entity_line_pool(s, w, b, m[:, :2]),                   # not [U, Ln - k + 1]
           lambda: entity_line_pool(s, w, b, m[:2]),
           lambda: entity_line_pool(s, w, b, torch.zeros(3, 4, dtype=torch.bool)),       # [U, Ln]: the mask of the lines, not of the positions
           lambda: entity_line_pool(s.numpy(), w, b, m),
           lambda: entity_line_pool(s, w, None, m)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError, match="entity_line_pool"):
            f()
            pytest.fail("case %d raised nothing" % i)
    with pytest.raises(ValueError, match=r"\[3, 3\].*\(3, 4, 6\).*\(2, 6, 2\).*\(3, 4\)"):    # the shapes are in the text
        entity_line_pool(s, w, b, torch.zeros(3, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"C = 6.*Ln = 4.*\(2, 5, 2\)"):
        entity_line_pool(s, w[:, :5], b, m)


def test_empty_batch():
    from recon_amd import entity_line_pool
    s, w, b, m, _ = inputs(*FIXTURE)
    w.requires_grad_(True)
    out = entity_line_pool(s[:0], w, b, m[:0])
    assert out.shape == (0, 2) and out.dtype == torch.float32


def test_a_fully_masked_entity_gives_minus_infinity_and_zero_gradients():
    from recon_amd import entity_line_pool
    c = case(SMALL_ODD)
    mask = c["mask"].clone()
    mask[2] = True
    for fn in (entity_line_pool, lambda *a: definition(*a, c["g_out"])[0]):
        out = fn(c["states"], c["weight"], c["bias"], mask)
        assert torch.isinf(out[2]).all() and (out[2] < 0).all() and torch.isfinite(out[[0, 1, 3, 4]]).all()
    got = run(entity_line_pool, c, mask=mask)
    want = definition(c["states"], c["weight"], c["bias"], mask, c["g_out"])
    assert torch.count_nonzero(got[1][2]) == 0 and torch.count_nonzero(want[1][2]) == 0 and (want[4][2] == NONE).all()
    others = c["g_out"].clone()
    others[2] = 0
    assert torch.allclose(got[3], others.sum(0), atol=1e-6) and torch.allclose(want[3], others.sum(0), atol=1e-6)
    for a, b in zip(got, want[:4]):
        assert torch.allclose(a, b, atol=1e-5)


def tie_case():
    """FIXTURE's shape with small integers for values (every sum exact in fp32 in any order) and lines 2, 3 copies of lines 0, 1: positions
    0 and 2 of every entity tie exactly; entity 1's position 0 is masked, so its first maximal unmasked position may be 2."""
    U, Ln, C, E, k = FIXTURE
    g = torch.Generator().manual_seed(11)
    states = torch.randint(-3, 4, (U, Ln, C), generator=g).float()
    states[:, 2:4] = states[:, 0:2]
    weight = torch.randint(-2, 3, (E, C, k), generator=g).float()
    bias = torch.randint(-2, 3, (E,), generator=g).float()
    mask = torch.zeros(U, Ln - k + 1, dtype=torch.bool)
    mask[1, 0] = True
    g_out = torch.randint(1, 4, (U, E), generator=g).float()
    ref = definition(states.double(), weight.double(), bias.double(), mask, g_out)
    return dict(shape=FIXTURE, states=states, weight=weight, bias=bias, mask=mask, g_out=g_out, ref=ref[:4], pos=ref[4])


def test_an_exact_tie_takes_the_lowest_position():
    c = tie_case()
    vals = torch.einsum("upcj,ecj->upe", c["states"].unfold(1, 2, 1), c["weight"]) + c["bias"]
    assert torch.equal(vals[:, 0], vals[:, 2])
    won_by_the_pair = vals[:, 0] > vals[:, 1]
    assert won_by_the_pair[0].any() or won_by_the_pair[2].any()          # the tie decides at least one output
    assert (c["pos"][[0, 2]][won_by_the_pair[[0, 2]]] == 0).all() and (c["pos"][1][won_by_the_pair[1]] == 2).all()
    good = definition(c["states"], c["weight"], c["bias"], c["mask"], c["g_out"])[:4]
    assert not failures(good, good, c["ref"], "exact tie stand-in")
    last = definition(c["states"], c["weight"], c["bias"], c["mask"], c["g_out"], "the gradient to the last maximal position")[:4]
    bad = failures(last, good, c["ref"], "exact tie, the gradient to the last maximal position")
    assert [b[0] for b in bad] == ["d_states"], bad                      # (d_weight reads equal lines at either position)


# ------------------------------------------------------------------------------------------------------------- the library's queries
def test_shape_queries_and_entity_groups_are_the_librarys():
    from recon_amd import _lib, line_pool
    L = _lib.lib()
    assert line_pool.MAX_ENTITY_GROUPS == G_CAP and line_pool.NO_POSITION == NONE
    ok = L.recon_line_pool_supported
    assert all(ok(*s) for s in SHAPES)
    assert ok(450, 32, 100, 8, 1) and ok(0, 32, 100, 8, 1) and ok(2 ** 30, 255, 1024, 64, 1) and ok(5, 258, 256, 64, 4) and ok(5, 300, 4, 1, 46)
    assert not ok(5, 256, 8, 4, 1) and not ok(5, 32, 1025, 8, 1) and not ok(5, 32, 513, 8, 2) and not ok(5, 32, 100, 65, 1)
    assert not ok(5, 4, 6, 2, 5) and not ok(5, 4, 6, 2, 0) and not ok(5, 4, 6, 0, 1) and not ok(5, 4, 0, 2, 1) and not ok(-1, 4, 6, 2, 1)
    ws = L.recon_line_pool_workspace_bytes
    for Ln, C, E, k in ((32, 100, 8, 1), (3, 4, 5, 2), (7, 5, 3, 3)):
        slab = E * (C * k + 1) * 4
        for U in (1, 2, 255, 256, 257, 450, 511, 512, 513, 1029, 10 ** 6):
            G, per = groups_of(U)
            assert ws(U, Ln, C, E, k) == -(-G * slab // 16) * 16, (U, G)
    assert groups_of(450) == (225, 2) and groups_of(256) == (256, 1) and groups_of(257) == (129, 2) and groups_of(10 ** 6) == (256, 3907)
    U, Ln, C, E, k = LONG_THIN
    G, per = groups_of(U)
    assert (G, per) == (206, 5) and 1 < per and 0 < U - (G - 1) * per < per        # several groups of more than one entity, the last short
    assert ws(*LONG_THIN) == -(-G * E * (C * k + 1) * 4 // 16) * 16
    assert ws(0, 32, 100, 8, 1) == 0 and ws(5, 256, 8, 4, 1) == 0


def test_status_codes_before_any_launch():
    from recon_amd import _lib
    L = _lib.lib()
    fake = 16                                                            # never dereferenced: every call returns before a launch
    fwd = lambda U, Ln, k: L.recon_line_pool_fwd(fake, 6, fake, fake, fake, U, Ln, 6, 2, k, fake, fake, None)
    assert fwd(0, 4, 2) == 0 and fwd(3, 4, 5) == -1 and fwd(-1, 4, 2) == -1 and fwd(3, 256, 1) == -2
    assert L.recon_line_pool_fwd(fake, 5, fake, fake, fake, 3, 4, 6, 2, 2, fake, fake, None) == -1          # a row stride below C
    bwd = lambda U, Ln, k, nbytes: L.recon_line_pool_bwd(fake, 6, fake, fake, fake, U, Ln, 6, 2, k, fake, fake, fake, fake, nbytes, None)
    assert bwd(3, 4, 5, 1 << 20) == -1 and bwd(3, 256, 1, 1 << 20) == -2 and bwd(3, 4, 2, 16) == -4
    assert L.recon_line_pool_bwd(fake, 6, fake, fake, fake, 3, 4, 6, 2, 2, None, None, None, None, 0, None) == 0       # nothing wanted


def test_the_four_entries_are_declared_bound_and_cite_the_reference():
    entries_declared_and_bound(ENTRIES, CITES)


# ------------------------------------------------------------------------------------------------------------- the model's switch
def _entity_embedding():
    from test_char_features_cpu import fixture_model
    g = load_golden("char_features1_eval")
    return fixture_model(g), [torch.from_numpy(g[k]) for k in ("words", "chars", "mask")]


def test_entity_embedding_switch(monkeypatch):
    from recon_amd import gpgnn
    assert isinstance(gpgnn.EntityEmbedding.fused_line_pool, bool)
    m, args = _entity_embedding()
    calls = []
    real = gpgnn.entity_line_pool
    monkeypatch.setattr(gpgnn, "entity_line_pool", lambda *a: calls.append(1) or real(*a))
    m.fused_line_pool = False
    want = m(*args)
    assert not calls
    m.fused_line_pool = True
    assert torch.equal(m(*args), want) and len(calls) == 1               # CPU tensors: the op runs the stock lines

    class Scaled(nn.Conv1d):                                             # not a plain nn.Conv1d: the old lines, through the module
        def forward(self, x):
            return 2 * super().forward(x)
    plain = m.conv1d_entity
    E, C, k = plain.weight.shape
    m.conv1d_entity = Scaled(C, E, k)
    m.conv1d_entity.load_state_dict(plain.state_dict())
    out = m(*args)
    assert len(calls) == 1 and torch.allclose(out, 2 * want, atol=1e-6)
    U, Ln = args[0].shape[:2]
    for kw in (dict(padding=1), dict(dilation=2), dict(stride=2), dict(groups=2), dict(bias=False)):     # plain, but not what the op computes
        if kw.get("groups", 1) > 1 and (C % 2 or E % 2):
            continue
        m.conv1d_entity = nn.Conv1d(C, E, 1 if "dilation" in kw and Ln < 2 * k - 1 else k, **kw)
        positions = m.conv1d_entity(torch.zeros(1, C, Ln)).shape[2]
        out = m(args[0], args[1], torch.zeros(U, positions, dtype=torch.bool))
        assert len(calls) == 1 and out.shape == (U, E), kw
    m.conv1d_entity = plain
    assert torch.equal(m(*args), want) and len(calls) == 2


# ------------------------------------------------------------------------------------------------------------- the band's guard
WRONG = ("the mask ignored", "the bias dropped", "the filter taps reversed", "the maximum over Ln positions")


def applies(wrong, shape):
    U, Ln, C, E, k = shape
    return {"the mask ignored": Ln - k + 1 > 1, "the filter taps reversed": k > 1, "the maximum over Ln positions": k > 1}.get(wrong, True)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fp32_restatement_passes_the_band_and_wrong_ones_fail(shape):
    c = case(shape)
    args = (c["states"], c["weight"], c["bias"], c["mask"], c["g_out"])
    good = definition(*args)[:4]
    assert not failures(good, good, c["ref"], "%s stand-in" % shape_id(shape))
    for wrong in WRONG:
        if applies(wrong, shape):
            assert failures(definition(*args, wrong)[:4], good, c["ref"], "%s %s" % (shape_id(shape), wrong)), \
                "%s stays inside the band at %s" % (wrong, shape_id(shape))


def test_every_wrong_restatement_applies_somewhere():
    for wrong in WRONG:
        assert sum(applies(wrong, s) for s in SHAPES) >= 4, wrong
