"""recon_amd.char_word_features with a PackedKeep (csrc/char_mask.hip: the masked char-CNN kernels and the bit draw) against the stock
sequence of models/models.py:57-61 with the same dropout factors in fp64 on the CPU, and against the training fixture written from the
reference's EntityEmbedding.

Tolerance: `op_checks.bound` of the error of the stock chain (fp32, same factors), run in the same test.

Gradient cells near a tie: g_out is zeroed at every (s, w, o) where, in fp64, the window's maximum and a position whose MASKED ROWS
X[t .. t + cfs) differ from the winner's are closer than 1e-5.  Rows are compared, not ids: all-masked and all-padding positions tie
exactly at the bias, and both sides pick the first.  At most 1 % of the cells may be zeroed.

The draw is checked against a numpy restatement of its definition (include/recon_hip.h, recon_char_keep_bits_draw) written out here."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from op_checks import band_failures, bound, calls_of, close, dev, peak_bytes, rel_err, rounded, same
from test_char_features_cpu import fixture_model, inputs
from test_char_features_gpu import REF_GEOMETRY, case, run

pytestmark = pytest.mark.gpu

#        S    W  max_char cfs C   Fo  V
CASES = [(1, 1, 1, 1, 1, 1, 2), (3, 3, 4, 3, 5, 6, 9), (24, 5, 4, 2, 3, 3, 8), (7, 2, 10, 3, 50, 50, 90), (65, 4, 6, 5, 33, 65, 40),
         (9, 3, 4, 3, 64, 8, 700), REF_GEOMETRY]
REF_WIDTHS, SLAB_SHAPE = (7, 2, 10, 3, 50, 50, 90), (9, 3, 4, 3, 64, 8, 700)
PARAMS = ("emb_weight", "conv_weight", "conv_bias")


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def factors(shape, p, Lc):
    """fp32 [S, Lc, C] factors in {0, fp32(1 / (1 - p))} of the recipe: rand(seed 7 + sum(shape)) >= p."""
    on = torch.rand(shape[0], Lc, shape[4], generator=torch.Generator().manual_seed(7 + sum(shape))) >= p
    return on.float() * f32(1.0 / (1.0 - p))


def on_dev(pk):
    from recon_amd.char_features import PackedKeep
    return PackedKeep(pk.bits.to(dev()), pk.scale, pk.C)


def near_ties_masked(chars, E, Wc, b, span, keep, margin=1e-5):
    """bool [S, W, Fo]: in fp64 the window's maximum and a position whose masked rows differ from the winner's are closer than `margin`."""
    cfs, S = Wc.shape[2], chars.shape[0]
    W = (chars.shape[1] - cfs + 1) // span
    x = F.embedding(chars, E.double()) * keep.double()                                            # [S, Lc, C]
    pre = F.conv1d(x.permute(0, 2, 1), Wc.double(), b.double()).view(S, -1, W, span)             # [S, Fo, W, span]
    top, at = pre.max(-1)
    rows = x.unfold(1, cfs, 1).reshape(S, W, span, -1)                                            # the cfs masked rows under every position
    same = torch.stack([(rows == rows[:, :, u:u + 1]).all(-1) for u in range(span)], 2)           # [S, W, u, t]: rows of t equal those of u
    other = ~same[torch.arange(S)[:, None, None], torch.arange(W)[None, None, :], at]             # [S, Fo, W, t]
    close = other & (top.unsqueeze(-1) - pre < margin)
    return close.any(-1).permute(0, 2, 1)


def oracle(chars, E, Wc, b, span, keep, g_out, padding_idx=0):
    from recon_amd.char_features import _chain
    p = [t.double().requires_grad_(True) for t in (E, Wc, b)]
    ref = _chain(chars, *p, span, keep.double(), padding_idx)                                     # the stock sequence, fp64, CPU
    ref.backward(g_out.double())
    return [ref.detach()] + [t.grad for t in p]


_CASES = {}


def masked_case(shape, p):
    """Inputs, factors (fp32 and packed), tie-masked g_out and the fp64 oracle of a (shape, p), computed once."""
    from recon_amd.char_features import pack_keep
    if (shape, p) not in _CASES:
        chars, E, Wc, b, span, g_out = inputs(*shape)
        keep = factors(shape, p, chars.shape[1])
        ties = near_ties_masked(chars, E, Wc, b, span, keep)
        share = ties.float().mean().item()
        assert share <= 0.01, share
        g_out = g_out.masked_fill(ties, 0.0)
        _CASES[shape, p] = (chars, E, Wc, b, span, g_out, keep, pack_keep(keep, f32(1.0 / (1.0 - p))), oracle(chars, E, Wc, b, span, keep, g_out),
                            int(ties.sum()))
    return _CASES[shape, p]


def masked_ran(monkeypatch):
    from recon_amd import char_features
    return calls_of(monkeypatch, char_features._CharWordFeaturesMasked, "apply")


# ---- 1. value and three gradients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradients(shape, p, monkeypatch):
    from recon_amd import _lib, char_word_features
    from recon_amd.char_features import _chain
    chars, E, Wc, b, span, g_out, keep, pk, ref, n_ties = masked_case(shape, p)
    S, W, max_char, cfs, C, Fo, V = shape
    calls = masked_ran(monkeypatch)
    op = run(char_word_features, chars, E, Wc, b, span, g_out, keep=on_dev(pk))
    if _lib.lib().recon_char_masked_supported(S, W, span, cfs, V, C, Fo):
        assert calls, "the masked kernels take this shape: the op must not run the chain"
    else:
        assert not calls
    chain = run(_chain, chars, E, Wc, b, span, g_out, keep=keep.to(dev()))
    assert op[0].shape == (S, W, Fo) and op[1].shape == E.shape and op[2].shape == Wc.shape and op[3].shape == b.shape
    print("char_masked %s p %.1f: %d of %d cells near a tie" % (shape, p, n_ties, S * W * Fo))
    failures = band_failures(("out",) + PARAMS, op, chain, ref, "char_masked %s p %.1f" % (shape, p))
    assert not failures, failures
    assert torch.count_nonzero(op[1][0]) == 0                                       # the padding row's gradient


# ---- 2. bit-equal repeats -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [REF_WIDTHS, SLAB_SHAPE], ids=["reference_widths", "workspace_slabs"])
def test_forward_and_backward_are_bitwise_reproducible(shape):
    from recon_amd import char_word_features
    chars, E, Wc, b, span, g_out, _, pk, _, _ = masked_case(shape, 0.5)
    a = run(char_word_features, chars, E, Wc, b, span, g_out, keep=on_dev(pk))
    c = run(char_word_features, chars, E, Wc, b, span, g_out, keep=on_dev(pk))
    same(a, c)


# ---- 3. edge cases ------------------------------------------------------------------------------------------------------------------
def test_all_bits_clear_gives_tanh_of_the_bias_exactly():
    from recon_amd import char_word_features
    from recon_amd.char_features import PackedKeep
    chars, E, Wc, b, span, g_out = inputs(9, 3, 10, 3, 50, 50, 90, seed=3)
    pk = PackedKeep(torch.zeros(9, chars.shape[1], 2, dtype=torch.int32, device=dev()), 2.0, 50)
    out, g_e, g_w, g_b = run(char_word_features, chars, E, Wc, b, span, g_out, keep=pk)
    assert torch.equal(out, torch.tanh(b.to(dev())).expand(9, 3, 50))
    assert torch.count_nonzero(g_e) == 0 and torch.count_nonzero(g_w) == 0
    want = (g_out.double() * (1 - torch.tanh(b.double()) ** 2)).sum((0, 1))
    e_chain = rel_err((g_out.to(dev()) * (1 - torch.tanh(b.to(dev())) ** 2)).sum((0, 1)), want)
    assert rel_err(g_b, want) <= bound(e_chain)


def test_all_bits_set_with_scale_one_agrees_with_the_table_form():
    from recon_amd import char_word_features
    from recon_amd.char_features import _chain, pack_keep
    chars, E, Wc, b, span, g_out, ref, _ = case(REF_WIDTHS)                         # the unmasked oracle and its tie-masked g_out
    pk = pack_keep(torch.ones(7, chars.shape[1], 50), 1.0)
    masked = run(char_word_features, chars, E, Wc, b, span, g_out, keep=on_dev(pk))
    table = run(char_word_features, chars, E, Wc, b, span, g_out)
    chain = run(_chain, chars, E, Wc, b, span, g_out)
    for m, t, c, r in zip(masked, table, chain, ref):
        assert rel_err(m, r) <= bound(rel_err(c, r))
        assert rel_err(m, t.double().cpu()) <= 2 * bound(rel_err(c, r))             # each is within the bound of the oracle


@pytest.mark.parametrize("shape,garbage", [((65, 4, 6, 5, 33, 65, 40), -2), ((24, 5, 4, 2, 3, 3, 8), -8)], ids=["C33", "C3"])
def test_bits_at_and_above_C_are_ignored(shape, garbage):
    from recon_amd import char_word_features
    from recon_amd.char_features import PackedKeep
    chars, E, Wc, b, span, g_out, _, pk, _, _ = masked_case(shape, 0.5)
    dirty = pk.bits.clone()
    dirty[:, :, -1] |= garbage                                                      # every bit from C % 32 up in the last word
    assert not torch.equal(dirty, pk.bits)
    a = run(char_word_features, chars, E, Wc, b, span, g_out, keep=on_dev(pk))
    c = run(char_word_features, chars, E, Wc, b, span, g_out, keep=on_dev(PackedKeep(dirty, pk.scale, pk.C)))
    same(a, c)


def test_int32_ids():
    from recon_amd import char_word_features
    chars, E, Wc, b, span, g_out, _, pk, ref, _ = masked_case(REF_WIDTHS, 0.5)
    a = run(char_word_features, chars, E, Wc, b, span, g_out, keep=on_dev(pk))
    c = run(char_word_features, chars.to(torch.int32), E, Wc, b, span, g_out, keep=on_dev(pk))
    same(a, c)
    assert rel_err(c[0], ref[0]) <= 2e-5


def test_strided_ids_are_read_in_place():
    from recon_amd import char_word_features
    shape = (24, 5, 4, 2, 3, 3, 8)
    chars, E, Wc, b, span, g_out, _, pk, _, _ = masked_case(shape, 0.5)
    wide = torch.full((24, chars.shape[1] + 3), 5, dtype=torch.int64)
    wide[:, :chars.shape[1]] = chars
    a = run(char_word_features, chars, E, Wc, b, span, g_out, keep=on_dev(pk))
    c = run(lambda ch, *r, **kw: char_word_features(ch[:, :chars.shape[1]], *r, **kw), wide, E, Wc, b, span, g_out, keep=on_dev(pk))
    same(a, c)


def test_nonzero_padding_idx():
    from recon_amd import char_word_features
    from recon_amd.char_features import _chain, pack_keep
    shape, pad = (24, 5, 4, 2, 3, 3, 8), 3
    chars, E, Wc, b, span, g_out = inputs(*shape, seed=4)
    assert bool((chars == pad).any())
    keep = factors(shape, 0.5, chars.shape[1])
    ties = near_ties_masked(chars, E, Wc, b, span, keep)
    assert ties.float().mean().item() <= 0.01
    g_out = g_out.masked_fill(ties, 0.0)
    ref = oracle(chars, E, Wc, b, span, keep, g_out, padding_idx=pad)
    got = run(char_word_features, chars, E, Wc, b, span, g_out, keep=on_dev(pack_keep(keep, 2.0)), padding_idx=pad)
    chain = run(_chain, chars, E, Wc, b, span, g_out, keep=keep.to(dev()), padding_idx=pad)
    assert torch.count_nonzero(got[1][pad]) == 0 and torch.count_nonzero(ref[1][pad]) == 0
    assert torch.count_nonzero(got[1][:pad]) > 0
    for f, c, r in zip(got, chain, ref):
        assert rel_err(f, r) <= bound(rel_err(c, r))


def test_create_graph_stays_differentiable():
    from recon_amd import char_word_features
    chars, E, Wc, b, span, g_out, _, pk, ref, _ = masked_case((3, 3, 4, 3, 5, 6, 9), 0.5)
    p = [t.to(dev()).requires_grad_(True) for t in (E, Wc, b)]
    out = char_word_features(chars.to(dev()), *p, span, keep=on_dev(pk))
    grads = torch.autograd.grad(out, p, g_out.to(dev()), create_graph=True)
    for g, r in zip(grads, ref[1:]):
        assert g.requires_grad and rel_err(g, r) <= 2e-5
    grads[1].square().sum().backward()
    assert p[0].grad is not None and torch.isfinite(p[0].grad).all()


def test_empty_batch():
    from recon_amd import char_word_features
    from recon_amd.char_features import PackedKeep
    chars, E, Wc, b, span, _ = inputs(2, 3, 4, 3, 5, 6, 9)
    pk = PackedKeep(torch.zeros(0, chars.shape[1], 1, dtype=torch.int32, device=dev()), 2.0, 5)
    out = char_word_features(chars[:0].to(dev()), E.to(dev()), Wc.to(dev()), b.to(dev()).requires_grad_(True), span, keep=pk)
    assert out.shape == (0, 3, 6) and out.is_cuda


# ---- 4. fixtures --------------------------------------------------------------------------------------------------------------------
def test_fixture_pool_output():
    """The op with the training fixture's recorded factors, packed, against the reference module's hooked max_pool output."""
    from recon_amd import char_word_features
    from recon_amd.char_features import _chain, pack_keep
    g = load_golden("char_features2_train")
    t = lambda k: torch.from_numpy(np.asarray(g[k]))
    chars = t("chars").reshape(-1, g["chars"].shape[-1]).to(dev())
    keep = t("keep").float().to(dev())
    E, Wc, b = (t(k).float().to(dev()) for k in ("sd.char_embeddings.embeddings.weight", "sd.conv1d.weight", "sd.conv1d.bias"))
    ref = torch.tanh(t("pool")).permute(0, 2, 1)
    e_f = rel_err(char_word_features(chars, E, Wc, b, int(g["word_span"]), keep=pack_keep(keep)), ref)
    e_c = rel_err(_chain(chars, E, Wc, b, int(g["word_span"]), keep), ref)
    print("char_masked fixture: op %.3e chain %.3e" % (e_f, e_c))
    assert e_f <= bound(e_c)


def test_fixture_entity_embedding_with_packed_dropout(monkeypatch):
    """EntityEmbedding with packed_char_dropout and the fixture's recorded factors replayed through draw_packed_keep: the output and the
    three gradients within test_fixture_entity_embedding's tolerances, through the masked function."""
    from recon_amd.char_features import pack_keep
    name = "char_features2_train"
    g = load_golden(name)
    m = fixture_model(g)
    keep = torch.from_numpy(g["keep"])
    m.packed_char_dropout = True
    m.char_embeddings.draw_packed_keep = lambda S, Lc, C_, device: pack_keep(keep.to(device=device, dtype=torch.float32))
    calls = masked_ran(monkeypatch)
    m.train().to(dev())
    t = lambda k: torch.from_numpy(g[k]).to(dev())
    out = m(t("words"), t("chars"), t("mask"))
    assert calls
    close(out, g["out"], atol=1e-4, what=name + " out")
    (out * t("G").float()).sum().backward()
    for k in ("char_embeddings.embeddings.weight", "conv1d.weight", "conv1d.bias"):
        close(dict(m.named_parameters())[k].grad, g["g." + k], atol=1e-4, rel_to_max=1e-4, what=name + " grad " + k)


# ---- 5. the draw --------------------------------------------------------------------------------------------------------------------
def philox_np(ctr, k0, k1):
    """Philox4x32-10 of 64-bit counters (words 2 and 3 zero) under the key (k0, k1): uint32 [n, 4]."""
    u = np.uint64
    c = [ctr & u(0xFFFFFFFF), ctr >> u(32), np.zeros_like(ctr), np.zeros_like(ctr)]
    k0, k1 = u(k0), u(k1)
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c[0], u(0xCD9E8D57) * c[2]
        c = [(p1 >> u(32)) ^ c[1] ^ k0, p1 & u(0xFFFFFFFF), (p0 >> u(32)) ^ c[3] ^ k1, p0 & u(0xFFFFFFFF)]
        k0, k1 = (k0 + u(0x9E3779B9)) & u(0xFFFFFFFF), (k1 + u(0xBB67AE85)) & u(0xFFFFFFFF)
    return np.stack(c, -1)


def draw_np(S, Lc, C, p, seed, offset):
    """The draw definition, element by element: bool [S, Lc, C]."""
    Gp, thr = (C + 3) // 4, min(2 ** 32 - 1, int(p * 2.0 ** 32))
    q, c = np.meshgrid(np.arange(S * Lc, dtype=np.uint64), np.arange(C, dtype=np.uint64), indexing="ij")
    words = philox_np((np.uint64(offset) + q * np.uint64(Gp) + c // np.uint64(4)).ravel(), seed & 0xFFFFFFFF, seed >> 32)
    return (words[np.arange(words.shape[0]), (c % np.uint64(4)).ravel().astype(np.int64)] >= thr).reshape(S, Lc, C)


def unpack(bits, C):
    b = bits.cpu().numpy().view(np.uint32)
    return ((b[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(b.shape[0], b.shape[1], -1)


@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("S,Lc,C", [(1, 1, 1), (2, 5, 33), (3, 14, 50)])
def test_draw_equals_its_definition(S, Lc, C, p):
    from recon_amd.char_features import draw_keep_bits, keep_threshold
    for seed, offset in ((12345, 0), ((1 << 40) + 977, 4 * 123457), ((1 << 63) + 5, (1 << 32) - 8)):
        want = draw_np(S, Lc, C, p, seed, offset)
        got = draw_keep_bits(S, Lc, C, keep_threshold(p), seed, offset, dev())
        assert got.dtype == torch.int32 and got.shape == (S, Lc, (C + 31) // 32)
        on = unpack(got, C)
        assert np.array_equal(on[:, :, :C].astype(bool), want), (seed, offset)
        assert not on[:, :, C:].any()                                                # bits at and above C are zero
        assert torch.equal(draw_keep_bits(S, Lc, C, keep_threshold(p), seed, offset, "cpu"), got.cpu())
        assert torch.equal(draw_keep_bits(S, Lc, C, keep_threshold(p), seed, offset, dev()), got)


def test_draw_packed_keep_follows_the_generator():
    from recon_amd.char_features import draw_packed_keep
    S, Lc, C, p = 3, 14, 50, 0.5
    gen = torch.Generator(device=dev())
    seed, offset = (1 << 40) + 31, 64
    gen.manual_seed(seed)
    gen.set_offset(offset)
    a = draw_packed_keep(S, Lc, C, p, dev(), generator=gen)
    assert a.scale == 2.0 and a.C == C and a.bits.is_cuda
    assert gen.get_offset() == offset + (S * Lc * 13 + 3) // 4 * 4                   # the counters consumed, rounded up to a multiple of 4
    b = draw_packed_keep(S, Lc, C, p, dev(), generator=gen)
    assert not torch.equal(a.bits, b.bits)                                           # consecutive draws differ
    gen.manual_seed(seed)
    gen.set_offset(offset)
    c = draw_packed_keep(S, Lc, C, p, "cpu", generator=gen)                          # the same (seed, offset) on the CPU path
    assert not c.bits.is_cuda and torch.equal(c.bits, a.bits.cpu())
    assert np.array_equal(unpack(a.bits, C)[:, :, :C].astype(bool), draw_np(S, Lc, C, p, seed, offset))
    torch.manual_seed(5)                                                             # the device's default generator
    d = draw_packed_keep(S, Lc, C, p, dev())
    e = draw_packed_keep(S, Lc, C, p, dev())
    torch.manual_seed(5)
    f = draw_packed_keep(S, Lc, C, p, dev())
    assert torch.equal(d.bits, f.bits) and not torch.equal(d.bits, e.bits)
    assert torch.equal(a.factors().cpu(), torch.from_numpy(draw_np(S, Lc, C, p, seed, offset)).float() * 2.0)


@pytest.mark.parametrize("p", [0.5, 0.1])
def test_draw_keeps_the_expected_share(p):
    from recon_amd.char_features import draw_packed_keep
    S, Lc, C = 64, 386, 50
    gen = torch.Generator(device=dev())
    gen.manual_seed(2024)
    pk = draw_packed_keep(S, Lc, C, p, dev(), generator=gen)
    n = S * Lc * C
    kept = int(unpack(pk.bits, C)[:, :, :C].sum())
    print("char_masked draw p %.1f: kept share %.6f" % (p, kept / n))
    assert abs(kept / n - (1 - p)) <= 6 * (p * (1 - p) / n) ** 0.5
    assert not unpack(pk.bits, C)[:, :, C:].any()


# ---- 6. memory ----------------------------------------------------------------------------------------------------------------------
def test_forward_materialises_nothing_of_size_S_Lc_C():
    """A forward at the reference's word and width geometry with a gradient wanted raises the allocated bytes by the output, the position
    bytes and the queried workspace, each a block of the allocator (the accounting of test_char_features_gpu.py: ten times the output and
    the workspace is below the S Lc C 4 bytes of the gathered embedding alone).  The bits are an input, 8 bytes per position."""
    from recon_amd import _lib, char_word_features
    S, W, max_char, cfs, C, Fo, V = REF_GEOMETRY
    chars, E, Wc, b, span, _, _, pk, _, _ = masked_case(REF_GEOMETRY, 0.5)
    chars, E, Wc, b = (x.to(dev()) for x in (chars, E, Wc, b))
    pk = on_dev(pk)
    assert pk.bits.numel() * 4 == S * chars.shape[1] * 8
    ws = _lib.lib().recon_char_masked_workspace_bytes(S, W, span, cfs, V, C, Fo, 0)
    allowed = rounded(S * W * Fo * 4) + rounded(ws)
    assert 10 * allowed < S * chars.shape[1] * C * 4
    allowed += rounded(S * W * Fo)
    E.requires_grad_(True)
    peak, out = peak_bytes(lambda: char_word_features(chars, E, Wc, b, span, keep=pk))
    print("char_masked memory: peak %d bytes, allowed %d, gathered embedding %d" % (peak, allowed, S * chars.shape[1] * C * 4))
    assert peak <= allowed, (peak, allowed)
    assert out.shape == (S, W, Fo) and out.grad_fn is not None
