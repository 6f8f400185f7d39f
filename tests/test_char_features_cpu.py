"""CPU-side checks of the char-CNN op (recon_amd/char_features.py, csrc/char_cnn.hip): the four entry points are declared, exported and
bound; the size queries answer without a GPU; on CPU tensors the op IS the stock sequence; and both fixtures written from the reference's
EntityEmbedding reproduce under the stock sequence in fp64, which pins fixture and chain to the reference."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, load_golden
from op_checks import state_dict_of

NAMES = ("recon_char_features_supported", "recon_char_features_workspace_bytes", "recon_char_features_fwd", "recon_char_features_bwd")
#        S    W  max_char cfs C   Fo  V
CASES = [(1, 1, 1, 1, 1, 1, 2), (3, 3, 4, 3, 5, 6, 9), (24, 5, 4, 2, 3, 3, 8), (7, 2, 10, 3, 50, 50, 90), (65, 4, 6, 5, 33, 65, 40),
         (19, 3, 10, 3, 50, 50, 300), (130, 32, 10, 3, 50, 50, 90)]


def test_entry_points_declared_exported_bound():
    from recon_amd import _lib
    header = open(os.path.join(ROOT, "include", "recon_hip.h")).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(h, name), name
        assert name in bound, name
    assert header.count("models/models.py:57-61") >= len(NAMES)
    assert _lib.lib().recon_version() == 2


@pytest.mark.parametrize("S,W,max_char,cfs,C,Fo,V", CASES)
def test_size_queries_answer_without_a_gpu(S, W, max_char, cfs, C, Fo, V):
    from recon_amd import _lib
    L = _lib.lib()
    geo = (S, W, max_char + cfs - 1, cfs, V, C, Fo)
    assert L.recon_char_features_supported(*geo) == 1
    table = cfs * V * Fo * 4
    fwd, bwd = L.recon_char_features_workspace_bytes(*geo, 0), L.recon_char_features_workspace_bytes(*geo, 1)
    assert table <= fwd < table + 512
    assert bwd >= 2 * table + Fo * 4 and bwd <= 513 * (table + Fo * 4) + 512
    assert fwd % 16 == 0 and bwd % 16 == 0


def test_shapes_outside_the_kernels_are_refused():
    from recon_amd import _lib
    L = _lib.lib()
    assert L.recon_char_features_supported(4, 2, 12, 3, 90, 50, 257) == 0          # Fo past four passes of 64
    assert L.recon_char_features_supported(4, 2, 63, 3, 90, 50, 50) == 0           # a word's ids past one wave's lanes
    assert L.recon_char_features_supported(0, 2, 12, 3, 90, 50, 50) == 0
    assert L.recon_char_features_workspace_bytes(4, 2, 63, 3, 90, 50, 50, 0) == 0
    fake = 16                                                                       # never dereferenced: both calls return before a launch
    fwd = lambda S, keep, ib=8: L.recon_char_features_fwd(fake, ib, 26, fake, fake, fake, keep, S, 2, 12, 3, 90, 50, 50, fake, None, fake, 1 << 20, None)
    assert fwd(0, None) == 0
    assert fwd(4, None, ib=2) == -1
    assert L.recon_char_features_fwd(fake, 8, 26, fake, fake, fake, None, 4, 2, 63, 3, 90, 50, 50, fake, None, fake, 1 << 20, None) == -2
    assert L.recon_char_features_fwd(fake, 8, 26, fake, fake, fake, None, 4, 2, 12, 3, 90, 50, 50, fake, None, fake, 16, None) == -4


def inputs(S, W, max_char, cfs, C, Fo, V, seed=0):
    """Per sequence a random number of words (0..W), each 1..max_char random ids in [1, V), the rest padding; E ~ N(0, 1) with row 0 zero,
    W xavier-scaled, bias ~ 0.1 N(0, 1).  CPU tensors.  The GPU files' cases: the seed is mixed with the shape, g_out is drawn too."""
    g = torch.Generator().manual_seed(1000 * seed + S + W + max_char + cfs + C + Fo + V)
    span = max_char + cfs - 1
    chars = torch.zeros(S, cfs - 1 + W * span, dtype=torch.int64)
    n_words = torch.randint(0, W + 1, (S,), generator=g)
    lens = torch.randint(1, max_char + 1, (S, W), generator=g)
    ids = torch.randint(1, V, (S, W, span), generator=g)
    live = (torch.arange(span)[None, None, :] < lens[:, :, None]) & (torch.arange(W)[None, :, None] < n_words[:, None, None])
    chars[:, :W * span] = (ids * live).view(S, W * span)
    E = torch.randn(V, C, generator=g)
    E[0] = 0
    Wc = torch.randn(Fo, C, cfs, generator=g) * (2.0 / (C * cfs + Fo * cfs)) ** 0.5
    b = 0.1 * torch.randn(Fo, generator=g)
    g_out = torch.randn(S, W, Fo, generator=g)
    return chars, E, Wc, b, span, g_out


def inputs_word_by_word(S, W, max_char, cfs, C, Fo, V, seed, dtype=torch.float32):
    """The CPU tests' inputs: the seed as it is, the ids drawn word by word in a Python loop (another stream than `inputs`), a dtype,
    no g_out."""
    g = torch.Generator().manual_seed(seed)
    span = max_char + cfs - 1
    chars = torch.zeros(S, cfs - 1 + W * span, dtype=torch.int64)
    for s in range(S):
        for w in range(int(torch.randint(0, W + 1, (1,), generator=g))):
            n = int(torch.randint(1, max_char + 1, (1,), generator=g))
            chars[s, w * span:w * span + n] = torch.randint(1, V, (n,), generator=g)
    E = torch.randn(V, C, generator=g, dtype=dtype)
    E[0] = 0
    Wc = torch.randn(Fo, C, cfs, generator=g, dtype=dtype) * (2.0 / (C * cfs + Fo * cfs)) ** 0.5
    b = 0.1 * torch.randn(Fo, generator=g, dtype=dtype)
    return chars, E, Wc, b, span


def stock(chars, E, Wc, b, span, keep=None):
    """models/models.py:57-61 written out: embedding (* dropout factors), conv1d, max_pool1d, tanh."""
    x = F.embedding(chars, E, padding_idx=0)
    if keep is not None:
        x = x * keep
    return torch.tanh(F.max_pool1d(F.conv1d(x.permute(0, 2, 1), Wc, b), span, span)).permute(0, 2, 1)


@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("ids", [torch.int64, torch.int32])
def test_cpu_tensors_run_the_stock_sequence_bit_for_bit(with_keep, ids):
    from recon_amd import char_word_features
    chars, E, Wc, b, span = inputs_word_by_word(7, 3, 4, 3, 5, 6, 9, seed=1)
    keep = F.dropout(torch.ones(chars.shape[0], chars.shape[1], 5), 0.5, True) if with_keep else None
    G = torch.randn(7, 3, 6)
    grads = []
    for fn in (lambda *a: char_word_features(a[0].to(ids), *a[1:], keep=keep), lambda *a: stock(*a, keep=keep)):
        p = [t.clone().requires_grad_(True) for t in (E, Wc, b)]
        y = fn(chars, *p, span)
        (y * G).sum().backward()
        grads.append([y.detach()] + [t.grad for t in p])
    for a, c in zip(*grads):
        assert torch.equal(a, c)
    assert grads[0][0].shape == (7, 3, 6)
    assert torch.count_nonzero(grads[0][1][0]) == 0                                 # the padding row


def test_shape_and_dtype_checks_raise():
    from recon_amd import char_word_features
    chars, E, Wc, b, span = inputs_word_by_word(4, 3, 4, 3, 5, 6, 9, seed=2)
    with pytest.raises(ValueError):
        char_word_features(chars[:, :-1], E, Wc, b, span)                           # Lc != cfs - 1 + W span
    with pytest.raises(ValueError):
        char_word_features(chars, E, Wc, b, 0)
    with pytest.raises(ValueError):
        char_word_features(chars.float(), E, Wc, b, span)
    with pytest.raises(ValueError):
        char_word_features(chars[0], E, Wc, b, span)
    with pytest.raises(ValueError):
        char_word_features(chars, E[:, :4], Wc, b, span)                            # C of the table and of the filters differ
    with pytest.raises(ValueError):
        char_word_features(chars, E, Wc, b[:-1], span)
    with pytest.raises(ValueError):
        char_word_features(chars, E.double(), Wc, b, span)
    with pytest.raises(ValueError):
        char_word_features(chars, E, Wc, b, span, keep=torch.ones(4, chars.shape[1], 4))
    out = char_word_features(chars[:0], E, Wc, b, span)
    assert out.shape == (0, 3, 6)


@pytest.mark.parametrize("name", ["char_features1_eval", "char_features2_train"])
def test_fixture_reproduces_under_the_chain_in_fp64(name):
    from recon_amd.char_features import _chain
    g = load_golden(name)
    t = lambda k: torch.from_numpy(np.asarray(g[k]))
    assert all(g[k].dtype == np.float64 for k in ("pool", "out", "sd.conv1d.weight", "g.conv1d.weight"))
    chars = t("chars").reshape(-1, g["chars"].shape[-1])
    keep = t("keep") if "keep" in g else None
    assert (keep is None) == (float(g["p"]) == 0.0)
    E, Wc, b = t("sd.char_embeddings.embeddings.weight"), t("sd.conv1d.weight"), t("sd.conv1d.bias")
    y = _chain(chars, E, Wc, b, int(g["word_span"]), keep, 0)
    pool = t("pool")                                                                # [S, Fo, W], before the tanh
    assert float((y - torch.tanh(pool).permute(0, 2, 1)).abs().max()) <= 1e-12
    assert (chars[0, 2:5] > 0).tolist() == [True, False, True]                      # padding inside a word
    assert bool((chars == 0).all(1).any()) or bool((chars[:, -1] == 0).all())       # and at the end of sequences


@pytest.mark.parametrize("name", ["char_features1_eval", "char_features2_train"])
def test_fixture_model_reproduces_on_cpu_in_fp64(name):
    """The whole EntityEmbedding with the fixture's parameters (strict load) through `_chain` (CPU tensors): output and the three gradients."""
    from recon_amd.gpgnn import EntityEmbedding
    g = load_golden(name)
    m = fixture_model(g).double()
    out = m(torch.from_numpy(g["words"]), torch.from_numpy(g["chars"]), torch.from_numpy(g["mask"]))
    assert float((out.detach() - torch.from_numpy(g["out"])).abs().max()) <= 1e-12
    (out * torch.from_numpy(g["G"])).sum().backward()
    for k in ("char_embeddings.embeddings.weight", "conv1d.weight", "conv1d.bias"):
        got = dict(m.named_parameters())[k].grad
        assert float((got - torch.from_numpy(g["g." + k])).abs().max()) <= 1e-12, k
    assert isinstance(m, EntityEmbedding)


def fixture_model(g):
    """recon_amd's EntityEmbedding at the fixture's sizes with its parameters loaded (strict) and, for the training fixture, the recorded
    dropout factors replayed through draw_keep."""
    import torch.nn as nn
    from recon_amd.gpgnn import EntityEmbedding
    sd = state_dict_of(g)
    (V, C), (Fo, _, cfs) = sd["char_embeddings.embeddings.weight"].shape, sd["conv1d.weight"].shape
    n_words, word_dim = sd["word_embeddings.weight"].shape
    hidden = sd["lstm.weight_hh_l0"].shape[1]
    ent_dim, _, ecfs = sd["conv1d_entity.weight"].shape
    p = float(g["p"])
    m = EntityEmbedding(word_dim + Fo, hidden, 1, 1, p, ent_dim, cfs, ecfs, nn.Embedding(n_words, word_dim, padding_idx=0), C,
                        int(g["word_span"]) - cfs + 1, list(range(V)), Fo)
    m.load_state_dict(sd, strict=True)
    if p > 0:
        keep = torch.from_numpy(g["keep"])
        m.train()
        m.char_embeddings.draw_keep = lambda S, Lc, C_, device: keep.to(device=device, dtype=m.conv1d.weight.dtype)
    else:
        m.eval()
    return m
