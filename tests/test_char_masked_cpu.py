"""CPU-side checks of the masked char-CNN (recon_amd/char_features.py, csrc/char_mask.hip): the five entry points are declared, exported
and bound; the size queries and refusals answer without a GPU; the Philox restatement meets its known answers; the packed mask round-trips;
and on CPU tensors the op with a PackedKeep IS the stock sequence with the unpacked factors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_char_features_cpu import inputs_word_by_word, stock

NAMES = ("recon_char_masked_supported", "recon_char_masked_workspace_bytes", "recon_char_keep_bits_draw", "recon_char_masked_fwd",
         "recon_char_masked_bwd")
#        S    W  max_char cfs C   Fo  V
CASES = [(1, 1, 1, 1, 1, 1, 2), (3, 3, 4, 3, 5, 6, 9), (24, 5, 4, 2, 3, 3, 8), (7, 2, 10, 3, 50, 50, 90), (65, 4, 6, 5, 33, 65, 40),
         (9, 3, 4, 3, 64, 8, 700), (130, 32, 10, 3, 50, 50, 90)]


def test_entry_points_declared_exported_bound():
    from recon_amd import _lib
    header = open(os.path.join(ROOT, "include", "recon_hip.h")).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(h, name), name
        assert name in bound, name
    assert header.count("models/models.py:57-61") >= 4 + len(NAMES)                # the table form's four entries and these


@pytest.mark.parametrize("S,W,max_char,cfs,C,Fo,V", CASES)
def test_size_queries_answer_without_a_gpu(S, W, max_char, cfs, C, Fo, V):
    from recon_amd import _lib
    L = _lib.lib()
    geo = (S, W, max_char + cfs - 1, cfs, V, C, Fo)
    assert L.recon_char_masked_supported(*geo) == 1
    fwd, bwd = L.recon_char_masked_workspace_bytes(*geo, 0), L.recon_char_masked_workspace_bytes(*geo, 1)
    slab = (V * C + Fo * C * cfs + Fo) * 4
    assert fwd >= cfs * C * Fo * 4 and fwd % 16 == 0                                # the filter bank, padded
    assert slab <= bwd <= 256 * slab + 512 and bwd % 16 == 0                        # one private accumulator set per workgroup
    assert fwd < S * (cfs - 1 + W * (max_char + cfs - 1)) * C * 4 or S < 8          # nothing of size S Lc C


def test_shapes_outside_the_kernels_are_refused():
    from recon_amd import _lib
    L = _lib.lib()
    assert L.recon_char_masked_supported(4, 2, 12, 3, 90, 64, 50) == 1
    assert L.recon_char_masked_supported(4, 2, 12, 3, 90, 65, 50) == 0             # C past one lane per channel
    assert L.recon_char_masked_supported(4, 2, 12, 3, 90, 50, 257) == 0            # Fo past 256
    assert L.recon_char_masked_supported(4, 2, 63, 3, 90, 50, 50) == 0             # span + cfs - 1 > 64
    assert L.recon_char_masked_supported(0, 2, 12, 3, 90, 50, 50) == 0
    for geo in ((4, 2, 12, 3, 90, 65, 50), (4, 2, 12, 3, 90, 50, 257), (4, 2, 63, 3, 90, 50, 50), (0, 2, 12, 3, 90, 50, 50)):
        assert L.recon_char_masked_workspace_bytes(*geo, 0) == 0 and L.recon_char_masked_workspace_bytes(*geo, 1) == 0


def test_bad_arguments_are_reported_before_any_launch():
    from recon_amd import _lib
    L = _lib.lib()
    fake = 16                                                                       # never dereferenced: every call returns before a launch
    fwd = lambda S, ib=8, C=50, ws=1 << 20: L.recon_char_masked_fwd(fake, ib, 26, fake, fake, fake, fake, 2.0, S, 2, 12, 3, 90, C, 50, fake, None,
                                                                    fake, ws, None)
    bwd = lambda S, ib=8, C=50, ws=1 << 30: L.recon_char_masked_bwd(fake, ib, 26, fake, fake, fake, 2.0, fake, fake, fake, S, 2, 12, 3, 90, C, 50, 0,
                                                                    fake, fake, fake, fake, ws, None)
    assert fwd(0) == 0                                                              # an empty batch launches nothing
    assert fwd(4, ib=2) == -1 and bwd(4, ib=2) == -1                                # a bad index_bytes
    assert fwd(4, C=65) == -2 and bwd(4, C=65) == -2                                # unsupported
    assert fwd(4, ws=16) == -4 and bwd(4, ws=16) == -4                              # a short workspace
    assert L.recon_char_keep_bits_draw(fake, -1, 50, 1 << 31, 1, 0, None) == -1
    assert L.recon_char_keep_bits_draw(fake, 4, 0, 1 << 31, 1, 0, None) == -1
    assert L.recon_char_keep_bits_draw(fake, 0, 50, 1 << 31, 1, 0, None) == 0


def test_philox_known_answers():
    from recon_amd.char_features import philox4x32_10
    hexes = lambda a: " ".join("%08x" % int(x) for x in a)
    assert hexes(philox4x32_10(np.zeros(4, np.uint32), np.zeros(2, np.uint32))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexes(philox4x32_10(np.full(4, 0xFFFFFFFF, np.uint32), np.full(2, 0xFFFFFFFF, np.uint32))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexes(philox4x32_10(np.array([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], np.uint32),
                               np.array([0xA4093822, 0x299F31D0], np.uint32))) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_cpu_draw_follows_its_definition_and_the_generator():
    from recon_amd.char_features import draw_keep_bits, draw_packed_keep, keep_threshold, philox4x32_10
    assert keep_threshold(0.5) == 1 << 31 and keep_threshold(0.0) == 0 and keep_threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1
    S, Lc, C, seed, offset = 2, 5, 33, (1 << 40) + 977, (1 << 32) - 8
    bits = draw_keep_bits(S, Lc, C, keep_threshold(0.1), seed, offset, "cpu")
    assert bits.dtype == torch.int32 and bits.shape == (S, Lc, 2)
    for q in (0, 7, 9):                                                             # element by element, across the carry into counter word 1
        for c in (0, 3, 4, 31, 32):
            ctr = offset + q * 9 + c // 4
            word = philox4x32_10(np.array([ctr & 0xFFFFFFFF, ctr >> 32, 0, 0], np.uint64), np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))[c % 4]
            assert bool((int(bits.view(-1, 2)[q, c // 32]) >> (c % 32)) & 1) == bool(int(word) >= keep_threshold(0.1)), (q, c)
    assert not bool(((bits[:, :, 1].to(torch.int64) & 0xFFFFFFFF) >> 1).any())     # bits at and above C are zero
    g = torch.Generator().manual_seed(11)
    a, b = draw_packed_keep(3, 14, 50, 0.5, "cpu", generator=g), draw_packed_keep(3, 14, 50, 0.5, "cpu", generator=g)
    c = draw_packed_keep(3, 14, 50, 0.5, "cpu", generator=torch.Generator().manual_seed(11))
    assert a.scale == 2.0 and torch.equal(a.bits, c.bits) and not torch.equal(a.bits, b.bits)
    f = a.factors()
    assert f.shape == (3, 14, 50) and set(f.unique().tolist()) == {0.0, 2.0}


def test_pack_keep_round_trips_exactly():
    from recon_amd.char_features import pack_keep
    for C, scale in ((1, 2.0), (3, 1.25), (32, 2.0), (33, 10.0 / 9.0), (50, 2.0), (64, 1.0)):
        scale = float(torch.tensor(scale, dtype=torch.float32))
        keep = (torch.rand(4, 7, C, generator=torch.Generator().manual_seed(C)) >= 0.5).float() * scale
        keep[0, 0, C - 1] = scale                                                   # the top bit of the last word in use
        pk = pack_keep(keep)
        assert pk.bits.dtype == torch.int32 and pk.bits.shape == (4, 7, (C + 31) // 32) and pk.bits.is_contiguous()
        assert pk.scale == scale and pk.C == C
        assert torch.equal(pk.factors(), keep)
        assert torch.equal(pack_keep(keep, scale).bits, pk.bits)
        assert pk.factors(torch.float64).dtype == torch.float64


def test_pack_keep_refuses_two_different_nonzero_values():
    from recon_amd.char_features import pack_keep
    keep = torch.zeros(2, 3, 5)
    keep[0, 0, 0], keep[1, 2, 4] = 2.0, 1.5
    with pytest.raises(ValueError):
        pack_keep(keep)
    with pytest.raises(ValueError):
        pack_keep(keep.clamp_max(1.5), scale=2.0)


@pytest.mark.parametrize("ids", [torch.int64, torch.int32])
def test_cpu_tensors_run_the_stock_sequence_bit_for_bit(ids):
    from recon_amd import char_word_features
    from recon_amd.char_features import pack_keep
    chars, E, Wc, b, span = inputs_word_by_word(7, 3, 4, 3, 5, 6, 9, seed=1)
    keep = (torch.rand(7, chars.shape[1], 5, generator=torch.Generator().manual_seed(3)) >= 0.5).float() * 2.0
    pk = pack_keep(keep)
    G = torch.randn(7, 3, 6)
    grads = []
    for fn in (lambda *a: char_word_features(a[0].to(ids), *a[1:], keep=pk), lambda *a: stock(*a, keep=keep)):
        p = [t.clone().requires_grad_(True) for t in (E, Wc, b)]
        y = fn(chars, *p, span)
        (y * G).sum().backward()
        grads.append([y.detach()] + [t.grad for t in p])
    for a, c in zip(*grads):
        assert torch.equal(a, c)
    assert torch.count_nonzero(grads[0][1][0]) == 0                                 # the padding row


def test_packed_keep_checks_raise():
    from recon_amd import char_word_features
    from recon_amd.char_features import PackedKeep
    chars, E, Wc, b, span = inputs_word_by_word(4, 3, 4, 3, 5, 6, 9, seed=2)
    Lc = chars.shape[1]
    good = torch.zeros(4, Lc, 1, dtype=torch.int32)
    assert char_word_features(chars, E, Wc, b, span, keep=PackedKeep(good, 2.0, 5)).shape == (4, 3, 6)
    for bad in (PackedKeep(torch.zeros(4, Lc, 2, dtype=torch.int32), 2.0, 5),       # KW
                PackedKeep(torch.zeros(4, Lc - 1, 1, dtype=torch.int32), 2.0, 5),   # Lc
                PackedKeep(torch.zeros(4, Lc, 1, dtype=torch.int64), 2.0, 5),       # dtype
                PackedKeep(good, 2.0, 4),                                           # C
                PackedKeep(torch.zeros(4, Lc, 2, dtype=torch.int32)[:, :, :1], 2.0, 5)):   # not contiguous
        with pytest.raises(ValueError):
            char_word_features(chars, E, Wc, b, span, keep=bad)
    out = char_word_features(chars[:0], E, Wc, b, span, keep=PackedKeep(good[:0], 2.0, 5))
    assert out.shape == (0, 3, 6)


def test_module_switch_draws_packed_factors():
    from recon_amd.char_features import PackedKeep
    from recon_amd.gpgnn import CharEmbeddings, EntityEmbedding
    assert EntityEmbedding.packed_char_dropout is False
    m = CharEmbeddings(9, 5, 0.5)
    pk = m.train().draw_packed_keep(3, 7, 5, torch.device("cpu"))
    assert isinstance(pk, PackedKeep) and pk.scale == 2.0 and pk.bits.shape == (3, 7, 1)
    assert m.eval().draw_packed_keep(3, 7, 5, torch.device("cpu")) is None
    assert CharEmbeddings(9, 5, 0.0).train().draw_packed_keep(3, 7, 5, torch.device("cpu")) is None
