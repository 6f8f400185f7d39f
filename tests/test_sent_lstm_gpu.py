"""recon_amd.pair_sentence_states (csrc/sent_lstm.hip) against the stock lines of models/models.py:160-184 in fp64 on the CPU, and against
the fixtures written from the reference's GPGNN and RECON_EAC.

Tolerance of value and gradients: `op_checks.bound` of the stock fp32 chain's own error on the GPU against fp64 on the same inputs, measured
in the test, for out, pos_table's gradient and the eight parameter gradients.  Weights uniform in +-1 / sqrt(H) (nn.LSTM's own init), tables N(0, 1)
with a non-zero padding row, markers over all Vp = 4 values.  No cell is excluded.  The figures measured on an MI355X are in DESIGN.md
section 21."""
import copy

import numpy as np
import pytest
import torch

from op_checks import band_failures, calls_of, dev, eac_fixture, gpgnn_fixture, peak_bytes, pinned, rel_err, rounded, same
from test_sent_lstm_cpu import VP, VW, inputs, stock

pytestmark = pytest.mark.gpu

G_BWD = 32                                      # the weight-gradient pass's row groups (sentence_lstm.BWD_MAX_ROW_GROUPS, asserted below)
WIDE_FROM = 2048                                # above this many sequences a tile is 32 rows (sentence_lstm.WIDE_TILE_FROM, asserted below)
LONG_THIN = (3, (2 * 16 * G_BWD + 5) // 3, 3, 3, 4, 5)         # 1029 sequences: every row group holds 33 x 3 rows, more than two tiles of 16
WIDE_FULL = (1, WIDE_FROM + 37, 2, 3, 3, 130)                  # 32-row tiles with a tail, two unit blocks per wave
WIDE_SMALL = (5, (WIDE_FROM + 37) // 5, 2, 4, 3, 20)           # 32-row tiles with a tail, one unit block per wave
REF_ONE = (1, 72, 36, 50, 3, 256)
#        B   C  T  Dw  P  H
CASES = [(1, 1, 1, 1, 1, 1), (2, 3, 3, 4, 3, 3), (3, 2, 5, 5, 3, 17), (2, 6, 4, 50, 3, 64), (1, 20, 3, 7, 3, 256), (3, 72, 2, 50, 3, 100),
         REF_ONE, LONG_THIN, WIDE_FULL, WIDE_SMALL]
NAMES = ("out", "pos_table", "weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
         "bias_ih_l0_reverse", "bias_hh_l0_reverse")

_CASES = {}


def case(shape, packed):
    """Inputs and the fp64 oracle (value, d_pos_table, the eight parameter gradients) of a shape, computed once and left unchanged."""
    if (shape, packed) not in _CASES:
        rnn, sentence, markers, word_table, pos_table, g_out, keep = inputs(*shape)
        B, C, T, Dw = shape[:4]
        r64 = copy.deepcopy(rnn).double()
        pt = pos_table.double().requires_grad_(True)
        ref = stock(r64, sentence, markers, word_table.double(), pt, keep.factors(torch.float64).view(B, C, T, Dw) if packed else None)
        ref.backward(g_out.double())
        _CASES[(shape, packed)] = (rnn, sentence, markers, word_table, pos_table, g_out, keep if packed else None,
                                   [ref.detach(), pt.grad] + [p.grad for p in r64.parameters()])
    return _CASES[(shape, packed)]


def run(fn, rnn, sentence, markers, word_table, pos_table, g_out, keep, ids=None):
    """[out, d_pos_table, eight parameter gradients] of fn on the GPU; the module in training mode, as MIOpen's backward needs."""
    m = copy.deepcopy(rnn).to(dev()).train()
    pt = pos_table.to(dev()).requires_grad_(True)
    s, k = (sentence.to(dev()), markers.to(dev())) if ids is None else ids(sentence.to(dev()), markers.to(dev()))
    out = fn(m, s, k, word_table.to(dev()), pt, keep)
    out.backward(g_out.to(dev()))
    return [out.detach(), pt.grad] + [p.grad for p in m.parameters()]


def on_gpu(keep):
    from recon_amd.char_features import PackedKeep
    return None if keep is None else PackedKeep(keep.bits.to(dev()), keep.scale, keep.C)


def chain_fn(m, s, k, wt, pt, keep):
    from recon_amd.sentence_lstm import _chain
    B, T = s.shape
    f = None if keep is None else keep.factors().view(B, k.shape[1], T, -1)
    return _chain(m, s, k, wt, pt, f)


def kernels_ran(monkeypatch):
    from recon_amd import sentence_lstm
    return calls_of(monkeypatch, sentence_lstm._PairSentenceStates, "apply")


def chain_ran(monkeypatch):
    from recon_amd import sentence_lstm
    return calls_of(monkeypatch, sentence_lstm, "_chain")


def test_row_split_and_tile_rule_are_the_librarys():
    from recon_amd import _lib, sentence_lstm
    L = _lib.lib()
    assert sentence_lstm.BWD_MAX_ROW_GROUPS == G_BWD and sentence_lstm.WIDE_TILE_FROM == WIDE_FROM
    B, C, T, Dw, P, H = LONG_THIN
    S = B * C
    slab = 2 * 4 * H * (Dw + P + H + 1 + VP) * 4
    groups = lambda b, c: round((L.recon_sent_lstm_workspace_bytes(b, c, T, Dw, P, H, VP, 1) - L.recon_sent_lstm_workspace_bytes(1, 1, T, Dw, P, H, VP, 1))
                                / slab) + 1
    per = -(-S // G_BWD)
    assert per * T > 32 and groups(B, C) == -(-S // per) and groups(B, C) > G_BWD - 2          # every group: more than two tiles of 16 rows
    assert groups(1, 1) == 1 and groups(1, 5) == 5 and groups(10 ** 4, 100) == G_BWD
    assert L.recon_sent_lstm_saved_bytes(B, C, T, Dw, P, H) == 2 * S * T * 5 * H * 4
    assert L.recon_sent_lstm_supported(50, 72, 36, 50, 3, 256) and L.recon_sent_lstm_supported(2, 2, 2, 61, 3, 256)
    assert not L.recon_sent_lstm_supported(2, 2, 2, 50, 3, 257) and not L.recon_sent_lstm_supported(2, 2, 2, 127, 2, 8)
    assert L.recon_sent_lstm_workspace_bytes(2, 2, 2, 50, 3, 8, 17, 1) == 0


@pytest.mark.parametrize("packed", [False, True], ids=["nokeep", "packed"])
@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradients(shape, packed, monkeypatch):
    from recon_amd import _lib, pair_sentence_states
    assert _lib.lib().recon_sent_lstm_supported(*shape)
    rnn, sentence, markers, word_table, pos_table, g_out, keep, ref = case(shape, packed)
    calls = kernels_ran(monkeypatch)
    fused = run(pair_sentence_states, rnn, sentence, markers, word_table, pos_table, g_out, on_gpu(keep))
    assert calls, "the kernels take this shape: the op must not run the chain"
    chain = run(chain_fn, rnn, sentence, markers, word_table, pos_table, g_out, on_gpu(keep))
    B, C, T, Dw, P, H = shape
    assert fused[0].shape == (B, C, 2 * H) and fused[1].shape == (VP, P)
    assert torch.count_nonzero(fused[1][0]) == 0                                # the padding row's gradient
    failures = band_failures(NAMES, fused, chain, ref, "sent_lstm %s %s" % (shape, "packed" if packed else "nokeep"))
    assert not failures, failures


def test_int32_ids_and_strided_id_views_give_the_same_bits():
    from recon_amd import pair_sentence_states
    rnn, sentence, markers, word_table, pos_table, g_out, keep, ref = case((3, 2, 5, 5, 3, 17), True)
    args = (rnn, sentence, markers, word_table, pos_table, g_out, on_gpu(keep))
    a = run(pair_sentence_states, *args)
    same(a, run(pair_sentence_states, *args, ids=lambda s, k: (s.to(torch.int32), k.to(torch.int32))))
    same(a, run(pair_sentence_states, *args, ids=lambda s, k: (s.to(torch.int32), k)))

    def strided(s, k):
        ws = torch.full((s.shape[0], s.shape[1] + 3), 99, dtype=s.dtype, device=s.device)
        wk = torch.full((k.shape[0], k.shape[1], k.shape[2] + 2), 99, dtype=k.dtype, device=k.device)
        ws[:, 1:1 + s.shape[1]] = s
        wk[:, :, 2:] = k
        return ws[:, 1:1 + s.shape[1]], wk[:, :, 2:]
    same(a, run(pair_sentence_states, *args, ids=strided))
    assert rel_err(a[0], ref[0]) <= 2e-5


def test_out_of_range_ids_behave_as_the_clamped_id():
    from recon_amd import pair_sentence_states
    rnn, sentence, markers, word_table, pos_table, g_out, keep, _ = case((3, 2, 5, 5, 3, 17), False)
    ws, wk = sentence.clone(), markers.clone()
    ws[0, 0], ws[2, 4], wk[0, 0, 0], wk[2, 1, 3] = -3, VW + 5, -1, 2 ** 40
    a = run(pair_sentence_states, rnn, ws.clamp(0, VW - 1), wk.clamp(0, VP - 1), word_table, pos_table, g_out, None)
    same(a, run(pair_sentence_states, rnn, ws, wk, word_table, pos_table, g_out, None))


def test_forward_and_backward_are_bitwise_reproducible():
    from recon_amd import pair_sentence_states
    for shape, packed in (((3, 2, 5, 5, 3, 17), True), (LONG_THIN, False), (LONG_THIN, True)):
        rnn, sentence, markers, word_table, pos_table, g_out, keep, _ = case(shape, packed)
        args = (rnn, sentence, markers, word_table, pos_table, g_out, on_gpu(keep))
        same(run(pair_sentence_states, *args), run(pair_sentence_states, *args))


def test_no_grad_allocates_no_saved_state_and_gives_the_training_forwards_bits():
    from recon_amd import _lib, pair_sentence_states
    shape = (3, 72, 2, 50, 3, 100)
    B, C, T, Dw, P, H = shape
    rnn, sentence, markers, word_table, pos_table, g_out, keep, _ = case(shape, True)
    m = copy.deepcopy(rnn).to(dev())
    s, k, wt, pt, kp = sentence.to(dev()), markers.to(dev()), word_table.to(dev()), pos_table.to(dev()).requires_grad_(True), on_gpu(keep)
    L = _lib.lib()
    trained = pair_sentence_states(m, s, k, wt, pt, kp)
    saved = trained.grad_fn.saved_tensors
    assert any(t is not None and t.dtype == torch.uint8 and t.numel() == L.recon_sent_lstm_saved_bytes(*shape) for t in saved)

    def forward():
        with torch.no_grad():
            return pair_sentence_states(m, s, k, wt, pt, kp)
    peak, out = peak_bytes(forward)
    allowed = rounded(B * C * 2 * H * 4) + rounded(L.recon_sent_lstm_workspace_bytes(*shape, VP, 0))
    print("sent_lstm memory (no_grad): peak %d bytes, allowed %d, saved state would be %d" % (peak, allowed, L.recon_sent_lstm_saved_bytes(*shape)))
    assert peak <= allowed < L.recon_sent_lstm_saved_bytes(*shape)
    assert out.grad_fn is None and torch.equal(out, trained.detach())


def test_second_backward_and_create_graph_take_the_recompute_branch(monkeypatch):
    from recon_amd import pair_sentence_states
    shape = (2, 3, 3, 4, 3, 3)
    rnn, sentence, markers, word_table, pos_table, g_out, keep, ref = case(shape, True)
    m = copy.deepcopy(rnn).to(dev()).train()
    pt = pos_table.to(dev()).requires_grad_(True)
    kernel_calls, chain_calls = kernels_ran(monkeypatch), chain_ran(monkeypatch)
    out = pair_sentence_states(m, sentence.to(dev()), markers.to(dev()), word_table.to(dev()), pt, on_gpu(keep))
    assert kernel_calls and not chain_calls
    leaves = [pt] + list(m.parameters())
    first = torch.autograd.grad(out, leaves, g_out.to(dev()), retain_graph=True)
    assert not chain_calls
    second = torch.autograd.grad(out, leaves, g_out.to(dev()), retain_graph=True)
    assert len(chain_calls) == 1
    third = torch.autograd.grad(out, leaves, g_out.to(dev()), create_graph=True)
    assert len(chain_calls) == 2
    for f, s, t, r in zip(first, second, third, ref[1:]):
        assert rel_err(f, r) <= 2e-5 and rel_err(s, r) <= 2e-5 and rel_err(t, r) <= 2e-5 and t.requires_grad
    third[1].square().sum().backward()
    assert pt.grad is not None and torch.isfinite(pt.grad).all()


def test_unsupported_shape_and_fp32_keep_run_the_chain(monkeypatch):
    from recon_amd import _lib, pair_sentence_states
    shape = (2, 2, 3, 4, 3, 257)
    assert not _lib.lib().recon_sent_lstm_supported(*shape)
    rnn, sentence, markers, word_table, pos_table, g_out, keep = inputs(*shape)
    kernel_calls, chain_calls = kernels_ran(monkeypatch), chain_ran(monkeypatch)
    a = run(pair_sentence_states, rnn, sentence, markers, word_table, pos_table, g_out, None)
    assert len(chain_calls) == 1 and not kernel_calls
    same(a, run(chain_fn, rnn, sentence, markers, word_table, pos_table, g_out, None))
    rnn, sentence, markers, word_table, pos_table, g_out, keep, _ = case((2, 3, 3, 4, 3, 3), True)
    f = keep.factors().view(2, 3, 3, 4).to(dev())
    run(pair_sentence_states, rnn, sentence, markers, word_table, pos_table, g_out, f)
    assert not kernel_calls


def test_empty_batch():
    from recon_amd import pair_sentence_states
    rnn, sentence, markers, word_table, pos_table, _, _ = inputs(2, 3, 3, 4, 3, 3)
    out = pair_sentence_states(rnn.to(dev()), sentence[:0].to(dev()), markers[:0].to(dev()), word_table.to(dev()), pos_table.to(dev()))
    assert out.shape == (0, 3, 6) and out.is_cuda


def _seeded_gpgnn():
    from recon_amd.gpgnn import GPGNN
    torch.manual_seed(5)
    p = {"max_num_nodes": 3, "embedding_dim": 2, "layer_number": 2, "projection_style": "untie", "non-linear1": "relu", "non-linear": "tanh",
         "dropout1": 0.5, "position_emb": 3, "units1": 4, "rnn1_layers": 1, "bidirectional": 1, "batch_size": 2}
    m = GPGNN(p, np.random.RandomState(0).randn(9, 5).astype("float32"), max_sent_len=4, n_out=3).to(dev()).train()
    m.fused_sentence_encoder, m.packed_word_dropout = True, True
    m.dropout2.p = 0.0
    return m


def test_packed_word_dropout_is_governed_by_the_seed(monkeypatch):
    m = _seeded_gpgnn()
    calls = kernels_ran(monkeypatch)
    g = torch.Generator().manual_seed(1)
    sent, mark = torch.randint(1, 9, (2, 4), generator=g).to(dev()), torch.randint(0, 4, (2, 6, 4), generator=g).to(dev())
    torch.manual_seed(3)
    a = m.encode(sent, mark)
    torch.manual_seed(3)
    b = m.encode(sent, mark)
    c = m.encode(sent, mark)
    assert len(calls) == 3
    assert torch.equal(a, b) and not torch.equal(a, c)


def _through_the_op(fixture, monkeypatch):
    pinned(*fixture, monkeypatch, "fused_sentence_encoder", kernels_ran(monkeypatch), lambda m: ([m.rnn1], "nn.LSTM.forward of rnn1 ran"),
           ["g.rnn1.", "g.pos_embedding.weight"])


@pytest.mark.parametrize("name", ["gpgnn1_untied", "gpgnn2_tied_n9"])
def test_gpgnn_fixture_through_the_op(name, monkeypatch):
    _through_the_op(gpgnn_fixture(name), monkeypatch)


def test_recon_eac_fixture_through_the_op(monkeypatch):
    _through_the_op(eac_fixture(), monkeypatch)
