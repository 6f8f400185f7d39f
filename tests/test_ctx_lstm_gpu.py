"""recon_amd.context_line_states (csrc/ctx_lstm.hip) against the stock lines of models/models.py:56-70 in fp64 on the CPU, and against the
fixture written from the reference's EntityEmbedding.

Tolerance of value and gradients: `op_checks.bound` of the stock fp32 chain's own error on the GPU against fp64 on the same inputs, measured
in the test.  Weights uniform in +-1 / sqrt(H) (nn.LSTM's own init), inputs N(0, 1).  No cell is excluded: the op makes no discrete choice.  The
figures measured on an MI355X are in DESIGN.md section 20."""
import copy
import ctypes

import pytest
import torch
from torch import nn

from conftest import load_golden
from op_checks import band_failures, calls_of, close, dev, peak_bytes, rel_err, rounded, same
from test_char_features_cpu import fixture_model
from test_ctx_lstm_cpu import VW, inputs, stock

pytestmark = pytest.mark.gpu

G_BWD = 128                                     # the backward's workgroup cap (context_lstm.BWD_MAX_WORKGROUPS, asserted below)
LONG_THIN = (2 * 16 * G_BWD + 5, 3, 3, 4, 5)
#        S   T  Dw  Fc  H
CASES = [(1, 1, 1, 1, 1), (3, 3, 4, 6, 3), (17, 5, 3, 4, 5), (33, 7, 0, 41, 64), (20, 2, 50, 50, 50), (130, 32, 50, 50, 50), LONG_THIN]
REF_WIDTHS = (130, 32, 50, 50, 50)
NAMES = ("out", "feat", "word_table", "weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse",
         "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")


_CASES = {}


def case(shape):
    """Inputs and the fp64 oracle (value, d_feat, d_table, the eight parameter gradients) of a shape, computed once and left unchanged."""
    if shape not in _CASES:
        lstm, feat, words, table, g_out = inputs(*shape)
        l64 = copy.deepcopy(lstm).double()
        f = feat.double().requires_grad_(True)
        tb = table.double().requires_grad_(True) if table is not None else None
        ref = stock(l64, f, words, tb)
        ref.backward(g_out.double())
        grads = [ref.detach(), f.grad, tb.grad if tb is not None else None] + [p.grad for p in l64.parameters()]
        _CASES[shape] = (lstm, feat, words, table, g_out, grads)
    return _CASES[shape]


def run(fn, lstm, feat, words, table, g_out, frozen_table=False, ids=None):
    """[out, d_feat, d_table (or None), eight parameter gradients] of fn on the GPU; the module in training mode, as MIOpen's backward needs."""
    m = copy.deepcopy(lstm).to(dev()).train()
    f = feat.to(dev()).requires_grad_(True)
    tb = table.to(dev()).requires_grad_(not frozen_table) if table is not None else None
    w = None if words is None else (words if ids is None else ids).to(dev())
    out = fn(m, f, w, tb)
    out.backward(g_out.to(dev()))
    return [out.detach(), f.grad, tb.grad if tb is not None else None] + [p.grad for p in m.parameters()]


def kernels_ran(monkeypatch):
    from recon_amd import context_lstm
    return calls_of(monkeypatch, context_lstm._ContextLineStates, "apply")


def chain_ran(monkeypatch):
    from recon_amd import context_lstm
    return calls_of(monkeypatch, context_lstm, "_chain")


def test_workgroup_cap_is_the_librarys():
    from recon_amd import _lib, context_lstm
    assert context_lstm.BWD_MAX_WORKGROUPS == G_BWD
    S, T, Dw, Fc, H = LONG_THIN
    slab = 2 * 4 * H * (Dw + Fc + H + 1) * 4
    n_slabs = _lib.lib().recon_ctx_lstm_workspace_bytes(S, T, Dw, Fc, H, 1) / slab
    per = -(-S // G_BWD)
    assert per > 32 and -(-S // per) - 1 < n_slabs <= -(-S // per) + 1 and n_slabs > 100            # every slab: more than two tiles of 16
    assert _lib.lib().recon_ctx_lstm_workspace_bytes(10 ** 6, T, Dw, Fc, H, 1) == (G_BWD * slab + 255) // 256 * 256


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradients(shape, monkeypatch):
    from recon_amd import _lib, context_line_states
    from recon_amd.context_lstm import _chain
    assert _lib.lib().recon_ctx_lstm_supported(*shape)
    lstm, feat, words, table, g_out, ref = case(shape)
    calls = kernels_ran(monkeypatch)
    fused = run(context_line_states, lstm, feat, words, table, g_out)
    assert calls, "the kernels take this shape: the op must not run the chain"
    chain = run(_chain, lstm, feat, words, table, g_out)
    S, T, Dw, Fc, H = shape
    assert fused[0].shape == (S, 2 * H) and fused[1].shape == (S, T, Fc)
    failures = band_failures(NAMES, fused, chain, ref, "ctx_lstm %s" % (shape,))
    assert not failures, failures


def test_int32_ids():
    from recon_amd import context_line_states
    lstm, feat, words, table, g_out, ref = case((17, 5, 3, 4, 5))
    a = run(context_line_states, lstm, feat, words, table, g_out)
    c = run(context_line_states, lstm, feat, words, table, g_out, ids=words.to(torch.int32))
    same(a, c)
    assert rel_err(c[0], ref[0]) <= 2e-5


def test_strided_feat_is_read_in_place():
    """A column slice of a wider tensor: the same bits as the contiguous copy, and under no_grad the forward's peak above the inputs is out
    plus the workspace — no S T Fc copy, no saved buffer."""
    from recon_amd import _lib, context_line_states
    lstm, feat, words, table, g_out, _ = case(REF_WIDTHS)
    S, T, Dw, Fc, H = REF_WIDTHS
    wide = torch.full((S, T, Fc + 5), 7.0)
    wide[:, :, 2:2 + Fc] = feat
    a = run(context_line_states, lstm, feat, words, table, g_out)
    c = run(lambda m, f, w, tb: context_line_states(m, f[:, :, 2:2 + Fc], w, tb), lstm, wide, words, table, g_out)
    same([a[0]] + a[2:], [c[0]] + c[2:])
    assert torch.equal(a[1], c[1][:, :, 2:2 + Fc]) and torch.count_nonzero(c[1][:, :, :2]) == 0 and torch.count_nonzero(c[1][:, :, 2 + Fc:]) == 0
    m = copy.deepcopy(lstm).to(dev())
    view, w, tb = wide.to(dev())[:, :, 2:2 + Fc], words.to(dev()), table.to(dev())
    allowed = rounded(S * 2 * H * 4) + rounded(_lib.lib().recon_ctx_lstm_workspace_bytes(S, T, Dw, Fc, H, 0))
    assert allowed < S * T * Fc * 4

    def forward():
        with torch.no_grad():
            return context_line_states(m, view, w, tb)
    peak, out = peak_bytes(forward)
    print("ctx_lstm memory (no_grad, strided feat): peak %d bytes, allowed %d, a copy of feat %d" % (peak, allowed, S * T * Fc * 4))
    assert peak <= allowed, (peak, allowed)
    assert torch.equal(out, a[0])


def test_out_of_range_ids_behave_as_the_clamped_id():
    from recon_amd import context_line_states
    lstm, feat, words, table, g_out, _ = case((17, 5, 3, 4, 5))
    wild = words.clone()
    wild[0, 0], wild[3, 2], wild[16, 4] = -3, VW + 5, 2 ** 40
    a = run(context_line_states, lstm, feat, words, table, g_out, ids=wild.clamp(0, VW - 1))
    c = run(context_line_states, lstm, feat, words, table, g_out, ids=wild)
    same(a, c)


def test_forward_and_backward_are_bitwise_reproducible():
    from recon_amd import context_line_states
    for shape in ((17, 5, 3, 4, 5), LONG_THIN):
        lstm, feat, words, table, g_out, _ = case(shape)
        same(run(context_line_states, lstm, feat, words, table, g_out), run(context_line_states, lstm, feat, words, table, g_out))


def test_frozen_table_gets_no_word_vector_gradient(monkeypatch):
    from recon_amd import _lib, context_line_states
    lstm, feat, words, table, g_out, _ = case((20, 2, 50, 50, 50))
    seen = []
    real = _lib.lib().recon_ctx_lstm_bwd
    monkeypatch.setattr(_lib.lib(), "recon_ctx_lstm_bwd", lambda *a: (seen.append(a), real(*a))[1])
    frozen = run(context_line_states, lstm, feat, words, table, g_out, frozen_table=True)
    live = run(context_line_states, lstm, feat, words, table, g_out)
    assert len(seen) == 2 and seen[0][19] is None and seen[1][19] is not None and seen[0][18] is not None      # d_word_vec, d_feat
    assert frozen[2] is None and live[2] is not None
    same(frozen[:2] + frozen[3:], live[:2] + live[3:])


def test_saved_state_is_what_the_library_sizes_and_nothing_else():
    from recon_amd import _lib, context_line_states
    lstm, feat, words, table, g_out, _ = case(REF_WIDTHS)
    S, T, Dw, Fc, H = REF_WIDTHS
    m = copy.deepcopy(lstm).to(dev())
    f, w, tb = feat.to(dev()).requires_grad_(True), words.to(dev()), table.to(dev())
    want = _lib.lib().recon_ctx_lstm_saved_bytes(S, T, Dw, Fc, H)
    assert want == 2 * S * T * 5 * H * 4
    allowed = rounded(S * 2 * H * 4) + rounded(_lib.lib().recon_ctx_lstm_workspace_bytes(S, T, Dw, Fc, H, 0)) + rounded(want)
    peak, out = peak_bytes(lambda: context_line_states(m, f, w, tb))
    print("ctx_lstm memory (grad): peak %d bytes, allowed %d" % (peak, allowed))
    assert peak <= allowed, (peak, allowed)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 5 + 8
    assert saved[0] is f or saved[0].data_ptr() == f.data_ptr()
    assert saved[1].data_ptr() == w.data_ptr() and saved[2].data_ptr() == tb.data_ptr() and saved[3].data_ptr() == out.data_ptr()
    assert saved[4].dtype == torch.uint8 and saved[4].numel() == want
    assert [s.data_ptr() for s in saved[5:]] == [p.data_ptr() for p in m.parameters()]


def test_create_graph_stays_differentiable(monkeypatch):
    from recon_amd import context_line_states
    lstm, feat, words, table, g_out, ref = case((3, 3, 4, 6, 3))
    m = copy.deepcopy(lstm).to(dev()).train()
    f, tb = feat.to(dev()).requires_grad_(True), table.to(dev()).requires_grad_(True)
    kernel_calls, chain_calls = kernels_ran(monkeypatch), chain_ran(monkeypatch)
    out = context_line_states(m, f, words.to(dev()), tb)
    assert kernel_calls and not chain_calls
    leaves = [f, tb] + list(m.parameters())
    grads = torch.autograd.grad(out, leaves, g_out.to(dev()), create_graph=True)
    assert chain_calls
    for g, r in zip(grads, ref[1:]):
        assert g.requires_grad and rel_err(g, r) <= 2e-5
    grads[3].square().sum().backward()
    assert f.grad is not None and torch.isfinite(f.grad).all() and torch.count_nonzero(f.grad) > 0


def test_second_backward_over_a_retained_graph_is_still_right():
    from recon_amd import context_line_states
    lstm, feat, words, table, g_out, ref = case((17, 5, 3, 4, 5))
    m = copy.deepcopy(lstm).to(dev())
    f = feat.to(dev()).requires_grad_(True)
    out = context_line_states(m, f, words.to(dev()), table.to(dev()))
    first, = torch.autograd.grad(out, f, g_out.to(dev()), retain_graph=True)
    second, = torch.autograd.grad(out, f, g_out.to(dev()))
    assert rel_err(first, ref[1]) <= 2e-5 and rel_err(second, ref[1]) <= 2e-5


def test_unsupported_shape_runs_the_chain(monkeypatch):
    from recon_amd import _lib, context_line_states
    from recon_amd.context_lstm import _chain
    shape = (4, 3, 200, 200, 64)                                                # 4 H (I + H) floats = 475 KB
    assert not _lib.lib().recon_ctx_lstm_supported(*shape)
    lstm, feat, words, table, g_out = inputs(*shape)
    kernel_calls, chain_calls = kernels_ran(monkeypatch), chain_ran(monkeypatch)
    a = run(context_line_states, lstm, feat, words, table, g_out)
    assert chain_calls and not kernel_calls
    same(a, run(_chain, lstm, feat, words, table, g_out))


def test_empty_batch():
    from recon_amd import context_line_states
    lstm, feat, words, table, _ = inputs(2, 3, 4, 6, 3)
    out = context_line_states(lstm.to(dev()), feat[:0].to(dev()).requires_grad_(True), words[:0].to(dev()), table.to(dev()))
    assert out.shape == (0, 6) and out.is_cuda


def test_c_abi_agrees_with_the_op_and_launches_nothing_for_an_empty_batch():
    from recon_amd import _lib, context_line_states
    shape = (17, 5, 3, 4, 5)
    S, T, Dw, Fc, H = shape
    lstm, feat, words, table, g_out, _ = case(shape)
    want = run(context_line_states, lstm, feat, words, table, g_out)
    L, d = _lib.lib(), dev()
    p = [q.detach().to(d).contiguous() for q in lstm.parameters()]
    f, w, tb, g = feat.to(d), words.to(d), table.to(d), g_out.to(d)
    out = torch.empty(S, 2 * H, device=d)
    saved = torch.empty(L.recon_ctx_lstm_saved_bytes(*shape), dtype=torch.uint8, device=d)
    ws = torch.empty(L.recon_ctx_lstm_workspace_bytes(*shape, 0), dtype=torch.uint8, device=d)
    st = _lib.current_stream()
    assert L.recon_ctx_lstm_fwd(w.data_ptr(), 8, T, tb.data_ptr(), VW, f.data_ptr(), Fc, *[q.data_ptr() for q in p], *shape, out.data_ptr(),
                                saved.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
    assert L.recon_ctx_lstm_fwd(w.data_ptr(), 8, T, tb.data_ptr(), VW, f.data_ptr(), Fc, *[q.data_ptr() for q in p], *shape, out.data_ptr(),
                                saved.data_ptr(), ws.data_ptr(), 16, st) == -4
    d_feat, d_wv = torch.empty(S, T, Fc, device=d), torch.empty(S, T, Dw, device=d)
    gp = [torch.empty_like(q) for q in p]
    ws = torch.empty(L.recon_ctx_lstm_workspace_bytes(*shape, 1), dtype=torch.uint8, device=d)
    assert L.recon_ctx_lstm_bwd(w.data_ptr(), 8, T, tb.data_ptr(), VW, f.data_ptr(), Fc, p[0].data_ptr(), p[1].data_ptr(), p[4].data_ptr(),
                                p[5].data_ptr(), g.data_ptr(), saved.data_ptr(), *shape, d_feat.data_ptr(), d_wv.data_ptr(),
                                *[q.data_ptr() for q in gp], ws.data_ptr(), ws.numel(), st) == 0
    g_table = torch.zeros(VW, Dw, device=d).index_add_(0, w.reshape(-1), d_wv.reshape(-1, Dw))
    assert torch.equal(out, want[0]) and torch.equal(d_feat, want[1])
    assert rel_err(g_table, want[2].double().cpu()) <= 2e-6                      # (another summation order than the embedding's backward)
    same(gp, want[3:])
    # S = 0: no pointer is touched forward (all NULL), the backward writes zeros to the eight parameter gradients
    assert L.recon_ctx_lstm_fwd(None, 8, 0, None, 0, None, 0, *[None] * 8, 0, T, Dw, Fc, H, None, None, None, 0, st) == 0
    for q in gp:
        q.fill_(1.0)
    assert L.recon_ctx_lstm_bwd(None, 8, 0, None, 0, None, 0, None, None, None, None, None, None, 0, T, Dw, Fc, H, None, None,
                                *[q.data_ptr() for q in gp], None, 0, st) == 0
    torch.cuda.synchronize()
    assert all(torch.count_nonzero(q) == 0 for q in gp)
    assert L.recon_ctx_lstm_fwd(w.data_ptr(), 8, T, tb.data_ptr(), VW, f.data_ptr(), Fc, *[q.data_ptr() for q in p], 1, T, 200, 200, 64,
                                out.data_ptr(), None, ws.data_ptr(), ws.numel(), st) == -2
    assert isinstance(L.recon_ctx_lstm_saved_bytes(1, T, 200, 200, 64), int) and L.recon_ctx_lstm_saved_bytes(1, T, 200, 200, 64) == 0
    assert ctypes.sizeof(ctypes.c_size_t) == 8


def test_fixture_entity_embedding(monkeypatch):
    """EntityEmbedding with the fixture's parameters (strict load) against the reference module's output and the gradient of every
    parameter at the whole-model bounds; the new kernels run and nn.LSTM.forward does not."""
    g = load_golden("ctx_lstm1")
    m = fixture_model(g)
    calls = kernels_ran(monkeypatch)
    monkeypatch.setattr(nn.LSTM, "forward", lambda *a, **k: pytest.fail("nn.LSTM.forward ran"))
    m.to(dev())
    t = lambda k: torch.from_numpy(g[k]).to(dev())
    out = m(t("words"), t("chars"), t("mask"))
    assert calls
    close(out, g["out"], atol=1e-4, what="ctx_lstm1 out")
    (out * t("G").float()).sum().backward()
    grads = {k: p.grad for k, p in m.named_parameters()}
    names = {k[2:] for k in g if k.startswith("g.")}
    assert names == set(grads) and len(names) == 14
    for k in sorted(names):
        close(grads[k], g["g." + k], atol=1e-4, rel_to_max=1e-4, what="ctx_lstm1 grad " + k)
