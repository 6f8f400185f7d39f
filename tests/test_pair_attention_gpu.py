"""recon_amd.pair_context_attention (csrc/pair_attn.hip) and recon_amd.ContextAware on the GPU, against the loop of
models/baselines.py:86-111 in float64 on the CPU and against the fixtures written from the reference's ContextAware.

Shapes, inputs and the oracle are those of tests/pair_attention_checks.py, guarded by tests/test_pair_attention_cpu.py; the band is
`op_checks.bound` of the fp32 loop's own error on the GPU, for out, g_states and g_weight.  The figures measured on an MI355X are in
DESIGN.md section 30."""
import numpy as np
import pytest
import torch
from torch import nn

from op_checks import calls_of, dev, peak_bytes, pinned, rel_err, rounded, same
from pair_attention_checks import (GRID, OVER, REF_TWO, case, context_aware_fixture, context_aware_for_epochs, failures, hand_written, ids, loop,
                                   run)
from stage_b_checks import join_rows, permutation, row_differences

pytestmark = pytest.mark.gpu


def kernels_ran(monkeypatch):
    from recon_amd import pair_attention
    return calls_of(monkeypatch, pair_attention._PairAttention, "apply"), calls_of(monkeypatch, pair_attention, "_chain")


@pytest.mark.parametrize("shape", GRID, ids=ids)
def test_value_and_gradients(shape, monkeypatch):
    from recon_amd import _lib, pair_context_attention
    c = case(shape)
    kernel, chain_calls = kernels_ran(monkeypatch)
    fused = run(pair_context_attention, c, dev())
    if shape == OVER:
        assert not _lib.lib().recon_pair_attention_supported(*shape)
        assert (len(kernel), len(chain_calls)) == (0, 1), "beyond MAX_PAIRS the op must run the chain"
    else:
        assert _lib.lib().recon_pair_attention_supported(*shape)
        assert (len(kernel), len(chain_calls)) == (1, 0), "the kernels take this shape: the op must not run the chain"
    chain = run(loop, c, dev())
    bad = failures(fused, chain, c["ref"], "%s" % (shape,))
    assert not bad, bad
    if shape[1] == 1:
        assert torch.count_nonzero(fused[0][:, :, shape[2]:]) == 0 and torch.count_nonzero(fused[2]) == 0       # ctx exactly 0


# ------------------------------------------------------------------------------------------------------------- the ABI, called directly
GUARD = 37


def guarded(numel, align=1):
    """(whole NaN-filled buffer, offset of `numel` elements behind a guard of at least GUARD elements whose address is a multiple of
    4 `align` bytes)."""
    whole = torch.full((numel + 2 * GUARD + align,), float("nan"), device=dev())
    at = GUARD
    while (whole.data_ptr() + 4 * at) % (4 * align):
        at += 1
    return whole, at


def untouched(whole, at, numel):
    return bool(torch.isnan(whole[:at]).all()) and bool(torch.isnan(whole[at + numel:]).all())


@pytest.mark.parametrize("shape", [(2, 17, 68), REF_TWO], ids=ids)
def test_entries_write_their_cells_and_nothing_else(shape):
    from recon_amd import _lib
    L = _lib.lib()
    B, C, D = shape
    c = case(shape)
    s = c["states"].to(dev())
    m = (c["states"] @ c["weight"].t()).to(dev())
    g = c["g_out"].to(dev())
    ld_out = 2 * D + 8
    out_w, out_at = guarded(B * C * ld_out, align=4)
    P_w, P_at = guarded(B * C * C)
    st = _lib.current_stream()
    _lib.check(L.recon_pair_attention_fwd(s.data_ptr(), D, m.data_ptr(), D, B, C, D, out_w.data_ptr() + 4 * out_at, ld_out, P_w.data_ptr() + 4 * P_at, st),
               "fwd")
    torch.cuda.synchronize()
    assert untouched(out_w, out_at, B * C * ld_out) and untouched(P_w, P_at, B * C * C)
    rows = out_w[out_at:out_at + B * C * ld_out].view(B, C, ld_out)
    assert torch.isnan(rows[:, :, 2 * D:]).all() and not torch.isnan(rows[:, :, :2 * D]).any()          # the stride's gap stays as it was
    assert torch.equal(rows[:, :, :D], s)
    P = P_w[P_at:P_at + B * C * C].view(B, C, C)
    assert torch.count_nonzero(torch.diagonal(P, dim1=1, dim2=2)) == 0
    assert (P.sum(dim=2) - 1).abs().max().item() <= 1e-6 and P.min().item() >= 0
    # the float64 reference over (states, memory) as two inputs
    s64, m64 = s.double().cpu().requires_grad_(True), m.double().cpu().requires_grad_(True)
    from recon_amd.pair_attention import _attend
    ref = _attend(s64, m64)
    ref.backward(c["g_out"].double())
    assert rel_err(rows[:, :, :2 * D], ref.detach()) <= 2e-5
    # the same forward without a P: the same bits in out
    out2 = torch.empty(B, C, 2 * D, device=dev())
    _lib.check(L.recon_pair_attention_fwd(s.data_ptr(), D, m.data_ptr(), D, B, C, D, out2.data_ptr(), 2 * D, None, st), "fwd without P")
    assert torch.equal(out2, rows[:, :, :2 * D])
    # ---- backward
    gs_w, gs_at = guarded(B * C * D)
    gm_w, gm_at = guarded(B * C * D)
    nbytes = L.recon_pair_attention_workspace_bytes(B, C, D, 1)
    ws_w, ws_at = guarded(nbytes // 4, align=4)
    Pc = P.contiguous()
    _lib.check(L.recon_pair_attention_bwd(s.data_ptr(), D, m.data_ptr(), D, Pc.data_ptr(), g.data_ptr(), 2 * D, B, C, D, gs_w.data_ptr() + 4 * gs_at,
                                          gm_w.data_ptr() + 4 * gm_at, ws_w.data_ptr() + 4 * ws_at, nbytes, st), "bwd")
    torch.cuda.synchronize()
    assert untouched(gs_w, gs_at, B * C * D) and untouched(gm_w, gm_at, B * C * D) and untouched(ws_w, ws_at, nbytes // 4)
    g_states, g_memory = gs_w[gs_at:gs_at + B * C * D].view(B, C, D), gm_w[gm_at:gm_at + B * C * D].view(B, C, D)
    assert not torch.isnan(g_states).any() and not torch.isnan(g_memory).any()
    assert rel_err(g_states, s64.grad) <= 2e-5 and rel_err(g_memory, m64.grad) <= 2e-5
    # one gradient alone: the same bits, the other buffer is not needed
    only = torch.empty(B, C, D, device=dev())
    _lib.check(L.recon_pair_attention_bwd(s.data_ptr(), D, m.data_ptr(), D, Pc.data_ptr(), g.data_ptr(), 2 * D, B, C, D, None, only.data_ptr(),
                                          ws_w.data_ptr() + 4 * ws_at, nbytes, st), "bwd g_memory")
    assert torch.equal(only, g_memory)
    _lib.check(L.recon_pair_attention_bwd(s.data_ptr(), D, m.data_ptr(), D, Pc.data_ptr(), g.data_ptr(), 2 * D, B, C, D, only.data_ptr(), None,
                                          ws_w.data_ptr() + 4 * ws_at, nbytes, st), "bwd g_states")
    assert torch.equal(only, g_states)


# ------------------------------------------------------------------------------------------------------------- bits
def test_forward_and_backward_are_bitwise_reproducible():
    from recon_amd import pair_context_attention
    for shape in ((2, 17, 68), REF_TWO, (3, 15, 36)):
        c = case(shape)
        same(run(pair_context_attention, c, dev()), run(pair_context_attention, c, dev()))


def test_second_backward_over_a_retained_graph_gives_the_same_bits(monkeypatch):
    from recon_amd import pair_context_attention
    c = case((2, 33, 100))
    s = c["states"].to(dev()).requires_grad_(True)
    w = c["weight"].to(dev()).requires_grad_(True)
    g = c["g_out"].to(dev())
    _, chain_calls = kernels_ran(monkeypatch)
    out = pair_context_attention(s, w)
    kept = out.clone()
    first = torch.autograd.grad(out, [s, w], g, retain_graph=True)
    second = torch.autograd.grad(out, [s, w], g, retain_graph=True)
    same(first, second)
    assert torch.equal(kept, out) and not chain_calls                   # the backward destroys nothing
    for a, r in zip(first, c["ref"][1:]):
        assert rel_err(a, r) <= 2e-5


def test_strided_states_and_g_out_give_the_contiguous_copys_bits(monkeypatch):
    from recon_amd import pair_context_attention
    kernel, chain_calls = kernels_ran(monkeypatch)

    def strided(x):
        wide = torch.full(x.shape[:2] + (x.shape[2] + 8,), 99.0, device=x.device)
        wide[:, :, 4:4 + x.shape[2]] = x
        v = wide[:, :, 4:4 + x.shape[2]]
        assert not v.is_contiguous()
        return v.detach()

    def permuted(x):
        v = x.transpose(0, 1).contiguous().transpose(0, 1)
        assert not v.is_contiguous() or x.shape[0] == 1
        return v
    for shape in ((2, 17, 68), (3, 15, 36)):
        c = case(shape)
        plain = run(pair_context_attention, c, dev())
        same(plain, run(pair_context_attention, c, dev(), states_of=strided))
        same(plain, run(pair_context_attention, c, dev(), g_of=strided))
        same(plain, run(pair_context_attention, c, dev(), g_of=permuted))
    assert len(kernel) == 8 and not chain_calls


def test_no_grad_gives_the_training_forwards_bits_and_allocates_no_p():
    from recon_amd import pair_context_attention
    B, C, D = REF_TWO
    c = case(REF_TWO)
    s = c["states"].to(dev()).requires_grad_(True)
    w = c["weight"].to(dev()).requires_grad_(True)
    out_bytes, mem_bytes, p_bytes = rounded(B * C * 2 * D * 4), rounded(B * C * D * 4), rounded(B * C * C * 4)

    def plain():
        with torch.no_grad():
            return pair_context_attention(s, w)
    peak, a = peak_bytes(plain)
    assert peak == out_bytes + mem_bytes, (peak, out_bytes, mem_bytes)
    peak, b = peak_bytes(lambda: pair_context_attention(s, w))
    assert peak == out_bytes + mem_bytes + p_bytes, (peak, out_bytes, mem_bytes, p_bytes)          # nothing of size B C (C - 1) D exists
    assert a.grad_fn is None and b.grad_fn is not None and torch.equal(a, b.detach())


def test_create_graph_and_other_dtypes_run_the_chain(monkeypatch):
    from recon_amd import pair_context_attention
    kernel, chain_calls = kernels_ran(monkeypatch)
    c = case((2, 17, 68))
    s = c["states"].to(dev()).requires_grad_(True)
    w = c["weight"].to(dev()).requires_grad_(True)
    out = pair_context_attention(s, w)
    assert len(kernel) == 1
    grads = torch.autograd.grad(out, [s, w], c["g_out"].to(dev()), create_graph=True)
    for a, r in zip(grads, c["ref"][1:]):
        assert rel_err(a, r) <= 2e-5 and a.requires_grad
    grads[0].square().sum().backward()
    assert w.grad is not None and torch.isfinite(w.grad).all()
    out = pair_context_attention(c["states"].to(dev()).double(), c["weight"].to(dev()).double())
    assert len(kernel) == 1 and len(chain_calls) == 1 and out.dtype == torch.float64
    assert rel_err(out, c["ref"][0]) <= 1e-12
    empty = pair_context_attention(s[:0], w)
    assert empty.shape == (0, 17, 136) and len(kernel) == 1


# ------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", ("context_aware1", "context_aware2"))
def test_context_aware_fixture_through_the_op(name, monkeypatch):
    def stock(m):
        assert type(m.linear1) is nn.Linear and m.linear1.bias is None
        return [m.linear1], "linear1's nn.Linear.forward ran"
    kernel, chain_calls = kernels_ran(monkeypatch)
    pinned(*context_aware_fixture(name, dev()), monkeypatch, "fused_ghost_attention", kernel, stock,
           ["g.linear1.weight", "g.linear2.weight", "g.rnn1.", "g.pos_embedding.weight"])
    assert not chain_calls


@pytest.mark.parametrize("dropout", (False, True))
def test_run_epoch_against_the_hand_written_loop(dropout, monkeypatch):
    """N = 7 in batches of 3: two training iterations under recon_amd.optim.Adam(max_grad_norm=0.25), then an evaluation pass with rows.
    Both loops run the same deterministic ops on the same values in the same order: every parameter, counter and row is equal.  With
    `dropout` the packed word dropout is on, in train mode, under one torch.manual_seed for both loops."""
    from recon_amd import EpochRows, RelationMetrics, StageBData, run_epoch
    from recon_amd.optim import Adam
    make, as_indices = context_aware_for_epochs(dev(), dropout)
    bs, order = 3, permutation(7, 3)
    data = StageBData.from_indices(as_indices).to(dev())
    adam = lambda m: Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-2, weight_decay=1e-4, max_grad_norm=0.25)
    kernel, chain_calls = kernels_ran(monkeypatch)
    b = make().train()
    train_b, test_b, parts = RelationMetrics(dev()), RelationMetrics(dev()), []
    torch.manual_seed(77)
    hand_written(b, as_indices, bs, order, adam(b), train_b, None, dev())
    b.eval()
    with torch.no_grad():
        hand_written(b, as_indices, bs, np.arange(7), None, test_b, parts, dev())
    a = make().train()
    train_a, test_a, rows_a = RelationMetrics(dev()), RelationMetrics(dev()), EpochRows.for_data(data)
    torch.manual_seed(77)
    run_epoch(a, data, bs, order=torch.from_numpy(order).to(dev()), optimizer=adam(a), metrics=train_a)
    a.eval()
    run_epoch(a, data, bs, metrics=test_a, rows=rows_a)
    assert len(kernel) == 8 and not chain_calls                         # four iterations per loop, each through the kernels
    fresh = dict(make().named_parameters())
    changed = 0
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k
        changed += int(p.requires_grad and not torch.equal(p, fresh[k]))
    assert changed >= 12                                                # the two iterations trained every trainable parameter
    assert train_a.result() == train_b.result() and train_a.result().batches == 2 and train_a.result().kept > 0
    assert test_a.result() == test_b.result() and test_a.result().batches == 2
    got = rows_a.result()
    assert got.pair.numel() == test_a.result().kept > 0
    assert row_differences(got, join_rows(parts)) == []
