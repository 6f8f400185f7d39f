"""recon_amd.sentence_conv_pool (csrc/sent_conv.hip) and recon_amd.CNN, PCNN and LSTM on the GPU, against the lines of
models/baselines.py:237-247 / :297-308 in float64 on the CPU and against the fixtures written from the reference's classes.

Cases, inputs, the oracle and the near-tie rule are those of tests/sentence_conv_checks.py, guarded by tests/test_sentence_conv_cpu.py; the
band is `op_checks.bound` of the stock fp32 chain's own error on the GPU, for out, both table gradients and every weight and bias
gradient.  The figures measured on an MI355X are in DESIGN.md section 31.

One assertion departs from the issue this op answers.  The issue asks that `peak_bytes` of a forward under no_grad be `rounded(out)`
alone.  The forward is two launches, and the first writes the weights K-major into a workspace (0.9 MB at the reference's widths), so
`test_no_grad_allocates_the_output_alone` asserts a peak of exactly out + that workspace, and that out alone stays allocated after the
call.  The assertion is exact, so it still shows that nothing of size B T Cin or B E T_out is allocated."""
import ctypes
import gc

import pytest
import torch
from torch import nn

from op_checks import calls_of, close, dev, peak_bytes, pinned, rel_err, rounded, same
from sentence_conv_checks import (GRID, ODD, ODD_P, OVER, REF_WIDTHS, REF_WIDTHS_P, baseline_fixture, case, failures, ids, inputs, lines, run,
                                  training_rows)

pytestmark = pytest.mark.gpu


def kernels_ran(monkeypatch):
    from recon_amd import sentence_conv
    return calls_of(monkeypatch, sentence_conv._SentenceConvPool, "apply"), calls_of(monkeypatch, sentence_conv, "_chain")


@pytest.mark.parametrize("shape", GRID, ids=ids)
def test_value_and_gradients(shape, monkeypatch):
    from recon_amd import sentence_conv_pool
    c = case(shape)
    kernel, chain_calls = kernels_ran(monkeypatch)
    fused = run(sentence_conv_pool, c, dev())
    if shape in OVER:
        assert (len(kernel), len(chain_calls)) == (0, 1), "beyond MAX_T the op must run the chain"
    else:
        assert (len(kernel), len(chain_calls)) == (1, 0), "the kernels take this shape: the op must not run the chain"
    chain = run(lines, c, dev())
    bad = failures(shape, fused, chain, c["ref"])
    assert not bad, bad
    assert torch.count_nonzero(fused[1][0]) == 0 and torch.count_nonzero(fused[2][0]) == 0       # the padding row


@pytest.mark.parametrize("activation", ("none", "tanh", "relu"))
@pytest.mark.parametrize("shape", (ODD, ODD_P), ids=ids)
def test_each_activation_with_and_without_the_factors(shape, activation, monkeypatch):
    from recon_amd import sentence_conv_pool
    kernel, chain_calls = kernels_ran(monkeypatch)
    for keep, pool_keep in ((True, True), (False, False), (True, False)):
        c = case(shape, activation=activation, keep=keep, pool_keep=pool_keep)
        kw = dict(activation=activation, keep="factors" if keep else None, pool_keep=pool_keep)
        fused = run(sentence_conv_pool, c, dev(), **kw)
        bad = failures(shape, fused, run(lines, c, dev(), **kw), c["ref"], "%s keep %s pool_keep %s" % (activation, keep, pool_keep))
        assert not bad, bad
    assert len(kernel) == 3 and not chain_calls


# ------------------------------------------------------------------------------------------------------------- the ABI, called directly
GUARD = 37


def guarded(numel, dtype=torch.float32):
    """(whole NaN-filled (0xEE-filled for bytes) buffer, the 16-byte aligned offset of `numel` elements behind a guard)."""
    fill = float("nan") if dtype.is_floating_point else 0xEE
    whole = torch.full((numel + 2 * GUARD + 16,), fill, dtype=dtype, device=dev())
    at = GUARD
    while (whole.data_ptr() + whole.element_size() * at) % 16:
        at += 1
    return whole, at


def untouched(whole, at, numel):
    ends = torch.cat([whole[:at], whole[at + numel:]])
    return bool(torch.isnan(ends).all()) if whole.dtype.is_floating_point else bool((ends == 0xEE).all())


@pytest.mark.parametrize("shape", [ODD, ODD_P, ("cnn", 33, 5, 3, 2, 4, (3,)), REF_WIDTHS_P], ids=ids)
def test_entries_write_their_cells_and_nothing_else(shape):
    from recon_amd import _lib
    L = _lib.lib()
    form, B, T, Dw, Dp, E, ks = shape
    c = case(shape)
    n, P, V, seg = len(ks), 2 * T + 1, c["word_table"].shape[0], int(form == "pcnn")
    nE = (3 if seg else n) * E
    d = lambda t: None if t is None else t.to(dev()).contiguous()
    sent, pos, word, p0, p1 = d(c["sentence"]), d(c["positions"]), d(c["word_table"]), d(c["pos_table_0"]), d(c["pos_table_1"])
    ws_, bs_, segs, keep, pk, g = [d(w) for w in c["weights"]], [d(b) for b in c["biases"]], d(c["segments"]), d(c["keep"]), d(c["pool_keep"]), d(c["g_out"])
    arr = (ctypes.c_int32 * n)(*ks)
    act = 1 if form == "cnn" else 2
    st = _lib.current_stream()
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    out_w, out_at = guarded(B * nE)
    at_w, at_at = guarded(B * nE, torch.uint8)
    nbytes = L.recon_sent_conv_workspace_bytes(B, T, Dw, Dp, P, E, arr, n, seg, 0)
    wk_w, wk_at = guarded(nbytes // 4)
    head = (sent.data_ptr(), sent.element_size(), pos.data_ptr(), pos.element_size(), word.data_ptr(), V, p0.data_ptr(), p1.data_ptr(), P, None, 1.0,
            keep.data_ptr(), _lib.ptr(segs), _lib.ptr_array(ws_))
    _lib.check(L.recon_sent_conv_fwd(*head, _lib.ptr_array(bs_), arr, n, pk.data_ptr(), act, B, T, Dw, Dp, E, out_w.data_ptr() + 4 * out_at,
                                     at_w.data_ptr() + at_at, status.data_ptr(), wk_w.data_ptr() + 4 * wk_at, nbytes, st), "fwd")
    torch.cuda.synchronize()
    assert untouched(out_w, out_at, B * nE) and untouched(at_w, at_at, B * nE) and untouched(wk_w, wk_at, nbytes // 4)
    assert int(status) == 0
    out, at = out_w[out_at:out_at + B * nE].view(B, nE), at_w[at_at:at_at + B * nE].view(B, nE)
    assert not torch.isnan(out).any() and not torch.isnan(wk_w[wk_at:wk_at + nbytes // 4]).any()
    assert rel_err(out, c["ref"][0]) <= 2e-5
    live = ~c["ties"]
    expect = c["at"].clone()
    if seg:                                                              # 255 where the float64 winner is the 0 of a zero-factor position
        zero = c["segments"].repeat_interleave(E, dim=1).gather(2, c["at"].unsqueeze(-1)).squeeze(-1) == 0
        assert torch.equal((at.cpu() == 255)[live], zero[live])
        live &= ~zero
    assert torch.equal(at.cpu().long()[live], expect[live])
    # the same forward without the bytes: the same bits in out
    out2 = torch.empty(B, nE, device=dev())
    _lib.check(L.recon_sent_conv_fwd(*head, _lib.ptr_array(bs_), arr, n, pk.data_ptr(), act, B, T, Dw, Dp, E, out2.data_ptr(), None,
                                     status.data_ptr(), wk_w.data_ptr() + 4 * wk_at, nbytes, st), "fwd without the bytes")
    assert torch.equal(out2, out)
    # ---- backward
    g0_w, g0_at = guarded(P * Dp)
    g1_w, g1_at = guarded(P * Dp)
    gw = [guarded(w.numel()) for w in ws_]
    gb = [guarded(E) for _ in bs_]
    nbytes = L.recon_sent_conv_workspace_bytes(B, T, Dw, Dp, P, E, arr, n, seg, 1)
    ws_w, ws_at = guarded(nbytes // 4)
    ptrs = lambda pairs: (ctypes.c_void_p * n)(*[w.data_ptr() + 4 * a for w, a in pairs])
    outc, atc = out.contiguous(), at.contiguous()
    tail = (arr, n, pk.data_ptr(), act, B, T, Dw, Dp, E, outc.data_ptr(), atc.data_ptr(), g.data_ptr(), 0)
    _lib.check(L.recon_sent_conv_bwd(*head, *tail, g0_w.data_ptr() + 4 * g0_at, g1_w.data_ptr() + 4 * g1_at, ptrs(gw), ptrs(gb),
                                     ws_w.data_ptr() + 4 * ws_at, nbytes, st), "bwd")
    torch.cuda.synchronize()
    assert untouched(g0_w, g0_at, P * Dp) and untouched(g1_w, g1_at, P * Dp) and untouched(ws_w, ws_at, nbytes // 4)
    grads = [g0_w[g0_at:g0_at + P * Dp].view(P, Dp), g1_w[g1_at:g1_at + P * Dp].view(P, Dp)]
    for (w_, a_), t in zip(gw + gb, ws_ + bs_):
        assert untouched(w_, a_, t.numel())
        grads.append(w_[a_:a_ + t.numel()].view(t.shape))
    for got, ref in zip(grads, c["ref"][1:]):
        assert not torch.isnan(got).any() and rel_err(got, ref) <= 2e-5
    # one gradient alone: the same bits, the other buffers are not needed
    only = torch.empty(P, Dp, device=dev())
    none = (ctypes.c_void_p * n)()
    _lib.check(L.recon_sent_conv_bwd(*head, *tail, None, only.data_ptr(), None, None, ws_w.data_ptr() + 4 * ws_at, nbytes, st), "bwd g_pos_table_1")
    assert torch.equal(only, grads[1])
    only = torch.empty_like(ws_[0])
    one = (ctypes.c_void_p * n)()
    one[0] = only.data_ptr()
    _lib.check(L.recon_sent_conv_bwd(*head, *tail, None, None, one, none, ws_w.data_ptr() + 4 * ws_at, nbytes, st), "bwd g_weight_0")
    assert torch.equal(only, grads[2])


# ------------------------------------------------------------------------------------------------------------- bits
def test_forward_and_backward_are_bitwise_reproducible():
    from recon_amd import sentence_conv_pool
    for shape in (ODD, ODD_P, ("cnn", 130, 12, 5, 3, 8, (3,)), REF_WIDTHS):
        c = case(shape)
        same(run(sentence_conv_pool, c, dev()), run(sentence_conv_pool, c, dev()))


def test_second_backward_over_a_retained_graph_gives_the_same_bits(monkeypatch):
    from recon_amd import sentence_conv_pool
    for shape in (ODD, ODD_P):
        c = case(shape)
        d = lambda t: t.to(dev())
        leaves = [d(c["pos_table_0"]).requires_grad_(True), d(c["pos_table_1"]).requires_grad_(True)]
        ws_, bs_ = [d(w).requires_grad_(True) for w in c["weights"]], [d(b).requires_grad_(True) for b in c["biases"]]
        _, chain_calls = kernels_ran(monkeypatch)
        out = sentence_conv_pool(d(c["sentence"]), d(c["positions"]), d(c["word_table"]), *leaves, ws_, bs_,
                                 segments=None if c["segments"] is None else d(c["segments"]), keep=d(c["keep"]), pool_keep=d(c["pool_keep"]),
                                 activation="tanh" if shape[0] == "cnn" else "relu")
        kept = out.clone()
        first = torch.autograd.grad(out, leaves + ws_ + bs_, d(c["g_out"]), retain_graph=True)
        second = torch.autograd.grad(out, leaves + ws_ + bs_, d(c["g_out"]), retain_graph=True)
        same(first, second)
        assert torch.equal(kept, out) and not chain_calls               # the backward destroys nothing
        for a, r in zip(first, c["ref"][1:]):
            assert rel_err(a, r) <= 2e-5


def test_packed_keep_and_factors_give_the_same_bits(monkeypatch):
    from recon_amd import sentence_conv_pool
    kernel, chain_calls = kernels_ran(monkeypatch)
    for shape in (ODD, ODD_P, ("cnn", 2, 9, 97, 2, 8, (3, 7))):
        c = case(shape)
        same(run(sentence_conv_pool, c, dev(), keep="factors"), run(sentence_conv_pool, c, dev(), keep="packed"))
    assert len(kernel) == 6 and not chain_calls


def test_id_widths_give_the_same_bits():
    from recon_amd import sentence_conv_pool
    c = case(ODD)
    plain = run(sentence_conv_pool, c, dev())
    same(plain, run(sentence_conv_pool, c, dev(), positions_of=lambda p: p.long()))
    same(plain, run(sentence_conv_pool, c, dev(), positions_of=lambda p: p.int()))
    c32 = dict(c, sentence=c["sentence"].int())
    same(plain, run(sentence_conv_pool, c32, dev()))


def test_an_id_out_of_range_raises():
    from recon_amd import sentence_conv_pool
    c = inputs(ODD)
    d = lambda t: t.to(dev())
    args = lambda sent, pos: (d(sent), d(pos), d(c["word_table"]), d(c["pos_table_0"]), d(c["pos_table_1"]), [d(w) for w in c["weights"]],
                              [d(b) for b in c["biases"]])
    for at, value in ((0, 23), (1, -1), (2, 10 ** 9)):
        sent = c["sentence"].clone()
        sent[at, 3] = value
        with pytest.raises(ValueError, match="sentence_conv_pool"):
            sentence_conv_pool(*args(sent, c["positions"]))
    for value in (19, -1):
        pos = c["positions"].clone()
        pos[1, 1, 2] = value
        with pytest.raises(ValueError, match="sentence_conv_pool"):
            sentence_conv_pool(*args(c["sentence"], pos))
    assert sentence_conv_pool(*args(c["sentence"], c["positions"])).shape == (3, 60)        # the flag was reset


def test_no_grad_allocates_the_output_alone():
    from recon_amd import sentence_conv_pool
    form, B, T, Dw, Dp, E, ks = REF_WIDTHS
    c = case(REF_WIDTHS)
    d = lambda t: t.to(dev())
    p0 = d(c["pos_table_0"]).requires_grad_(True)
    ws_ = [d(w).requires_grad_(True) for w in c["weights"]]
    args = (d(c["sentence"]), d(c["positions"]), d(c["word_table"]), p0, d(c["pos_table_1"]), ws_, [d(b) for b in c["biases"]])
    out_bytes, at_bytes, packed_bytes = rounded(B * 3 * E * 4), rounded(B * 3 * E), rounded(sum(ks) * 60 * E * 4)
    gc.collect()

    def plain():
        with torch.no_grad():
            return sentence_conv_pool(*args, activation="tanh")
    peak, a = peak_bytes(plain)
    assert peak == out_bytes + packed_bytes, (peak, out_bytes, packed_bytes)       # the output, and the K-major weights (the forward's workspace) while the call runs
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    a2 = plain()
    assert torch.cuda.memory_allocated() - base == out_bytes            # what stays is the output alone
    peak, b = peak_bytes(lambda: sentence_conv_pool(*args, activation="tanh"))
    assert peak == out_bytes + at_bytes + packed_bytes, (peak, out_bytes, at_bytes, packed_bytes)   # nothing of size B T Cin or B E T exists
    assert a.grad_fn is None and b.grad_fn is not None and torch.equal(a, b.detach()) and torch.equal(a, a2)


def test_create_graph_other_dtypes_and_a_trained_word_table_run_the_chain(monkeypatch):
    from recon_amd import sentence_conv_pool
    kernel, chain_calls = kernels_ran(monkeypatch)
    c = case(ODD)
    d = lambda t: t.to(dev())
    p0, p1 = d(c["pos_table_0"]).requires_grad_(True), d(c["pos_table_1"]).requires_grad_(True)
    ws_, bs_ = [d(w).requires_grad_(True) for w in c["weights"]], [d(b).requires_grad_(True) for b in c["biases"]]
    out = sentence_conv_pool(d(c["sentence"]), d(c["positions"]), d(c["word_table"]), p0, p1, ws_, bs_, keep=d(c["keep"]),
                             pool_keep=d(c["pool_keep"]), activation="tanh")
    assert len(kernel) == 1 and not chain_calls
    grads = torch.autograd.grad(out, [p0, p1] + ws_ + bs_, d(c["g_out"]), create_graph=True)
    assert len(chain_calls) == 1
    for a, r in zip(grads, c["ref"][1:]):
        assert rel_err(a, r) <= 2e-5 and a.requires_grad
    grads[2].square().sum().backward()
    assert p0.grad is not None and torch.isfinite(p0.grad).all()
    got = run(sentence_conv_pool, c, dev(), dtype=torch.float64)
    assert len(kernel) == 1 and len(chain_calls) == 2 and rel_err(got[0], c["ref"][0]) <= 1e-12
    word = d(c["word_table"]).requires_grad_(True)
    out = sentence_conv_pool(d(c["sentence"]), d(c["positions"]), word, p0, p1, ws_, bs_)
    out.sum().backward()
    assert len(kernel) == 1 and len(chain_calls) == 3 and word.grad is not None
    del out, grads, got
    gc.collect()                                                        # (a create_graph graph is a reference cycle: its memory goes now, not inside a later test's measurement)


# ------------------------------------------------------------------------------------------------------------- the models
@pytest.mark.parametrize("name", ("cnn1", "pcnn1"))
def test_fixture_through_the_op(name, monkeypatch):
    def stock(m):
        convs = [c for c in m.modules() if isinstance(c, nn.Conv1d)]
        assert len(convs) == (3 if name == "cnn1" else 1)
        return convs + [m.word_embedding, m.pos_embedding_0, m.pos_embedding_1], "a stock Conv1d or Embedding forward ran"
    kernel, chain_calls = kernels_ran(monkeypatch)
    required = ["g.pos_embedding_0.weight", "g.pos_embedding_1.weight", "g.linear1.weight"] + (["g.cnn_3.", "g.cnn_5.", "g.cnn_7."] if name == "cnn1"
                                                                                              else ["g.cnn."])
    pinned(*baseline_fixture(name, dev()), monkeypatch, "fused_sentence_conv", kernel, stock, required)
    assert not chain_calls


def test_lstm_fixture_and_the_context_aware_encoder():
    import recon_amd
    from recon_amd.gpgnn import pair_states
    m, g, out_of, name = baseline_fixture("lstm_baseline1", dev())
    m.train()
    out = out_of(m)
    close(out, g["out"], atol=1e-4, what=name + " logits")
    (out * torch.from_numpy(g["G"]).to(dev())).sum().backward()
    seen = 0
    for k, v in m.named_parameters():
        if "g." + k in g:
            close(v.grad, g["g." + k], atol=1e-4, rel_to_max=1e-4, what=name + " grad " + k)
            seen += 1
    assert seen == 11                                                    # pos_embedding, eight of rnn1, two of linear2
    # ContextAware's encoder on the same ids at C = 1: the same kernels on the same values
    ca = recon_amd.ContextAware({"max_num_nodes": None, "dropout1": 0.0, "position_emb": 3, "units1": 4, "rnn1_layers": 1, "bidirectional": 1},
                                g["emb"], 9, 7, MAX_EDGES_PER_GRAPH=1).to(dev())
    ca.load_state_dict({k: v for k, v in m.state_dict().items() if k.startswith(("word_embedding", "pos_embedding", "rnn1"))}, strict=False)
    sent, mark = torch.from_numpy(g["sent"]).to(dev()), torch.from_numpy(g["mark"]).to(dev())
    with torch.no_grad():
        a = pair_states(m, sent, mark.unsqueeze(1))
        b = pair_states(ca, sent, mark.unsqueeze(1))
        assert torch.equal(a, b)
        assert torch.equal(m(sent, mark), m.linear2(a.reshape(3, -1)))


@pytest.mark.parametrize("name", ("cnn1", "pcnn1"))
def test_one_seed_gives_both_paths_the_same_factors(name, monkeypatch):
    """dropout1 = 0.5, train mode, packed_word_dropout off: the fused path hands the op torch's own draws in the stock lines' order and
    shapes, so one forward under one seed is the unfused forward to rounding — and differs from the forward under another seed."""
    kernel, chain_calls = kernels_ran(monkeypatch)
    m, g, out_of, _ = baseline_fixture(name, dev())
    m.dropout1.p = 0.5
    m.train()
    outs = {}
    for fused, seed in ((True, 3), (False, 3), (True, 4)):
        m.fused_sentence_conv = fused
        torch.manual_seed(seed)
        outs[fused, seed] = out_of(m).detach()
    assert len(kernel) == 2 and not chain_calls
    close(outs[True, 3], outs[False, 3], atol=1e-6, rel_to_max=1e-5, what=name + " one seed")
    assert not torch.equal(outs[True, 3], outs[True, 4])


class Recorded(nn.Module):
    """dropout1 with recorded factors: call i multiplies by factors[i].  Both paths call it in the stock lines' order and shapes."""

    def __init__(self, p, factors):
        super().__init__()
        self.p, self.factors, self.calls = p, factors, 0

    def forward(self, x):
        f = self.factors[self.calls]
        self.calls += 1
        return x * f


@pytest.mark.parametrize("form", ("cnn", "pcnn"))
def test_five_adam_steps_against_the_stock_lines(form, monkeypatch):
    """Five steps under recon_amd.optim.Adam with relation_objective, dropout1 = 0.5 in train mode with the same recorded factors for both
    models: the parameters agree within the band's cap.  eps = 1e-3: Adam's step is m / (sqrt(v) + eps).  At PCNN's cnn.weight[0, 0, 1] the
    op's fixed-order sum is exactly 0 while the stock convolution's backward leaves -9.3e-10, one rounding of a sum that cancels (measured
    on an MI355X, in some processes and not in others); under eps = 1e-8 that alone is a first step of 8.5e-5, 2.3e-4 of max |w|.  That
    is the optimiser's conditioning, not a difference of the gradients, which agree to 6e-8 at every step.  The other gradients here are
    1e-5 .. 1 against sqrt(v) of the same size, so eps = 1e-3 damps their steps alike in both models and every trainable parameter still
    moves (asserted)."""
    import recon_amd
    from recon_amd import relation_objective
    from recon_amd.optim import Adam
    from sentence_conv_checks import P_MODEL
    kernel, chain_calls = kernels_ran(monkeypatch)
    sent, pos, seg, labels = training_rows(dev(), form)
    emb = inputs((form, 12, 9, 5, 3, 4, (3,)))["word_table"].numpy()
    g = torch.Generator().manual_seed(12)
    draw = lambda *shape: ((torch.rand(*shape, generator=g) < 0.5).float() * 2).to(dev())
    factors = []
    for _ in range(5):                                                   # per step: the word factors, then the pooled ones as the lines draw them
        factors += [draw(12, 9, 5)] + ([draw(12, 4) for _ in range(3)] if form == "cnn" else [draw(12, 12)])

    def trained(fused):
        torch.manual_seed(11)
        m = (recon_amd.CNN if form == "cnn" else recon_amd.PCNN)(dict(P_MODEL, dropout1=0.5), emb, 9, 7).to(dev()).train()
        m.fused_sentence_conv = fused
        m.dropout1 = Recorded(0.5, factors)
        start = [p.detach().clone() for p in m.parameters()]
        opt = Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-3, eps=1e-3)
        for _ in range(5):
            opt.zero_grad()
            out = m(sent, pos) if form == "cnn" else m(sent, pos, seg)
            relation_objective(out, labels).loss.backward()
            opt.step()
        assert m.dropout1.calls == len(factors)
        return m, start
    (a, start), (b, _) = trained(True), trained(False)
    assert len(kernel) == 5 and not chain_calls
    for (k, p), q, s0 in zip(a.named_parameters(), b.parameters(), start):
        e = rel_err(p, q.detach().double().cpu())
        print("%s %s: fused against stock %.3e" % (form, k, e))
        assert e <= 2e-5, k
        assert p.requires_grad != torch.equal(p.detach(), s0), k       # every trainable parameter moved, the word table did not
    gc.collect()
