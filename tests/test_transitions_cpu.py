"""recon_amd.pair_transitions without a GPU: the import, the stock lines on CPU tensors (bit for bit), every argument error, the shape
queries of the C ABI, `GPGNN.transitions` in both projection styles, and the guard of the band tests/test_transitions_gpu.py holds the
kernels to.

The input generator, the g_out construction, the fp64 reference and the comparison live here and are imported by the GPU file.  Inputs:
x ~ N(0, 1), weights and biases uniform in +-1 / sqrt(K), from a seeded torch.Generator.  Band: `op_checks.bound` of the stock fp32 chain's
error on the same inputs, applied by `op_checks.band_failures`.  Relu's kink: a pre-activation within rounding of zero flips act' between fp32 and fp64 and moves a weight
gradient by far more than the band (for the stock chain too), so g_out is zero wherever the fp64 pre-activation has magnitude below
2^-12 max |pre| — a mask from fp64 alone (the fp32 pre-activation's error is about 6e-7 of the maximum: a margin of 400).

Guard: an fp32 CPU restatement of the algebra passes the band at every shape and activation (e_chain is then its own error), and four
wrong restatements fail it wherever they apply: no bias; act' omitted; two layers swapped in d_x; the last row group left out of d_b."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from op_checks import band_failures

G_WGRAD = 8                                     # the weight-gradient pass's row groups (transitions.WGRAD_MAX_ROW_GROUPS, asserted below)
GROUP_ROWS = 32                                 # a group holds at least this many rows: G = min(G_WGRAD, ceil(M / 32))
LONG_THIN = (2 * 16 * G_WGRAD + 5, 8, 16, 2)    # 261 rows: every row group holds 33 rows, more than two tiles of 16 and a tail
REF_ONE = (72, 512, 256, 3)                     # one sentence at the reference's widths
REF_BATCH = (3600, 512, 256, 3)                 # the reference's batch
#         M   K   N1  L
SHAPES = [(1, 4, 1, 1), (17, 20, 24, 3), REF_ONE, (531, 36, 100, 2), LONG_THIN, REF_BATCH]
ACTS = ("relu", "tanh", "linear")
SEEDS = {(1, 4, 1, 1): 2}                       # the one output of the smallest shape is positive: relu leaves something to check (asserted below)
KINK = 2.0 ** -12


def names(L):
    return ["T%d" % l for l in range(L)] + ["d_x"] + ["d_W%d" % l for l in range(L)] + ["d_b%d" % l for l in range(L)]


def inputs(M, K, N1, L, seed=0):
    """x, L weights, L biases and L raw output gradients (before the kink mask), fp32 on the CPU."""
    g = torch.Generator().manual_seed(1000 * seed + M + 3 * K + 5 * N1 + 7 * L)
    s = 1.0 / math.sqrt(K)
    x = torch.randn(M, K, generator=g)
    Ws = [(torch.rand(N1, K, generator=g) * 2 - 1) * s for _ in range(L)]
    bs = [(torch.rand(N1, generator=g) * 2 - 1) * s for _ in range(L)]
    raw = [torch.randn(M, N1, generator=g) for _ in range(L)]
    return x, Ws, bs, raw


def act64(pre, act):
    return pre if act == "linear" else getattr(torch, act)(pre)


_CASES = {}


def case(shape, act):
    """Inputs, the masked g_out and the fp64 oracle [T_l..., d_x, d_W_l..., d_b_l...] of a shape and activation, computed once and left
    unchanged; `share` is the zeroed share of g_out."""
    if (shape, act) not in _CASES:
        x, Ws, bs, raw = inputs(*shape, seed=SEEDS.get(shape, 0))
        x64 = x.double().requires_grad_(True)
        W64 = [W.double().requires_grad_(True) for W in Ws]
        b64 = [b.double().requires_grad_(True) for b in bs]
        pre = [x64 @ W.t() + b for W, b in zip(W64, b64)]
        top = max(p.detach().abs().max().item() for p in pre)
        keep = [(p.detach().abs() >= KINK * top) for p in pre]                       # from fp64 alone
        g_out = [r * k.float() for r, k in zip(raw, keep)]
        T = [act64(p, act) for p in pre]
        torch.autograd.backward(T, [g.double() for g in g_out])
        ref = [t.detach() for t in T] + [x64.grad] + [W.grad for W in W64] + [b.grad for b in b64]
        share = 1.0 - sum(k.sum().item() for k in keep) / sum(k.numel() for k in keep)
        _CASES[(shape, act)] = dict(x=x, Ws=Ws, bs=bs, g_out=g_out, ref=ref, share=share)
    return _CASES[(shape, act)]


def run(fn, c, act, device="cpu", x_of=None):
    """[T_l..., d_x, d_W_l..., d_b_l...] of fn(x, Ws, bs, act) on `device`, with the case's g_out."""
    x = c["x"].to(device)
    x = (x if x_of is None else x_of(x)).requires_grad_(True)
    Ws = [W.to(device).requires_grad_(True) for W in c["Ws"]]
    bs = [b.to(device).requires_grad_(True) for b in c["bs"]]
    Ts = fn(x, Ws, bs, act)
    torch.autograd.backward(list(Ts), [g.to(device) for g in c["g_out"]])
    return [t.detach() for t in Ts] + [x.grad] + [W.grad for W in Ws] + [b.grad for b in bs]


def failures(got, chain, ref, label=""):
    return band_failures(names((len(ref) - 1) // 3), got, chain, ref, "transitions " + label)


def groups_of(M):
    G = max(1, min(G_WGRAD, -(-M // GROUP_ROWS)))
    per = -(-M // G)
    return -(-M // per), per


# ------------------------------------------------------------------------------------------------------------- the op on the CPU
def test_import():
    from recon_amd import pair_transitions
    from recon_amd.transitions import pair_transitions as same
    assert pair_transitions is same


@pytest.mark.parametrize("act", ACTS + ("sigmoid",))
def test_cpu_tensors_run_the_stock_lines_bitwise(act):
    from recon_amd import pair_transitions
    c = case((17, 20, 24, 3), "relu")

    def inline(x, Ws, bs, name):
        out = []
        for W, b in zip(Ws, bs):
            T = F.linear(x, W, b)
            if name != "linear":
                T = getattr(F, name)(T)
            out.append(T)
        return out
    a, b = run(pair_transitions, c, act), run(inline, c, act)
    assert len(a) == len(b) == 10
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    x3 = c["x"][:16].reshape(2, 8, 20)
    Ts = pair_transitions(x3, c["Ws"], [None, c["bs"][1], None], act)
    assert isinstance(Ts, tuple) and len(Ts) == 3 and all(t.shape == (2, 8, 24) for t in Ts)
    assert torch.equal(Ts[0], inline(x3, c["Ws"][:1], [None], act)[0])


def test_argument_errors():
    from recon_amd import pair_transitions
    x, Ws, bs, _ = inputs(5, 8, 6, 2)
    bad = [lambda: pair_transitions(x, Ws, bs, "no_such_function"),
           lambda: pair_transitions(x, Ws, bs, None),
           lambda: pair_transitions(x.numpy(), Ws, bs, "relu"),
           lambda: pair_transitions(x.long(), Ws, bs, "relu"),
           lambda: pair_transitions(torch.tensor(1.0), Ws, bs, "relu"),
           lambda: pair_transitions(x, [], [], "relu"),
           lambda: pair_transitions(x, Ws, bs[:1], "relu"),
           lambda: pair_transitions(x, [Ws[0], Ws[1][:5]], bs, "relu"),               # not one shape
           lambda: pair_transitions(x, [W[:, :4] for W in Ws], bs, "relu"),           # K mismatch
           lambda: pair_transitions(x, [W[0] for W in Ws], bs, "relu"),               # not [N1, K]
           lambda: pair_transitions(x, [W.double() for W in Ws], bs, "relu"),
           lambda: pair_transitions(x, Ws, [bs[0], bs[1][:5]], "relu"),
           lambda: pair_transitions(x, Ws, [bs[0], bs[1].double()], "relu"),
           lambda: pair_transitions(x, Ws, [bs[0], 3.0], "relu")]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError, match="pair_transitions"):
            f()
            pytest.fail("case %d raised nothing" % i)
    with pytest.raises(ValueError, match=r"\(6, 8\).*\(5, 8\)|\[\(6, 8\), \(5, 8\)\]"):       # the shapes are in the text
        pair_transitions(x, [Ws[0], Ws[1][:5]], bs, "relu")


def test_shape_queries_and_row_split_are_the_librarys():
    from recon_amd import _lib, transitions
    L = _lib.lib()
    assert transitions.WGRAD_MAX_ROW_GROUPS == G_WGRAD
    ok = L.recon_pair_transitions_supported
    assert all(ok(*s) for s in SHAPES)
    assert ok(1, 4, 1, 1) and ok(2 ** 24, 1024, 1024, 8) and ok(0, 512, 256, 3) and ok(7, 1000, 1023, 5)
    assert not ok(2 ** 24 + 1, 512, 256, 3) and not ok(5, 6, 8, 1) and not ok(5, 1028, 8, 1) and not ok(5, 0, 8, 1)
    assert not ok(5, 8, 0, 1) and not ok(5, 8, 1025, 1) and not ok(5, 8, 8, 0) and not ok(5, 8, 8, 9) and not ok(-1, 8, 8, 1)
    ws = L.recon_pair_transitions_workspace_bytes
    K, N1, Ly = 8, 16, 2
    slab = Ly * N1 * (K + 1) * 4
    assert slab % 16 == 0
    for M in (1, 31, 32, 33, 64, 65, 255, 256, 257, LONG_THIN[0], 3600, 2 ** 24):
        G, per = groups_of(M)
        assert ws(M, K, N1, Ly, 1) == G * slab, (M, G)
        assert ws(M, K, N1, Ly, 0) == 0
    assert groups_of(LONG_THIN[0]) == (G_WGRAD, 33) and groups_of(3600) == (8, 450) and groups_of(17) == (1, 17) and groups_of(72) == (3, 24)
    assert ws(0, K, N1, Ly, 1) == 0 and ws(5, 6, N1, Ly, 1) == 0
    assert ws(3, 4, 1, 1, 1) % 16 == 0 and ws(3, 4, 1, 1, 1) >= 5 * 4


# ------------------------------------------------------------------------------------------------------------- the model's method
def _gpgnn(style, L, fused):
    from recon_amd.gpgnn import GPGNN
    torch.manual_seed(5)
    p = {"max_num_nodes": 3, "embedding_dim": 2, "layer_number": L, "projection_style": style, "non-linear1": "relu", "non-linear": "tanh",
         "dropout1": 0.5, "position_emb": 3, "units1": 4, "rnn1_layers": 1, "bidirectional": 1, "batch_size": 2}
    m = GPGNN(p, np.random.RandomState(0).randn(9, 5).astype("float32"), max_sent_len=4, n_out=3)
    m.fused_transitions = fused
    return m


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("style,L", [("untie", 2), ("tie", 2), ("untie", 1)])
def test_gpgnn_transitions_gives_todays_tensors_on_the_cpu(style, L, fused):
    m = _gpgnn(style, L, fused)
    assert isinstance(type(m).fused_transitions, bool)
    x = torch.randn(2, 6, 8, generator=torch.Generator().manual_seed(2))
    p = m.p
    if m.tied:                                                          # the lines GPGNN.forward held before the method existed
        T = m.representation_to_adj(x)
        if p['non-linear'] != "linear":
            T = getattr(F, p['non-linear'])(T)
        want = [T] * L
    else:
        want = []
        for i in range(L):
            T = m.representation_to_adj[i](x)
            if p['non-linear1'] != "linear":
                T = getattr(F, p['non-linear1'])(T)
            want.append(T)
    got = m.transitions(x)
    assert isinstance(got, list) and len(got) == L
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    if m.tied:
        assert all(t is got[0] for t in got)
    # a replaced projection module still works: the method then makes the calls it made before
    class Twice(nn.Module):
        def __init__(self, lin):
            super().__init__()
            self.lin = lin

        def forward(self, v):
            return 2 * self.lin(v)
    if m.tied:
        m.representation_to_adj = Twice(m.representation_to_adj)
    else:
        m.representation_to_adj[0] = Twice(m.representation_to_adj[0])
    again = m.transitions(x)
    assert torch.equal(again[0], getattr(F, p['non-linear'] if m.tied else p['non-linear1'])(2 * (m.representation_to_adj if m.tied
                                                                                                  else m.representation_to_adj[0]).lin(x)))


# ------------------------------------------------------------------------------------------------------------- the band's guard
WRONG = ("no bias", "act' omitted", "layers swapped in d_x", "last row group left out of d_b")


def restated(c, act, wrong=None):
    """The op's algebra in fp32 torch on the CPU (torch's own summation order inside a product; d_b by row groups as the kernels cut them)."""
    x, Ws, bs, gs = c["x"], c["Ws"], c["bs"], c["g_out"]
    L, M = len(Ws), x.shape[0]
    Ts, dpre = [], []
    for W, b, g in zip(Ws, bs, gs):
        pre = x @ W.t() if wrong == "no bias" else x @ W.t() + b
        T = act64(pre, act)
        d = {"relu": (T > 0).float(), "tanh": 1 - T * T, "linear": torch.ones_like(T)}[act]
        Ts.append(T)
        dpre.append(g if wrong == "act' omitted" else g * d)
    order = list(range(L))
    if wrong == "layers swapped in d_x":
        order[0], order[-1] = order[-1], order[0]
    d_x = torch.zeros_like(x)
    for l in range(L):
        d_x = d_x + dpre[l] @ Ws[order[l]]
    G, per = groups_of(M)
    cut = G - 1 if wrong == "last row group left out of d_b" else G
    d_W = [d.t() @ x for d in dpre]
    d_b = []
    for d in dpre:
        s = torch.zeros(d.shape[1])
        for g in range(cut):
            s = s + d[g * per:(g + 1) * per].sum(0)
        d_b.append(s)
    return Ts + [d_x] + d_W + d_b


def applies(wrong, shape, act):
    M, K, N1, L = shape
    # (relu' differs from 1 only at a non-positive output: the smallest shape's one output is positive)
    return {"act' omitted": act == "tanh" or (act == "relu" and M * N1 * L > 1), "layers swapped in d_x": L >= 2, "last row group left out of d_b": groups_of(M)[0] >= 2}.get(wrong, True)


def test_g_out_mask_conditions():
    for shape in SHAPES:
        for act in ACTS:
            c = case(shape, act)
            assert c["share"] <= 0.01, (shape, c["share"])
            if shape[0] * shape[2] * shape[3] < 100:
                assert c["share"] == 0.0, (shape, c["share"])
    assert case(SHAPES[0], "relu")["share"] == 0.0 and case(SHAPES[0], "relu")["ref"][0].item() > 0.1
    for shape in SHAPES[1:]:                                            # relu is neither dead nor the identity anywhere else
        assert 0.2 < (case(shape, "relu")["ref"][0] > 0).double().mean().item() < 0.8


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_restatement_passes_the_band_and_wrong_ones_fail(shape, act):
    c = case(shape, act)
    good = restated(c, act)
    assert not failures(good, good, c["ref"], "%s %s stand-in" % (shape, act))
    for wrong in WRONG:
        if applies(wrong, shape, act):
            assert failures(restated(c, act, wrong), good, c["ref"], "%s %s %s" % (shape, act, wrong)), "%s stays inside the band at %s %s" % (wrong, shape, act)


def test_every_wrong_restatement_applies_somewhere():
    for wrong in WRONG:
        assert sum(applies(wrong, s, a) for s in SHAPES for a in ACTS) >= 6, wrong
