"""Shared by tests/test_sentence_conv_cpu.py, tests/test_sentence_conv_gpu.py and tools/sentence_conv_bench.py: the grid of cases, the
seeded inputs, the lines of models/baselines.py:237-247 / :297-308 restated as the oracle (float64) and as "the stock chain" (float32), an
fp32 restatement of the op's definition with named mistakes, the near-tie rule, the comparison and the fixtures' models.  Not a test module
and not a conftest.

A case is (form, B, T, Dw, Dp, E, windows), form "cnn" (pad 0, one pooled block per window) or "pcnn" (one odd window, pad k // 2, three
segment blocks).  Inputs, from a torch.Generator seeded by the case: V = 23 words, P = 2 T + 1 positions; ids >= 1 with a zero tail of
random length per row (none in row 0) and the last row all zeros when B >= 2; tables ~ U(-1, 1); weights ~ U(-a, a) with Xavier's
a = sqrt(6 / (Cin k + E k)); biases ~ U(-1, 1) / sqrt(Cin k); word factors and pooled factors in {0, 2} (p = 0.5); PCNN masks as
`get_pcnn_mask` gives them (semanticgraph/graph_utils.py:141-152): three contiguous runs of ones over the real tokens, zeros on the tail;
g_out ~ N(0, 1).  The default activation is the models': tanh for cnn, relu for pcnn.

Band: `op_checks.bound` of the stock fp32 chain's error on the same inputs on the device where the op ran, for out, both table gradients
and every weight and bias gradient.

The maximum is a discrete choice.  An output is flagged, and its g_out zeroed, when in float64 a position whose window differs from the
winner's (another gathered x window, or another segment factor; two zero-factor positions are the same 0) lies within 1e-5 of the
winner — which covers the 0 of a zero-factor position — or when relu's argument is within 1e-5 of 0 without being that exact 0.
Windows with identical ids over all taps tie exactly and take identical gradients: they do not count.  At most 1 % of a case's outputs
may be flagged."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from conftest import load_golden
from op_checks import band_failures, state_dict_of

from recon_amd.sentence_conv import MAX_T

V_WORDS = 23
MAX_TIE_SHARE = 0.01
MARGIN = 1e-5
CITES = "models/baselines.py:237-247"
ENTRIES = ("recon_sent_conv_supported", "recon_sent_conv_workspace_bytes", "recon_sent_conv_fwd", "recon_sent_conv_bwd")

REF_WIDTHS = ("cnn", 5, 36, 50, 3, 256, (3, 5, 7))       # the reference's widths at model_params.json's batch; 4 + 1 rows over two workgroups
REF_WIDTHS_P = ("pcnn", 5, 36, 50, 3, 256, (3,))
ODD = ("cnn", 3, 9, 5, 3, 20, (3, 5, 7))                 # Cin = 11, E = 20: nothing a multiple of 4 or 16
ODD_P = ("pcnn", 3, 9, 5, 3, 20, (3,))
LONGEST = ("cnn", 2, MAX_T, 6, 2, 17, (3,))
TOO_LONG = ("cnn", 2, MAX_T + 1, 6, 2, 17, (3,))         # must run `_chain` and still be right
TOO_LONG_P = ("pcnn", 2, MAX_T + 1, 6, 2, 17, (3,))
OVER = (TOO_LONG, TOO_LONG_P)
GRID = [
    ("cnn", 1, 3, 1, 1, 1, (3,)),                        # one output position
    ("cnn", 1, 7, 5, 3, 4, (3, 5, 7)),                   # k = T for the last window
    ODD, ODD_P,
    ("cnn", 2, 17, 6, 2, 17, (3,)),                      # one past a 16-position tile
    ("pcnn", 2, 17, 6, 2, 17, (3,)),
    REF_WIDTHS, REF_WIDTHS_P,
    ("cnn", 130, 12, 5, 3, 8, (3,)),                     # many rows: 12 per workgroup, 26 row groups of 5 in the backward
    ("pcnn", 130, 12, 5, 3, 8, (3,)),
    # one case on each side of every chunking of csrc/sent_conv.hip
    ("cnn", 2, 9, 5, 3, 64, (3,)), ("cnn", 2, 9, 5, 3, 65, (3,)),          # the forward's 64-channel tile (the backward's of 32: 2 | 3)
    ("cnn", 2, 9, 5, 3, 32, (3,)), ("cnn", 2, 9, 5, 3, 33, (3,)),          # the backward's 32-channel tile
    ("cnn", 2, 9, 96, 2, 8, (3, 7)), ("cnn", 2, 9, 97, 2, 8, (3, 7)),      # Cin = 100 | 101: one staged chunk | two; 512 cells per pass: k = 7 takes two
    ("pcnn", 2, 9, 97, 2, 8, (7,)),
    ("cnn", 32, 5, 3, 2, 4, (3,)), ("cnn", 33, 5, 3, 2, 4, (3,)),          # 32 weight-gradient groups of 1 | 17 of 2
    ("cnn", 257, 5, 3, 2, 4, (3,)),                                          # 129 position-table groups of 2 (256 of 1 below)
    ("cnn", 4, 36, 5, 3, 8, (3,)), ("pcnn", 4, 36, 5, 3, 8, (3,)),          # rows per workgroup: 4 x 36 = 144 positions | 3 x 38 (the 4th alone)
    LONGEST, ("pcnn", 2, MAX_T, 6, 2, 17, (9,)),                            # the largest T; with the widest window and its halo
    TOO_LONG, TOO_LONG_P,
    ("pcnn", 2, 1, 5, 3, 4, (3,)),                       # T = 1, k = 3: every tap but one in the halo
    ("pcnn", 3, 9, 5, 3, 20, (5,)),                      # the wider window
    ("cnn", 2, 12, 5, 3, 8, (2, 3, 4, 9)),               # four weights, even windows, the widest window
    # the position-table backward with the weight's position columns staged in LDS | read from L2 (k_sc_bwd_pos<true | false>):
    # 186 + 3 E + ceil(3 E / 4) + 18 E floats against 15360
    ("pcnn", 2, 9, 5, 3, 697, (3,)), ("pcnn", 2, 9, 5, 3, 698, (3,)),
    # the slab cap of the weight gradients, 2^24 floats over all groups: a slab of 505 800 floats allows 33 groups (32 taken: 40 rows in 20 groups of
    # 2), one of 863 232 allows 19 (14 groups of 3); the second is also E at its limit
    ("cnn", 40, 9, 50, 3, 600, (3, 5, 7)), ("cnn", 40, 9, 50, 3, 1024, (3, 5, 7)),
    # the weight-gradient pass's staged chunk at T = 128 with its halo: 8192 / 130 - 1 = 62 channels, Cin = 62 | 63 (one pass | two).  In the
    # PCNN form: under tanh a maximum over 126 positions of Cin = 63 against E = 8 saturates every output, and tanh' = 1 - out^2 then
    # cancels in fp32 in the stock chain as in the op (both 7e-4 from float64, measured), which no band of 2e-5 can hold
    ("pcnn", 2, MAX_T, 58, 2, 8, (3,)), ("pcnn", 2, MAX_T, 59, 2, 8, (3,)),
    ("pcnn", 2, MAX_T, 97, 2, 17, (9,)),                 # the forward at its LDS limit: one row, 9 tiles, 152 rows of 100 floats, two channel chunks
    ("cnn", 2, 9, 314, 3, 8, (3,)),                      # Cin at its limit of 320: four staged chunks
]
TIE_SHARE_CASES = [REF_WIDTHS, REF_WIDTHS_P, LONGEST, ("pcnn", 2, MAX_T, 6, 2, 17, (9,)), ODD, ODD_P, ("cnn", 1, 7, 5, 3, 4, (3, 5, 7)),
                   ("pcnn", 2, 1, 5, 3, 4, (3,))]
WRONG = ("max over T", "taps shifted", "tables swapped", "padding row trained", "segments as -inf", "bias after segments",
         "pool_keep not in the gradient")


def ids(case):
    return "%s-%s-%s" % (case[0], "x".join(map(str, case[1:6])), "_".join(map(str, case[6])))


def names(case):
    n = len(case[6])
    return ["out", "g_pos_table_0", "g_pos_table_1"] + ["g_weight_%d" % i for i in range(n)] + ["g_bias_%d" % i for i in range(n)]


def default_activation(case):
    return "tanh" if case[0] == "cnn" else "relu"


def inputs(case):
    form, B, T, Dw, Dp, E, windows = case
    g = torch.Generator().manual_seed(7919 * B + 131 * T + 17 * Dw + 29 * Dp + 31 * E + 37 * sum(windows) + (1 if form == "pcnn" else 0))
    P, Cin = 2 * T + 1, Dw + 2 * Dp
    real = torch.randint(1, T + 1, (B,), generator=g)                    # real tokens per row
    real[0] = T
    if B >= 2:
        real[B - 1] = 0
    live = torch.arange(T)[None, :] < real[:, None]
    sentence = torch.randint(1, V_WORDS, (B, T), generator=g) * live
    positions = (torch.randint(1, P, (B, 2, T), generator=g) * live[:, None, :]).to(torch.int8 if P <= 127 else torch.int64)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    c = dict(case=case, sentence=sentence, positions=positions, word_table=u(V_WORDS, Dw), pos_table_0=u(P, Dp), pos_table_1=u(P, Dp),
             weights=[u(E, Cin, k) * math.sqrt(6.0 / (Cin * k + E * k)) for k in windows],
             biases=[u(E) / math.sqrt(Cin * k) for k in windows])
    n_out = 3 if form == "pcnn" else len(windows)
    c["keep"] = (torch.rand(B, T, Dw, generator=g) < 0.5).float() * 2
    c["pool_keep"] = (torch.rand(B, n_out * E, generator=g) < 0.5).float() * 2
    c["segments"] = None
    if form == "pcnn":
        seg = torch.zeros(B, 3, T)
        for b in range(B):
            n = int(real[b])
            if n:
                lo, hi = sorted(torch.randint(0, n, (2,), generator=g).tolist())
                seg[b, 0, :lo] = 1                                       # (get_pcnn_mask: i < left[-1]; left[0] <= i < right[-1]; i > right[0])
                seg[b, 1, lo:hi + 1] = 1
                seg[b, 2, hi + 1:n] = 1
        c["segments"] = seg
    c["g_out"] = torch.randn(B, n_out * E, generator=g)
    return c


def lines(sentence, positions, word_table, pos_table_0, pos_table_1, weights, biases, segments=None, keep=None, pool_keep=None,
          activation="none", pos_padding_idx=0):
    """models/baselines.py:237-247 (segments None) and :297-308, with the two dropout1 products as explicit factors."""
    word_embeddings = F.embedding(sentence.long(), word_table)
    if keep is not None:
        word_embeddings = word_embeddings * keep
    pos_embeddings_0 = F.embedding(positions[:, 0, :].long(), pos_table_0, padding_idx=pos_padding_idx)
    pos_embeddings_1 = F.embedding(positions[:, 1, :].long(), pos_table_1, padding_idx=pos_padding_idx)
    merged_embeddings = torch.cat([word_embeddings, pos_embeddings_0, pos_embeddings_1], dim=2)
    merged_embeddings = merged_embeddings.transpose(1, 2)
    act = {"none": lambda v: v, "tanh": torch.tanh, "relu": F.relu}[activation]
    drop = (lambda v, at: v) if pool_keep is None else (lambda v, at: v * pool_keep[:, at:at + v.shape[1]])
    if segments is None:
        E = weights[0].shape[0]
        outs = [act(drop(torch.max(F.conv1d(merged_embeddings, w, b), dim=2)[0], i * E)) for i, (w, b) in enumerate(zip(weights, biases))]
        return torch.cat(outs, dim=1)
    E, k = weights[0].shape[0], weights[0].shape[2]
    cnn_output = F.conv1d(merged_embeddings, weights[0], biases[0], padding=int(k / 2))
    left = torch.max(cnn_output * segments[:, 0].unsqueeze(1).repeat(1, E, 1), dim=2)[0]
    middle = torch.max(cnn_output * segments[:, 1].unsqueeze(1).repeat(1, E, 1), dim=2)[0]
    right = torch.max(cnn_output * segments[:, 2].unsqueeze(1).repeat(1, E, 1), dim=2)[0]
    return act(drop(torch.cat([left, middle, right], dim=1), 0))


def run(fn, c, device="cpu", dtype=torch.float32, activation=None, keep="factors", pool_keep=True, g_out=None, positions_of=None):
    """[out, g_pos_table_0, g_pos_table_1, g_weight..., g_bias...] of fn(...) on `device` in `dtype` with the case's g_out.  keep:
    "factors", "packed" (a PackedKeep of the same factors) or None."""
    from recon_amd.char_features import pack_keep
    f = lambda t: t.to(device=device, dtype=dtype, copy=True)            # (copies: the case's own tensors stay leaves without a grad)
    p0, p1 = f(c["pos_table_0"]).requires_grad_(True), f(c["pos_table_1"]).requires_grad_(True)
    ws, bs = [f(w).requires_grad_(True) for w in c["weights"]], [f(b).requires_grad_(True) for b in c["biases"]]
    kp = None if keep is None else (f(c["keep"]) if keep == "factors" else pack_keep(c["keep"].to(device), 2.0))
    positions = c["positions"].to(device)
    out = fn(c["sentence"].to(device), positions if positions_of is None else positions_of(positions), f(c["word_table"]), p0, p1, ws, bs,
             segments=None if c["segments"] is None else f(c["segments"]), keep=kp, pool_keep=f(c["pool_keep"]) if pool_keep else None,
             activation=activation or default_activation(c["case"]), pos_padding_idx=0)
    out.backward(f(c["g_out"] if g_out is None else g_out))
    return [out.detach(), p0.grad, p1.grad] + [w.grad for w in ws] + [b.grad for b in bs]


# ------------------------------------------------------------------------------------------------------------- the definition, restated
def windows_of(x, k, pad, tail=0, shift=0):
    """x [B, T, Cin] -> [B, T_out + tail, Cin k]: row t holds x[t + j - pad + shift] for the k taps, in a weight's own (c, j) order."""
    xp = F.pad(x, (0, 0, pad, pad + tail + shift))
    return xp.unfold(1, k, 1)[:, shift:].reshape(x.shape[0], -1, x.shape[2] * k)


def pooled_values(c, dtype=torch.float64, wrong=None, leaves=None):
    """[(v [B, n_out E, T_out], same [B, T_out, T_out] or None)] per window: the values the maximum runs over, and which positions hold
    the same window as which.  leaves: (pos_table_0, pos_table_1, weights, biases) to differentiate through."""
    form, B, T, Dw, Dp, E, ks = c["case"]
    f = lambda t: t.to(dtype)
    p0, p1, ws, bs = leaves if leaves is not None else (f(c["pos_table_0"]), f(c["pos_table_1"]), [f(w) for w in c["weights"]],
                                                          [f(b) for b in c["biases"]])
    if wrong == "tables swapped":
        p0, p1 = p1, p0
    pad_idx = None if wrong == "padding row trained" else 0
    pos = c["positions"].long()
    x = torch.cat([F.embedding(c["sentence"], f(c["word_table"])) * f(c["keep"]) if c["use_keep"] else F.embedding(c["sentence"], f(c["word_table"])),
                   F.embedding(pos[:, 0], p0, padding_idx=pad_idx), F.embedding(pos[:, 1], p1, padding_idx=pad_idx)], dim=2)
    res = []
    for w, b, k in zip(ws, bs, ks):
        pad = k // 2 if form == "pcnn" else 0
        X = windows_of(x, k, pad, tail=k - 1 if (wrong == "max over T" and form == "cnn") else 0, shift=1 if wrong == "taps shifted" else 0)
        conv = X @ w.reshape(E, -1).t()                                  # [B, T_out, E]
        if form == "cnn":
            res.append(((conv + b).transpose(1, 2), X))
            continue
        seg = f(c["segments"])                                           # [B, 3, T]
        if wrong == "bias after segments":
            v = conv.transpose(1, 2).unsqueeze(1) * seg.unsqueeze(2) + b[None, None, :, None]
        else:
            v = (conv + b).transpose(1, 2).unsqueeze(1) * seg.unsqueeze(2)   # [B, 3, E, T]
            if wrong == "segments as -inf":
                v = (conv + b).transpose(1, 2).unsqueeze(1).expand(B, 3, E, T).masked_fill((seg == 0).unsqueeze(2), float("-inf"))
                v = torch.where(torch.isinf(v).all(dim=3, keepdim=True), torch.zeros_like(v), v)
        res.append((v.reshape(B, 3 * E, -1), X))
    return res


def first_argmax(v):
    """The lowest position of the maximum over the last dimension."""
    top = v.max(dim=-1, keepdim=True).values
    T = v.shape[-1]
    return torch.where(v == top, torch.arange(T), torch.full((), T)).min(dim=-1).values


def restated(c, wrong=None, activation=None, last_tie=False):
    """The op's definition in fp32 torch on the CPU — unfold, one product per window, bias, segment product, the lowest maximal position,
    pool_keep, the activation — wrong in one named way on request; and the positions it picked."""
    dtype = torch.float32
    f = lambda t: t.to(dtype).clone().requires_grad_(True)
    p0, p1, ws, bs = f(c["pos_table_0"]), f(c["pos_table_1"]), [f(w) for w in c["weights"]], [f(b) for b in c["biases"]]
    act = activation or default_activation(c["case"])
    blocks, picked = [], []
    for v, _ in pooled_values(c, dtype, wrong, (p0, p1, ws, bs)):
        at = first_argmax(v)
        if last_tie:
            at = v.shape[-1] - 1 - first_argmax(v.flip(-1))
        blocks.append(v.gather(2, at.unsqueeze(-1)).squeeze(-1))
        picked.append(at)
    pooled = torch.cat(blocks, dim=1)
    if c["use_pool_keep"]:
        pk = c["pool_keep"].to(dtype)
        pooled = (pooled * pk).detach() + pooled - pooled.detach() if wrong == "pool_keep not in the gradient" else pooled * pk
    out = {"none": lambda t: t, "tanh": torch.tanh, "relu": F.relu}[act](pooled)
    out.backward(c["g_out"].to(dtype))
    return [out.detach(), p0.grad, p1.grad] + [w.grad for w in ws] + [b.grad for b in bs], torch.cat(picked, dim=1)


def near_ties(c, activation):
    """(bool [B, n_out E] of the flagged outputs, the float64 positions [B, n_out E])."""
    flags, picked = [], []
    for i, (v, X) in enumerate(pooled_values(c)):
        B, N, T_out = v.shape
        at = first_argmax(v)
        best = v.gather(2, at.unsqueeze(-1))
        same_x = (X.unsqueeze(2) == X.unsqueeze(1)).all(dim=3)           # [B, T_out, T_out]
        same = same_x[torch.arange(B)[:, None], at]                      # [B, N, T_out]: position t holds the winner's window
        if c["segments"] is not None:
            E = N // 3
            seg = c["segments"].double().repeat_interleave(E, dim=1)     # [B, 3 E, T]
            seg_at = seg.gather(2, at.unsqueeze(-1))
            same = (same & (seg == seg_at)) | ((seg == 0) & (seg_at == 0))
        flag = ((best - v < MARGIN) & ~same).any(dim=2)
        if activation == "relu":
            pk = c["pool_keep"].double()[:, i * N:(i + 1) * N] if c["use_pool_keep"] else torch.ones_like(best.squeeze(-1))
            exact = (seg_at == 0).squeeze(-1) if c["segments"] is not None else torch.zeros_like(flag)     # the 0 of a zero-factor position
            flag |= ((best.squeeze(-1) * pk).abs() < MARGIN) & (pk != 0) & ~exact
        flags.append(flag)
        picked.append(at)
    return torch.cat(flags, dim=1), torch.cat(picked, dim=1)


_CASES = {}


def case(shape, activation=None, keep=True, pool_keep=True):
    """Inputs, the tie-masked g_out and the float64 oracle of a case, computed once and left unchanged."""
    key = (shape, activation, keep, pool_keep)
    if key not in _CASES:
        c = inputs(shape)
        c["use_keep"], c["use_pool_keep"] = keep, pool_keep
        act = activation or default_activation(shape)
        c["ties"], c["at"] = near_ties(c, act)
        c["g_out"] = c["g_out"].masked_fill(c["ties"], 0.0)
        c["ref"] = run(lines, c, dtype=torch.float64, activation=act, keep="factors" if keep else None, pool_keep=pool_keep)
        _CASES[key] = c
    return _CASES[key]


def failures(case_, got, chain, ref, label=""):
    return band_failures(names(case_), got, chain, ref, "sentence_conv %s %s" % (ids(case_), label))


# ------------------------------------------------------------------------------------------------------------- the models
P_MODEL = {"dropout1": 0.0, "position_emb": 3, "units1": 4, "rnn1": "LSTM", "rnn1_layers": 1, "bidirectional": True, "window_size": 3}
KEYS = {"cnn1": 10, "pcnn1": 6, "lstm_baseline1": 13}


def baseline_fixture(name, device="cpu", dtype=torch.float32):
    """(model, fixture, model -> logits, name) of a fixture written from the reference's CNN, PCNN or LSTM
    (tests/golden/gen_golden_baselines.py)."""
    import recon_amd
    g = load_golden(name)
    cls = {"cnn1": recon_amd.CNN, "pcnn1": recon_amd.PCNN, "lstm_baseline1": recon_amd.LSTM}[name]
    m = cls(dict(P_MODEL), g["emb"], 9, 7)
    sd = state_dict_of(g)
    assert sorted(m.state_dict()) == sorted(sd) and len(sd) == KEYS[name]
    m.load_state_dict(sd, strict=True)
    m.to(device=device, dtype=dtype)
    t = lambda k: torch.from_numpy(g[k]).to(device)
    if name == "pcnn1":
        return m, g, lambda m: m(t("sent"), t("mark"), t("mask").to(dtype)), name
    return m, g, lambda m: m(t("sent"), t("mark")), name


def training_rows(device, form, B=12, T=9, seed=5):
    """Rows of the per-pair preprocessing for five optimiser steps: (sentence, positions, mask or None, labels)."""
    g = torch.Generator().manual_seed(seed)
    c = inputs((form, B, T, 5, 3, 4, (3,)))
    labels = torch.randint(0, 7, (B,), generator=g)
    seg = None if c["segments"] is None else c["segments"].to(device)
    return c["sentence"].to(device), c["positions"].long().clamp(max=2 * T).to(device), seg, labels.to(device)
