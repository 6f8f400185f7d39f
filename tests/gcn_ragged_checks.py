"""The float32 GraphConvolution over a ragged batch (recon_amd/gcn_layers.py _GcnRaggedFunction, csrc/gcn_ragged.hip): inputs, shapes,
the float64 reference (models/layers.py:57-63 per graph, differentiated by hand under a given ReLU mask), a float32 restatement in the
kernels' order with its eight wrong variants, and the checks both test files apply.  Not a test module: tests/test_gcn_ragged_cpu.py
and tests/test_gcn_ragged_gpu.py import from it.

The band is tests/op_checks.py's: relative to max |fp64|, an output may be off by bound(e_chain) = min(max(4 e_chain, 2^-20), 2e-5),
e_chain being the error of the stock float32 torch ops on the same inputs and device.  Gradients are compared under the op's OWN ReLU
mask; the mask itself is checked wherever the float64 pre-activation is further than the forward's bound from zero (and where it is
exactly zero: an all-zero adjacency row without a bias), and the cells in between — not asked about — may be 0.1 % of a case's cells."""
import functools

import numpy as np
import torch

import op_checks

# sizes / in / out: the smallest shapes at which the kernels can go wrong — one node, one feature; one graph either side of the
# 32-row tile; odd sizes with a 65- and a 100-node graph and 136 = 2 x 64 + 8 columns; 63 / 64 / 65 columns; 70 graphs; a first graph
# longer than the four chunks requested at once (129); the largest graphs of BASELINE.json configs[4] (256, two groups of chunks)
SHAPES = (
    ((1,), 7, 5),
    ((1, 1, 1), 1, 1),
    ((31, 32, 33), 24, 16),
    ((5, 32, 17, 65, 100, 1, 33), 40, 136),
    ((64, 65), 33, 63),
    ((16, 15), 12, 65),
    ((3,) * 70, 24, 16),
    ((129, 64), 33, 64),
    ((256, 255, 200), 48, 72),
)
ZERO_ROW = ((5, 32, 17, 65, 100, 1, 33), 2, 3)      # (sizes, graph, row): an all-zero adjacency row, so that its output is relu(bias)
NAMES = ("out", "g_x", "g_adj", "g_weight", "g_bias")
MARGIN_CAP = 1e-3                                   # cells the mask check does not ask about: at most 0.1 % of a case's cells


def shape_id(s):
    sizes, I, O = s
    return "%s_%dx%d" % ("-".join(map(str, sizes)) if len(sizes) <= 7 else "%dx%d" % (sizes[0], len(sizes)), I, O)


class Case:
    """CPU float32 inputs of one call: x [N, in], mats (one [n_b, n_b] per graph), w [in, out], b [out] or None, G [N, out] (grad_out)."""

    def __init__(self, sizes, I, O, bias):
        self.sizes, self.I, self.O = tuple(sizes), I, O
        self.N = sum(sizes)
        g = torch.Generator().manual_seed(1000 * self.N + 10 * I + O)
        self.x = torch.randn(self.N, I, generator=g)
        self.mats = []
        for bi, n in enumerate(sizes):
            a = (torch.rand(n, n, generator=g) < max(0.05, 4.0 / n)).float() + torch.eye(n)
            a = a / a.sum(-1, keepdim=True)                              # row-normalised, random at density max(0.05, 4 / n) + identity
            if (self.sizes, bi) == ZERO_ROW[:2]:
                a[ZERO_ROW[2]] = 0.0
            self.mats.append(a)
        stdv = 1.0 / O ** 0.5                                            # the layer's own init
        self.w = (torch.rand(I, O, generator=g) * 2 - 1) * stdv
        self.b = (torch.rand(O, generator=g) * 2 - 1) * stdv if bias else None
        self.G = torch.randn(self.N, O, generator=g)
        self.node_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.adj_ptr = np.concatenate([[0], np.cumsum([n * n for n in sizes])]).astype(np.int64)

    def values(self):
        return torch.cat([m.reshape(-1) for m in self.mats])


@functools.lru_cache(maxsize=None)
def case(sizes, I, O, bias):
    return Case(sizes, I, O, bias)


# ------------------------------------------------------------------------------------------------- the layer in stock torch ops
def forward(c, dtype, device):
    """(pre, out, support) of models/layers.py:57-63 per graph, in `dtype` on `device`, through torch's own ops."""
    x, w = c.x.to(device=device, dtype=dtype), c.w.to(device=device, dtype=dtype)
    sup = x @ w
    pre = torch.cat([m.to(device=device, dtype=dtype) @ sup[r0:r0 + n] for m, n, r0 in zip(c.mats, c.sizes, c.node_ptr[:-1])]) if c.N else sup
    if c.b is not None:
        pre = pre + c.b.to(device=device, dtype=dtype)
    return pre, torch.relu(pre), sup


def grads(c, mask, sup, dtype, device, want):
    """(g_x, g_adj, g_weight, g_bias) of sum(out * G), the ReLU's derivative GIVEN as `mask`; None where `want` says so or there is no bias."""
    x, w = c.x.to(device=device, dtype=dtype), c.w.to(device=device, dtype=dtype)
    gpre = c.G.to(device=device, dtype=dtype) * mask.to(device=device, dtype=dtype)
    g_sup = torch.cat([m.to(device=device, dtype=dtype).t() @ gpre[r0:r0 + n] for m, n, r0 in zip(c.mats, c.sizes, c.node_ptr[:-1])])
    g_adj = torch.cat([(gpre[r0:r0 + n] @ sup[r0:r0 + n].t()).reshape(-1) for n, r0 in zip(c.sizes, c.node_ptr[:-1])])
    wx, wadj, ww, wb = want
    return (g_sup @ w.t() if wx else None, g_adj if wadj else None, x.t() @ g_sup if ww else None,
            gpre.sum(0) if (wb and c.b is not None) else None)


@functools.lru_cache(maxsize=None)
def reference(c):
    """The float64 forward of a case, computed once: (pre64, out64, support64) on the CPU."""
    return forward(c, torch.float64, "cpu")


# ------------------------------------------------------------------------------------------------- the restatement
WRONG = ("adj_transposed_fwd", "adj_not_transposed_bwd", "row_base_off_by_one_graph", "adj_ptr_from_n", "bias_left_out", "mask_from_grad_out",
         "g_adj_operands_swapped", "g_bias_one_graph")


def _mm32(a, b):
    """a @ b in float32, the contraction index walked in order with one accumulator per cell (the MFMA's k-ordered chain)."""
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b[None, k, :]
    return acc


def restate(c, wrong=None):
    """csrc/gcn_ragged.hip in numpy float32: support over all rows; per graph b, rows node_ptr[b].., adjacency at adj_ptr[b], the aggregate
    with + bias and ReLU; backward: adj_b^T @ (G * (out > 0)), g_adj = gpre @ support^T per graph, the per-graph column sums added in graph
    order (16 runs of consecutive graphs, combined in order), g_x and g_weight over all rows.  `wrong`: one of WRONG.
    Returns [out, g_x, g_adj, g_weight, g_bias] as CPU tensors (g_bias None without a bias)."""
    assert wrong is None or wrong in WRONG
    f = np.float32
    x, w, G, vals = c.x.numpy(), c.w.numpy(), c.G.numpy(), c.values().numpy()
    B, O = len(c.sizes), c.O
    node = c.node_ptr
    adjp = c.adj_ptr if wrong != "adj_ptr_from_n" else c.node_ptr
    sup = _mm32(x, w)

    def rows(b):
        r0 = node[b - 1] if (wrong == "row_base_off_by_one_graph" and b > 0) else node[b]
        return slice(r0, r0 + c.sizes[b])

    def block(b):
        n = c.sizes[b]
        return vals[adjp[b]:adjp[b] + n * n].reshape(n, n)

    out = np.zeros((c.N, O), f)
    for b in range(B):
        m = block(b)
        pre = _mm32(m.T if wrong == "adj_transposed_fwd" else m, sup[rows(b)])
        if c.b is not None and wrong != "bias_left_out":
            pre = pre + c.b.numpy()
        out[node[b]:node[b + 1]] = np.maximum(pre, f(0))
    gpre = np.where((G if wrong == "mask_from_grad_out" else out) > 0, G, f(0)).astype(f)
    g_sup = np.zeros((c.N, O), f)
    g_adj = np.zeros(vals.shape, f)
    colsum = np.zeros((B, O), f)
    for b in range(B):
        m, n, r = block(b), c.sizes[b], slice(node[b], node[b + 1])
        g_sup[r] = _mm32(m if wrong == "adj_not_transposed_bwd" else m.T, gpre[rows(b)])
        ga = _mm32(sup[rows(b)], gpre[rows(b)].T) if wrong == "g_adj_operands_swapped" else _mm32(gpre[rows(b)], sup[rows(b)].T)
        g_adj[c.adj_ptr[b]:c.adj_ptr[b] + n * n] = ga.reshape(-1)
        for k in range(n):                                               # the chunks' rows in k order
            colsum[b] += gpre[rows(b)][k]
    per = (B + 15) // 16
    g_b = np.zeros(O, f)
    for g in range(16):
        run = np.zeros(O, f)
        for b in range(g * per, min(B, (g + 1) * per)):
            run += colsum[b]
        g_b += run
    if wrong == "g_bias_one_graph":
        g_b = colsum[0].copy()
    res = [out, _mm32(g_sup, w.T), g_adj, _mm32(x.T, g_sup), g_b if c.b is not None else None]
    return [None if r is None else torch.from_numpy(np.ascontiguousarray(r)) for r in res]


# ------------------------------------------------------------------------------------------------- the checks
def margin_cells(c, bound_fwd=2e-5):
    """(cells the mask check does not ask about, cells): 0 < |pre64| <= bound * max |pre64|.  Default: the widest bound the band allows."""
    pre64 = reference(c)[0]
    thr = bound_fwd * pre64.abs().max().item() if pre64.numel() else 0.0
    return int(((pre64.abs() <= thr) & (pre64 != 0)).sum()), pre64.numel()


def failures(c, got, device, label, want=(True, True, True, True)):
    """What of `got` = [out, g_x, g_adj, g_weight, g_bias] (None where `want` = (x, adj, weight, bias) says so or there is no bias) misses
    its check, as a list: band misses (name, e_op, e_chain) and mask misses ("mask", cells, asked); prints every figure.  The chain —
    the stock float32 torch ops — runs on `device`."""
    pre64, out64, sup64 = reference(c)
    pre32, out32, sup32 = forward(c, torch.float32, device)
    out = got[0].detach().cpu()
    mask = out > 0
    ref = (out64,) + grads(c, mask, sup64, torch.float64, "cpu", want)
    chain = (out32,) + grads(c, mask, sup32, torch.float32, device, want)
    bad = op_checks.band_failures(NAMES, got, chain, ref, label)
    b_fwd = op_checks.bound(op_checks.rel_err(out32, out64))
    thr = b_fwd * pre64.abs().max().item()
    asked = (pre64.abs() > thr) | (pre64 == 0)
    wrong = int((asked & (mask != (pre64 > 0))).sum())
    skipped, cells = margin_cells(c, b_fwd)
    print("%s mask: %d wrong of %d asked, %d of %d inside the margin" % (label, wrong, int(asked.sum()), skipped, cells))
    if wrong:
        bad.append(("mask", wrong, int(asked.sum())))
    if skipped > MARGIN_CAP * cells:
        bad.append(("margin", skipped, cells))
    return bad


def header_struct_typedefs():
    """The struct typedefs of include/recon_hip.h (comments stripped)."""
    import os
    import re
    from conftest import ROOT
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "recon_hip.h")).read(), flags=re.S)
    return set(re.findall(r"\}\s*(recon_[a-z0-9_]+)\s*;", text))
