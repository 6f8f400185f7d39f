"""Every edge-pass kernel instance of the aggregate-then-project attention (csrc/gat_atp.hip) against the float64 oracle.

atp_shape() maps the layer widths (F, R, H) to a key vec * 1000 + kr * 10 + log2(ht) — load width, register rows per lane, heads per
wave — and ATP_DISPATCH instantiates K1' (k_gat_atp_fwd), K2' (k_gat_atp_bwd), the source pass and the hub-piece kernels from it.  Each
instance has its own tails, head-group masks and register layout, so each gets a row of ATP_ROWS at widths that select it
(recon_gat_atp_instance says which one a row really runs).  tests/test_atp_instances_cpu.py fails when a reachable key has no row.

Every row runs through gat_heads on one graph with isolated destination rows, duplicate edges and a destination and a source row of
well over HUB_CHUNK edges (both hub-piece kernels), in train mode with dropout factors (TRAIN = true, then the backward), once more for
bit-equality, under no_grad without dropout (TRAIN = false), and on the same edges without hub pieces (the persistent K2' grid).  The
vec = 4, kr = 1 rows also run K2' without the LDS row ring and without the persistent grid (RECON_K2_LDS_RING / RECON_K2_PERSIST = 0).
Each fp32 row runs in all three GEMM families (conftest.GEMM_FAMILIES: f16 x 2 planes 1 / 2, bf16 x 3, exact fp32).  bf16 rows read
bf16 x / edge_embed in place under family 2 and go through the up-cast fallback under the others, at the same bar.

Bars: fp32 rows as test_gat_gpu.py::test_gat_heads_vs_oracle, bf16 rows as test_gat_gpu.py::test_cfg5_bf16_attention_at_the_benched_shapes."""
import collections

import numpy as np
import pytest
import torch

from oracle import recon_oracle as O

pytestmark = pytest.mark.gpu

Row = collections.namedtuple("Row", "key F R D H dtype note concat ee_grad")


def _row(key, F, R, D, H, dtype, note, concat=True, ee_grad=True):
    return Row(key, F, R, D, H, dtype, note, concat, ee_grad)


# (key, F, R, D, H, dtype, note) [+ concat, ee_grad].  kr boundaries: vec 4 at 256 / 512 / 1024 columns, vec 2 at 128 / 256 / 512;
# "planes" = the f16 x 2 V planes family 2 writes: 2 where F, R % 8 == 0, 1 where only (2F + R) % 8 == 0 (D % 8 == 0 both), else none
ATP_ROWS = [
    _row(4010, 252, 36, 16, 1, "fp32", "F's last float4 group on lane 62: one register row, 63 lanes", concat=False),
    _row(4011, 12, 8, 16, 2, "fp32", "pair of heads, exact; W = 32 with F % 8 = 4: planes 1"),
    _row(4012, 68, 20, 16, 3, "fp32", "3 of 4 heads: partial group"),
    _row(4012, 64, 32, 8, 4, "fp32", "4 of 4 heads: exact group, planes 2"),
    _row(4013, 36, 44, 16, 5, "fp32", "5 of 8 heads: partial group"),
    _row(4013, 40, 16, 16, 8, "fp32", "8 of 8 heads: exact group, planes 2"),
    _row(4013, 24, 16, 8, 11, "fp32", "11 heads: a full group and 3 of 8"),
    _row(4020, 260, 100, 16, 1, "fp32", "F just above 256: second register row holds one float4 group"),
    _row(4021, 8, 264, 16, 2, "fp32", "R just above 256, pair of heads, planes 2"),
    _row(4022, 4, 300, 16, 3, "fp32", "R above 256, 3 of 4 heads"),
    _row(4022, 296, 16, 8, 4, "fp32", "F above 256, 4 of 4 heads, planes 2"),
    _row(4022, 264, 8, 8, 6, "fp32", "6 heads: a full group and 2 of 4"),
    _row(4040, 516, 40, 16, 1, "fp32", "F just above 512: third register row one group, fourth empty; planes 1"),
    _row(4040, 20, 1020, 8, 1, "fp32", "R = 1020: the fourth register row 63 lanes", concat=False),
    _row(4041, 16, 520, 16, 2, "fp32", "R just above 512, pair of heads, planes 2"),
    _row(4041, 900, 28, 8, 4, "fp32", "F = 900 ends in the fourth register row, two pairs of heads"),
    _row(4041, 520, 24, 8, 3, "fp32", "3 heads: a full pair and 1 of 2"),
    _row(4080, 1028, 20, 16, 1, "fp32", "F just above 1024: out_att-like single head", concat=False),
    _row(4080, 16, 1032, 8, 3, "fp32", "R just above 1024, 3 heads one per wave, planes 2"),
    _row(4080, 2040, 12, 8, 2, "fp32", "F = 2040: the eighth register row 62 lanes, 2 heads one per wave"),
    _row(2010, 50, 50, 16, 1, "fp32", "the reference's 50-wide features and relations"),
    _row(2011, 6, 20, 16, 2, "fp32", "pair of heads; (2F + R) % 8 == 0: planes 1"),
    _row(2012, 30, 14, 16, 3, "fp32", "3 of 4 heads"),
    _row(2012, 50, 100, 16, 4, "fp32", "50 / 100 widths, 4 of 4 heads, planes 1"),
    _row(2013, 18, 2, 16, 5, "fp32", "5 of 8 heads, R = 2: one lane of relation columns"),
    _row(2013, 22, 4, 16, 8, "fp32", "8 of 8 heads, planes 1"),
    _row(2013, 10, 6, 8, 11, "fp32", "11 heads: a full group and 3 of 8"),
    _row(2020, 130, 14, 16, 1, "fp32", "F just above 128 (the reference's 130-type width)"),
    _row(2021, 134, 4, 16, 2, "fp32", "F above 128, pair of heads, planes 1"),
    _row(2022, 130, 6, 16, 3, "fp32", "3 of 4 heads"),
    _row(2022, 6, 132, 16, 4, "fp32", "R above 128, 4 of 4 heads, planes 1"),
    _row(2023, 130, 2, 16, 5, "fp32", "5 of 8 heads at two register rows"),
    _row(2023, 138, 20, 8, 8, "fp32", "8 of 8 heads at two register rows, planes 1"),
    _row(2040, 300, 50, 16, 1, "fp32", "the reference's 300 / 50 widths: F just above 256"),
    _row(2040, 2, 510, 8, 1, "fp32", "R = 510: the fourth register row 63 lanes", concat=False),
    _row(2041, 50, 260, 16, 2, "fp32", "R just above 256, pair of heads, planes 1"),
    _row(2041, 6, 450, 8, 2, "fp32", "R = 450 ends in the fourth register row, pair of heads"),
    _row(2042, 262, 10, 16, 3, "fp32", "3 of 4 heads at four register rows"),
    _row(2042, 130, 300, 8, 4, "fp32", "4 of 4 heads at four register rows, planes 1"),
    _row(2042, 400, 10, 8, 5, "fp32", "F = 400 ends in the fourth register row, 5 heads: a full group and 1 of 4"),
    _row(2080, 514, 2, 16, 1, "fp32", "F just above 512", concat=False),
    _row(2080, 1022, 6, 8, 1, "fp32", "F = 1022: the eighth register row 63 lanes"),
    _row(2081, 2, 518, 16, 3, "fp32", "R just above 512, 3 heads: a full pair and 1 of 2"),
    _row(2081, 514, 4, 8, 2, "fp32", "F above 512, pair of heads, planes 1"),
    _row(2081, 2, 1000, 8, 4, "fp32", "R = 1000 ends in the eighth register row, two pairs of heads"),
    # bf16 x / edge_embed read in place (recon_gat_atp_bf16_io_supported: vec 4, F, R, D % 8 == 0, at most 8 heads).  kr = 1: K2' with
    # the LDS row ring, with the bf16 g_edge_embed store (ee_grad) and without it (edge embeddings that need no gradient)
    _row(4010, 200, 200, 32, 1, "bf16", "the benched 200 / 200 widths, bf16 g_edge_embed store"),
    _row(4010, 40, 248, 16, 1, "bf16", "edge embeddings without a gradient: the ring instance without the bf16 store", ee_grad=False),
    _row(4011, 16, 8, 16, 2, "bf16", "pair of heads, bf16 g_edge_embed store"),
    _row(4012, 24, 56, 16, 3, "bf16", "3 of 4 heads, bf16 g_edge_embed store"),
    _row(4012, 64, 32, 8, 4, "bf16", "4 of 4 heads, edge embeddings without a gradient", ee_grad=False),
    _row(4013, 8, 64, 16, 5, "bf16", "5 of 8 heads, bf16 g_edge_embed store"),
    _row(4013, 40, 16, 8, 8, "bf16", "8 of 8 heads, edge embeddings without a gradient", ee_grad=False),
    _row(4020, 264, 8, 16, 1, "bf16", "F just above 256"),
    _row(4021, 16, 264, 16, 2, "bf16", "R just above 256, pair of heads"),
    _row(4022, 264, 264, 8, 3, "bf16", "F = R above 256, 3 of 4 heads"),
    _row(4040, 8, 1000, 16, 1, "bf16", "R = 1000 ends in the fourth register row"),
    _row(4041, 520, 16, 16, 2, "bf16", "F just above 512, pair of heads"),
    _row(4080, 1800, 8, 16, 2, "bf16", "F = 1800 ends in the eighth register row, 2 heads one per wave"),
]


def row_id(r):
    return "k%d-H%d-F%dR%d-%s%s" % (r.key, r.H, r.F, r.R, r.dtype, "" if r.ee_grad else "-nogee")


def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


def atp_graph(seed):
    """COO [2, E] over N = 200 nodes (E ~ 1.2 k): destination 1 has 150 in-edges and source 2 feeds 140 edges, a few more of each from the
    repeats (HUB_CHUNK = 64: three pieces each), destinations 5 and 192 ... 199 have no in-edges, 40 random edges appear twice and one
    three times; columns shuffled."""
    rs = np.random.RandomState(seed)
    N = 200
    degs = rs.randint(1, 11, size=N)
    degs[1] = 150
    degs[[5] + list(range(192, 200))] = 0
    dst = np.repeat(np.arange(N), degs)
    src = rs.randint(0, N, size=dst.size)
    src[src == 2] = 3
    src[rs.permutation(dst.size)[:140]] = 2
    edge = np.stack([dst, src])
    dup = edge[:, rs.randint(0, dst.size, size=40)]
    one = edge[:, [7]]
    edge = np.concatenate([edge, dup, one, one], axis=1)
    edge = edge[:, rs.permutation(edge.shape[1])]
    return torch.from_numpy(edge).long(), N


def _colscale(n):
    """per-column factors in [0.25, 1.75]: a column read in place of another, or twice, is far outside the bar"""
    return 0.25 + 1.5 * torch.from_numpy(((np.arange(n) * 7) % 13) / 12.0).float()


def _inputs(row, seed):
    edge, N = atp_graph(seed)
    E, F_, R, D, H = edge.shape[1], row.F, row.R, row.D, row.H
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, F_, generator=g) * _colscale(F_)
    ee = torch.randn(E, R, generator=g) * 0.5 * _colscale(R)
    if row.dtype == "bf16":
        x, ee = x.to(torch.bfloat16), ee.to(torch.bfloat16)
    a = torch.stack([O.xavier_normal((D, 2 * F_ + R), 1.414, g) for _ in range(H)]) * 0.5
    a2 = torch.cat([O.xavier_normal((1, D), 1.414, g) for _ in range(H)])
    keep = (torch.rand(H, E, generator=g) > 0.25).float() / 0.75
    G = torch.randn(N, H * D, generator=g)
    if row.dtype == "bf16":
        G = G.to(torch.bfloat16)
    return edge, N, x, ee, a, a2, keep, G


_REF = {}


def _reference(row, seed, edge, x, ee, a, a2, keep, G):
    """float64 oracle per head on the inputs as the kernels see them (bf16 rows: the bf16 values): the train-mode output and gradients with
    the recorded keep factors, and the no-dropout output"""
    key = (row, seed)
    if key in _REF:
        return _REF[key]
    D = row.D
    x64, ee64 = x.double(), ee.double()
    out, out_eval, g_a, g_a2, g_x, g_ee = [], [], [], [], 0, 0
    for h in range(row.H):
        r = O.gat_layer_backward(x64, edge, ee64, None, None, a[h].double(), a2[h:h + 1].double(), 0.2, row.concat,
                                 G[:, h * D:(h + 1) * D].double(), mask=keep[h].double())
        out.append(r["out"])
        g_a.append(r["g_a"])
        g_a2.append(r["g_a_2"])
        g_x, g_ee = g_x + r["g_x"], g_ee + r["g_edge_embed"]
        out_eval.append(O.gat_layer_forward(x64, edge, ee64, None, None, a[h].double(), a2[h:h + 1].double(), 0.2, row.concat))
    _REF[key] = ref = dict(out=torch.cat(out, 1), g_x=g_x, g_edge_embed=g_ee, g_a=torch.stack(g_a), g_a_2=torch.cat(g_a2), eval=torch.cat(out_eval, 1))
    return ref


def _bar(row, name):
    """(atol, rel_to_max) of test_gat_heads_vs_oracle (fp32) / test_cfg5_bf16_attention_at_the_benched_shapes (bf16)"""
    if row.dtype == "bf16" and name in ("out", "eval", "g_x", "g_edge_embed"):
        return 1e-5, 2.0 ** -8
    return (1e-4, 1e-4) if name in ("out", "eval") else (1e-5, 1e-4)


def _close(actual, desired, atol, rel_to_max, what):
    """test_gat_gpu.close(), returning max |error| / max |desired|"""
    actual, desired = actual.numpy().astype(np.float64), desired.numpy()
    assert actual.shape == desired.shape, "%s: shape %s, oracle %s" % (what, actual.shape, desired.shape)
    assert np.isfinite(actual).all(), what + ": non-finite values"
    mx = np.abs(desired).max() if desired.size else 0.0
    err = np.abs(actual - desired).max() if desired.size else 0.0
    assert err <= atol + rel_to_max * mx, "%s: max abs err %.3e > tol %.3e" % (what, err, atol + rel_to_max * mx)
    return err / mx if mx > 0 else err


def _check(row, got, ref, what, worst):
    """every output of `got` against the oracle (out, g_a, g_a_2 head by head); worst[name] = the largest relative error seen"""
    D = row.D
    for name, v in got.items():
        atol, rel = _bar(row, name)
        if name in ("out", "eval"):
            parts = [(v[:, h * D:(h + 1) * D], ref[name][:, h * D:(h + 1) * D], " h%d" % h) for h in range(row.H)]
        elif name in ("g_a", "g_a_2"):
            parts = [(v[h], ref[name][h], " h%d" % h) for h in range(row.H)]
        else:
            parts = [(v, ref[name], "")]
        for act, des, tag in parts:
            e = _close(act, des, atol, rel, "%s %s %s%s" % (row_id(row), what, name, tag))
            worst[name] = max(worst.get(name, 0.0), e)


def _run(row, graph, x, ee, a, a2, keep, G, train=True):
    """one gat_heads call through the ATP kernels (train: with the keep factors, then the backward of G): outputs as float32 on the host"""
    from recon_amd import gat_layers
    d = dev()
    xd, eed = x.to(d).requires_grad_(train), ee.to(d).requires_grad_(train and row.ee_grad)
    ad, a2d = a.to(d).requires_grad_(train), a2.to(d).requires_grad_(train)
    want = torch.bfloat16 if row.dtype == "bf16" else torch.float32
    if not train:
        with torch.no_grad():
            out = gat_layers.gat_heads(xd, eed, ad, a2d, graph, None, 0.2, row.concat)
        assert out.dtype == want and out.shape == (graph.N, row.H * row.D)
        return dict(eval=out.float().cpu())
    out = gat_layers.gat_heads(xd, eed, ad, a2d, graph, keep.to(d), 0.2, row.concat)
    assert out.dtype == want and out.shape == (graph.N, row.H * row.D)
    out.backward(G.to(d))
    res = dict(out=out, g_x=xd.grad, g_a=ad.grad, g_a_2=a2d.grad)
    if row.ee_grad:
        res["g_edge_embed"] = eed.grad
    assert xd.grad.dtype == want and (eed.grad is None) == (not row.ee_grad)
    if row.ee_grad:
        assert eed.grad.dtype == want
    return {k: v.detach().float().cpu() for k, v in res.items()}


def pytest_generate_tests(metafunc):
    # here rather than as a mark so that the row comes first in the test ids (k4041-H2-F16R520-fp32-gemm_hx2); conftest adds the GEMM family
    if "row" in metafunc.fixturenames:
        metafunc.parametrize("row", ATP_ROWS, ids=[row_id(r) for r in ATP_ROWS])


def test_atp_instance_vs_oracle(row, gemm_family, recon_config, monkeypatch, record_property):
    from recon_amd import _lib, gat_layers, graph as graph_mod
    monkeypatch.setattr(gat_layers, "_GAT_PATH", "atp")
    L = _lib.lib()
    d = dev()
    seed = row.key * 37 + row.H
    edge, N, x, ee, a, a2, keep, G = _inputs(row, seed)
    E = edge.shape[1]
    assert L.recon_gat_atp_instance(row.F, row.R, row.H) == row.key, "the row's widths select another instance"
    assert L.recon_gat_atp_supported(N, E, row.F, row.R, row.D, row.H) == 1
    if row.dtype == "bf16":
        assert L.recon_gat_atp_bf16_io_supported(row.F, row.R, row.D, row.H) == 1
    ref = _reference(row, seed, edge, x, ee, a, a2, keep, G)
    edge_d = edge.to(d)
    graph = graph_mod.prepare_graph(edge_d, None, N)
    assert graph.n_hub >= 1 and graph.n_hub_src >= 1 and graph.n_rows == 0        # hub pieces on both sides, rows not compacted
    worst = {}
    first = _run(row, graph, x, ee, a, a2, keep, G)
    _check(row, first, ref, "train", worst)
    again = _run(row, graph, x, ee, a, a2, keep, G)
    for name, v in first.items():
        assert torch.equal(v, again[name]), "%s: %s differs between two identical calls (fixed-order sums)" % (row_id(row), name)
    _check(row, _run(row, graph, x, ee, a, a2, None, G, train=False), ref, "no_grad", worst)
    # the same edges walked one row per wave (the hub graph above is resolved: its tables stay as they are): K2' on its persistent grid
    monkeypatch.setattr(graph_mod, "HUB_CHUNK", 0)
    flat = graph_mod.prepare_graph(edge_d, None, N)
    assert flat.n_hub == 0 and flat.n_rows == 0
    _check(row, _run(row, flat, x, ee, a, a2, keep, G), ref, "no hub pieces", worst)
    if row.key // 10 == 401:                                   # vec = 4, kr = 1: the K2' instances and grids the switches reach
        recon_config("RECON_K2_PERSIST", "0")                  # one wave per row instead of persistent waves
        _check(row, _run(row, flat, x, ee, a, a2, keep, G), ref, "no persistent grid", worst)
        recon_config("RECON_K2_LDS_RING", "0")                 # K2' without the LDS row ring (and so without the bf16 g_edge_embed store)
        _check(row, _run(row, graph, x, ee, a, a2, keep, G), ref, "no LDS ring", worst)
    for name, v in sorted(worst.items()):
        record_property("worst_rel_" + name, "%.3e" % v)
