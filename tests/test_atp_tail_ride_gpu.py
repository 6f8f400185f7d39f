"""The last two launches of the attention backward in the f16 x 2 family (csrc/gat_atp.hip, csrc/gemm_hx2.hip): the fixed-order reduce of
the skinny products' partial sums, which rides as extra workgroups behind the tiles of the weight-gradient product V^T g_h
(skinny_reduce_block in k_gemm_hx2_kmajor) wherever that launch follows in the same call, and k_atp_weights_finish, whose tile blocks
take their tiles in an order that keeps the neighbours of a row band on one XCD (a permutation of the tiles, with a remainder wherever
their number is no multiple of 8).

Every case runs the full gat_heads forward + backward against the float64 oracle at the bars of tests/test_atp_instances_gpu.py (its
_close and _bar), in every GEMM family (conftest: the bf16 x 3 and exact-fp32 families keep k_skinny_reduce).  Riding and the launch
of its own are compared bit for bit on g_u itself: the four phases of recon_gat_atp_bwd_phase as four calls cannot ride.

Rider shapes: the smallest (8 heads of 8 columns, one tile per head, 4 + 4 + 4 reduce blocks); element counts nj * K of 72 | 72 | 72 and
60 | 60 | 72 (no multiple of the block's 16: a partial last block per job) over 100 nodes (4 slices, the last one of 4 rows); a
product without rows beside two live ones (no edges at all; and edges into the first half of the nodes only, which also compacts the
rows); 9 heads and a source-side hub, which keep the launch of their own.
Last-pass shapes: D = 8, W = 24 (one partial tile a head, 8 tiles: `smallest`; 3 and 1 tiles, fewer than the 8 chunks of the order, in the
3- and 1-head cases); D = 40, W = 104 (a second tile column of 8 columns, W no multiple of 32, 2 x 4 x 2 = 16 tiles); the D = 36, W = 100 of
the same kind is no f16 x 2 shape (both must be multiples of 8) and runs here through the family's fall-back, as a guard of that;
ragged_72 has 3 x 3 x 1 = 9 tiles (remainder 1), tiles_15 15 (remainder 7), ragged_60 2 x 3 = 6; split counts 1 (every shape of at most 255 rows), 2, 3, 4, 5, 8, 10, 12, 17
and the largest the plan gives a one-tile product (64), each read back from recon_gat_atp_bwd_ride_plan."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import recon_oracle as O
from test_atp_instances_gpu import Row, _bar, _close, dev

pytestmark = pytest.mark.gpu

# name: (N, edges per node, F, R, D, H, kind, rides in the f16 x 2 family)
CASES = {
    "smallest": (32, 3, 8, 8, 8, 8, "plain", True),
    "ragged_72": (100, 3, 24, 24, 16, 3, "plain", True),
    "ragged_60": (100, 3, 20, 24, 16, 3, "plain", True),
    "tiles_15": (100, 3, 24, 24, 16, 5, "plain", True),
    "no_edges": (70, 0, 8, 8, 8, 3, "plain", True),
    "half_dst": (64, 3, 8, 8, 8, 3, "half", True),
    "h9": (70, 4, 8, 8, 8, 9, "plain", False),
    "source_hub": (70, 4, 8, 8, 8, 3, "hub", False),
    "d40_w104": (70, 4, 40, 24, 40, 2, "plain", True),
    "d36_w100": (70, 4, 34, 32, 36, 1, "plain", False),
    "splits_2": (256, 2, 8, 8, 8, 1, "plain", True),
    "splits_3": (384, 2, 8, 8, 8, 1, "plain", True),
    "splits_4": (512, 2, 8, 8, 8, 1, "plain", True),
    "splits_5": (640, 2, 8, 8, 8, 1, "plain", True),
    "splits_8": (1024, 2, 8, 8, 8, 1, "plain", True),
    "splits_10": (1280, 2, 8, 8, 8, 1, "plain", True),
    "splits_12": (1536, 2, 8, 8, 8, 1, "plain", True),
    "splits_17": (2176, 2, 8, 8, 8, 1, "plain", True),
    "splits_max": (8192, 2, 8, 8, 8, 1, "plain", True),
}
# the split count each splits_* case is there for; splits_max: whatever the plan says
SPLITS = {"splits_2": 2, "splits_3": 3, "splits_4": 4, "splits_5": 5, "splits_8": 8, "splits_10": 10, "splits_12": 12, "splits_17": 17}
NAMES = ("out", "g_x", "g_edge_embed", "g_a", "g_a_2")


def edges_of(name):
    """COO [2, E], row 0 the destinations.  plain: every node has `per` in-edges from random sources, the last 5 nodes feed none, 10 edges
    appear twice.  half: in-edges into the first half of the nodes only.  hub: node 7 is the source of 100 edges (HUB_CHUNK = 64: its walk
    runs in pieces)."""
    N, per, _, _, _, H, kind, _ = CASES[name]
    rs = np.random.RandomState(7 * N + 13 * H + len(name))
    if per == 0:
        return np.zeros((2, 0), dtype=np.int64)
    dst = np.repeat(np.arange(N // 2 if kind == "half" else N), per)
    src = rs.randint(0, N - 5, size=dst.size)
    if kind == "hub":
        src[rs.permutation(dst.size)[:100]] = 7
    edge = np.stack([dst, src])
    edge = np.concatenate([edge, edge[:, :10]], axis=1)
    return edge[:, rs.permutation(edge.shape[1])]


def plan_of(name, NR=None):
    """(rides, plan[10]) of recon_gat_atp_bwd_ride_plan for the case (NR: destination rows; the nodes unless the graph compacts them)"""
    from recon_amd import _lib
    N, _, F_, R, D, H, _, _ = CASES[name]
    E = edges_of(name).shape[1]
    plan = (ctypes.c_int32 * 10)()
    rides = _lib.lib().recon_gat_atp_bwd_ride_plan(N if NR is None else NR, N, E, F_, R, D, H, plan)
    return rides, list(plan)


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs of a case and its float64 oracle, computed once and shared by the tests below"""
    N, _, F_, R, D, H, _, _ = CASES[name]
    edge = torch.from_numpy(edges_of(name)).long()
    E = edge.shape[1]
    g = torch.Generator().manual_seed(N + 3 * E + H + F_)
    x = torch.randn(N, F_, generator=g)
    ee = torch.randn(E, R, generator=g) * 0.5
    a = torch.stack([O.xavier_normal((D, 2 * F_ + R), 1.414, g) for _ in range(H)]) * 0.5
    a2 = torch.cat([O.xavier_normal((1, D), 1.414, g) for _ in range(H)])
    G = torch.randn(N, H * D, generator=g)
    out, g_a, g_a2, g_x, g_ee = [], [], [], 0, 0
    for h in range(H):
        r = O.gat_layer_backward(x.double(), edge, ee.double(), None, None, a[h].double(), a2[h:h + 1].double(), 0.2, True,
                                 G[:, h * D:(h + 1) * D].double())
        out.append(r["out"]); g_a.append(r["g_a"]); g_a2.append(r["g_a_2"])
        g_x, g_ee = g_x + r["g_x"], g_ee + r["g_edge_embed"]
    ref = dict(out=torch.cat(out, 1), g_x=g_x, g_edge_embed=g_ee, g_a=torch.stack(g_a), g_a_2=torch.cat(g_a2))
    return dict(edge=edge, x=x, ee=ee, a=a, a2=a2, G=G, ref=ref)


class _Phased:
    """the library with recon_gat_atp_bwd replaced by the four phases of recon_gat_atp_bwd_phase, one call each, on the same stream"""

    def __init__(self, L):
        self._L = L

    def __getattr__(self, name):
        return getattr(self._L, name)

    def recon_gat_atp_bwd(self, g, b, stream):
        for mask in (1, 2, 4, 8):
            rc = self._L.recon_gat_atp_bwd_phase(g, b, mask, stream)
            if rc != 0:
                return rc
        return 0


def _run(name, monkeypatch, phased=False):
    """{out, g_x, g_edge_embed, g_a, g_a_2, g_u} of the case through the aggregate-then-project kernels, and the graph.  g_u [H, W] is
    read out of the backward's scratch allocation (gat_layers._carve: its seventh slice)."""
    from recon_amd import _lib, gat_layers, graph as graph_mod
    N, _, F_, R, D, H, kind, _ = CASES[name]
    c = _case(name)
    d = dev()
    monkeypatch.setattr(gat_layers, "_GAT_PATH", "atp")
    monkeypatch.setattr(gat_layers, "_OVERLAP", False)
    if phased:
        proxy = _Phased(_lib.lib())
        monkeypatch.setattr(_lib, "lib", lambda: proxy)
    carved = []
    carve = gat_layers._carve

    def keep_carve(dev_, sizes):
        res = carve(dev_, sizes)
        carved.append((len(sizes), res))
        return res
    monkeypatch.setattr(gat_layers, "_carve", keep_carve)
    gr = graph_mod.prepare_graph(c["edge"].to(d), None, N)
    assert (gr.n_hub_src >= 1) == (kind == "hub")
    assert (gr.n_rows == N // 2) if kind == "half" else (gr.n_rows == 0)
    leaves = [t.to(d).requires_grad_(True) for t in (c["x"], c["ee"], c["a"], c["a2"])]
    out = gat_layers.gat_heads(*leaves, gr, None, 0.2, True)
    grads = torch.autograd.grad(out, leaves, c["G"].to(d))
    torch.cuda.synchronize()
    got = {nm: t.detach().cpu() for nm, t in zip(NAMES, (out,) + tuple(grads))}
    bwd = [res for n, res in carved if n == 11]
    assert len(bwd) == 1, "the backward's scratch allocation"
    buf, ptrs = bwd[0]
    got["g_u"] = gat_layers._view_f32(buf, ptrs[6], H * (2 * F_ + R)).clone().cpu()
    return got, gr


def _check(name, got):
    _, _, F_, R, D, H, _, _ = CASES[name]
    row = Row(0, F_, R, D, H, "fp32", name, True, True)
    ref = _case(name)["ref"]
    for nm in NAMES:
        atol, rel = _bar(row, nm)
        if nm in ("out", "g_a", "g_a_2"):                           # head by head, as test_atp_instances_gpu._check
            for h in range(H):
                act = got[nm][:, h * D:(h + 1) * D] if nm == "out" else got[nm][h]
                des = ref[nm][:, h * D:(h + 1) * D] if nm == "out" else ref[nm][h]
                _close(act, des, atol, rel, "%s %s h%d" % (name, nm, h))
        else:
            _close(got[nm], ref[nm], atol, rel, "%s %s" % (name, nm))


@pytest.mark.parametrize("name", list(CASES))
def test_tail_vs_oracle(name, gemm_family, monkeypatch):
    got, gr = _run(name, monkeypatch)
    N, _, F_, R, D, H, _, rides = CASES[name]
    says, plan = plan_of(name, gr.n_rows or N)
    if rides:                                                       # (the plan speaks for a graph without source-side hub pieces)
        assert says == 1, "the case was chosen to ride"
    elif name != "source_hub":
        assert says == 0
    if name in SPLITS:
        assert plan[6] == SPLITS[name]
    elif name == "splits_max":
        assert plan[6] > 32, "the cap of the split choice, far above the benchmark's 12"
    elif N < 256:
        assert plan[6] == 1
    _check(name, got)


@pytest.mark.parametrize("name", ["smallest", "ragged_72", "ragged_60", "no_edges", "half_dst", "d40_w104", "splits_12", "splits_max"])
def test_riding_reduce_equals_the_launch_of_its_own(name, gemm_family, monkeypatch):
    """g_u — and with it every gradient — is the same bits whether the reduce's blocks ride behind the weight-gradient tiles (one call) or
    run as k_skinny_reduce (INPUTS and WEIGHTS issued in two calls)."""
    one, _ = _run(name, monkeypatch)
    four, _ = _run(name, monkeypatch, phased=True)
    assert torch.equal(one["g_u"], four["g_u"]), "g_u"
    for nm in NAMES:
        assert torch.equal(one[nm], four[nm]), nm
