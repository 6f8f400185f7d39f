"""The tail of the attention backward (csrc/gat_atp.hip): the source walk and the partial sums of the skinny products g_u = [Gs_dst | Gs_src]^T x,
g_sigma^T ee in one launch (k_gat_atp_src_skinny: up to 8 heads, no source-side hub pieces), k_skinny_reduce and the last kernel — against the
fp64 oracle with the tolerances of test_gat_gpu.py, against the phased backward bit for bit, and run to run.

Shapes: F = R = D of 8 and 16 (f16 x 2 needs multiples of 8) with 1, 3 and 8 heads; row counts of the three products (rows with in-edges,
nodes, edges) that are one slice (<= 32 rows), several slices with a short last one (70 = 2 x 32 + 6, 300 = 9 x 32 + 12), whole slices
(64, 320) and slices of more than two iterations (40 000 edges / 1024 -> 40 rows each); no edges at all; compacted rows; a relation table;
and the two shapes that keep the separate launches (a source-side hub, 11 heads)."""
import functools

import numpy as np
import pytest
import torch

from oracle import recon_oracle as O

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


def close(actual, desired, atol=1e-4, rel_to_max=1e-4, what=""):
    actual = actual.detach().cpu().numpy() if torch.is_tensor(actual) else actual
    desired = desired.detach().cpu().numpy() if torch.is_tensor(desired) else desired
    tol = atol + rel_to_max * (np.abs(desired).max() if desired.size else 0.0)
    err = np.abs(actual - desired).max() if desired.size else 0.0
    assert np.isfinite(actual).all(), what + ": non-finite values"
    assert err <= tol, "%s: max abs err %.3e > tol %.3e" % (what, err, tol)


# name: (N, E, F = R = D, H, kind)
CASES = {
    "h1_f8": (70, 300, 8, 1, "plain"),
    "h3_f16": (70, 300, 16, 3, "plain"),
    "h8_f8": (70, 300, 8, 8, "plain"),
    "h8_f16": (70, 300, 16, 8, "plain"),
    "one_slice": (20, 30, 8, 3, "plain"),
    "whole_slices": (64, 320, 8, 3, "plain"),
    "long_slices": (2000, 40000, 8, 3, "plain"),
    "no_edges": (70, 0, 8, 3, "plain"),
    "compacted": (70, 300, 16, 3, "compact"),
    "table": (70, 300, 8, 8, "table"),
    "source_hub": (70, 300, 8, 3, "hub"),
    "h11": (70, 300, 8, 11, "plain"),
}


def _edges(N, E, kind, rs):
    """The last 5 nodes have no out-edges, the first 5 no in-edges, 20 edges appear twice.  compact: 8 nodes take all the in-edges.
    hub: node 7 is the source of 100 edges (more than HUB_CHUNK = 64: its walk runs in pieces)."""
    if E == 0:
        return np.zeros((2, 0), dtype=np.int64)
    lo, hi = min(5, N // 4), N - min(5, N // 4)
    src = rs.randint(0, hi, size=E)
    dst = rs.randint(lo, N, size=E)
    if kind == "compact":
        dst = (lo + 7 * np.arange(8))[np.arange(E) % 8]
    if kind == "hub":
        src[rs.permutation(E)[:100]] = 7
    k = min(20, E // 3)
    src[E - k:], dst[E - k:] = src[:k], dst[:k]
    return np.stack([dst, src])                                       # row 0: destinations (test_gat_gpu._hub_graph)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of a case and its fp64 oracle (outputs and the four gradients), computed once and shared by the tests below."""
    N, E, F_, H, kind = CASES[name]
    R = D = F_
    rs = np.random.RandomState(len(name) + 7 * N + E + H)
    g = torch.Generator().manual_seed(N + 3 * E + H + F_)
    edge = torch.from_numpy(_edges(N, E, kind, rs)).long()
    x = torch.randn(N, F_, generator=g)
    nrel = 11
    ee = torch.randn(nrel if kind == "table" else E, R, generator=g) * 0.5
    ee_index = torch.randint(0, nrel, (E,), generator=g) if kind == "table" else None
    a = torch.stack([O.xavier_normal((D, 2 * F_ + R), 1.414, g) for _ in range(H)]) * 0.5
    a2 = torch.cat([O.xavier_normal((1, D), 1.414, g) for _ in range(H)])
    G = torch.randn(N, H * D, generator=g)
    ee_e = ee[ee_index] if kind == "table" else ee
    ref = {"out": [], "g_a": [], "g_a_2": [], "g_x": torch.zeros(N, F_, dtype=torch.float64), "g_ee": torch.zeros(E, R, dtype=torch.float64)}
    for h in range(H):
        r = O.gat_layer_backward(x.double(), edge, ee_e.double(), None, None, a[h].double(), a2[h:h + 1].double(), 0.2, True,
                                 G[:, h * D:(h + 1) * D].double())
        ref["out"].append(r["out"]); ref["g_a"].append(r["g_a"]); ref["g_a_2"].append(r["g_a_2"])
        ref["g_x"] += r["g_x"]; ref["g_ee"] += r["g_edge_embed"]
    if kind == "table":
        ref["g_ee"] = torch.zeros(nrel, R, dtype=torch.float64).index_add_(0, ee_index, ref["g_ee"])
    want = [torch.cat(ref["out"], 1).float(), ref["g_x"].float(), ref["g_ee"].float(), torch.stack(ref["g_a"]).float(),
            torch.cat(ref["g_a_2"]).float()]
    return dict(N=N, E=E, H=H, kind=kind, edge=edge, x=x, ee=ee, ee_index=ee_index, a=a, a2=a2, G=G, want=want)


class _Phased:
    """The library with recon_gat_atp_bwd replaced by the four phases of recon_gat_atp_bwd_phase, one call each, on the same stream."""

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
    """[out, g_x, g_edge_embed, g_a, g_a_2] of the case on the device (aggregate-then-project kernels, f16 x 2 family: conftest.gemm_family)."""
    from recon_amd import _lib, gat_layers, graph as graph_mod
    c = _case(name)
    d = dev()
    monkeypatch.setattr(gat_layers, "_GAT_PATH", "atp")
    monkeypatch.setattr(gat_layers, "_OVERLAP", False)
    if phased:
        proxy = _Phased(_lib.lib())
        monkeypatch.setattr(_lib, "lib", lambda: proxy)
    gr = graph_mod.prepare_graph(c["edge"].to(d), None, c["N"])
    assert (gr.n_hub_src >= 1) == (c["kind"] == "hub")
    assert (gr.n_rows == 8) if c["kind"] == "compact" else (gr.n_rows == 0)
    leaves = [t.to(d).requires_grad_(True) for t in (c["x"], c["ee"], c["a"], c["a2"])]
    idx = c["ee_index"].to(d) if c["ee_index"] is not None else None
    out = gat_layers.gat_heads(*leaves, gr, None, 0.2, True, ee_index=idx)
    grads = torch.autograd.grad(out, leaves, c["G"].to(d))
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in (out,) + tuple(grads)]


NAMES = ("out", "g_x", "g_edge_embed", "g_a", "g_a_2")


@pytest.mark.parametrize("name", list(CASES))
def test_tail_gradients_vs_oracle(name, monkeypatch):
    got = _run(name, monkeypatch)
    for nm, u, v in zip(NAMES, got, _case(name)["want"]):
        assert u.shape == v.shape, nm
        if v.numel():
            if nm == "out":
                close(u, v, what=nm)
            else:
                close(u, v, atol=1e-4, rel_to_max=1e-4, what=nm)


@pytest.mark.parametrize("name", ["h8_f16", "long_slices", "no_edges", "source_hub"])
def test_one_call_backward_equals_phased(name, monkeypatch):
    """PREPARE, INPUTS, WEIGHTS and FINISH as four calls give the bits of the one call."""
    one = _run(name, monkeypatch)
    four = _run(name, monkeypatch, phased=True)
    for nm, u, v in zip(NAMES, one, four):
        assert torch.equal(u, v), nm


@pytest.mark.parametrize("name", ["h8_f16", "long_slices"])
def test_two_runs_are_bit_equal(name, monkeypatch):
    for nm, u, v in zip(NAMES, _run(name, monkeypatch), _run(name, monkeypatch)):
        assert torch.equal(u, v), nm
