"""The float32 GraphConvolution over a ragged batch on the GPU (recon_amd/gcn_layers.py _GcnRaggedFunction, csrc/gcn_ragged.hip) against
the float64 reference of tests/gcn_ragged_checks.py: through the layer and through the C ABI (guarded buffers, bitwise reproducible),
beside the dense layer at equal sizes, through a row-strided input, through gcn_stack, at the parity bound of three stacked layers,
on both GEMM families, and its rejections.  On a tree without the float32 path every call here raises TypeError."""
import ctypes as C

import pytest
import torch

import gcn_ragged_checks as R
import op_checks

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, -1, -2
GUARD = 37


def dev():
    return op_checks.dev()


def make_layer(c, d):
    from recon_amd.gcn_layers import GraphConvolution
    layer = GraphConvolution(c.I, c.O, bias=c.b is not None)
    with torch.no_grad():
        layer.weight.copy_(c.w)
        if c.b is not None:
            layer.bias.copy_(c.b)
    return layer.to(d)


def run_layer(c, d, want_x=True, want_v=True, x=None):
    """[out, g_x, g_adj, g_weight, g_bias] of one forward + backward through GraphConvolution."""
    from recon_amd.gcn_layers import RaggedAdjacency
    layer = make_layer(c, d)
    x = (c.x.to(d) if x is None else x).detach().requires_grad_(want_x)
    rag = RaggedAdjacency(c.values().to(d).requires_grad_(want_v), c.sizes)
    out = layer(x, rag)
    assert out.dtype == torch.float32 and out.shape == (c.N, c.O)
    (out * c.G.to(d)).sum().backward()
    return [out.detach(), x.grad, rag.values.grad, layer.weight.grad, layer.bias.grad if c.b is not None else None]


@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_gcn_ragged_layer_vs_fp64(shape, bias):
    """Forward, the four gradients and the ReLU mask, with `input` and `adj.values` requiring a gradient or not."""
    c, d = R.case(*shape, bias), dev()
    for want_x in (True, False):
        for want_v in (True, False):
            got = run_layer(c, d, want_x, want_v)
            assert (got[1] is None) == (not want_x) and (got[2] is None) == (not want_v)
            bad = R.failures(c, got, d, "%s x%d v%d" % (R.shape_id(shape), want_x, want_v), want=(want_x, want_v, True, True))
            assert not bad, bad


def test_gcn_ragged_zero_row_is_relu_bias():
    sizes, g, row = R.ZERO_ROW
    c = R.case(sizes, 40, 136, True)
    out = run_layer(c, dev())[0].cpu()
    assert torch.equal(out[int(c.node_ptr[g]) + row], torch.relu(c.b))


# ------------------------------------------------------------------------------------------------- the C ABI
class Guarded:
    """n floats inside a NaN-filled buffer, GUARD elements of it on either side."""

    def __init__(self, n, d):
        self.n, self.buf = n, torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=d)
        self.t = self.buf[GUARD:GUARD + n]

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[GUARD + self.n:]).all())

    def ptr(self):
        return self.t.data_ptr()


def tiles_of(sizes, d):
    return torch.tensor([(b, i) for b, n in enumerate(sizes) for i in range((n + 31) // 32)], dtype=torch.int32).reshape(-1, 2).to(d)


def abi_call(c, d, split):
    """One recon_gcn_ragged_fwd + recon_gcn_ragged_bwd with buffers the test owns: ([out, g_x, g_adj, g_weight, g_bias], support, guards ok)."""
    from recon_amd import _lib
    L = _lib.lib()
    B, N, I, O, n_max = len(c.sizes), c.N, c.I, c.O, max(c.sizes)
    x, vals, w, G = c.x.to(d), c.values().to(d), c.w.to(d), c.G.to(d)
    b = c.b.to(d) if c.b is not None else None
    node = torch.from_numpy(c.node_ptr).to(torch.int32).to(d)
    adjp = torch.from_numpy(c.adj_ptr).to(d)
    tiles = tiles_of(c.sizes, d)
    assert L.recon_gcn_ragged_supported(B, N, n_max, I, O) == OK
    sup, out, g_sup, g_x, g_adj, g_w, g_b = (Guarded(n, d) for n in (N * O, N * O, N * O, N * I, vals.numel(), I * O, O))
    part = Guarded(L.recon_gcn_ragged_bwd_partial_floats(B, N, I, O), d)
    w_split = _lib.workspace(L.recon_gcn_split_bytes(I, O), d) if split else None
    gs_split = _lib.workspace(L.recon_gcn_bwd_split_bytes(1, N, O), d) if split else None
    st = _lib.current_stream()
    rc = L.recon_gcn_ragged_fwd(x.data_ptr(), I, vals.data_ptr(), w.data_ptr(), _lib.ptr(b), node.data_ptr(), adjp.data_ptr(), tiles.data_ptr(),
                                tiles.shape[0], B, N, n_max, I, O, sup.ptr(), out.ptr(), _lib.ptr(w_split), st)
    assert rc == OK, rc
    rc = L.recon_gcn_ragged_bwd(x.data_ptr(), I, vals.data_ptr(), w.data_ptr(), node.data_ptr(), adjp.data_ptr(), tiles.data_ptr(), tiles.shape[0],
                                B, N, n_max, I, O, sup.ptr(), out.ptr(), _lib.ptr(w_split), G.data_ptr(), g_sup.ptr(), part.ptr(), g_x.ptr(), g_adj.ptr(),
                                g_w.ptr(), g_b.ptr() if b is not None else None, _lib.ptr(gs_split), st)
    assert rc == OK, rc
    torch.cuda.synchronize()
    bufs = (sup, out, g_sup, g_x, g_adj, g_w, g_b, part)
    got = [out.t.view(N, O).clone(), g_x.t.view(N, I).clone(), g_adj.t.clone(), g_w.t.view(I, O).clone(), g_b.t.clone() if b is not None else None]
    return got, sup.t.clone(), g_sup.t.clone(), all(g.intact() for g in bufs)


@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_gcn_ragged_c_abi(shape, bias, gemm_family):
    """Every output inside a NaN-filled buffer behind a 37-element guard: written completely, the guards intact, inside the band, and two
    calls agree bit for bit."""
    c, d = R.case(*shape, bias), dev()
    split = gemm_family == "1"
    got, sup, g_sup, intact = abi_call(c, d, split)
    assert intact
    for t in got + [sup, g_sup]:
        assert t is None or not torch.isnan(t).any()
    bad = R.failures(c, got, d, "abi " + R.shape_id(shape))
    assert not bad, bad
    got2, sup2, g_sup2, intact2 = abi_call(c, d, split)
    assert intact2
    op_checks.same(got + [sup, g_sup], got2 + [sup2, g_sup2])


def test_gcn_ragged_status_codes():
    """Every status code of the four entries, each rejection before any launch (the outputs stay NaN), and B == 0 launches nothing."""
    from recon_amd import _lib
    L, d = _lib.lib(), dev()
    S = L.recon_gcn_ragged_supported
    assert S(3, 96, 33, 24, 16) == OK and S(0, 0, 0, 24, 16) == OK and S(65535, 65535, 1, 1, 1) == OK
    for bad in ((-1, 0, 0, 4, 4), (3, 96, 33, 0, 16), (3, 96, 33, 24, -1), (0, 5, 5, 4, 4), (3, 0, 0, 4, 4), (3, 96, 31, 24, 16), (3, 96, 97, 24, 16),
                (3, -1, 1, 4, 4)):
        assert S(*bad) == INVALID, bad
    for big in ((65536, 65536, 1, 4, 4), (65535, 2 ** 31, 40000, 4, 4), (2, 65535 * 32 + 2, 65535 * 32 + 1, 4, 4)):
        assert S(*big) == UNSUPPORTED, big
    P = L.recon_gcn_ragged_bwd_partial_floats
    assert P(0, 0, 4, 4) == 64 and P(3, 96, 24, 16) >= 24 * 16 + 3 * 16

    c = R.case((31, 32, 33), 24, 16, True)
    B, N, I, O, n_max = 3, c.N, c.I, c.O, 33
    x, vals, w, b, G = c.x.to(d), c.values().to(d), c.w.to(d), c.b.to(d), c.G.to(d)
    node, adjp = torch.from_numpy(c.node_ptr).to(torch.int32).to(d), torch.from_numpy(c.adj_ptr).to(d)
    tiles = tiles_of(c.sizes, d)
    sup, out, g_sup, g_x, part = (Guarded(n, d) for n in (N * O, N * O, N * O, N * I, P(B, N, I, O)))
    st = _lib.current_stream()

    def fwd(**k):
        a = dict(x=x.data_ptr(), ldx=I, adj=vals.data_ptr(), w=w.data_ptr(), bias=b.data_ptr(), node=node.data_ptr(), adjp=adjp.data_ptr(),
                 tiles=tiles.data_ptr(), n_tiles=tiles.shape[0], B=B, N=N, n_max=n_max, I=I, O=O, sup=sup.ptr(), out=out.ptr(), w_split=None)
        a.update(k)
        return L.recon_gcn_ragged_fwd(a["x"], a["ldx"], a["adj"], a["w"], a["bias"], a["node"], a["adjp"], a["tiles"], a["n_tiles"], a["B"], a["N"],
                                      a["n_max"], a["I"], a["O"], a["sup"], a["out"], a["w_split"], st)

    def bwd(**k):
        a = dict(x=x.data_ptr(), ldx=I, adj=vals.data_ptr(), w=w.data_ptr(), node=node.data_ptr(), adjp=adjp.data_ptr(), tiles=tiles.data_ptr(),
                 n_tiles=tiles.shape[0], B=B, N=N, n_max=n_max, I=I, O=O, sup=sup.ptr(), out=out.ptr(), w_split=None, gout=G.data_ptr(),
                 g_sup=g_sup.ptr(), part=part.ptr(), g_x=g_x.ptr())
        a.update(k)
        return L.recon_gcn_ragged_bwd(a["x"], a["ldx"], a["adj"], a["w"], a["node"], a["adjp"], a["tiles"], a["n_tiles"], a["B"], a["N"], a["n_max"],
                                      a["I"], a["O"], a["sup"], a["out"], a["w_split"], a["gout"], a["g_sup"], a["part"], a["g_x"], None, None, None,
                                      None, st)

    for key in ("x", "adj", "w", "node", "adjp", "tiles", "sup", "out"):
        assert fwd(**{key: None}) == INVALID, key
        assert bwd(**{key: None}) == INVALID, key
    for key in ("gout", "g_sup", "part"):
        assert bwd(**{key: None}) == INVALID, key
    for call in (fwd, bwd):
        assert call(I=0) == INVALID and call(O=-3) == INVALID and call(ldx=I - 1) == INVALID
        assert call(n_tiles=0) == INVALID and call(n_tiles=2) == INVALID and call(n_tiles=N // 32 + 4) == INVALID
        assert call(N=2 ** 31, B=65535, n_max=40000, n_tiles=2 ** 26) == UNSUPPORTED
        assert call(B=65536, N=65536, n_max=1, n_tiles=65536) == UNSUPPORTED
        assert call(B=0, N=0, n_max=0, n_tiles=0) == OK                       # no graphs: nothing is launched
    torch.cuda.synchronize()
    for g in (sup, out, g_sup, g_x, part):
        assert torch.isnan(g.buf).all()                                       # nothing above wrote anything
    assert fwd() == OK and bwd() == OK
    torch.cuda.synchronize()
    assert all(g.intact() for g in (sup, out, g_sup, g_x, part))
    assert not torch.isnan(out.t).any() and not torch.isnan(g_x.t).any()


# ------------------------------------------------------------------------------------------------- beside the other paths
@pytest.mark.parametrize("sizes, I, O_", (((3,) * 70, 24, 16), ((32,) * 4, 24, 16)), ids=("3x70", "32x4"))
def test_gcn_ragged_equal_sizes_beside_dense(sizes, I, O_):
    """Equal sizes also run as a dense [B, n, in] call: both results lie inside the band (equal bits are not asked for)."""
    c, d = R.case(sizes, I, O_, True), dev()
    bad = R.failures(c, run_layer(c, d), d, "ragged")
    assert not bad, bad
    layer = make_layer(c, d)
    B, n = len(sizes), sizes[0]
    x = c.x.to(d).view(B, n, I).requires_grad_(True)
    adj = torch.stack(c.mats).to(d).requires_grad_(True)
    out = layer(x, adj)
    (out * c.G.to(d).view(B, n, O_)).sum().backward()
    got = [out.detach().reshape(c.N, O_), x.grad.reshape(c.N, I), adj.grad.reshape(-1), layer.weight.grad, layer.bias.grad]
    bad = R.failures(c, got, d, "dense")
    assert not bad, bad


def test_gcn_ragged_strided_input_same_bits():
    """`input` as rows of 40 inside rows of 56 is read in place and gives the bits of the contiguous call."""
    c, d = R.case((5, 32, 17, 65, 100, 1, 33), 40, 136, True), dev()
    wide = torch.full((c.N, 56), float("nan"), device=d)
    wide[:, :40] = c.x.to(d)
    view = wide[:, :40]
    assert not view.is_contiguous()
    op_checks.same(run_layer(c, d, x=view), run_layer(c, d))


def test_gcn_ragged_repeated_backward_and_inplace_edit():
    """Any number of backwards per forward; an in-place edit of the result is caught (the tensor returned is the tensor saved)."""
    from recon_amd.gcn_layers import RaggedAdjacency
    c, d = R.case((31, 32, 33), 24, 16, True), dev()
    layer = make_layer(c, d)
    x = c.x.to(d).requires_grad_(True)
    rag = RaggedAdjacency(c.values().to(d).requires_grad_(True), c.sizes)
    out = layer(x, rag)
    loss = (out * c.G.to(d)).sum()
    params = [x, rag.values, layer.weight, layer.bias]
    g1 = torch.autograd.grad(loss, params, retain_graph=True)
    g2 = torch.autograd.grad(loss, params, retain_graph=True)
    op_checks.same(list(g1), list(g2))
    out.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.grad(loss, params)


def _stack(d, widths, seed):
    from recon_amd.gcn_layers import GraphConvolution
    torch.manual_seed(seed)
    return [GraphConvolution(i, o).to(d) for i, o in zip(widths[:-1], widths[1:])]


def test_gcn_ragged_stack_same_bits_as_loop():
    """gcn_stack over three float32 layers with a ragged batch: the bits of the layer loop, and a gradient for every parameter."""
    from recon_amd.gcn_layers import RaggedAdjacency, gcn_stack
    c, d = R.case((31, 32, 33), 24, 16, True), dev()
    layers = _stack(d, (24, 16, 16, 16), 3)
    res = []
    for run in (lambda x, a: gcn_stack(x, a, layers), lambda x, a: layers[2](layers[1](layers[0](x, a), a), a)):
        for l in layers:
            l.zero_grad()
        x = c.x.to(d).requires_grad_(True)
        rag = RaggedAdjacency(c.values().to(d).requires_grad_(True), c.sizes)
        out = run(x, rag)
        (out * c.G.to(d)).sum().backward()
        grads = [x.grad, rag.values.grad] + [p.grad.clone() for l in layers for p in l.parameters()]
        assert all(g is not None and torch.isfinite(g).all() for g in grads) and len(grads) == 8
        res.append([out.detach()] + grads)
    op_checks.same(res[0], res[1])


def test_gcn_ragged_three_layers_parity_bound():
    """Three stacked layers on [9, 16, 33] graphs at width 32 stay within 1e-4 absolute of the float64 forward: the parity bound."""
    from recon_amd.gcn_layers import RaggedAdjacency, gcn_stack
    c, d = R.case((9, 16, 33), 32, 32, True), dev()
    layers = _stack(d, (32, 32, 32, 32), 5)
    with torch.no_grad():
        out = gcn_stack(c.x.to(d), RaggedAdjacency(c.values().to(d), c.sizes), layers)
    h = c.x.double()
    for l in layers:
        w, b = l.weight.detach().cpu().double(), l.bias.detach().cpu().double()
        h = torch.cat([torch.relu(m.double() @ (h[r0:r0 + n] @ w) + b) for m, n, r0 in zip(c.mats, c.sizes, c.node_ptr[:-1])])
    err = (out.cpu().double() - h).abs().max().item()
    print("three layers: max abs err %.3e" % err)
    assert err <= 1e-4


@pytest.mark.parametrize("family", ("0", "1"), ids=("gemm_f32", "gemm_bx3"))
def test_gcn_ragged_both_gemm_families(family, monkeypatch):
    from recon_amd import gat_layers as _gl
    from recon_amd import _lib
    monkeypatch.setattr(_gl, "_GEMM_BX3", family)
    asked = op_checks.calls_of(monkeypatch, _lib, "workspace")
    c, d = R.case((31, 32, 33), 24, 16, True), dev()
    got = run_layer(c, d)
    assert len(asked) == (2 if family == "1" else 0)                          # the term planes of W and of g_support: only the split-precision form
    bad = R.failures(c, got, d, "family " + family)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------- rejections and neighbours
def test_gcn_ragged_rejections():
    from recon_amd import _lib
    from recon_amd.gcn_layers import GraphConvolution, RaggedAdjacency
    c, d = R.case((16, 15), 12, 65, True), dev()
    layer = make_layer(c, d)
    x, vals = c.x.to(d), c.values().to(d)
    with pytest.raises(TypeError, match="float32.*bfloat16"):
        layer(x, RaggedAdjacency(vals.to(torch.bfloat16), c.sizes))
    with pytest.raises(TypeError, match="bfloat16.*float32"):
        layer.to(torch.bfloat16)(x.to(torch.bfloat16), RaggedAdjacency(vals, c.sizes))
    layer = make_layer(c, d)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        make_layer(c, "cpu")(c.x, RaggedAdjacency(c.values(), c.sizes))
    with pytest.raises(ValueError):
        layer(x[:-1], RaggedAdjacency(vals, c.sizes))
    many = _lib.MAX_BATCH + 1
    with pytest.raises(NotImplementedError):
        GraphConvolution(2, 2).to(d)(torch.zeros(many, 2, device=d), RaggedAdjacency(torch.ones(many, device=d), [1] * many))


def test_gcn_ragged_empty_batch_launches_nothing(monkeypatch):
    from recon_amd import _lib
    from recon_amd.gcn_layers import GraphConvolution, RaggedAdjacency
    d = dev()
    layer = GraphConvolution(6, 4).to(d)
    x = torch.zeros(0, 6, device=d, requires_grad=True)
    rag = RaggedAdjacency(torch.zeros(0, device=d), [])
    real = _lib.lib()

    class NoLaunch:
        def __getattr__(self, name):
            if name in ("recon_gcn_ragged_fwd", "recon_gcn_ragged_bwd"):
                pytest.fail(name + " called for an empty batch")
            return getattr(real, name)
    monkeypatch.setattr(_lib, "lib", lambda: NoLaunch())
    out = layer(x, rag)
    assert out.shape == (0, 4) and out.dtype == torch.float32
    out.sum().backward()
    assert x.grad.shape == (0, 6) and not layer.weight.grad.any() and not layer.bias.grad.any()


def test_gcn_ragged_bf16_call_still_runs():
    """The bfloat16 ragged call on the same graphs, untouched: the float32 result rounded to bf16 precision."""
    from recon_amd.gcn_layers import RaggedAdjacency
    c, d = R.case((5, 32, 17, 65, 100, 1, 33), 40, 136, True), dev()
    ref = run_layer(c, d)[0]
    layer = make_layer(c, d).to(torch.bfloat16)
    out = layer(c.x.to(d).to(torch.bfloat16), RaggedAdjacency(c.values().to(d).to(torch.bfloat16), c.sizes))
    assert out.dtype == torch.bfloat16 and out.shape == ref.shape
    op_checks.close(out.float(), ref, atol=1e-3, rel_to_max=1.5e-2, what="bf16 ragged beside float32 ragged")
