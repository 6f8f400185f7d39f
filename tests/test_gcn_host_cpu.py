"""The host frame of recon_amd/gcn_layers.py, on tensor metadata alone (bf16 CPU tensors; no library, no device).

1. Row-stride rules: a table of views with the row stride (or None) that the two walkers this frame replaced gave for each — literals,
   produced by running those two functions on the same views, never recomputed from the code under test.
2. _padded_result / _grad_view: shape, strides, storage offset and tag of the inline code they replaced.
3. The plane cache: hit, miss, the `.data` blind spot and the invalidate call, the clear at 64 entries, the weight kept alive.
4. The forward body stores nothing on the context it is handed (the shared _NO_GRAD_CTX cannot be written to at all).
"""
import gc
import weakref

import pytest
import torch

from recon_amd import _lib
from recon_amd import gcn_layers as G

N, B = 3, 2
BF = torch.bfloat16


def _view(shape, ld, offset=0, last=1, lead_extra=0, lead1_stride=None):
    """A bf16 view of `shape` = [..., n, feat] over rows of stride ld; leading dims continue the row sequence unless told otherwise."""
    st, acc = [last], ld
    for d in reversed(shape[:-1]):
        st.append(acc)
        acc *= d
    st = list(reversed(st))
    if lead_extra:
        st[-3] += lead_extra
    if lead1_stride is not None:
        assert shape[0] == 1
        st[0] = lead1_stride
    need = offset + sum((s - 1) * k for s, k in zip(shape, st)) + 1
    return torch.zeros(need + 64, dtype=BF).as_strided(shape, st, offset)


def _table():
    rows = {}
    for feat in (6, 8, 22, 300):
        up = G._up8(feat)
        for kind, shape in (("2d", (N, feat)), ("3d", (B, N, feat)), ("4d", (1, B, N, feat))):
            for sname, ld in (("feat", feat), ("up8", up), ("up8+8", up + 8), ("feat+1", feat + 1), ("feat+2", feat + 2)):
                rows["%s f%d ld=%s" % (kind, feat, sname)] = (_view(shape, ld), feat)
        rows["3d f%d offset 1" % feat] = (_view((B, N, feat), up, offset=1), feat)
        rows["3d f%d offset 4" % feat] = (_view((B, N, feat), up, offset=4), feat)
        rows["3d f%d offset 8" % feat] = (_view((B, N, feat), up, offset=8), feat)
        rows["2d f%d last stride 2" % feat] = (_view((N, feat), 2 * up, last=2), feat)
        rows["3d f%d broken lead" % feat] = (_view((B, N, feat), up, lead_extra=8), feat)
        rows["4d f%d broken lead" % feat] = (_view((1, B, N, feat), up, lead_extra=up), feat)
        rows["4d f%d lead of 1, stride 12345" % feat] = (_view((1, B, N, feat), up, lead1_stride=12345), feat)
        rows["1d f%d" % feat] = (torch.zeros(feat, dtype=BF), feat)
    return rows


# name -> (MFMA rule with the tag, MFMA rule without the tag, MFMA rule with pads unread, masked rule): what
# (_rows_view(tagged t, feat), _rows_view(t, feat), _rows_view(t, feat, pads_read=False), _rows_in_place(t, feat)) returned before this frame
EXPECTED = {
    '2d f6 ld=feat': (None, None, None, 6),
    '2d f6 ld=up8': (8, None, 8, 8),
    '2d f6 ld=up8+8': (16, None, 16, 16),
    '2d f6 ld=feat+1': (None, None, None, None),
    '2d f6 ld=feat+2': (8, None, 8, 8),
    '3d f6 ld=feat': (None, None, None, 6),
    '3d f6 ld=up8': (8, None, 8, 8),
    '3d f6 ld=up8+8': (16, None, 16, 16),
    '3d f6 ld=feat+1': (None, None, None, None),
    '3d f6 ld=feat+2': (8, None, 8, 8),
    '4d f6 ld=feat': (None, None, None, 6),
    '4d f6 ld=up8': (8, None, 8, 8),
    '4d f6 ld=up8+8': (16, None, 16, 16),
    '4d f6 ld=feat+1': (None, None, None, None),
    '4d f6 ld=feat+2': (8, None, 8, 8),
    '3d f6 offset 1': (None, None, None, None),
    '3d f6 offset 4': (None, None, None, 8),
    '3d f6 offset 8': (8, None, 8, 8),
    '2d f6 last stride 2': (None, None, None, None),
    '3d f6 broken lead': (None, None, None, None),
    '4d f6 broken lead': (None, None, None, None),
    '4d f6 lead of 1, stride 12345': (8, None, 8, 8),
    '1d f6': (None, None, None, None),
    '2d f8 ld=feat': (8, 8, 8, 8),
    '2d f8 ld=up8': (8, 8, 8, 8),
    '2d f8 ld=up8+8': (16, 16, 16, 16),
    '2d f8 ld=feat+1': (None, None, None, None),
    '2d f8 ld=feat+2': (None, None, None, 10),
    '3d f8 ld=feat': (8, 8, 8, 8),
    '3d f8 ld=up8': (8, 8, 8, 8),
    '3d f8 ld=up8+8': (16, 16, 16, 16),
    '3d f8 ld=feat+1': (None, None, None, None),
    '3d f8 ld=feat+2': (None, None, None, 10),
    '4d f8 ld=feat': (8, 8, 8, 8),
    '4d f8 ld=up8': (8, 8, 8, 8),
    '4d f8 ld=up8+8': (16, 16, 16, 16),
    '4d f8 ld=feat+1': (None, None, None, None),
    '4d f8 ld=feat+2': (None, None, None, 10),
    '3d f8 offset 1': (None, None, None, None),
    '3d f8 offset 4': (None, None, None, 8),
    '3d f8 offset 8': (8, 8, 8, 8),
    '2d f8 last stride 2': (None, None, None, None),
    '3d f8 broken lead': (None, None, None, None),
    '4d f8 broken lead': (None, None, None, None),
    '4d f8 lead of 1, stride 12345': (8, 8, 8, 8),
    '1d f8': (None, None, None, None),
    '2d f22 ld=feat': (None, None, None, 22),
    '2d f22 ld=up8': (24, None, 24, 24),
    '2d f22 ld=up8+8': (32, None, 32, 32),
    '2d f22 ld=feat+1': (None, None, None, None),
    '2d f22 ld=feat+2': (24, None, 24, 24),
    '3d f22 ld=feat': (None, None, None, 22),
    '3d f22 ld=up8': (24, None, 24, 24),
    '3d f22 ld=up8+8': (32, None, 32, 32),
    '3d f22 ld=feat+1': (None, None, None, None),
    '3d f22 ld=feat+2': (24, None, 24, 24),
    '4d f22 ld=feat': (None, None, None, 22),
    '4d f22 ld=up8': (24, None, 24, 24),
    '4d f22 ld=up8+8': (32, None, 32, 32),
    '4d f22 ld=feat+1': (None, None, None, None),
    '4d f22 ld=feat+2': (24, None, 24, 24),
    '3d f22 offset 1': (None, None, None, None),
    '3d f22 offset 4': (None, None, None, 24),
    '3d f22 offset 8': (24, None, 24, 24),
    '2d f22 last stride 2': (None, None, None, None),
    '3d f22 broken lead': (None, None, None, None),
    '4d f22 broken lead': (None, None, None, None),
    '4d f22 lead of 1, stride 12345': (24, None, 24, 24),
    '1d f22': (None, None, None, None),
    '2d f300 ld=feat': (None, None, None, 300),
    '2d f300 ld=up8': (304, None, 304, 304),
    '2d f300 ld=up8+8': (312, None, 312, 312),
    '2d f300 ld=feat+1': (None, None, None, None),
    '2d f300 ld=feat+2': (None, None, None, 302),
    '3d f300 ld=feat': (None, None, None, 300),
    '3d f300 ld=up8': (304, None, 304, 304),
    '3d f300 ld=up8+8': (312, None, 312, 312),
    '3d f300 ld=feat+1': (None, None, None, None),
    '3d f300 ld=feat+2': (None, None, None, 302),
    '4d f300 ld=feat': (None, None, None, 300),
    '4d f300 ld=up8': (304, None, 304, 304),
    '4d f300 ld=up8+8': (312, None, 312, 312),
    '4d f300 ld=feat+1': (None, None, None, None),
    '4d f300 ld=feat+2': (None, None, None, 302),
    '3d f300 offset 1': (None, None, None, None),
    '3d f300 offset 4': (None, None, None, 304),
    '3d f300 offset 8': (304, None, 304, 304),
    '2d f300 last stride 2': (None, None, None, None),
    '3d f300 broken lead': (None, None, None, None),
    '4d f300 broken lead': (None, None, None, None),
    '4d f300 lead of 1, stride 12345': (304, None, 304, 304),
    '1d f300': (None, None, None, None),
}


def _tagged(t):
    u = t.as_strided(t.shape, t.stride(), t.storage_offset())
    u._recon_padded = True
    return u


def test_row_stride_table_is_complete():
    assert sorted(_table()) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_row_stride_rules(name):
    t, feat = _table()[name]
    want = EXPECTED[name]
    got = (G._rows_view(_tagged(t), feat), G._rows_view(t, feat), G._rows_view(t, feat, pads_read=False), G._row_stride(t, feat, G._MASKED))
    assert got == want
    assert (G._row_stride(_tagged(t), feat, G._MFMA), G._row_stride(t, feat, G._MFMA), G._row_stride(t, feat, G._MFMA_UNREAD),
            G._row_stride(t, feat, G._MASKED)) == want
    # the tag only matters where the pad columns are read
    assert G._rows_view(_tagged(t), feat, pads_read=False) == want[2] and G._row_stride(_tagged(t), feat, G._MASKED) == want[3]


def test_rows_or_packed_and_grad_rows():
    t = _view((B, N, 22), 24)
    assert G._rows_or_packed(t, 22, G._MFMA, True)[0].shape == (B * N, 24)            # untagged: repacked, pads zeroed
    u = _tagged(t)
    r, ld = G._rows_or_packed(u, 22, G._MFMA, True)
    assert r is u and ld == 24
    r, ld = G._rows_or_packed(t, 22, G._MFMA_UNREAD, False)
    assert r is t and ld == 24
    g32 = torch.ones(B, N, 22)                                                          # fp32, contiguous, odd multiple of 2: cast, then masked in place
    r, ld = G._grad_rows(g32, 22, G._MASKED)
    assert r.dtype == BF and ld == 22 and r.shape == (B, N, 22)
    r, ld = G._grad_rows(g32, 22, G._MFMA_UNREAD)
    assert r.dtype == BF and ld == 24 and r.shape == (B * N, 24) and bool((r[:, :22] == 1).all())
    nc = torch.ones(B, 22, N, dtype=BF).transpose(1, 2)                                 # non-contiguous gradient
    r, ld = G._grad_rows(nc, 22, G._MASKED)
    assert ld == 24 and r.shape == (B * N, 24)


def _inline_result(out_p, lead, feat, ld):
    """What the four forwards spelled out before _padded_result."""
    if ld == feat:
        return out_p.view(lead + (feat,))
    out = out_p.as_strided(lead + (feat,), G._strides(lead, ld), out_p.storage_offset())
    out._recon_padded = True
    return out


def _inline_grad(g, shape, feat, ld):
    return g.view(shape) if ld == feat else g.as_strided(shape, G._strides(shape[:-1], ld))


def _same_view(a, b):
    return (a.shape == b.shape and a.stride() == b.stride() and a.storage_offset() == b.storage_offset() and a.data_ptr() == b.data_ptr()
            and getattr(a, "_recon_padded", False) == getattr(b, "_recon_padded", False))


@pytest.mark.parametrize("lead", [(N,), (B, N), (2, B, N)])
@pytest.mark.parametrize("feat,ld", [(8, 8), (24, 24), (6, 8), (22, 24), (300, 304)])
@pytest.mark.parametrize("layer", [0, 2])
def test_padded_result_and_grad_view(lead, feat, ld, layer):
    rows = 1
    for d in lead:
        rows *= d
    acts = torch.ones(3, rows, ld, dtype=BF)
    out_p = acts[layer]                                          # layer 2: a non-zero storage offset, the stack's last layer
    assert (out_p.storage_offset() != 0) == (layer == 2)
    want = _inline_result(out_p, lead, feat, ld)
    got = G._padded_result(out_p, lead, feat, ld, zero_tail=False)
    assert _same_view(got, want) and tuple(got.shape) == lead + (feat,)
    assert getattr(got, "_recon_padded", False) == (feat < ld)
    assert bool((out_p == 1).all())                              # zero_tail=False leaves the pad columns alone
    got = G._padded_result(out_p, lead, feat, ld, zero_tail=True)
    assert _same_view(got, want) and bool((out_p[:, :feat] == 1).all()) and bool((out_p[:, feat:] == 0).all())
    assert bool((acts[1] == 1).all())
    shape = lead + (feat,)
    g = G._grad_view(out_p, shape, feat, ld)
    assert _same_view(g, _inline_grad(out_p, shape, feat, ld)) and not hasattr(g, "_recon_padded")
    assert G._grad_view(None, shape, feat, ld) is None


def _keep_planes(c, w, planes):
    """What a forward does on a miss: look up, then insert under the key the look-up built."""
    key, hit = c.find(w, w.shape[0], w.shape[1], w.device)
    assert hit is None
    c.put(key, planes, w)


def _kept(c, w):
    return c.find(w, w.shape[0], w.shape[1], w.device)[1]


def test_plane_cache_hit_miss_and_the_data_blind_spot():
    c = G._PlaneCache()
    w = torch.ones(6, 4, dtype=BF)
    planes = torch.zeros(16, dtype=torch.uint8)
    _keep_planes(c, w, planes)
    assert _kept(c, w) is planes                                 # same (data_ptr, _version): hit
    assert _kept(c, torch.ones(6, 4, dtype=BF)) is None          # another tensor
    w.data.add_(1)                                               # autograd's version counter does not see a write through .data
    assert _kept(c, w) is planes
    c.drop(w)                                                    # ... which is what the invalidate call is for
    assert _kept(c, w) is None
    _keep_planes(c, w, planes)
    w.add_(1)                                                    # through the tensor: the version moves, the key misses
    assert _kept(c, w) is None


def test_plane_cache_is_emptied_by_the_insertion_that_finds_64_entries():
    c = G._PlaneCache()
    ws = [torch.ones(2, 2, dtype=BF) for _ in range(65)]
    for i, w in enumerate(ws[:64]):
        _keep_planes(c, w, i)
    assert len(c) == 64 and _kept(c, ws[0]) == 0 and _kept(c, ws[63]) == 63
    _keep_planes(c, ws[64], 64)
    assert len(c) == 1 and _kept(c, ws[64]) == 64 and _kept(c, ws[0]) is None


def test_plane_cache_keeps_its_weight_alive():
    c = G._PlaneCache()
    w = torch.ones(2, 2, dtype=BF)
    ref = weakref.ref(w)
    _keep_planes(c, w, None)
    del w
    gc.collect()
    assert ref() is not None                                     # its data_ptr is the key: the address must not be reused while the entry lives
    c.clear()
    gc.collect()
    assert ref() is None


def test_invalidating_one_layer_leaves_the_other_and_the_stack_cache(monkeypatch):
    monkeypatch.setattr(G, "_PLANES", G._PlaneCache())
    monkeypatch.setattr(G, "_STACK_PLANES", G._PlaneCache())
    a, b = G.GraphConvolution(6, 4).to(BF), G.GraphConvolution(6, 4).to(BF)
    for l in (a, b):
        _keep_planes(G._PLANES, l.weight, l)
        _keep_planes(G._STACK_PLANES, l.weight, l)
    a.invalidate_planes()
    assert [v[0] for v in G._PLANES.values()] == [b]
    assert len(G._STACK_PLANES) == 2                             # the layer's call leaves what gcn_stack() keeps ...
    G.invalidate_stack_planes()
    assert len(G._STACK_PLANES) == 0 and len(G._PLANES) == 1     # ... and the stack's call leaves the layers'
    b.reset_parameters()                                         # reset_parameters, load_state_dict and _apply call invalidate_planes
    assert len(G._PLANES) == 0
    _keep_planes(G._PLANES, a.weight, a)
    a.load_state_dict(a.state_dict())
    assert len(G._PLANES) == 0
    _keep_planes(G._PLANES, a.weight, a)
    a.float()
    assert len(G._PLANES) == 0


class _StubLib:
    """Stands in for the ctypes handle: sizes answered, launches recorded and answered with 0."""

    def __init__(self):
        self.calls = []

    def recon_gcn_b16_planes_bytes(self, I, O):
        return 256

    def recon_gcn_b16_fwd(self, args, stream):
        a = args._obj
        self.calls.append({f: getattr(a, f) for f, _ in a._fields_})
        return 0


class _ReadOnlyCtx:
    needs_input_grad = (False, False, False, False, False)

    def __setattr__(self, name, value):
        raise AssertionError("the forward body wrote ctx.%s" % name)

    def save_for_backward(self, *tensors):
        raise AssertionError("the forward body called ctx.save_for_backward")


def test_forward_body_returns_what_is_to_be_saved_and_leaves_ctx_alone(monkeypatch):
    stub = _StubLib()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    monkeypatch.setattr(_lib, "current_stream", lambda: 0)
    monkeypatch.setattr(G, "_PLANES", G._PlaneCache())
    x, adj = torch.ones(B, N, 6, dtype=BF), torch.ones(B, N, N, dtype=BF)
    w, b = torch.ones(6, 22, dtype=BF), torch.ones(22, dtype=BF)
    geo = (B * N, B, N, None, (B, N), (B, N, N), (B, N, 0), "")
    for ctx in (_ReadOnlyCtx(), G._NO_GRAD_CTX):
        out, saved, meta = G._b16_forward(ctx, geo, x, adj, w, b, True)
        assert tuple(out.shape) == (B, N, 22) and out.stride() == (N * 24, 24, 1) and out._recon_padded
        assert len(saved) == 7 and saved[0] is x and saved[4] is None and saved[5].shape == (B * N, 24)      # fused: no `support`
        assert meta == (geo, 6, 22, 6, 24)                       # contiguous even rows, read in place under no_grad: ldx = 6
    assert not hasattr(G._NO_GRAD_CTX, "__dict__") and not hasattr(G._NO_GRAD_CTX, "meta")
    with pytest.raises(AttributeError):
        G._NO_GRAD_CTX.meta = 1
    first, second = stub.calls
    assert first["w_planes_valid"] == 0 and second["w_planes_valid"] == 1 and first["w_planes"] == second["w_planes"]      # the cache hit
    assert (first["B"], first["n"], first["in_features"], first["out_features"], first["ldx"], first["lds"], first["ldo"]) == (B, N, 6, 22, 6, 24, 24)
    assert first["support"] is None and first["node_ptr"] is None and first["adj_ptr"] is None and first["total_rows"] == 0
    assert first["x"] == x.data_ptr() and first["adj"] == adj.data_ptr() and first["weight"] == w.data_ptr() and first["bias"] == b.data_ptr()
