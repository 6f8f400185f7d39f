"""The stage-A tail kernels on the GPU against float64: csrc/norm.hip (recon_rows_normalize_fwd / _bwd, models._SkipMaskNormalize,
models.normalize_rows_), csrc/loss.hip (recon_transe_margin_fwd / _fwd_keys / _bwd, losses.batch_gat_loss), csrc/rel_mm.hip
(recon_rel_rows_mm / _wgrad, sep_space.rel_rows_mm), and SpKBGATModified on a batch from which no edge survives the dead-row pruning.

Shapes, inputs, float64 references, bands and checks are those of tests/stage_a_tail_checks.py, which tests/test_stage_a_tail_cpu.py guards;
here `Abi` drives the C entry points with every output inside a NaN-filled buffer.  The chain behind every band is the stock fp32 torch
lines on the GPU.  The worst error / bound ratios measured on an MI355X are in DESIGN.md section 29."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stage_a_tail_checks as sa
from op_checks import bound, calls_of, dev
from stage_a_tail_checks import INVALID, OK, UNSUPPORTED, f32

pytestmark = pytest.mark.gpu


class Abi:
    """The C ABI as a backend of stage_a_tail_checks: inputs are copied to the device, every output is a Guarded buffer copied there and back."""

    def __init__(self):
        from recon_amd import _lib
        self.device, self.lib, self.stream = dev(), _lib.lib(), _lib.current_stream

    def _in(self, a, misaligned=False):
        if a is None:
            return None, None
        t = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        if misaligned:                                                  # a view one float into a larger buffer: 4-byte aligned only
            buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=self.device)
            buf[1:1 + t.numel()] = t.reshape(-1)
            t = buf[1:1 + t.numel()]
            assert t.data_ptr() % 16 == 4
        return t, t.data_ptr()

    def _out(self, g):
        if g is None:
            return None, None
        t = torch.from_numpy(g.buf).to(self.device)
        assert t.data_ptr() % 16 == 0
        return t, t.data_ptr() + g.off * g.dtype.itemsize

    @staticmethod
    def _back(rc, *pairs):
        for g, t in pairs:
            if g is not None:
                g.buf[:] = t.cpu().numpy()
        return rc

    def norm_fwd(self, ew, skip, mask, N, C, eps, y, norm):
        (yt, yp), (nt, npt) = self._out(y), self._out(norm)
        (_e, ep), (_s, sp), (_m, mp) = self._in(ew), self._in(skip), self._in(mask)
        rc = self.lib.recon_rows_normalize_fwd(yp if ew is None else ep, sp, mp, N, C, eps, yp, npt, self.stream())
        return self._back(rc, (y, yt), (norm, nt))

    def norm_bwd(self, gy, y, norm, mask, N, C, eps, gt, gskip):
        (tt, tp), (st, sp) = self._out(gt), self._out(gskip)
        (_a, gp), (_b, yp), (_c, np_), (_d, mp) = self._in(gy), self._in(y), self._in(norm), self._in(mask)
        rc = self.lib.recon_rows_normalize_bwd(gp, yp, np_, mp, N, C, eps, tp, sp, self.stream())
        return self._back(rc, (gt, tt), (gskip, st))

    def margin_fwd(self, ent, rel, tri, n_pos, reps, D, margin, terms, loss, ent_key, rel_key, misaligned=False):
        (tt, tp), (lt, lp), (et, ekp), (rt, rkp) = self._out(terms), self._out(loss), self._out(ent_key), self._out(rel_key)
        (_e, ep), (_r, rp), (_t, trp) = self._in(ent, misaligned), self._in(rel, misaligned), self._in(tri)
        rc = self.lib.recon_transe_margin_fwd(ep, rp, trp, n_pos, reps, D, float(margin), tp, lp, ekp, rkp, None, self.stream())
        return self._back(rc, (terms, tt), (loss, lt), (ent_key, et), (rel_key, rt))

    def margin_fwd_keys(self, ent, rel, tri, n_pos, reps, D, margin, terms, loss, keys, n_entities, misaligned=False):
        (tt, tp), (lt, lp), (kt, kp) = self._out(terms), self._out(loss), self._out(keys)
        (_e, ep), (_r, rp), (_t, trp) = self._in(ent, misaligned), self._in(rel, misaligned), self._in(tri)
        rc = self.lib.recon_transe_margin_fwd_keys(ep, rp, trp, n_pos, reps, D, float(margin), tp, lp, kp, n_entities, self.stream())
        return self._back(rc, (terms, tt), (loss, lt), (keys, kt))

    def margin_bwd(self, ent, rel, tri, n_pos, reps, D, terms, g, rows, misaligned=False):
        (rt, rp_) = self._out(rows)
        (_e, ep), (_r, rp), (_t, trp), (_m, tp) = self._in(ent, misaligned), self._in(rel, misaligned), self._in(tri), self._in(terms)
        _g, gp = self._in(None if g is None else np.array([g], f32))
        gr = None if rp_ is None else rp_ + 4 * (4 * n_pos * reps * D)
        rc = self.lib.recon_transe_margin_bwd(ep, rp, trp, n_pos, reps, D, tp, gp, rp_, gr, self.stream())
        return self._back(rc, (rows, rt))

    def rel_mm(self, x, order, rel, W, T, IN, OUT, trans, out):
        (ot, op) = self._out(out)
        (_x, xp), (_o, orp), (_r, rp), (_w, wp) = self._in(x), self._in(order), self._in(rel), self._in(W)
        rc = self.lib.recon_rel_rows_mm(xp, orp, rp, wp, T, IN, OUT, trans, op, self.stream())
        return self._back(rc, (out, ot))

    def rel_wgrad(self, x, g, order, seg, R, D, OUT, gW):
        (wt, wp) = self._out(gW)
        (_x, xp), (_g, gp), (_o, orp), (_s, sp) = self._in(x), self._in(g), self._in(order), self._in(seg)
        rc = self.lib.recon_rel_rows_mm_wgrad(xp, gp, orp, sp, R, D, OUT, wp, self.stream())
        return self._back(rc, (gW, wt))


def T(a, **kw):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev(), **kw)


# ============================================================================================================= 1. norm.hip
@pytest.mark.parametrize("form", sa.NORM_FORMS)
@pytest.mark.parametrize("N,C", sa.NORM_SHAPES)
def test_rows_normalize_through_the_c_abi(N, C, form):
    assert sa.norm_failures(Abi(), N, C, form) == []


@pytest.mark.parametrize("N,C", sa.NORM_SHAPES)
def test_the_python_entry_points_give_the_c_abis_bits(N, C):
    from recon_amd import models
    c = sa.norm_case(N, C, "skip_mask")
    (y, _, g_t, g_skip), rc, _ = sa.norm_run(Abi(), c)
    assert rc == [OK, OK]
    ew, skip = T(c["ew"]).requires_grad_(True), T(c["skip"]).requires_grad_(True)
    out = models._SkipMaskNormalize.apply(ew, skip, T(c["mask"]))
    a, b = torch.autograd.grad(out, [ew, skip], T(c["gy"]))
    assert sa.bits_equal(out.detach().cpu().numpy(), y) and sa.bits_equal(a.cpu().numpy(), g_t) and sa.bits_equal(b.cpu().numpy(), g_skip)
    only_ew = torch.autograd.grad(models._SkipMaskNormalize.apply(ew, skip.detach(), T(c["mask"])), [ew], T(c["gy"]))[0]       # g_skip == null
    assert torch.equal(only_ew, a)
    p = sa.norm_case(N, C, "plain")
    (y_plain, _, _, _), rc, _ = sa.norm_run(Abi(), p)
    t = T(p["ew"])
    assert models.normalize_rows_(t) is t and sa.bits_equal(t.cpu().numpy(), y_plain)


def test_normalize_rows_takes_f_normalize_for_a_view_and_a_cpu_tensor(monkeypatch):
    from recon_amd import _lib, models
    c = sa.norm_case(9, 37, "plain")
    want = F.normalize(T(c["ew"]), p=2, dim=1)
    lib_calls = calls_of(monkeypatch, _lib, "lib")
    wide = torch.zeros(9, 45, device=dev())
    wide[:, 4:41] = T(c["ew"])
    view = wide[:, 4:41]
    assert not view.is_contiguous()
    assert models.normalize_rows_(view) is view and torch.equal(view, want) and not wide[:, :4].any() and not wide[:, 41:].any()
    cpu = torch.from_numpy(c["ew"].copy())
    assert models.normalize_rows_(cpu) is cpu and torch.equal(cpu, F.normalize(torch.from_numpy(c["ew"]), p=2, dim=1))
    assert not lib_calls                                                # neither went to the kernel


def test_rows_normalize_rejections_launch_nothing():
    be = Abi()
    lib, s = be.lib, be.stream()
    buf = torch.full((64,), 7.0, device=dev())
    p = buf.data_ptr()
    for N, C, eps in ((-1, 4, 1e-12), (2, 0, 1e-12), (2, -3, 1e-12), (2, 4, 0.0), (2, 4, -1e-12)):
        assert lib.recon_rows_normalize_fwd(p, None, None, N, C, eps, p + 128, None, s) == INVALID
        assert lib.recon_rows_normalize_bwd(p, p, p, None, N, C, eps, p + 128, None, s) == INVALID
    assert lib.recon_rows_normalize_fwd(None, None, None, 2, 4, 1e-12, p, None, s) == INVALID              # ew
    assert lib.recon_rows_normalize_fwd(p, None, None, 2, 4, 1e-12, None, None, s) == INVALID              # y
    for args in ((None, p, p, None), (p, None, p, None), (p, p, None, None)):                              # g_y, y, norm
        assert lib.recon_rows_normalize_bwd(*args, 2, 4, 1e-12, p + 128, None, s) == INVALID
    assert lib.recon_rows_normalize_bwd(p, p, p, None, 2, 4, 1e-12, None, None, s) == INVALID              # g_t
    assert lib.recon_rows_normalize_fwd(None, None, None, 0, 4, 1e-12, None, None, s) == OK                # N == 0: nothing to do
    assert lib.recon_rows_normalize_bwd(None, None, None, None, 0, 4, 1e-12, None, None, s) == OK
    assert bool((buf == 7.0).all())


def test_a_non_finite_skip_row_is_dropped_under_mask_zero_and_spread_otherwise():
    """What the code does, and where it leaves the reference: `0 * out_entity` would turn a NaN skip row into a NaN output row; the
    kernel's mask == 0 branch (like the dead-row pruning in front of it) never reads that row."""
    from recon_amd import models
    c = sa.norm_case(9, 37, "skip_mask")
    skip, mask = c["skip"].copy(), c["mask"].copy()
    assert mask[4] == 0 and mask[1] != 0
    skip[4], skip[1] = np.nan, np.nan
    y = models._SkipMaskNormalize.apply(T(c["ew"]), T(skip), T(mask)).cpu().numpy()
    want = F.normalize(torch.from_numpy(c["ew"][4:5]).double(), p=2, dim=1).numpy()
    assert np.isfinite(y[4]).all() and np.abs(y[4] - want[0]).max() <= 2e-5 * np.abs(want).max()
    assert np.isnan(y[1]).all()
    rest = [r for r in range(9) if r not in (1, 4)]
    assert sa.row_errors(y[rest], c["ref"][0][rest])[0] <= 2e-5
    stock = F.normalize(T(c["ew"]) + T(mask).unsqueeze(-1) * T(skip), p=2, dim=1)
    assert torch.isnan(stock[4]).all()                                  # the reference's lines spread it


# ============================================================================================================= 2. loss.hip
@pytest.mark.parametrize("D,mis", sa.MARGIN_WIDTHS)
def test_transe_margin_through_the_c_abi(D, mis):
    for n_pos, reps in sa.MARGIN_PAIRS:
        assert sa.margin_failures(Abi(), sa.margin_case(D, n_pos, reps, mis)) == []


def test_transe_margin_propagates_nan():
    from recon_amd.gat_layers import nan_raised
    nan_raised(dev())                                                   # enables the device's NaN word and clears it
    assert sa.margin_nan_failures(Abi()) == []
    assert nan_raised(dev())                                            # raised by the kernel, and cleared again for whoever reads it next


def test_aligned_and_misaligned_tables_agree_within_the_band():
    be = Abi()
    for n_pos, reps in sa.MARGIN_PAIRS:
        a, m = sa.margin_case(200, n_pos, reps, False), sa.margin_case(200, n_pos, reps, True)
        ta, tm = sa.margin_run(be, a)[0]["joint"][0], sa.margin_run(be, m)[0]["joint"][0]
        chain = sa.margin_ref(a["ent"], a["rel"], a["tri"], n_pos, reps, a["margin"], torch.float32, dev())["terms"]
        scale = sa.margin_scale(a["ref"], a["margin"])
        e_chain = float(np.abs(chain.astype(np.float64) - a["ref"]["terms"]).max()) / scale
        diff = float(np.abs(ta.astype(np.float64) - tm).max()) / scale
        print("D200 %dx%d aligned against misaligned: %.3e of the scale, bound %.3e" % (n_pos, reps, diff, bound(e_chain)))
        assert diff <= bound(e_chain)


@pytest.mark.parametrize("D,mis", sa.MARGIN_WIDTHS)
def test_batch_gat_loss_table_gradients(D, mis, monkeypatch):
    """losses.batch_gat_loss with a MarginRankingLoss (the kernels; entity-only and relation-only take the separate-key form) against float64
    autograd, the band from the op-sequence fallback on the same inputs; upstream gradient 1.5."""
    from recon_amd import losses
    be = Abi()
    fused = calls_of(monkeypatch, losses._TransEMarginLoss, "apply")
    bad = []
    for n_pos, reps in ((5, 2), (67, 4)):
        c = sa.margin_case(D, n_pos, reps, mis)
        margin, tri = float(c["margin"]), T(c["tri"])
        e64, r64 = torch.from_numpy(c["ent"]).double().requires_grad_(True), torch.from_numpy(c["rel"]).double().requires_grad_(True)
        t64 = torch.from_numpy(c["tri"])
        pos, neg = t64[:n_pos].repeat(reps, 1), t64[n_pos:]
        pn = torch.norm(e64[pos[:, 0]] + r64[pos[:, 1]] - e64[pos[:, 2]], p=1, dim=1)
        nn = torch.norm(e64[neg[:, 0]] + r64[neg[:, 1]] - e64[neg[:, 2]], p=1, dim=1)
        loss64 = F.margin_ranking_loss(pn, nn, -torch.ones(n_pos * reps, dtype=torch.float64), margin=margin)
        ref = [a.numpy() for a in torch.autograd.grad(loss64 * 1.5, [e64, r64])]
        l64 = loss64.item()
        scale = sa.margin_scale(c["ref"], c["margin"])

        def run(loss_fn, want_e, want_r):
            ent, rel = be._in(c["ent"], mis)[0].view(sa.N_ENT, D).requires_grad_(want_e), be._in(c["rel"], mis)[0].view(sa.N_REL, D).requires_grad_(want_r)
            loss = losses.batch_gat_loss(loss_fn, tri, ent, rel, valid_invalid_ratio_gat=reps // 2)
            (loss * 1.5).backward()
            return loss.detach().item(), (ent.grad.cpu().numpy() if want_e else None), (rel.grad.cpu().numpy() if want_r else None)
        stock = lambda a, b, y: F.margin_ranking_loss(a, b, y, margin=margin)
        del fused[:]
        chain = run(stock, True, True)
        assert not fused                                                # any other loss function takes the op sequence
        for want_e, want_r in ((True, True), (True, False), (False, True)):
            del fused[:]
            got = run(torch.nn.MarginRankingLoss(margin=margin), want_e, want_r)
            assert len(fused) == 1
            label = "D%d%s %dx%d grads %s%s" % (D, "m" if mis else "", n_pos, reps, "e" if want_e else "", "r" if want_r else "")
            sa._band("margin", "batch_gat_loss", label, abs(got[0] - l64) / scale, abs(chain[0] - l64) / scale, bad)
            for what, f, ch, r in zip(("g_entity", "g_relation"), got[1:], chain[1:], ref):
                if f is not None:
                    e = lambda a: float(np.abs(a.astype(np.float64) - r).max() / np.abs(r).max())
                    sa._band("margin", what, label, e(f), e(ch), bad)
    assert bad == []


def test_a_pre_clamp_value_of_exactly_zero():
    """The documented deviation (csrc/kg_sep.hip, csrc/loss.hip): a pair whose pn - nn + margin is exactly 0 is inactive on the fused path;
    torch's clamp_min backward, and so the op-sequence fallback, passes its gradient.  Integer tables: every sum is exact."""
    from recon_amd import losses
    c = sa.zero_case()

    def grads(loss_fn):
        ent, rel = T(c["ent"]).requires_grad_(True), T(c["rel"]).requires_grad_(True)
        loss = losses.batch_gat_loss(loss_fn, T(c["tri"]), ent, rel, valid_invalid_ratio_gat=1)
        loss.backward()
        return loss.item(), ent.grad.cpu().numpy(), rel.grad.cpu().numpy()

    def expected(active):                                               # float64, pair by pair
        ge, gr = np.zeros((5, 4)), np.zeros((2, 4))
        for j in active:
            for (h, r, t), sgn in ((c["tri"][j % 3], 1.0), (c["tri"][3 + j], -1.0)):
                s = sgn * np.sign(c["ent"][h].astype(np.float64) + c["rel"][r] - c["ent"][t]) / 6.0
                ge[h] += s
                ge[t] -= s
                gr[r] += s
        return ge, gr
    fused = grads(torch.nn.MarginRankingLoss(margin=1.0))
    stock = grads(lambda a, b, y: F.margin_ranking_loss(a, b, y, margin=1.0))
    assert fused[0] == stock[0] == np.float32(2.0) / np.float32(6.0)
    for got, active in ((fused, [1]), (stock, [0, 1])):
        for a, want in zip(got[1:], expected(active)):
            assert np.abs(a - want).max() <= 1e-6
    assert np.abs(expected([1])[0] - expected([0, 1])[0]).max() >= 0.16  # the two rules differ here, and only through pair 0


def test_transe_margin_rejections_launch_nothing():
    be = Abi()
    lib, s = be.lib, be.stream()
    buf = torch.full((256,), 7.0, device=dev())
    tri = torch.zeros(64, 3, dtype=torch.int64, device=dev())
    e, r, t, o = buf.data_ptr(), buf.data_ptr() + 256, tri.data_ptr(), buf.data_ptr() + 512
    fwd = lambda ent, rel, tr, n_pos, reps, D, terms, loss: lib.recon_transe_margin_fwd(ent, rel, tr, n_pos, reps, D, 1.0, terms, loss, None, None, None, s)
    keys = lambda ent, rel, tr, n_pos, reps, D, terms, loss, k, n: lib.recon_transe_margin_fwd_keys(ent, rel, tr, n_pos, reps, D, 1.0, terms, loss, k, n, s)
    bwd = lambda ent, rel, tr, n_pos, reps, D, terms, g, ge, gr: lib.recon_transe_margin_bwd(ent, rel, tr, n_pos, reps, D, terms, g, ge, gr, s)
    for n_pos, reps, D in ((0, 2, 4), (2, 0, 4), (2, -1, 4), (2, 2, 0), (2, 2, -4), (-2, 2, 4)):
        assert fwd(e, r, t, n_pos, reps, D, o, o + 64) == INVALID
        assert keys(e, r, t, n_pos, reps, D, o, o + 64, t, 4) == INVALID
        assert bwd(e, r, t, n_pos, reps, D, o, o + 64, o + 128, o + 256) == INVALID
    for i in range(5):                                                  # a null entity / relation / triples / terms / loss
        a = [e, r, t, 2, 2, 4, o, o + 64]
        a[i if i < 3 else i + 3] = None
        assert fwd(*a) == INVALID and keys(*a, t, 4) == INVALID
    assert keys(e, r, t, 2, 2, 4, o, o + 64, None, 4) == INVALID and keys(e, r, t, 2, 2, 4, o, o + 64, t, 0) == INVALID
    for i in (0, 1, 2, 6, 7, 8, 9):
        a = [e, r, t, 2, 2, 4, o, o + 64, o + 128, o + 256]
        a[i] = None
        assert bwd(*a) == INVALID
    # more pairs than an entry point takes: checked in front of the launch, so small real buffers do
    assert fwd(e, r, t, 1 << 31, 1, 4, o, o + 64) == UNSUPPORTED and fwd(e, r, t, 1 << 29, 4, 4, o, o + 64) == UNSUPPORTED
    assert keys(e, r, t, ((1 << 31) - 4) // 6 + 1, 1, 4, o, o + 64, t, 4) == UNSUPPORTED
    # the vector path (D % 4 == 0, aligned tables) with a row block that is only 4-byte aligned
    assert bwd(e, r, t, 2, 2, 4, o, o + 64, o + 128 + 4, o + 256) == INVALID and bwd(e, r, t, 2, 2, 4, o, o + 64, o + 128, o + 256 + 4) == INVALID
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


# ============================================================================================================= 3. rel_mm.hip
def test_rel_rows_mm_above_48_kb_of_lds():
    """in_dim 769 and 1024: the launcher's hipFuncSetAttribute branch."""
    for shape in sa.BIG_LDS:
        assert sa.rel_failures(Abi(), shape) == []


@pytest.mark.parametrize("shape", [s for s in sa.REL_SHAPES if s not in sa.BIG_LDS], ids=lambda s: "x".join(map(str, s)))
def test_rel_rows_mm_through_the_c_abi(shape):
    assert sa.rel_failures(Abi(), shape) == []


@pytest.mark.parametrize("shape", sa.REL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rel_rows_mm_public_op(shape):
    from recon_amd.sep_space import rel_rows_mm
    c = sa.rel_case(shape)
    abi, rc, _ = sa.rel_run(Abi(), c)
    assert rc == [OK, OK, OK]
    x, W = T(c["x"]).requires_grad_(True), T(c["W"]).requires_grad_(True)
    out = rel_rows_mm(x, T(c["rel"]), W)
    gx, gW = torch.autograd.grad(out, [x, W], T(c["g"]))
    got = [a.detach().cpu().numpy() for a in (out, gx, gW)]
    bad = []
    sa.rel_band(got, c, dev(), "x".join(map(str, shape)) + " op", bad)
    assert bad == []
    for what, a, b in zip(sa.REL_OUT, got, abi):
        assert sa.bits_equal(a, b), what


def test_rel_rows_mm_rejections():
    from recon_amd.sep_space import rel_rows_mm
    d = dev()
    rel = torch.zeros(2, dtype=torch.int64, device=d)
    with pytest.raises(ValueError):
        rel_rows_mm(torch.zeros(2, 1025, device=d), rel, torch.zeros(1, 1025, 4, device=d))
    with pytest.raises(ValueError):
        rel_rows_mm(torch.zeros(2, 4, device=d), rel, torch.zeros(1, 4, 513, device=d))
    be = Abi()
    lib, s = be.lib, be.stream()
    buf = torch.full((256,), 7.0, device=d)
    idx = torch.zeros(64, dtype=torch.int64, device=d)
    p, q = buf.data_ptr(), idx.data_ptr()
    mm = lambda T_, IN, OUT, tr=0: lib.recon_rel_rows_mm(p, q, q, p + 256, T_, IN, OUT, tr, p + 512, s)
    wg = lambda R, D, OUT: lib.recon_rel_rows_mm_wgrad(p, p + 256, q, q, R, D, OUT, p + 512, s)
    assert mm(2, 1025, 4) == INVALID and mm(2, 1025, 4, 1) == INVALID
    assert mm(-1, 4, 4) == INVALID and mm(2, 0, 4) == INVALID and mm(2, 4, 0) == INVALID and mm(2, -4, 4) == INVALID and mm(2, 4, -4) == INVALID
    assert wg(1, 4, 513) == UNSUPPORTED
    assert wg(-1, 4, 4) == INVALID and wg(1, 0, 4) == INVALID and wg(1, 4, 0) == INVALID and wg(1, -4, 4) == INVALID and wg(1, 4, -4) == INVALID
    assert mm(0, 4, 4) == OK and wg(0, 4, 4) == OK
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


# ============================================================================================================= 4. no edge survives the pruning
@pytest.mark.parametrize("nhop", [False, True], ids=["1hop", "2hop"])
def test_spkbgat_when_no_edge_survives_the_pruning(nhop, monkeypatch):
    """Batch entities without in-edges: prune_batch keeps nothing and both layers see a [2, 0] view.  Every row is then the skip connection
    alone, F.normalize(E W_entities), and the pruned run agrees with the one that evaluates every row."""
    from recon_amd import models
    d = dev()
    rs = np.random.RandomState(11)
    Ne, n_rel, E = 40, 5, 90
    edge = torch.from_numpy(np.stack([rs.randint(0, 20, E), rs.randint(0, 40, E)])).long().to(d)        # row 0: destinations, all below 20
    et = torch.from_numpy(rs.randint(0, n_rel, E)).long().to(d)
    quads = torch.from_numpy(np.stack([rs.randint(0, 40, 30), rs.randint(0, n_rel, 30), rs.randint(0, n_rel, 30), rs.randint(0, 20, 30)], 1)).long().to(d)
    quads = quads if nhop else quads[:0]
    batch = torch.tensor([30, 31, 32, 33, 30, 37], device=d)            # no in-edges; sources of some
    assert bool(torch.isin(edge[1], batch).any())
    g = torch.Generator().manual_seed(0)
    ent_emb, rel_emb = torch.randn(Ne, 16, generator=g), torch.randn(n_rel, 16, generator=g)
    G = torch.randn(Ne, 16, generator=g).to(d)
    res = {}
    for prune in (True, False):
        monkeypatch.setattr(models, "PRUNE_DEAD_ROWS", prune)
        torch.manual_seed(0)
        m = models.SpKBGATModified(ent_emb.clone(), rel_emb.clone(), [8, 16], [16, 16], 0.0, 0.2, [2, 2], None).to(d)
        m.eval()
        if prune:
            seen = []
            real = m.sparse_gat_1.forward
            monkeypatch.setattr(m.sparse_gat_1, "forward", lambda *a, **k: (seen.append(tuple(a[3].shape)), real(*a, **k))[1])
        out_e, out_r, mask = m(None, batch, (edge, et), quads)
        if prune:
            assert seen == [(2, 0)]
        assert float(mask.sum()) == 5.0                                 # the distinct batch entities
        ((out_e * G).sum() + out_r.sum()).backward()
        grads = [p_.grad for _, p_ in sorted(m.named_parameters()) if p_.grad is not None]
        assert all(bool(torch.isfinite(t).all()) for t in [out_e, out_r] + grads)
        res[prune] = [out_e.detach(), out_r.detach()] + grads
        W = m.W_entities.detach()
    ref = F.normalize(F.normalize(ent_emb.double(), p=2, dim=1) @ W.double().cpu(), p=2, dim=1).numpy()
    chain = F.normalize(F.normalize(ent_emb.to(d), p=2, dim=1) @ W, p=2, dim=1).cpu().numpy()
    e_chain = sa.row_errors(chain, ref)[0]
    for prune in (True, False):
        e = sa.row_errors(res[prune][0].cpu().numpy(), ref)[0]
        print("no edge survives, prune %s: out_entity %.3e chain %.3e bound %.3e" % (prune, e, e_chain, bound(e_chain)))
        assert e <= bound(e_chain)
    assert len(res[True]) == len(res[False]) > 4
    for a_, b_ in zip(res[True], res[False]):
        assert float((a_ - b_).abs().max()) <= 1e-5 + 1e-4 * float(b_.abs().max())
