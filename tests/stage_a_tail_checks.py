"""Shared by tests/test_stage_a_tail_cpu.py and tests/test_stage_a_tail_gpu.py: the three small stage-A kernel families that had no test
file of their own — csrc/norm.hip (mask + skip + L2 row normalisation), csrc/loss.hip (the TransE margin loss) and csrc/rel_mm.hip (the
per-relation map of GAT_sep_space) — held to float64.  Here are the shape tables, the seeded input makers, the float64 references, a
float32 NumPy restatement of every kernel in the kernel's own summation order (`Restated`; `wrong=` makes it wrong in one named way) and
the checks.  A check drives a *backend*: `Restated` on the CPU, the C ABI in the GPU file; both write their outputs into `Guarded`
buffers.  Not a test module and not a conftest.

Bands.  `op_checks.bound` of the stock fp32 chain's own error (the same torch lines in fp32 on the backend's device), measured per case.
  norm.hip   every error per ROW, relative to that row's max |float64|; the op's worst row against bound() of the chain's worst row; a row
             whose reference is all zero must be exactly zero.  `norm` alone gets one term more: where the squares are denormal in fp32 the
             sum of squares carries an absolute error of up to C half-quanta (C 2^-150), which is C 2^-151 / |t| on the norm — from the
             number format, negligible (1e-43 / |t|) for every ordinary row.
  loss.hip   `terms`, and `loss`, their mean, relative to max_j (pn_j + nn_j + |margin|), the quantities the subtraction cancels; keys and
             the gradient rows exactly.
  rel_mm.hip per tensor, relative to max |float64|; relations without rows give exact zeros."""
import numpy as np
import torch
import torch.nn.functional as F

from op_checks import bound

f32 = np.float32
EPS = 1e-12
OK, INVALID, UNSUPPORTED = 0, -1, -2


# ------------------------------------------------------------------------------------------------------------- guarded outputs
class Guarded:
    """`n` cells of `dtype` inside a larger buffer pre-filled with a bit pattern (a NaN for floats); cell 0 lies `lead` cells past a
    16-byte boundary of the buffer (whose base a backend keeps 16-byte aligned)."""
    PAD = 16
    FILL = {4: 0x7FC0BEEF, 8: 0x7FF8DEADBEEF0BAD}

    def __init__(self, n, dtype=np.float32, lead=1):
        self.n, self.dtype, self.off = int(n), np.dtype(dtype), self.PAD + lead
        self.bits = np.dtype("u%d" % self.dtype.itemsize)
        self.buf = np.full(self.n + 2 * self.PAD + lead, self.FILL[self.dtype.itemsize], self.bits).view(self.dtype)

    def cells(self):
        return self.buf[self.off:self.off + self.n]

    def intact(self):
        """Every cell outside [0, n) is bit for bit the fill."""
        b = self.buf.view(self.bits)
        fill = self.FILL[self.dtype.itemsize]
        return bool((b[:self.off] == fill).all() and (b[self.off + self.n:] == fill).all())

    def written(self):
        """No cell inside [0, n) still holds the fill."""
        return not bool((self.cells().view(self.bits) == self.FILL[self.dtype.itemsize]).any())


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


RATIOS = {}                                       # (kernel, output) -> the worst error / bound ratio seen in this process


def _band(kernel, what, label, e_op, e_chain, bad):
    b = bound(e_chain)
    ratio = e_op / b
    RATIOS[(kernel, what)] = max(RATIOS.get((kernel, what), 0.0), ratio if ratio == ratio else float("inf"))
    print("stage_a_tail %s %s %s: op %.3e chain %.3e bound %.3e ratio %.3f" % (kernel, what, label, e_op, e_chain, b, ratio))
    if not e_op <= b:
        bad.append("%s %s %s: %.3e > %.3e" % (kernel, what, label, e_op, b))


# ------------------------------------------------------------------------------------------------------------- fp32 in the kernels' order
def fma32(a, b, c):
    """fmaf: the product of two fp32 numbers is exact in fp64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def wave_sum(v):
    """group_sum<64>: lane l adds lane l ^ 1, then l ^ 2, ... — a balanced tree over neighbouring lanes.  v [..., 64]."""
    for _ in range(6):
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _lanes(a):
    """[n, C] -> [n, steps, 64]: lane l holds columns l, l + 64, ... (zero padded)."""
    n, C = a.shape
    steps = (C + 63) // 64
    p = np.zeros((n, steps * 64), f32)
    p[:, :C] = a
    return p.reshape(n, steps, 64)


class Restated:
    """The kernels of norm.hip, loss.hip and rel_mm.hip once more in float32 NumPy, in the kernels' order of operations."""
    WRONG_NORM = ("no_clamp", "clamp_squared", "mask_onoff", "gskip_unmasked", "dot_wrong_axis")
    WRONG_MARGIN = ("pos_div", "weight_npos", "sign0_one", "swap_head_tail", "rel_no_offset", "second_row_unset", "nan_clamped")
    WRONG_REL = ("drop_partial_round", "drop_tail_rows", "untransposed")
    device = torch.device("cpu")

    def __init__(self, wrong=None):
        assert wrong is None or wrong == "past_end" or wrong in self.WRONG_NORM + self.WRONG_MARGIN + self.WRONG_REL
        self.wrong = wrong

    def _put(self, g, val):
        if g is None:
            return
        g.cells()[:] = np.asarray(val, g.dtype).ravel()
        if self.wrong == "past_end":
            g.buf[g.off + g.n] = 0

    # ---- norm.hip
    def norm_fwd(self, ew, skip, mask, N, C, eps, y, norm):
        if N < 0 or C <= 0 or not eps > 0:
            return INVALID
        if N == 0:
            return OK
        if y is None:
            return INVALID
        ew = (y.cells().copy() if ew is None else ew).reshape(N, C)               # ew None: y aliases ew
        eps = f32(eps)
        t = ew
        if skip is not None:
            skip = skip.reshape(N, C)
            mv = np.ones(N, f32) if mask is None else mask
            on = np.ones(N, bool) if mask is None else mask != 0
            if self.wrong == "mask_onoff":
                mv = on.astype(f32)
            t = np.where(on[:, None], fma32(mv[:, None], skip, ew), ew)
        tl = _lanes(t)
        ss = np.zeros((N, 64), f32)
        for k in range(tl.shape[1]):
            ss = fma32(tl[:, k], tl[:, k], ss)
        ss = wave_sum(ss)
        nr = np.sqrt(ss)
        with np.errstate(all="ignore"):
            if self.wrong == "no_clamp":
                inv = f32(1) / nr
            elif self.wrong == "clamp_squared":
                inv = f32(1) / np.sqrt(np.maximum(ss, eps))
            else:
                inv = f32(1) / np.maximum(nr, eps)
            self._put(y, t * inv[:, None])
        self._put(norm, nr)
        return OK

    def norm_bwd(self, gy, y, norm, mask, N, C, eps, gt, gskip):
        if N < 0 or C <= 0 or not eps > 0:
            return INVALID
        if N == 0:
            return OK
        if gy is None or y is None or norm is None or gt is None:
            return INVALID
        gy, y, eps = gy.reshape(N, C), y.reshape(N, C), f32(eps)
        if self.wrong == "dot_wrong_axis":
            dot = np.broadcast_to((gy * y).sum(0, dtype=f32)[None, :], (N, C))
        else:
            a, b = _lanes(gy), _lanes(y)
            dot = np.zeros((N, 64), f32)
            for k in range(a.shape[1]):
                dot = fma32(a[:, k], b[:, k], dot)
            dot = wave_sum(dot)[:, None]
        with np.errstate(all="ignore"):
            if self.wrong == "no_clamp":
                clamped, inv = np.zeros(N, bool), f32(1) / norm
            elif self.wrong == "clamp_squared":
                clamped, inv = norm * norm < eps, f32(1) / np.sqrt(np.maximum(norm * norm, eps))
            else:
                clamped, inv = norm < eps, f32(1) / np.maximum(norm, eps)
            g = np.where(clamped[:, None], gy * inv[:, None], (gy - y * dot) * inv[:, None]).astype(f32)
        mv = np.ones(N, f32) if (mask is None or self.wrong == "gskip_unmasked") else mask
        self._put(gt, g)
        self._put(gskip, mv[:, None] * g)
        return OK

    # ---- loss.hip
    @staticmethod
    def _vec4(D, misaligned):
        return D % 4 == 0 and D <= 512 and not misaligned

    def _row_l1(self, ent, rel, rows, D, vec4):
        """|h + r - t|_1 of each triple in the lanes' order, and x."""
        x = (ent[rows[:, 0]] + rel[rows[:, 1]]) - ent[rows[:, 2]]
        a = np.abs(x)
        n = a.shape[0]
        if vec4:                                                        # lane l: columns 4 l .. 4 l + 3, then 256 + 4 l .. 256 + 4 l + 3
            p = np.zeros((n, 512), f32)
            p[:, :D] = a
            p = p.reshape(n, 2, 64, 4).transpose(0, 2, 1, 3).reshape(n, 64, 8)
            s = np.zeros((n, 64), f32)
            for k in range(8):
                s = s + p[:, :, k]
        else:
            p = _lanes(a)
            s = np.zeros((n, 64), f32)
            for k in range(p.shape[1]):
                s = s + p[:, k]
        return wave_sum(s), x

    def _margin_fwd(self, ent, rel, tri, n_pos, reps, D, margin, terms, loss, misaligned):
        P = n_pos * reps
        j = np.arange(P)
        tp = j // reps if self.wrong == "pos_div" else j % n_pos
        tn = n_pos + j
        vec4 = self._vec4(D, misaligned)
        pn, _ = self._row_l1(ent, rel, tri[tp], D, vec4)
        nn, _ = self._row_l1(ent, rel, tri[tn], D, vec4)
        v = (pn - nn) + f32(margin)
        t = np.fmax(f32(0), v) if self.wrong == "nan_clamped" else np.where(np.isnan(v), v, np.maximum(f32(0), v))
        self._put(terms, t)
        s = np.zeros(256, f32)                                          # k_transe_mean: thread i adds terms i, i + 256, ...; then the LDS tree
        for k in range(0, P, 256):
            chunk = np.zeros(256, f32)
            chunk[:min(256, P - k)] = t[k:k + 256]
            s = s + chunk
        off = 128
        while off:
            s[:off] = s[:off] + s[off:2 * off]
            off //= 2
        self._put(loss, s[:1] / f32(P))
        return tp, tn

    def _keys(self, g, blocks, add):
        if g is None:
            return
        row = np.concatenate(blocks).astype(np.int64) + add
        both = np.stack([row, row])
        if self.wrong == "second_row_unset":
            both[1] = g.cells().reshape(2, -1)[1]
        self._put(g, both)

    @staticmethod
    def _margin_args(ent, rel, tri, n_pos, reps, D):
        if n_pos == 0 and reps > 0 and D > 0:
            return INVALID
        if ent is None or rel is None or tri is None or n_pos <= 0 or reps <= 0 or D <= 0:
            return INVALID
        return OK

    def margin_fwd(self, ent, rel, tri, n_pos, reps, D, margin, terms, loss, ent_key, rel_key, misaligned=False):
        if self._margin_args(ent, rel, tri, n_pos, reps, D) or terms is None or loss is None:
            return INVALID
        if n_pos * reps > (1 << 31) - 4:
            return UNSUPPORTED
        tp, tn = self._margin_fwd(ent, rel, tri, n_pos, reps, D, margin, terms, loss, misaligned)
        h, t = (2, 0) if self.wrong == "swap_head_tail" else (0, 2)
        self._keys(ent_key, [tri[tp, h], tri[tp, t], tri[tn, h], tri[tn, t]], 0)
        self._keys(rel_key, [tri[tp, 1], tri[tn, 1]], 0)
        return OK

    def margin_fwd_keys(self, ent, rel, tri, n_pos, reps, D, margin, terms, loss, keys, n_entities, misaligned=False):
        if self._margin_args(ent, rel, tri, n_pos, reps, D) or terms is None or loss is None or keys is None or n_entities <= 0:
            return INVALID
        if n_pos * reps > ((1 << 31) - 4) // 6:
            return UNSUPPORTED
        tp, tn = self._margin_fwd(ent, rel, tri, n_pos, reps, D, margin, terms, loss, misaligned)
        h, t = (2, 0) if self.wrong == "swap_head_tail" else (0, 2)
        off = 0 if self.wrong == "rel_no_offset" else n_entities
        if keys is not None:
            row = np.concatenate([tri[tp, h], tri[tp, t], tri[tn, h], tri[tn, t], tri[tp, 1] + off, tri[tn, 1] + off]).astype(np.int64)
            both = np.stack([row, row])
            if self.wrong == "second_row_unset":
                both[1] = keys.cells().reshape(2, -1)[1]
            self._put(keys, both)
        return OK

    def margin_bwd(self, ent, rel, tri, n_pos, reps, D, terms, g, rows, misaligned=False):
        """rows: the [6 P, D] block — entity rows (pos heads | pos tails | neg heads | neg tails), then relation rows (pos | neg)."""
        if self._margin_args(ent, rel, tri, n_pos, reps, D) or terms is None or g is None or rows is None:
            return INVALID
        if self._vec4(D, misaligned) and rows.off % 4:
            return INVALID
        P = n_pos * reps
        j = np.arange(P)
        tp = j // reps if self.wrong == "pos_div" else j % n_pos
        tn = n_pos + j
        w = np.where(terms > 0, f32(g) / f32(n_pos if self.wrong == "weight_npos" else P), f32(0)).astype(f32)[:, None]
        sign = (lambda x: np.where(x >= 0, f32(1), f32(-1))) if self.wrong == "sign0_one" else np.sign
        xp = (ent[tri[tp, 0]] + rel[tri[tp, 1]]) - ent[tri[tp, 2]]
        xn = (ent[tri[tn, 0]] + rel[tri[tn, 1]]) - ent[tri[tn, 2]]
        gp, gn = w * sign(xp), -w * sign(xn)
        self._put(rows, np.concatenate([gp, -gp, gn, -gn, gp, gn]))
        return OK

    # ---- rel_mm.hip
    def rel_mm(self, x, order, rel, W, T, IN, OUT, trans, out):
        if T < 0 or IN <= 0 or OUT <= 0 or IN > 1024:
            return INVALID
        if T == 0:
            return OK
        if x is None or order is None or rel is None or W is None or out is None:
            return INVALID
        x = x.reshape(T, IN)
        Wsel = W[rel]                                                   # [T, D, Dout]
        if trans and self.wrong != "untransposed":
            Wsel = Wsel.transpose(0, 2, 1)
        assert Wsel.shape[1:] == (IN, OUT)
        acc = np.zeros((T, OUT), f32)
        for k in range(IN):                                             # rows outside a run add x * 0 * w: nothing
            acc = fma32(x[:, k:k + 1], Wsel[:, k, :], acc)
        self._put(out, acc)
        return OK

    def rel_wgrad(self, x, g, order, seg, R, D, OUT, gW):
        if R < 0 or D <= 0 or OUT <= 0:
            return INVALID
        if OUT > 512:
            return UNSUPPORTED
        if R == 0:
            return OK
        if x is None or g is None or order is None or seg is None or gW is None:
            return INVALID
        x, g = x.reshape(-1, D), g.reshape(-1, OUT)
        res = np.zeros((R, D, OUT), f32)
        for r in range(R):
            rows = order[seg[r]:seg[r + 1]]
            if self.wrong == "drop_partial_round":
                rows = rows[:len(rows) // 8 * 8]
            for t in rows:                                              # eight rows a round, in the sorted order
                res[r] = fma32(x[t][:, None], g[t][None, :], res[r])
        if self.wrong == "drop_tail_rows" and gW is not None:
            keep = gW.cells().reshape(R, D, OUT)[:, D // 16 * 16:, :].copy()
            res[:, D // 16 * 16:, :] = keep
        self._put(gW, res)
        return OK


# ============================================================================================================= 1. norm.hip
#               N  C
NORM_SHAPES = [(1, 1), (4, 1), (3, 37), (9, 37), (4, 63), (5, 64), (9, 65), (4, 128), (3, 200), (9, 200), (5, 257)]
NORM_FORMS = ("plain", "skip_mask", "skip_nomask", "mask_noskip")
MASK_VALUES = (1.0, 0.5, 2.0, -1.0, 0.0)
_NORM = {}


def norm_case(N, C, form):
    """fp32 inputs: N(0, 1) times a per-row scale from {1e-3, 1, 1e3}; from N = 3 on the last three rows are special — a row with entries of
    about 1e-20 (squares denormal in fp32), a row of norm 3e-13 < eps, and a row that is exactly zero under mask 0.  With them the float64
    reference (y, norm, g_t, g_skip; None where the form has none) on the fp32 inputs, computed once and left unchanged."""
    if (N, C, form) in _NORM:
        return _NORM[(N, C, form)]
    rs = np.random.RandomState(1000 * N + C)
    scales = np.array([1e-3, 1.0, 1e3])
    ew = rs.randn(N, C) * scales[rs.randint(0, 3, N)][:, None]
    skip = rs.randn(N, C) * scales[rs.randint(0, 3, N)][:, None]
    mask = np.array([MASK_VALUES[i % 5] for i in range(N)])
    special = {}
    if N >= 3:
        tiny, small, zero = N - 3, N - 2, N - 1
        special = dict(tiny=tiny, small=small, zero=zero)
        ew[tiny] = 1e-20 * rs.uniform(0.5, 2.0, C) * rs.choice([-1.0, 1.0], C)
        skip[tiny] = 0.5e-20 * rs.uniform(0.5, 2.0, C) * rs.choice([-1.0, 1.0], C)
        mask[tiny] = 2.0
        z = rs.randn(C) + (C == 1)
        ew[small] = z * (3e-13 / np.linalg.norm(z))
        z = rs.randn(C) + (C == 1)
        skip[small] = z * (1e-13 / np.linalg.norm(z))
        mask[small] = 0.5
        ew[zero] = 0.0
        mask[zero] = 0.0
    c = dict(N=N, C=C, form=form, ew=ew.astype(f32), gy=rs.randn(N, C).astype(f32), special=special,
             skip=skip.astype(f32) if form in ("skip_mask", "skip_nomask") else None,
             mask=mask.astype(f32) if form in ("skip_mask", "mask_noskip") else None)
    c["ref"] = norm_chain(c, torch.float64, torch.device("cpu"))
    _NORM[(N, C, form)] = c
    return c


def norm_chain(c, dtype, device):
    """The stock lines: F.normalize(ew + mask[:, None] * skip, p=2, dim=1, eps=1e-12) and its autograd -> [y, norm, g_t, g_skip] (numpy)."""
    T = lambda a: None if a is None else torch.from_numpy(a).to(device=device, dtype=dtype)
    ew, skip, mask, gy = T(c["ew"]).requires_grad_(True), T(c["skip"]), T(c["mask"]), T(c["gy"])
    t = ew
    if skip is not None:
        skip.requires_grad_(True)
        t = ew + (skip if mask is None else mask.unsqueeze(-1) * skip)
    y = F.normalize(t, p=2, dim=1, eps=EPS)
    grads = torch.autograd.grad(y, [ew] + ([skip] if skip is not None else []), gy)
    n = lambda a: a.detach().cpu().numpy()
    return [n(y), n(t.norm(p=2, dim=1)), n(grads[0]), n(grads[1]) if skip is not None else None]


def norm_run(be, c, want_gskip=True, in_place=False):
    """Forward then backward (on the y and norm the forward wrote) -> ([y, norm, g_t, g_skip], return codes, guards)."""
    N, C = c["N"], c["C"]
    y, norm = Guarded(N * C), None if in_place else Guarded(N)
    if in_place:                                                        # what normalize_rows_ passes: y == ew, no norm
        y.cells()[:] = c["ew"].ravel()
    skip = c["skip"]
    rc = [be.norm_fwd(None if in_place else c["ew"], skip, c["mask"], N, C, EPS, y, norm)]
    guards = dict(y=y, norm=norm)
    out = [y.cells().reshape(N, C).copy(), None if in_place else norm.cells().copy(), None, None]
    if not in_place:
        gt = Guarded(N * C)
        gs = Guarded(N * C) if (skip is not None and want_gskip) else None
        rc.append(be.norm_bwd(c["gy"], out[0], out[1], c["mask"] if skip is not None else None, N, C, EPS, gt, gs))
        guards.update(g_t=gt, g_skip=gs)
        out[2] = gt.cells().reshape(N, C).copy()
        out[3] = None if gs is None else gs.cells().reshape(N, C).copy()
    return out, rc, guards


def row_errors(got, ref, scale=None):
    """(worst over the rows with a non-zero reference of max |got - ref| / max |ref|, the rows whose reference is all zero but `got` is not).
    `scale` replaces max |ref| row by row."""
    got, ref = np.asarray(got, np.float64).reshape(ref.shape[0], -1), np.asarray(ref, np.float64).reshape(ref.shape[0], -1)
    scale = np.abs(ref).max(1) if scale is None else scale
    live = scale > 0
    with np.errstate(all="ignore"):
        worst = float(np.max(np.abs(got[live] - ref[live]).max(1) / scale[live])) if live.any() else 0.0
    dead = [int(r) for r in np.nonzero(~live)[0] if np.any(got[r] != 0)]
    return worst, dead


NORM_OUT = ("y", "norm", "g_t", "g_skip")


def norm_failures(be, N, C, form):
    """Every check of part 1 on one shape and form; prints the figures."""
    c = norm_case(N, C, form)
    ref, chain = c["ref"], norm_chain(c, torch.float32, be.device)
    label = "%dx%d %s" % (N, C, form)
    bad = []
    got, rc, guards = norm_run(be, c)
    if any(rc):
        return ["%s: return codes %s" % (label, rc)]
    for what, f, ch, r in zip(NORM_OUT, got, chain, ref):
        if (f is None) != (r is None):
            bad.append("%s %s: None against a tensor" % (label, what))
            continue
        if r is None:
            continue
        e_c, _ = row_errors(ch, r)
        if what == "norm":                                              # the denormal term of the module docstring, taken off the error row by row
            r64, f64 = r.astype(np.float64), f.astype(np.float64)
            with np.errstate(all="ignore"):
                slack = np.where(r64 > 0, C * 2.0 ** -151 / r64, 0.0)
                excess = np.maximum(np.abs(f64 - r64) - slack, 0.0)
                excess = np.where(np.isnan(f64), np.nan, excess)
                e_f = float(np.max(np.where(r64 > 0, excess / r64, 0.0)))
            dead = [int(i) for i in np.nonzero(r64 == 0)[0] if f[i] != 0]
        else:
            scale = None
            if C == 1 and what in ("g_t", "g_skip"):
                # one column: above eps y = +-1 and g_y - y (y . g_y) is zero by total cancellation, so the float64 "reference" is its own
                # rounding noise; these rows are measured against the two terms that cancel, |g_y| / |t| (times |mask| for g_skip)
                nr = ref[1].astype(np.float64)
                scale = np.abs(r).max(1).astype(np.float64)
                free = nr >= EPS
                scale[free] = np.abs(c["gy"][free, 0]) / nr[free] * (np.abs(c["mask"][free]) if (what == "g_skip" and c["mask"] is not None) else 1.0)
            e_f, dead = row_errors(f, r, scale)
            e_c, _ = row_errors(ch, r, scale)
        _band("norm", what, label, e_f, e_c, bad)
        if dead:
            bad.append("%s %s: rows %s must be exactly zero" % (label, what, dead))
    for what, g in guards.items():
        if g is not None and not (g.intact() and g.written()):
            bad.append("%s guard %s" % (label, what))
    again, _, _ = norm_run(be, c)
    for what, a, b in zip(NORM_OUT, got, again):
        if a is not None and not bits_equal(a, b):
            bad.append("%s %s: two calls differ" % (label, what))
    if form == "plain":                                                 # y == ew, norm == null
        (y2, _, _, _), rc2, g2 = norm_run(be, c, in_place=True)
        if any(rc2) or not bits_equal(y2, got[0]):
            bad.append("%s in place: other bits than into a separate y" % label)
        if not g2["y"].intact():
            bad.append("%s guard y (in place)" % label)
    if form == "skip_mask":                                             # g_skip == null: the same g_t
        no_gs, rc3, g3 = norm_run(be, c, want_gskip=False)
        if any(rc3) or not bits_equal(no_gs[2], got[2]):
            bad.append("%s g_skip == null: other g_t" % label)
        if not g3["g_t"].intact():
            bad.append("%s guard g_t (g_skip == null)" % label)
    return bad


# ============================================================================================================= 2. loss.hip
#                 D  tables one float into a larger buffer (16-byte alignment lost)
MARGIN_WIDTHS = [(1, False), (3, False), (37, False),                   # scalar
                 (4, False), (64, False), (252, False), (256, False),   # vector, first step only; 252 ends on lane 62
                 (260, False), (508, False), (512, False),              # vector, second step: one lane, 63 lanes, all lanes
                 (516, False), (1028, False),                           # scalar by size, D % 4 == 0
                 (200, True), (200, False)]                             # scalar by alignment; the vector path at the same width
MARGIN_PAIRS = [(1, 1), (3, 1), (5, 2), (7, 6), (67, 4)]                # pairs % 4 = 1, 3, 2, 2, 0; 1, 3, 10, 42, 268 pairs
N_ENT, N_REL = 29, 5
_MARGIN = {}


def zero_columns(D):
    return sorted({0, D // 3, D // 2, D - 1})[:min(4, D - 1)]


def margin_inputs(D, n_pos, reps, seed):
    rs = np.random.RandomState(seed)
    ent, rel = rs.randn(N_ENT, D).astype(f32), rs.randn(N_REL, D).astype(f32)
    P = n_pos * reps
    tri = np.stack([rs.randint(0, N_ENT, n_pos + P), rs.randint(0, N_REL, n_pos + P), rs.randint(0, N_ENT, n_pos + P)], 1).astype(np.int64)
    same = tri[:, 0] == tri[:, 2]
    tri[same, 2] = (tri[same, 0] + 1 + rs.randint(0, N_ENT - 1, int(same.sum()))) % N_ENT      # head == tail only where planted
    tri[0, 2] = tri[0, 0]                                               # the planted positive with head == tail ...
    rel[tri[0, 1], zero_columns(D)] = 0.0                               # ... and its relation row's exactly-zero columns: x == 0 there
    # pn of that positive is only |r|, far below an ordinary nn: its first negative is of the same kind (head == tail, the next relation, no
    # zeros), so that this pair can be active and the zero signs reach the gradient rows
    tri[n_pos] = (tri[n_pos, 0], (tri[0, 1] + 1) % N_REL, tri[n_pos, 0])
    return ent, rel, tri


def margin_ref(ent, rel, tri, n_pos, reps, margin, dtype=torch.float64, device=torch.device("cpu")):
    """The reference's op sequence (GAT/main.py:344-376) -> dict of numpy: pn, nn, v, terms, loss."""
    T = lambda a: torch.from_numpy(a).to(device)
    e, r, tr = T(ent).to(dtype), T(rel).to(dtype), T(tri)
    pos, neg = tr[:n_pos].repeat(reps, 1), tr[n_pos:]
    pn = torch.norm(e[pos[:, 0]] + r[pos[:, 1]] - e[pos[:, 2]], p=1, dim=1)
    nn = torch.norm(e[neg[:, 0]] + r[neg[:, 1]] - e[neg[:, 2]], p=1, dim=1)
    y = -torch.ones(n_pos * reps, dtype=dtype, device=device)
    terms = F.margin_ranking_loss(pn, nn, y, margin=float(margin), reduction="none")
    n = lambda a: a.detach().cpu().numpy()
    return dict(pn=n(pn), nn=n(nn), v=n(pn - nn + float(margin)), terms=n(terms), loss=n(terms.mean()))


def margin_scale(ref, margin):
    return float(np.max(ref["pn"] + ref["nn"] + abs(float(margin))))


def margin_x(c):
    """float64 x = h + r - t of the positive and the negative of every pair, and |h| + |r| + |t|."""
    ent, rel, tri, n_pos = c["ent"].astype(np.float64), c["rel"].astype(np.float64), c["tri"], c["n_pos"]
    j = np.arange(c["P"])
    out = []
    for rows in (tri[j % n_pos], tri[n_pos + j]):
        h, r, t = ent[rows[:, 0]], rel[rows[:, 1]], ent[rows[:, 2]]
        out.append((h + r - t, np.abs(h) + np.abs(r) + np.abs(t)))
    return out


def margin_conditions(c):
    """The conditions on the inputs of a case, as the list of those violated."""
    ref, bad = c["ref"], []
    if not np.abs(ref["v"]).min() > 2e-5 * margin_scale(ref, c["margin"]):          # 2e-5: the most op_checks.bound ever allows
        bad.append("a pre-clamp value within the forward band of 0")
    if c["P"] >= 3 and not ((ref["v"] > 0).any() and (ref["v"] < 0).any()):
        bad.append("active and inactive pairs do not both occur")
    if not (ref["v"][::c["n_pos"]] > 0).any():
        bad.append("no active pair holds the planted positive: its exact zeros of x would go unchecked")
    zeros = near = 0
    for x, mag in margin_x(c):
        zeros += int((x == 0).sum())
        near += int(((x != 0) & (np.abs(x) <= 4 * 2.0 ** -24 * mag)).sum())
    if near:
        bad.append("%d |x| within rounding of zero" % near)
    if zeros != c["planted_zeros"]:
        bad.append("%d exact zeros of x, planted %d" % (zeros, c["planted_zeros"]))
    return bad


def margin_case(D, n_pos, reps, misaligned=False):
    """Tables of N(0, 1), uniform ids, the planted positive; `margin` splits the sorted float64 pn - nn at the widest gap of the middle half,
    so that active and inactive pairs both occur and no pre-clamp value is near 0.  The first seed whose case meets margin_conditions."""
    key = (D, n_pos, reps, misaligned)
    if key in _MARGIN:
        return _MARGIN[key]
    P = n_pos * reps
    for seed in range(100 * D + P, 100 * D + P + 50):
        ent, rel, tri = margin_inputs(D, n_pos, reps, seed)
        d = margin_ref(ent, rel, tri, n_pos, reps, 0.0)["v"]
        s = np.sort(d)
        if P == 1:
            margin = f32(1.0 - s[0])
        else:
            lo, hi = max(1, P // 4), max(2, 3 * P // 4 + 1)
            k = lo + int(np.argmax(s[lo:hi] - s[lo - 1:hi - 1]))
            margin = f32(-(s[k] + s[k - 1]) / 2)
        c = dict(D=D, n_pos=n_pos, reps=reps, P=P, misaligned=misaligned, ent=ent, rel=rel, tri=tri, margin=margin, seed=seed,
                 planted_zeros=reps * len(zero_columns(D)), ref=margin_ref(ent, rel, tri, n_pos, reps, margin))
        if not margin_conditions(c):
            _MARGIN[key] = c
            return c
    raise AssertionError("no seed meets the conditions at %s" % (key,))


def expected_keys(c, joint):
    tri, n_pos = c["tri"], c["n_pos"]
    j = np.arange(c["P"])
    tp, tn = tri[j % n_pos], tri[n_pos + j]
    e = np.concatenate([tp[:, 0], tp[:, 2], tn[:, 0], tn[:, 2]])
    r = np.concatenate([tp[:, 1], tn[:, 1]])
    if joint:
        row = np.concatenate([e, r + N_ENT])
        return np.stack([row, row])
    return np.stack([e, e]), np.stack([r, r])


def expected_rows(c, terms, g):
    """The [6 P, D] gradient rows: +-fl(g / P) or 0 with the sign of float64 x, rows of inactive pairs zero."""
    (xp, _), (xn, _) = margin_x(c)
    w = np.where(terms > 0, f32(g) / f32(c["P"]), f32(0)).astype(f32)[:, None]
    gp, gn = (w * np.sign(xp)).astype(f32), (-w * np.sign(xn)).astype(f32)
    return np.concatenate([gp, -gp, gn, -gn, gp, gn])


def margin_run(be, c, g_up=(1.0, 1.5)):
    """All forward forms and the backward of a case -> dict of outputs, return codes, guards."""
    D, n_pos, reps, P, mis = c["D"], c["n_pos"], c["reps"], c["P"], c["misaligned"]
    args = (c["ent"], c["rel"], c["tri"], n_pos, reps, D)
    out, rcs, guards = {}, [], {}
    for form, (we, wr) in dict(both=(1, 1), ent=(1, 0), rel=(0, 1), none=(0, 0)).items():
        terms, loss = Guarded(P), Guarded(1)
        ek = Guarded(2 * 4 * P, np.int64) if we else None
        rk = Guarded(2 * 2 * P, np.int64) if wr else None
        rcs.append(be.margin_fwd(*args, c["margin"], terms, loss, ek, rk, mis))
        out["sep_" + form] = (terms.cells().copy(), loss.cells().copy(), None if ek is None else ek.cells().reshape(2, -1).copy(),
                              None if rk is None else rk.cells().reshape(2, -1).copy())
        guards.update({"terms " + form: terms, "loss " + form: loss, "ent_key " + form: ek, "rel_key " + form: rk})
    terms, loss, keys = Guarded(P), Guarded(1), Guarded(2 * 6 * P, np.int64)
    rcs.append(be.margin_fwd_keys(*args, c["margin"], terms, loss, keys, N_ENT, mis))
    out["joint"] = (terms.cells().copy(), loss.cells().copy(), keys.cells().reshape(2, -1).copy())
    guards.update({"terms joint": terms, "loss joint": loss, "keys": keys})
    for g in g_up:
        rows = Guarded(6 * P * D, lead=0 if Restated._vec4(D, mis) else 1)      # the vector path needs a 16-byte aligned row block
        rcs.append(be.margin_bwd(*args, out["joint"][0], f32(g), rows, mis))
        out["rows %g" % g] = rows.cells().reshape(6 * P, D).copy()
        guards["rows %g" % g] = rows
    return out, rcs, guards


def margin_failures(be, c):
    """Every check of part 2 that runs through the backend on one case; prints the figures."""
    label = "D%d%s %dx%d" % (c["D"], "m" if c["misaligned"] else "", c["n_pos"], c["reps"])
    ref, scale = c["ref"], margin_scale(c["ref"], c["margin"])
    chain = margin_ref(c["ent"], c["rel"], c["tri"], c["n_pos"], c["reps"], c["margin"], torch.float32, be.device)
    out, rcs, guards = margin_run(be, c)
    if any(rcs):
        return ["%s: return codes %s" % (label, rcs)]
    bad = []
    terms, loss, keys = out["joint"]
    err = lambda a, what: float(np.max(np.abs(np.asarray(a, np.float64) - ref[what])))
    _band("margin", "terms", label, err(terms, "terms") / scale, err(chain["terms"], "terms") / scale, bad)
    _band("margin", "loss", label, err(loss[0], "loss") / scale, err(chain["loss"], "loss") / scale, bad)     # the mean of terms: their scale
    if not bits_equal(keys, expected_keys(c, True)):
        bad.append("%s joint keys" % label)
    ke, kr = expected_keys(c, False)
    for form in ("both", "ent", "rel", "none"):
        t2, l2, ek, rk = out["sep_" + form]
        if not (bits_equal(t2, terms) and bits_equal(l2, loss)):
            bad.append("%s separate-key form (%s): other terms / loss than the joint form" % (label, form))
        if (ek is not None and not bits_equal(ek, ke)) or (rk is not None and not bits_equal(rk, kr)):
            bad.append("%s separate keys (%s)" % (label, form))
    for g in (1.0, 1.5):
        want = expected_rows(c, terms, g)
        if not np.array_equal(out["rows %g" % g], want):
            bad.append("%s gradient rows at g = %g: %d elements differ" % (label, g, int((out["rows %g" % g] != want).sum())))
    if not np.array_equal(terms > 0, ref["v"] > 0):
        bad.append("%s the active set differs from float64's" % label)
    for what, g in guards.items():
        if g is not None and not (g.intact() and g.written()):
            bad.append("%s guard %s" % (label, what))
    again, _, _ = margin_run(be, c)
    for k in out:
        for a, b in zip(out[k] if isinstance(out[k], tuple) else (out[k],), again[k] if isinstance(again[k], tuple) else (again[k],)):
            if a is not None and not bits_equal(a, b):
                bad.append("%s %s: two calls differ" % (label, k))
    return bad


def margin_nan_failures(be):
    """clamp_min of the reference propagates NaN: an entity row of NaN gives NaN terms exactly where float64 has them, and a NaN loss."""
    D, n_pos, reps = 37, 5, 2
    ent, rel, tri = margin_inputs(D, n_pos, reps, 7)
    ent[tri[1, 0]] = np.nan
    ref = margin_ref(ent, rel, tri, n_pos, reps, 1.0)
    assert np.isnan(ref["terms"]).any() and not np.isnan(ref["terms"]).all()
    terms, loss = Guarded(n_pos * reps), Guarded(1)
    rc = be.margin_fwd(ent, rel, tri, n_pos, reps, D, f32(1.0), terms, loss, None, None, False)
    bad = []
    if rc or not np.array_equal(np.isnan(terms.cells()), np.isnan(ref["terms"])) or not np.isnan(loss.cells()[0]):
        bad.append("NaN terms / loss: rc %d, terms %s, loss %s" % (rc, terms.cells(), loss.cells()))
    return bad


def zero_case():
    """Small-integer tables and an integer margin: pair 0 has pn - nn + margin == 0 exactly (every fp32 sum is exact), pair 1 is active,
    pairs 2 to 5 inactive.  D = 4, n_pos = 3, reps = 2 (batch_gat_loss takes an even number of copies)."""
    ent = np.array([[0, 0, 0, 0], [1, 2, 0, -1], [3, 0, 1, 1], [0, -2, 2, 0], [5, 5, 5, 5]], f32)
    rel = np.array([[1, 0, -1, 2], [0, 1, 1, 0]], f32)
    #               pn: |e1 + r0 - e0| = |2 2 -1 1| = 6      |e2 + r1 - e3| = |3 3 0 1| = 7      |e0 + r0 - e1| = |0 -2 -1 3| = 6
    #               nn: |e2 + r0 - e0| = |4 0 0 3| = 7 ... with margin 1: 6 - 7 + 1 = 0
    tri = np.array([[1, 0, 0], [2, 1, 3], [0, 0, 1],
                    [2, 0, 0],                      # nn = 7:  v = 6 - 7 + 1 = 0
                    [1, 1, 0],                      # |1 3 1 -1| = 6: v = 7 - 6 + 1 = 2
                    [4, 0, 0],                      # |6 5 4 7| = 22: v = 6 - 22 + 1 = -15
                    [4, 0, 0], [4, 0, 0], [4, 0, 0]], np.int64)         # the second copy: -15, -14, -15
    c = dict(D=4, n_pos=3, reps=2, P=6, misaligned=False, ent=ent, rel=rel, tri=tri, margin=f32(1.0))
    c["ref"] = margin_ref(ent, rel, tri, 3, 2, 1.0)
    assert c["ref"]["v"].tolist() == [0.0, 2.0, -15.0, -15.0, -14.0, -15.0]
    return c


# ============================================================================================================= 3. rel_mm.hip
#              T   D    Dout R
REL_SHAPES = [(1, 1, 1, 1),            # the smallest case
              (17, 15, 17, 3),         # D % 16 = 15 in the weight gradient's tiles; T % 16 = 1
              (16, 768, 8, 2),         # exactly 48 KB of LDS: the ordinary launch
              (33, 769, 8, 2),         # the first width above it
              (5, 1024, 4, 2),         # the limit
              (20, 24, 256, 3), (20, 24, 257, 3), (9, 8, 512, 2),     # one or two columns per thread; the backward's transposed product at in_dim = 512
              (40, 16, 16, 6)]         # hand-written ids: segments of 8, 9, 1 and 0 rows
BIG_LDS = [(33, 769, 8, 2), (5, 1024, 4, 2)]
HAND_IDS = [4] * 3 + [1] * 8 + [3] + [2] * 9 + [4] * 19               # relation 0 and 5 empty; 1: 8 rows, 2: 9, 3: 1, 4: 22
_REL = {}


def rel_case(shape):
    if shape in _REL:
        return _REL[shape]
    T, D, Dout, R = shape
    rs = np.random.RandomState(T + 3 * D + 5 * Dout + 7 * R)
    if shape == (40, 16, 16, 6):
        rel = np.array(HAND_IDS, np.int64)[rs.permutation(T)]           # unsorted
        assert np.bincount(rel, minlength=R).tolist() == [0, 8, 9, 1, 22, 0]
    else:
        rel = rs.randint(0, R, T).astype(np.int64)
    c = dict(shape=shape, x=rs.randn(T, D).astype(f32), W=(rs.randn(R, D, Dout) / np.sqrt(D)).astype(f32), rel=rel,
             g=rs.randn(T, Dout).astype(f32), order=np.argsort(rel, kind="stable").astype(np.int32),
             seg=np.concatenate([[0], np.cumsum(np.bincount(rel, minlength=R))]).astype(np.int32))
    c["ref"] = rel_chain(c, torch.float64, torch.device("cpu"))
    _REL[shape] = c
    return c


def rel_chain(c, dtype, device):
    """torch.bmm(x.unsqueeze(1), W[rel]) and its autograd -> [out, g_x, g_W] (numpy)."""
    T = lambda a: torch.from_numpy(a).to(device)
    x, W = T(c["x"]).to(dtype).requires_grad_(True), T(c["W"]).to(dtype).requires_grad_(True)
    out = torch.bmm(x.unsqueeze(1), W[T(c["rel"])]).squeeze(1)
    gx, gW = torch.autograd.grad(out, [x, W], T(c["g"]).to(dtype))
    return [a.detach().cpu().numpy() for a in (out, gx, gW)]


def rel_run(be, c):
    T, D, Dout, R = c["shape"]
    out, gx, gW = Guarded(T * Dout), Guarded(T * D), Guarded(R * D * Dout)
    rc = [be.rel_mm(c["x"], c["order"], c["rel"], c["W"], T, D, Dout, 0, out),
          be.rel_mm(c["g"], c["order"], c["rel"], c["W"], T, Dout, D, 1, gx),
          be.rel_wgrad(c["x"], c["g"], c["order"], c["seg"], R, D, Dout, gW)]
    return [out.cells().reshape(T, Dout).copy(), gx.cells().reshape(T, D).copy(), gW.cells().reshape(R, D, Dout).copy()], rc, dict(out=out, g_x=gx, g_W=gW)


REL_OUT = ("out", "g_x", "g_W")


def rel_band(got, c, device, label, bad):
    """The band of part 3 on [out, g_x, g_W] (numpy) plus the exact zeros of relations without rows."""
    ref, chain = c["ref"], rel_chain(c, torch.float32, device)
    for what, f, ch, r in zip(REL_OUT, got, chain, ref):
        e = lambda a: float(np.max(np.abs(np.asarray(a, np.float64) - r)) / np.abs(r).max())
        _band("rel_mm", what, label, e(f), e(ch), bad)
    R = c["shape"][3]
    empty = [r for r in range(R) if c["seg"][r] == c["seg"][r + 1]]
    if any(np.any(got[2][r] != 0) for r in empty):
        bad.append("%s g_W of a relation without rows is not exactly zero" % label)


def rel_failures(be, shape):
    c = rel_case(shape)
    label = "x".join(map(str, shape))
    got, rc, guards = rel_run(be, c)
    if any(rc):
        return ["%s: return codes %s" % (label, rc)]
    bad = []
    rel_band(got, c, be.device, label, bad)
    for what, g in guards.items():
        if not (g.intact() and g.written()):
            bad.append("%s guard %s" % (label, what))
    again, _, _ = rel_run(be, c)
    for what, a, b in zip(REL_OUT, got, again):
        if not bits_equal(a, b):
            bad.append("%s %s: two calls differ" % (label, what))
    return bad
