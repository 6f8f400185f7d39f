"""Every edge kernel instance of the project-then-aggregate attention (csrc/gat.hip) against float64, through the C ABI
(recon_gat_edge_fwd, recon_gat_bwd without its GEMMs) with buffers the test owns.

pick_shape() maps a head width D and what the pointers allow to (VEC, G, KR) — load width, lanes per (node, head) group, register rows
per lane — and RECON_DISPATCH_SHAPE instantiates k_gat_edge_fwd<TRAIN = true / false>, k_gat_edge_bwd and k_gat_src_gather for each of the
21 shapes.  recon_gat_edge_instance() names the shape as vec * 10000 + g * 100 + kr; every row of PROJ_ROWS carries the key it must
select.  tests/test_proj_instances_cpu.py fails when a reachable key has no row, and runs this file's harness on a float32 restatement
and on nine subtly wrong ones.

Rows per key: one whose D ends inside the last register row (lanes of the group inactive), one at the key's exact upper width, and for
KR = 4 / 8 one with three / five live register rows.  VEC = 2 / 1 at D % 4 == 0 exists only for operands that are 8 / 4 bytes aligned:
those rows (`off` = 2 / 1) place P, Q, a_2, out, grad_out, Gm, gP and partial two / one floats into their buffers and use
ld_out = ld_gout = H * D + off.  Half of the other rows have `pad` = 4: ld_out = H * D + 4 and ld_gout = H * D + 8, which no load width
minds, so every VEC also sees leading dimensions that differ from H * D and from each other.  Graphs: `small` (N = 203: in- and
out-degrees 0 ... 9 and ~150, duplicated edges, eight trailing nodes without in-edges), `tall8 ... tall64` (a second, partly filled pass of the backward's node loop), `tiny` (one workgroup), `none` (E = 0).

Reference: the operation as include/recon_hip.h states it, in float64 torch on the CPU; the backward is autograd through that forward.
Bands (u = 2^-24; M = |P_dst| + |P_src| + |Q|; first-order bounds of the float32 evaluation, doubled for the second order):
  m       2u M
  sigma   tau = (D + 2) u sum_d |a_2| M
  w       relative rho = lambda tau + (|lambda sigma| + 4) u, lambda = 1 (sigma > 0) or alpha: the argument's error, its rounding, and
          expf (1 ulp = 2u in the HIP math tables) with the final rounding
  Z       relative zeta = max rho + (deg + 1) u
  U       dU = sum_k keep w (|m| (rho + (deg + 2) u) + 2u M)
  out     dy = (dU + |U| (zeta + u)) / Z + 2u |out|  (expm1f: 1 ulp)
  backward, which is given the device's own out, sigma and Z (errors dy, tau, zeta against the reference):
  g_h     d = |g_y| dy + 2u |g_h| where ELU is on its exponential side;  g_h h: |g_y| dy (1 + |h|) + 4u |g_h h|  (h = log1p(y))
  g_U     (d + |g_h| (zeta + u)) / Z;   g_Z: (sum_d d(g_h h) + (D + 2) u sum_d |g_h h| + |dot| (zeta + u)) / Z
  t       sum_d (d g_U |m| + |g_U| 2u M) + (D + 2) u sum_d |g_U| |m|;   g_w: keep dt + d g_Z + 2u (|keep t| + |g_Z|)
  g_s     lambda w (d g_w + |g_w| (rho + 3u))
  Gm      keep w (d g_U + |g_U| (rho + u)) + d g_s |a_2| + 2u (|keep w g_U| + |g_s a_2|)
  gP      sum of d Gm + (degree + 1) u sum |Gm| over the row's slots (destination rows) / the source's slots
  g_a_2   sum_k (d g_s |m| + |g_s| 2u M) + (E + 64) u sum_k |g_s m|: one chain of at most E additions, the LDS and partial-row sums

LeakyReLU's kink: the inputs are made so that every |sigma| is at least 96 tau_max (asserted at 64 tau per edge by the CPU file); two
destinations of `small` have all their scores near +60 and -150 (w ~ 1e-26 and ~ e^(150 alpha)), every w stays inside [1e-30, 1e30].

Every buffer the library writes or reads through an offset pointer is a view inside memory filled with one NaN pattern, which must
still surround it afterwards (and fill the pad columns of out).  Tables, reference and harness are module-level and touch no device.
"""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
GUARD = 64                                      # floats of NaN in front of and behind every view (256 bytes)
NAN_BITS = 0x7FC0BEEF
SLACK = 2.0                                     # second order
FLOOR = 1e-30
ALIGN = {0: 4, 2: 2, 1: 1}                      # off -> align_floats
HEAD_SCALE = (1.0, 0.45, 1.7)
NODE_POS, NODE_NEG = 30, 40                     # destinations of `small` whose scores sit near +60 / -150
ERR_INVALID, ERR_UNSUPPORTED = -1, -2

Row = collections.namedtuple("Row", "key D H concat alpha graph off pad seed note")

# (vec, g, kr) -> (tail D, exact D[, D with three / five live register rows]) in units of vec 4; vec 2 / 1 rows below
_SHAPES = [(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 8)]
_D4 = [(20, 32), (44, 64), (100, 128), (200, 256), (388, 512), (900, 1024, 600), (1900, 2048, 1100)]
_D2 = [(10, 16), (22, 32), (50, 64), (102, 128), (198, 256), (450, 512, 302), (950, 1024, 550)]        # tails and 302 / 550: D % 4 == 2
_D1 = [(5, 8), (13, 16), (25, 32), (51, 64), (101, 128), (225, 256, 161), (481, 512, 301)]             # odd D, 25: the reference's width


def _rows():
    rows = []

    def add(key, D, off, note, H=None, graph="small", pad=None):
        i = len(rows)
        H = H if H is not None else (1, 2, 3)[i % 3]
        pad = pad if pad is not None else (4 if off == 0 and i % 4 in (1, 2) else 0)
        rows.append(Row(key, D, H, i % 2 == 0, 0.35 if i % 3 == 1 else 0.2, graph, off, pad, 100 + i, note))

    for vec, widths in ((4, _D4), (2, _D2), (1, _D1)):
        exact_off = {4: 0, 2: 2, 1: 1}[vec]
        for (g, kr), ds in zip(_SHAPES, widths):
            key = vec * 10000 + g * 100 + kr
            add(key, ds[0], 0, "ends inside the last register row", H=1 if ds[0] == 1900 else None)
            add(key, ds[1], exact_off, "exact upper width", H=3 if ds[1] == 2048 else None)
            if len(ds) > 2:
                add(key, ds[2], 0, "%d live register rows of %d" % (kr // 2 + 1, kr), H=2 if ds[2] == 1100 else None)
    # D = 64 at what the pointers and leading dimensions allow
    add(41601, 64, 0, "demoted: 16-byte operands, ld = H D", H=2, pad=0)
    add(23201, 64, 2, "demoted: 8-byte operands, ld = H D + 2", H=2)
    add(16401, 64, 1, "demoted: 4-byte operands, ld = H D + 1", H=2)
    for g, D in ((8, 4), (16, 36), (32, 68), (64, 132)):
        add(40000 + g * 100 + 1, D, 0, "second pass of the backward's node loop", H=1, graph="tall%d" % g)
    add(40801, 20, 0, "one workgroup", H=2, graph="tiny")
    add(23201, 50, 0, "no edges", H=2, graph="none")
    return rows


PROJ_ROWS = _rows()
KEYS = sorted({v * 10000 + g * 100 + kr for v in (4, 2, 1) for g, kr in _SHAPES})


def row_id(r):
    return "k%d-D%d-H%d-%s-o%d" % (r.key, r.D, r.H, r.graph, r.off)


def key_parts(key):
    return key // 10000, key // 100 % 100, key % 100


# ------------------------------------------------------------------------------------------------------------------------ graphs
SMALL_DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9)
_GRAPHS, _CSR = {}, {}


def small_graph():
    """COO [2, E] (row 0 = destination) over N = 203 nodes, E ~ 1.3 k: destination 1 has ~150 in-edges and source 2 feeds ~140; destinations
    10 ... 17 have in-degrees 1, 2, 3, 4, 5, 7, 8, 9 and sources 20 ... 27 those out-degrees exactly; destination 5 and the last eight nodes
    have no in-edges, source 28 no out-edges; node 202 is a source and node 0 a destination; 40 edges appear twice and one three times;
    columns shuffled."""
    rs = np.random.RandomState(20240917)
    N = 203
    degs = rs.randint(1, 11, size=N)
    degs[1] = 150
    degs[10:18] = SMALL_DEGREES[1:]
    degs[[5] + list(range(195, 203))] = 0
    dst = np.repeat(np.arange(N), degs)
    src = rs.randint(0, N, size=dst.size)
    special = np.isin(src, [2] + list(range(20, 29)))
    src[special] = 50 + src[special] * 3                      # sources 2, 20 ... 28 get exactly what follows
    pos = rs.permutation(dst.size)
    src[pos[:140]] = 2
    at = 140
    for node, d in zip(range(20, 28), SMALL_DEGREES[1:]):
        src[pos[at:at + d]] = node
        at += d
    src[pos[at:at + 3]] = 202
    edge = np.stack([dst, src])
    free = np.nonzero(~np.isin(dst, range(10, 18)) & ~np.isin(src, range(20, 29)))[0]
    dup = edge[:, free[rs.permutation(free.size)[:40]]]
    one = edge[:, [free[7]]]
    edge = np.concatenate([edge, dup, one, one], axis=1)
    return edge[:, rs.permutation(edge.shape[1])], N


def tall_graph(g):
    """N = 256 (256 / g) + (256 / g) / 2 + 1 nodes, E = 2 N: k_gat_edge_bwd's 256 workgroups make a second pass in which only the first
    (256 / g) / 2 + 1 groups of the first workgroup have a node; every such node has an in-edge."""
    gpb = 256 // g
    N = 256 * gpb + gpb // 2 + 1
    rs = np.random.RandomState(g)
    dst, src = rs.randint(0, N, size=2 * N), rs.randint(0, N, size=2 * N)
    second = np.arange(256 * gpb, N)
    dst[:second.size] = second
    edge = np.stack([dst, src])
    return edge[:, rs.permutation(2 * N)], N


def graph_edges(name):
    if name not in _GRAPHS:
        if name == "small":
            _GRAPHS[name] = small_graph()
        elif name.startswith("tall"):
            _GRAPHS[name] = tall_graph(int(name[4:]))
        elif name == "tiny":
            _GRAPHS[name] = (np.array([[0, 2, 0, 2, 2], [1, 0, 2, 0, 1]]), 3)
        else:
            _GRAPHS[name] = (np.zeros((2, 0), dtype=np.int64), 37)
    return _GRAPHS[name]


def csr(name):
    """The index arrays of recon_graph in numpy's stable order (tests/test_gat_gpu.py::test_graph_build holds GraphCSR to the same)."""
    if name not in _CSR:
        edge, N = graph_edges(name)
        eid = np.argsort(edge[0], kind="stable")
        dst, src = edge[0][eid], edge[1][eid]
        deg, outdeg = np.bincount(edge[0], minlength=N), np.bincount(edge[1], minlength=N)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))
        _CSR[name] = dict(N=N, E=edge.shape[1], eid=t(eid), dst=t(dst), src=t(src), deg=t(deg), outdeg=t(outdeg),
                          rowptr=t(np.concatenate([[0], np.cumsum(deg)])), rowptr_src=t(np.concatenate([[0], np.cumsum(outdeg)])),
                          slot_by_src=t(np.argsort(src, kind="stable")))
    return _CSR[name]


# ---------------------------------------------------------------------------------------------------------- inputs and float64
def _colscale(n, mul=7):
    """per-column factors in [0.25, 1.75]: a column read in place of another, or twice, is far outside every band"""
    return 0.25 + 1.5 * torch.from_numpy(((np.arange(n) * mul) % 13) / 12.0).float()


def alpha32(row):
    return float(np.float32(row.alpha))                      # what the kernels multiply by


def _scores64(row, c, P, Q, a2, h):
    """(m, M, sigma, tau) of head h in float64"""
    Pd, Ps, Qh, ah = P[0, h].double(), P[1, h].double(), Q[h].double(), a2[h].double()
    m = (Pd[c["dst"]] + Ps[c["src"]]) + Qh
    M = Pd[c["dst"]].abs() + Ps[c["src"]].abs() + Qh.abs()
    return m, M, m @ ah, (row.D + 2) * U32 * (M @ ah.abs())


def make_inputs(row):
    """float32 P [2, H, N, D], Q [H, E, D] and keep [H, E] (both drawn in edge order, stored in slot order: the same rows whatever order a
    build gives equal destinations), a_2 [H, D], grad_out [N, H D]."""
    c = csr(row.graph)
    N, E, D, H = c["N"], c["E"], row.D, row.H
    g = torch.Generator().manual_seed(row.seed)
    hs = torch.tensor(HEAD_SCALE[:H])
    P = torch.randn(2, H, N, D, generator=g) * _colscale(D) * hs[None, :, None, None]
    Q = (torch.randn(H, E, D, generator=g) * _colscale(D, 5) * hs[:, None, None])[:, c["eid"]].contiguous()
    a2 = torch.randn(H, D, generator=g) * _colscale(D, 3)
    keep = ((torch.rand(H, E, generator=g) > 0.3).float() / 0.7)[:, c["eid"]].contiguous()
    gout = torch.randn(N, H * D, generator=g) * _colscale(D, 11).repeat(H)
    pick = torch.rand(H, E, generator=g, dtype=torch.float64)[:, c["eid"]]
    for h in range(H if E else 0):
        _, _, s0, _ = _scores64(row, c, P, Q, a2, h)
        a2[h] = (a2[h].double() * (2.5 / float(s0.std(unbiased=False)))).float()         # scores spread over about +-6
        _, _, s0, tau = _scores64(row, c, P, Q, a2, h)
        lo = max(0.25, 96.0 * float(tau.max()))
        sign = torch.where(s0 < 0, -1.0, 1.0).double()
        target = torch.where(s0.abs() < lo, sign * lo * (1.0 + 0.5 * pick[h]), s0)
        if row.graph == "small":
            target = torch.where(c["dst"] == NODE_POS, 58.0 + 4.0 * pick[h], target)
            target = torch.where(c["dst"] == NODE_NEG, -152.0 + 4.0 * pick[h], target)
        ah = a2[h].double()
        Q[h] = (Q[h].double() + (target - s0)[:, None] * (ah / (ah @ ah))[None, :]).float()
    return dict(P=P, Q=Q, a2=a2, keep=keep, gout=gout)


def _seg(index, values, n):
    return torch.zeros((n,) + tuple(values.shape[1:]), dtype=values.dtype).index_add_(0, index, values)


def forward64(row, c, Pd, Ps, Qh, ah, keep):
    """One head of the header's formulas in float64 (autograd-capable): dict(m, sigma, w, Z, U, h, out)"""
    al = alpha32(row)
    m = (Pd[c["dst"]] + Ps[c["src"]]) + Qh
    sigma = m @ ah
    w = torch.exp(-torch.where(sigma > 0, sigma, al * sigma))
    Z = _seg(c["dst"], w, c["N"])
    Z = torch.where(Z == 0, torch.full_like(Z, 1e-12), Z)
    U = _seg(c["dst"], (keep * w)[:, None] * m, c["N"])
    hh = U / Z[:, None]
    out = torch.where(hh > 0, hh, torch.expm1(hh)) if row.concat else hh
    return dict(m=m, sigma=sigma, w=w, Z=Z, U=U, h=hh, out=out)


def forward_bands(row, c, f, M, tau, keep):
    """first-order bands of one head's forward (see the file header): dict(dm, rho, zeta, out, sigma, Z)"""
    al, N = alpha32(row), c["N"]
    lam = torch.where(f["sigma"] > 0, 1.0, al).double()
    rho = lam * tau + ((lam * f["sigma"]).abs() + 4) * U32
    deg = c["deg"].double()
    rmax = torch.zeros(N, dtype=torch.float64).scatter_reduce_(0, c["dst"], rho, "amax", include_self=True)
    zeta = rmax + (deg + 1) * U32
    dm = 2 * U32 * M
    dU = _seg(c["dst"], (keep * f["w"])[:, None] * (f["m"].abs() * (rho + (deg[c["dst"]] + 2) * U32)[:, None] + dm), N)
    dy = (dU + f["U"].abs() * (zeta + U32)[:, None]) / f["Z"][:, None] + 2 * U32 * f["out"].abs()
    return dict(dm=dm, rho=rho, zeta=zeta, lam=lam, out=dy, sigma=tau, Z=zeta * f["Z"])


def backward_bands(row, c, f, b, ah, keep, gy):
    """magnitudes of one head's backward in float64 from the header's formulas, and the first-order bands built from them:
    dict(Gm, gPd, gPs, ga2) of (value, band); the values are only cross-checked against autograd by the CPU file"""
    N, E, D = c["N"], c["E"], row.D
    dst, src = c["dst"], c["src"]
    hh, Z, m, w = f["h"], f["Z"], f["m"], f["w"]
    dy, zeta, rho, lam, dm = b["out"], b["zeta"], b["rho"], b["lam"], b["dm"]
    if row.concat:
        neg = (hh <= dy).double()                                        # where the device may be on ELU's exponential side
        gh = torch.where(hh <= 0, gy * torch.exp(hh), gy)
    else:
        neg, gh = torch.zeros_like(hh), gy
    prod = gh * hh
    dgh = neg * (gy.abs() * dy + 2 * U32 * gh.abs())
    dprod = gy.abs() * dy * (1 + neg * hh.abs()) + 4 * U32 * prod.abs()
    zu = (zeta + U32)[:, None]
    gU = gh / Z[:, None]
    dgU = (dgh + gh.abs() * zu) / Z[:, None]
    dot = prod.sum(1)
    ddot = dprod.sum(1) + (D + 2) * U32 * prod.abs().sum(1)
    gZ = -dot / Z
    dgZ = (ddot + dot.abs() * (zeta + U32)) / Z
    gUe, dgUe = gU[dst], dgU[dst]
    t = (gUe * m).sum(1)
    dt = (dgUe * m.abs() + gUe.abs() * dm).sum(1) + (D + 2) * U32 * (gUe.abs() * m.abs()).sum(1)
    gw = keep * t + gZ[dst]
    dgw = keep * dt + dgZ[dst] + 2 * U32 * ((keep * t).abs() + gZ[dst].abs())
    gs = -gw * w * lam
    dgs = lam * w * (dgw + gw.abs() * (rho + 3 * U32))
    kw = keep * w
    Gm = kw[:, None] * gUe + gs[:, None] * ah[None, :]
    dGm = kw[:, None] * (dgUe + gUe.abs() * (rho + U32)[:, None]) + dgs[:, None] * ah.abs()[None, :] \
        + 2 * U32 * ((kw[:, None] * gUe).abs() + (gs[:, None] * ah[None, :]).abs())
    deg, outdeg = c["deg"].double(), c["outdeg"].double()
    gPd = (_seg(dst, Gm, N), _seg(dst, dGm, N) + ((deg + 1) * U32)[:, None] * _seg(dst, Gm.abs(), N))
    gPs = (_seg(src, Gm, N), _seg(src, dGm, N) + ((outdeg + 1) * U32)[:, None] * _seg(src, Gm.abs(), N))
    ga2 = (gs @ m, dgs @ m.abs() + gs.abs() @ dm + (E + 64) * U32 * (gs.abs() @ m.abs()))
    return dict(Gm=(Gm, dGm), gPd=gPd, gPs=gPs, ga2=ga2)


Case = collections.namedtuple("Case", "row c inp ref band info")
_CASES = collections.OrderedDict()


def make_case(row):
    """Inputs, float64 reference and bands of a row (the last two rows stay cached: the GEMM-family passes of a row follow each other).
    ref / band: out, eval [N, H D]; sigma [H, E]; Z [H, N]; Gm [H, E, D]; gP [2, H, N, D]; g_a_2 [H, D].
    info: w_min, w_max, margin (the smallest |sigma| / tau) and `formula` (the largest distance, in bands, between autograd and the
    hand-written backward the bands are built from)."""
    if row in _CASES:
        _CASES.move_to_end(row)
        return _CASES[row]
    c, inp = csr(row.graph), make_inputs(row)
    N, E, D, H = c["N"], c["E"], row.D, row.H
    ref, band = collections.defaultdict(list), collections.defaultdict(list)
    info = dict(w_min=float("inf"), w_max=0.0, margin=float("inf"), formula=0.0)
    for h in range(H):
        leaves = [t.double().requires_grad_(True) for t in (inp["P"][0, h], inp["P"][1, h], inp["Q"][h], inp["a2"][h])]
        keep, gy = inp["keep"][h].double(), inp["gout"][:, h * D:(h + 1) * D].double()
        f = forward64(row, c, *leaves, keep)
        grads = torch.autograd.grad((f["out"] * gy).sum(), leaves, allow_unused=True)
        grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
        with torch.no_grad():
            f = {k: v.detach() for k, v in f.items()}
            Pd, Ps, Qh, ah = (t.detach() for t in leaves)
            _, M, _, tau = _scores64(row, c, inp["P"], inp["Q"], inp["a2"], h)
            fb = forward_bands(row, c, f, M, tau, keep)
            ones = torch.ones_like(keep)
            fe = forward64(row, c, Pd, Ps, Qh, ah, ones)
            fbe = forward_bands(row, c, fe, M, tau, ones)
            bb = backward_bands(row, c, f, fb, ah, keep, gy)
            for name, val, bnd in (("out", f["out"], fb["out"]), ("eval", fe["out"], fbe["out"]), ("sigma", f["sigma"], fb["sigma"]),
                                   ("Z", f["Z"], fb["Z"]), ("Gm", grads[2], bb["Gm"][1]), ("gPd", grads[0], bb["gPd"][1]),
                                   ("gPs", grads[1], bb["gPs"][1]), ("g_a_2", grads[3], bb["ga2"][1])):
                ref[name].append(val)
                band[name].append(SLACK * bnd + FLOOR)
            for name, g in (("Gm", grads[2]), ("gPd", grads[0]), ("gPs", grads[1]), ("ga2", grads[3])):
                if g.numel():
                    info["formula"] = max(info["formula"], float(((bb[name][0] - g).abs() / (SLACK * bb[name][1] + FLOOR)).max()))
            if E:
                info["w_min"], info["w_max"] = min(info["w_min"], float(f["w"].min())), max(info["w_max"], float(f["w"].max()))
                info["margin"] = min(info["margin"], float((f["sigma"].abs() / tau).min()))
    stk =lambda name: (torch.stack(ref[name]), torch.stack(band[name]))
    R, B = {}, {}
    for name in ("out", "eval"):
        R[name], B[name] = torch.cat(ref[name], 1), torch.cat(band[name], 1)
    for name in ("sigma", "Z", "Gm", "g_a_2"):
        R[name], B[name] = stk(name)
    R["gP"] = torch.stack([torch.stack(ref["gPd"]), torch.stack(ref["gPs"])])
    B["gP"] = torch.stack([torch.stack(band["gPd"]), torch.stack(band["gPs"])])
    case = Case(row, c, inp, R, B, info)
    _CASES[row] = case
    while len(_CASES) > 2:
        _CASES.popitem(last=False)
    return case


# ------------------------------------------------------------------------------------------------------------------ the harness
# A backend answers
#   fwd(case, train) -> dict(out [N, H D], and for train: sigma [H, E], Z [H, N]) of float32 CPU tensors
#   bwd(case, out, sigma, Z) -> dict(Gm [H, E, D], gP [2, H, N, D], g_a_2 [H, D])
def _held(name, got, ref, band, ratios):
    """Assert a finite result of the reference's shape with |got - ref| <= band elementwise; ratios[name] = the worst error / band."""
    assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s, reference %s" % (name, tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    q = (got.double() - ref).abs() / band
    worst = float(q.max())
    ratios[name] = max(ratios.get(name, 0.0), worst)
    if worst > 1.0:
        at = np.unravel_index(int(q.argmax()), tuple(q.shape))
        raise AssertionError("%s: error / band = %.3f at %s (got %.9g, reference %.9g)" % (name, worst, at, float(got[at]), float(ref[at])))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_row(backend, row, repeat=True):
    """One row of PROJ_ROWS with every assertion it carries; returns {output: worst error / band}."""
    case = make_case(row)
    c, R, B = case.c, case.ref, case.band
    N, E, D, H = c["N"], c["E"], row.D, row.H
    ratios = {}
    f1 = backend.fwd(case, True)
    for name in ("out", "sigma", "Z"):
        _held(name, f1[name], R[name], B[name], ratios)
    _held("eval", backend.fwd(case, False)["out"], R["eval"], B["eval"], ratios)
    empty = c["deg"] == 0
    if bool(empty.any()):                                                # rows without in-edges: act(0 / 1e-12) = 0 exactly
        assert not bool(f1["out"][empty].any()), "rows without in-edges: out is not 0"
        assert bool((f1["Z"][:, empty] == torch.tensor(1e-12, dtype=torch.float32)).all()), "rows without in-edges: Z is not 1e-12"
    b1 = backend.bwd(case, f1["out"], f1["sigma"], f1["Z"])
    for name in ("Gm", "gP", "g_a_2"):
        _held(name, b1[name], R[name], B[name], ratios)
    if bool(empty.any()):
        assert not bool(b1["gP"][0][:, empty].any()), "rows without in-edges: gP[0] is not 0"
    if E == 0:
        assert not bool(b1["gP"].any()) and not bool(b1["g_a_2"].any()), "no edges: a non-zero gradient"
    if repeat:
        f2 = backend.fwd(case, True)
        b2 = backend.bwd(case, f1["out"], f1["sigma"], f1["Z"])
        for name in ("out", "sigma", "Z"):
            assert _same_bits(f1[name], f2[name]), "%s differs between two identical calls (fixed-order sums)" % name
        for name in ("Gm", "gP", "g_a_2"):
            assert _same_bits(b1[name], b2[name]), "%s differs between two identical calls (fixed-order sums)" % name
    return ratios


def _report(rid, ratios):
    print("PROJ_INST %s %s" % (rid, " ".join("%s=%.4f" % kv for kv in sorted(ratios.items()))))


# --------------------------------------------------------------------------------------------------------------- on the device
def _dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


class _View:
    """n floats, `off` floats past a 256-byte boundary, inside a buffer filled with one NaN pattern (GUARD floats and more on both sides)."""

    def __init__(self, n, off=0, data=None):
        self.n, self.off = n, off
        self.buf = torch.full((n + 2 * GUARD + 4,), NAN_BITS, dtype=torch.int32, device=_dev())
        assert self.buf.data_ptr() % 256 == 0
        self.lo = GUARD + off
        self.ptr = self.buf.data_ptr() + 4 * self.lo
        if data is not None:
            assert data.numel() == n and data.dtype == torch.float32
            self.words().copy_(data.contiguous().view(-1).view(torch.int32))

    def words(self):
        return self.buf[self.lo:self.lo + self.n]

    def surroundings_intact(self):
        return bool((self.buf[:self.lo] == NAN_BITS).all()) and bool((self.buf[self.lo + self.n:] == NAN_BITS).all())

    def untouched(self):
        return bool((self.buf == NAN_BITS).all())

    def get(self, *shape):
        return self.words().view(torch.float32).cpu().clone().view(*shape)


def _padded(t, ld):
    """[N, C] float32 -> [N, ld] with the NaN pattern in the pad columns"""
    full = torch.full((t.shape[0], ld), NAN_BITS, dtype=torch.int32).view(torch.float32)
    full[:, :t.shape[1]] = t
    return full


_DEV_GRAPHS = {}


def device_graph(name):
    """GraphCSR of a graph of this file, its index arrays held to csr()"""
    if name not in _DEV_GRAPHS:
        from recon_amd.graph import GraphCSR
        edge, N = graph_edges(name)
        G = GraphCSR(torch.from_numpy(np.ascontiguousarray(edge)).long().to(_dev()), N)
        G.c
        torch.cuda.synchronize()
        c = csr(name)
        for mine, theirs in (("rowptr", G.rowptr_dst), ("src", G.src), ("eid", G.eid), ("rowptr_src", G.rowptr_src), ("slot_by_src", G.slot_by_src)):
            assert torch.equal(theirs.cpu().long(), c[mine]), "%s: GraphCSR.%s differs from numpy's stable order" % (name, mine)
        _DEV_GRAPHS[name] = G
    return _DEV_GRAPHS[name]


class DeviceBackend:
    """The two library calls on views this class owns."""

    def __init__(self):
        from recon_amd import _lib
        self.L, self._lib = _lib.lib(), _lib
        self._up = None
        self.dummy = _View(16)                                           # x, a, edge_embed: required, never read without the GEMMs

    def _inputs(self, case):
        if self._up is None or self._up[0] is not case:
            row, inp = case.row, case.inp
            self._up = (case, dict(P=_View(inp["P"].numel(), row.off, inp["P"]), Q=_View(inp["Q"].numel(), row.off, inp["Q"]),
                                   a2=_View(inp["a2"].numel(), row.off, inp["a2"]), keep=_View(inp["keep"].numel(), 0, inp["keep"]),
                                   gout=_View(case.c["N"] * self.ld_gout(row), row.off, _padded(inp["gout"], self.ld_gout(row)))))
        return self._up[1]

    @staticmethod
    def ld(row):
        return row.H * row.D + row.off + row.pad

    @staticmethod
    def ld_gout(row):
        return row.H * row.D + row.off + 2 * row.pad

    def _args(self, case, d, out, sigma, Z, keep, ld=None, D=None):
        row, c = case.row, case.c
        A = self._lib.GatFwdArgs
        return A(N=c["N"], E=c["E"], F=1, R=1, D=D or row.D, H=row.H, concat=int(row.concat), alpha=row.alpha, x=self.dummy.ptr,
                 edge_embed=self.dummy.ptr, a=self.dummy.ptr, a_2=d["a2"].ptr, keep=keep, P=d["P"].ptr, Q=d["Q"].ptr, sigma=sigma, Z=Z,
                 out=out, ld_out=self.ld(row) if ld is None else ld)

    def fwd(self, case, train, expect=0):
        row, c = case.row, case.c
        N, E, D, H = c["N"], c["E"], row.D, row.H
        G, d, ld = device_graph(row.graph), self._inputs(case), self.ld(row)
        out, sigma, Z = _View(N * ld, row.off), _View(H * E), _View(H * N)
        args = self._args(case, d, out.ptr, sigma.ptr if train else None, Z.ptr if train else None, d["keep"].ptr if train else None)
        rc = self.L.recon_gat_edge_fwd(C.byref(G.c), C.byref(args), self._lib.current_stream())
        torch.cuda.synchronize()
        assert rc == expect, "recon_gat_edge_fwd returned %d" % rc
        for name, v, written in (("out", out, rc == 0), ("sigma", sigma, train and rc == 0), ("Z", Z, train and rc == 0)):
            if written:
                assert v.surroundings_intact(), "written outside " + name
            else:
                assert v.untouched(), "%s was written by a call that must not" % name
        for name, v in d.items():
            assert v.surroundings_intact(), "written around the input " + name
        if rc != 0:
            return None
        full = out.words().view(N, ld)
        assert bool((full[:, H * D:] == NAN_BITS).all()), "the pad columns of out were written"
        res = dict(out=full[:, :H * D].view(torch.float32).cpu().clone())
        if train:
            res.update(sigma=sigma.get(H, E), Z=Z.get(H, N))
        return res

    def bwd(self, case, out, sigma, Z, expect=0):
        row, c = case.row, case.c
        N, E, D, H = c["N"], c["E"], row.D, row.H
        G, d, ld = device_graph(row.graph), self._inputs(case), self.ld(row)
        outv = _View(N * ld, row.off, _padded(out, ld))
        sv, zv = _View(H * E, 0, sigma), _View(H * N, 0, Z)
        Gm, gP, ga2 = _View(H * E * D, row.off), _View(2 * H * N * D, row.off), _View(H * D)
        floats = self.L.recon_gat_bwd_partial_floats(N, E, 1, 1, D, H)
        partial = _View(floats, row.off)
        B = self._lib.GatBwdArgs(fwd=self._args(case, d, outv.ptr, sv.ptr, zv.ptr, d["keep"].ptr), grad_out=d["gout"].ptr, ld_gout=self.ld_gout(row),
                                 Gm=Gm.ptr, gP=gP.ptr, partial=partial.ptr, g_x=None, g_edge_embed=None, g_a=None, g_a_2=ga2.ptr)
        rc = self.L.recon_gat_bwd(C.byref(G.c), C.byref(B), self._lib.current_stream())
        torch.cuda.synchronize()
        assert rc == expect, "recon_gat_bwd returned %d" % rc
        for name, v in (("Gm", Gm), ("gP", gP), ("g_a_2", ga2), ("partial", partial), ("out", outv), ("sigma", sv), ("Z", zv)):
            if rc == 0:
                assert v.surroundings_intact(), "written outside " + name
            elif name in ("Gm", "gP", "g_a_2", "partial"):
                assert v.untouched(), "%s was written by a refused call" % name
        for name, v in d.items():
            assert v.surroundings_intact(), "written around the input " + name
        if rc != 0:
            return None
        return dict(Gm=Gm.get(H, E, D), gP=gP.get(2, H, N, D), g_a_2=ga2.get(H, D))


def pytest_generate_tests(metafunc):
    # here rather than as a mark so that the row comes first in the test ids; conftest adds the GEMM family
    if "row" in metafunc.fixturenames:
        metafunc.parametrize("row", PROJ_ROWS, ids=[row_id(r) for r in PROJ_ROWS])


def test_proj_instance_within_fp64_bands(row):
    from recon_amd import _lib
    assert _lib.lib().recon_gat_edge_instance(row.D, ALIGN[row.off]) == row.key, "the row's width and alignment select another instance"
    _report(row_id(row), check_row(DeviceBackend(), row))


def test_proj_no_edges_gives_zero_rows():
    """E = 0: the call succeeds and out = act(0) = 0 (Z = 1e-12, gradients zero: asserted by check_row for every row without in-edges)."""
    row = [r for r in PROJ_ROWS if r.graph == "none"][0]
    be = DeviceBackend()
    f = be.fwd(make_case(row), True)
    assert not bool(f["out"].any()) and f["out"].shape == (csr("none")["N"], row.H * row.D)
    assert not bool(be.fwd(make_case(row), False)["out"].any())


@pytest.mark.parametrize("D, off", [(2052, 0), (1026, 0), (1026, 2), (513, 0), (513, 1)])
def test_proj_refuses_widths_beyond_eight_register_rows(D, off):
    from recon_amd import _lib
    L = _lib.lib()
    assert L.recon_gat_edge_instance(D, ALIGN[off]) == -1
    row = Row(-1, D, 1, True, 0.2, "tiny", off, 0, 7, "refused")
    case = Case(row, csr("tiny"), make_inputs(row), None, None, None)
    be = DeviceBackend()
    assert be.fwd(case, True, expect=ERR_UNSUPPORTED) is None
    assert be.fwd(case, False, expect=ERR_UNSUPPORTED) is None
    N, E = case.c["N"], case.c["E"]
    assert be.bwd(case, torch.zeros(N, D), torch.zeros(1, E), torch.ones(1, N), expect=ERR_UNSUPPORTED) is None


def test_proj_rejects_keep_without_z_and_a_short_ld_out():
    row = [r for r in PROJ_ROWS if r.graph == "tiny"][0]
    case = make_case(row)
    be = DeviceBackend()
    G, d = device_graph("tiny"), be._inputs(case)
    N, ld = case.c["N"], be.ld(row)
    out = _View(N * ld)
    for args in (be._args(case, d, out.ptr, None, None, d["keep"].ptr),                            # keep on an inference call
                 be._args(case, d, out.ptr, None, None, None, ld=row.H * row.D - 1)):              # rows would overlap
        assert be.L.recon_gat_edge_fwd(C.byref(G.c), C.byref(args), be._lib.current_stream()) == ERR_INVALID
    torch.cuda.synchronize()
    assert out.untouched()
