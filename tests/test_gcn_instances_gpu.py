"""Every kernel of the bfloat16 GraphConvolution family (csrc/gcn_b16.hip and the parts of gemm_b16.hip it drives) against float64,
element by element, through the C ABI with buffers the test owns: recon_gcn_b16_fwd / _bwd (fixed-size and ragged),
recon_gcn_b16_stack_fwd, recon_gcn_b16_stack_train_fwd / _bwd and recon_gcn_b16_transposed_planes.

recon_gcn_b16_fwd_instance() / recon_gcn_b16_bwd_instance() name what a call launches (include/recon_hip.h); every row of GCN_ROWS
carries the key it must select.  tests/test_gcn_instances_cpu.py fails when a reachable key has no row, and runs this file's harness on
a float32-accumulate, bf16-round-to-nearest restatement of every stage (which must pass every band) and on nine subtly wrong ones (each
of which must fail).

Reference: float64 torch on the CPU of relu(adj @ (x @ W) + b) (models/layers.py:57-63) and its hand-written gradients
    gpre = grad_out * (out > 0),  g_support = adj^T gpre,  g_x = g_support W^T,  g_adj = gpre support^T,  g_W = x^T g_support,
    g_b = sum over rows of gpre.
Bands: u = 2^-8 (one bf16 round-to-nearest), v = 2^-23 (one fp32 accumulation step, doubled for the matrix cores' internal order); the
sum of the terms times 1 + 2^-6 for the second order.  First-order worst-case bounds: no measured figure enters, no element is excluded.
Where a product's operands and its result are all in memory, one rounding against float64 of the DEVICE's own operands:
    support                                  u |s|   + (I + 2) v sum |x| |W|
    out        given the device's support    u |pre| + (n + 2) v (sum |adj| |s| + |b|)        (ReLU is 1-Lipschitz: no mask exclusion)
    g_support  given grad_out, device out    u |.|   + (n + 2) v sum |adj| |gpre|             (the mask is the device's out > 0)
    g_x        given the device's g_support  u |.|   + (O + 2) v sum |g_support| |W|
    g_adj      given the device's support    u |.|   + (O + 2) v sum |gpre| |s|
    g_W        given the device's g_support  u |.|   + (rows + splits + 2) v sum |x| |g_support|
    g_b                                      u |.|   + (rows + 2) v sum |gpre|
Where the first product never leaves registers or LDS (the fused forward; every stack layer given the device's previous activation;
the stack backward's g_support_l given the device's g_support_l+1), two roundings against unstaged float64: the inner result's band
(its rounding u |inner| and its accumulation term) carried through |adj|, plus the outer product's own band as above.

Every buffer the library writes is a view inside memory filled with one NaN pattern, with a guard in front and behind, which must be
intact afterwards; the pad columns of out, support, g_support and of the stack's activations and g_support must be exactly zero up to the row stride.  Inputs: bf16 normal
x, W scaled by in^-0.5, a non-symmetric row-normalised adjacency with self loops that differs from graph to graph (a transpose or a graph
mix-up shows), a non-zero bias, a bf16 normal grad_out; `neg` rows flip the sign of adjacency entries so that |adj| in the bands matters.
Tables, reference, bands and harness are module-level and touch no device.
"""
import collections
import ctypes as C
import math
import types
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -8
V = 2.0 ** -23
SECOND = 1.0 + 2.0 ** -6
GUARD = 64                                      # elements of the fill pattern in front of and behind every view
NAN16, INF16, NAN32 = 0x7FD3, 0x7F80, 0x7FC0BEEF
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -2
F4, F2, GEMM, RAGGED = 1, 2, 3, 4               # forward keys
FUSED, AGG = 1, 2                               # backward paths
NO_BIAS, RIDES, ALONE = 0, 1, 2

Row = collections.namedtuple("Row", "kind key B n I O opts")


def opt(r, name, default=None):
    return dict(r.opts).get(name, default)


def bkey(path, g_adj, bias, splits):
    return path * 100000 + (1 if g_adj else 0) * 10000 + bias * 1000 + splits


def km_plan(M, N, K, count=1):
    """(splits, rows per split) of the k-major weight-gradient GEMM for a [K, M]^T [K, N] product: the rule of csrc/gemm_bx3.hip
    bx3_kmajor_split_k + gemm_tile16.h splitk_plan, restated (128 x 208 tiles, K steps of 32, at most K / 128 and 64 splits, 512
    workgroups aimed at)"""
    tiles = -(-M // 128) * -(-N // 208) * count
    assert tiles < 256
    max_s = min(64, max(1, K // 128))
    s = max(1, min(512 // tiles, max_s))
    kps = -(-(-(-max(K, 1) // s)) // 32) * 32
    return -(-max(K, 1) // kps), kps


def stack_km_plan(ins, D, rows, wanted):
    """(splits, rows per split) of the ONE k-major launch behind k_gcn_b16_stack_bwd: the products x_l^T g_support_l of the layers whose
    weight gradient is wanted share the split count of the largest of them (csrc/gcn_b16.hip recon_gcn_b16_stack_train_bwd,
    gemm_b16.hip gemm_b16_kmajor_multi)"""
    return km_plan(max(ins[l] for l in wanted), D, rows, len(wanted))


def stack_partial_floats(B, n, I, D, L):
    """recon_gcn_b16_stack_bwd_partial_floats restated: the partials of every layer at the largest split count any subset of the layers
    may run with, the per-graph column sums of the L bias gradients, and one"""
    sk = max(km_plan(M, D, B * n, c)[0] for M in (max(I, D), D) for c in range(1, L + 1))
    return sk * I * D + (L - 1) * sk * D * D + L * B * D + 1


def up8(v):
    return (v + 7) // 8 * 8


def kp(v):
    return (v + 31) // 32 * 32


def _sizes(r):
    return list(opt(r, "sizes") or [r.n] * r.B)


def _bwd_key(B, n, I, O, g_x=True, g_adj=False, g_w=True, g_b=True, force_agg=False, rows=None, ldgx=None, lds=None):
    rows = B * n if rows is None else rows
    fused = (not force_agg and not g_adj and g_x and n <= 32 and up8(O) <= 320 and up8(I) <= 320 and (lds or up8(O)) <= kp(O))
    bias = NO_BIAS if not g_b else (RIDES if g_w else ALONE)
    return bkey(FUSED if fused else AGG, g_adj, bias, km_plan(I, O, rows)[0] if g_w else 0)


def _rows():
    rows = []

    def add(kind, key, B, n, I, O, **kw):
        rows.append(Row(kind, key, B, n, I, O, tuple(sorted(kw.items()))))

    # ---- fused forward, 8-byte loads.  O around the wave parts of 80 columns, n around the row tile, B around four graphs per
    # workgroup, I around the K steps of 32
    O4 = (76, 80, 84, 156, 160, 164, 236, 240, 244, 300, 316, 320)
    n4, B4, I4 = (12, 16, 20, 28, 32), (1, 4, 5, 7), (2, 30, 32, 34, 64, 300, 320, 520)
    fused4 = [(1, 4, 8, 4)] + [(B4[i % 4], n4[i % 5], I4[i % 8], o) for i, o in enumerate(O4)]
    for i, (B, n, I, O) in enumerate(fused4):
        add("fwd", F4, B, n, I, O, neg=(i == 3))
    add("fwd", F4, 5, 16, 64, 80, bias=False)
    add("fwd", F4, 5, 12, 30, 84, ldx=30, xfill="inf")                  # in-place masked K tail: the next row / the guard behind
    add("fwd", F4, 3, 8, 34, 16, ldx=36, xfill="inf")                   # two cells of Inf behind each row's last feature
    add("fwd", F4, 5, 20, 300, 300, ldx=312, xfill="nan")               # padded rows, NaN in the pads (inference)
    add("fwd", F4, 5, 20, 64, 300, ldo=320)                             # pad columns 300 .. 320 of the last column tile
    add("fwd", F4, 2, 4, 8, 4, ldo=48)                                  # pad columns past the first column tile
    # ---- fused forward, element loads
    fused2 = [(1, 1, 8, 5), (5, 2, 30, 130), (7, 9, 33, 158), (4, 17, 64, 162), (3, 31, 300, 318)]
    for i, (B, n, I, O) in enumerate(fused2):
        add("fwd", F2, B, n, I, O, neg=(i == 2), ldx=I + (I & 1))
    add("fwd", F2, 5, 16, 32, 80, adj_off=1)                            # vector-friendly shape, adj at a 2-byte offset
    add("fwd", F2, 5, 16, 32, 80, bias_off=1)
    add("fwd", F2, 6, 32, 64, 320, adj_off=1, bias_off=1)
    add("fwd", F2, 3, 12, 16, 82)                                       # n % 4 == 0, out % 4 != 0
    # ---- GEMM + aggregate (`support` given): the shapes above, 32-row tiles and 32-wide contraction chunks, 64-column blocks
    for i, (B, n, I, O) in enumerate(fused4 + fused2):
        add("fwd", GEMM, B, n, I, O, support=True, neg=(i == 5))
    for i, (n, O) in enumerate(((33, 63), (64, 64), (65, 65), (100, 328))):
        add("fwd", GEMM, (3, 2, 2, 2)[i], n, (20, 33, 64, 40)[i], O, support=True)
    add("fwd", GEMM, 5, 16, 64, 80, support=True, cfg=(("RECON_GCN_FUSED", "0"),))
    add("fwd", GEMM, 3, 9, 24, 204, support=True, lds=224, ldo=216)     # support's pad columns past the GEMM's last column tile (208)
    add("fwd", GEMM, 2, 5, 8, 5, support=True, bias=False, lds=16, ldo=24)
    # ---- ragged
    add("fwd", RAGGED, 5, 256, 24, 40, support=True, sizes=(1, 5, 32, 33, 256), neg=True)
    add("fwd", RAGGED, 70, 3, 8, 12, support=True, sizes=(3,) * 70)
    add("fwd", RAGGED, 2, 129, 33, 70, support=True, sizes=(129, 64))
    add("fwd", 0, 3, 1, 8, 8, support=True, sizes=(0, 0, 0))            # total_rows == 0: nothing is launched, nothing written
    # ---- backward, fused
    nb, Bb, Ib, Ob = (2, 4, 9, 16, 17, 31, 32), (1, 5, 7), (7, 8, 33, 300, 320), (5, 16, 136, 300, 320)
    for i, n in enumerate(nb):
        B, I, O = Bb[i % 3], Ib[i % 5], Ob[i % 5]
        g_b, g_w = i % 2 == 0, i % 3 != 1
        add("bwd", _bwd_key(B, n, I, O, g_w=g_w, g_b=g_b), B, n, I, O, g_b=g_b, g_w=g_w, neg=(i == 2))
    add("bwd", _bwd_key(7, 32, 320, 320), 7, 32, 320, 320)
    add("bwd", _bwd_key(5, 16, 8, 16, g_w=False, g_b=False), 5, 16, 8, 16, g_w=False, g_b=False)
    add("bwd", _bwd_key(3, 12, 40, 12, g_b=False), 3, 12, 40, 12, bias=False, g_b=False)
    # ---- backward, aggregate + GEMM
    add("bwd", _bwd_key(5, 16, 33, 136, g_x=False), 5, 16, 33, 136, g_x=False)
    add("bwd", _bwd_key(5, 16, 33, 136, g_x=False, g_w=False), 5, 16, 33, 136, g_x=False, g_w=False)       # colsum of the aggregate, reduced alone
    add("bwd", _bwd_key(3, 8, 328, 16), 3, 8, 328, 16)                  # in rounded up to 8 = 328: past the fused tile
    add("bwd", _bwd_key(3, 8, 16, 328), 3, 8, 16, 328, support=True)    # out = 328: past the fused forward too
    add("bwd", _bwd_key(5, 16, 64, 80, force_agg=True), 5, 16, 64, 80, cfg=(("RECON_GCN_FUSED_BWD", "0"),))
    add("bwd", _bwd_key(3, 33, 20, 63), 3, 33, 20, 63, support=True, neg=True)
    add("bwd", _bwd_key(2, 100, 24, 65), 2, 100, 24, 65, support=True)
    add("bwd", _bwd_key(70, 2, 8, 12, g_w=False), 70, 2, 8, 12, g_w=False)                                 # k_gcn_b16_bias_reduce, 70 graphs: per = 2
    add("bwd", _bwd_key(70, 2, 8, 12, g_w=False, g_x=False), 70, 2, 8, 12, g_w=False, g_x=False)
    add("bwd", _bwd_key(4, 8, 16, 4, lds=40), 4, 8, 16, 4, lds=40)      # g_support's row stride past kp(out): the aggregate writes every pad column
    for n in (1, 17, 33):
        add("bwd", _bwd_key(3, n, 24, 37, g_adj=True), 3, n, 24, 37, support=True, g_adj=True, neg=(n == 17))
    add("bwd", _bwd_key(2, 8, 16, 24, g_adj=True, g_x=False, g_w=False, g_b=False), 2, 8, 16, 24, support=True, g_adj=True, g_x=False, g_w=False, g_b=False)
    # ---- weight gradient, split-K regimes at in = out = 8: one split, an intermediate count, more than 16 (k_b16_reduce: per = 2)
    add("bwd", bkey(FUSED, 0, RIDES, 1), 4, 32, 8, 8)
    add("bwd", bkey(FUSED, 0, RIDES, 4), 16, 32, 8, 8)
    add("bwd", bkey(FUSED, 0, RIDES, 17), 68, 32, 8, 8)
    add("bwd", bkey(FUSED, 0, NO_BIAS, 17), 68, 32, 8, 8, g_b=False, bias=False)
    # ---- the remaining combinations of path, d adj, bias mode and split regime (in = out = 8 at 512 and 2176 rows: 4 and 17 splits)
    add("bwd", bkey(FUSED, 0, NO_BIAS, 4), 16, 32, 8, 8, g_b=False)
    add("bwd", bkey(AGG, 0, NO_BIAS, 0), 3, 8, 16, 16, g_x=False, g_w=False, g_b=False)
    add("bwd", bkey(AGG, 0, NO_BIAS, 1), 3, 8, 16, 16, g_x=False, g_b=False)
    add("bwd", bkey(AGG, 1, NO_BIAS, 1), 3, 8, 16, 16, support=True, g_adj=True, g_b=False)
    add("bwd", bkey(AGG, 1, ALONE, 0), 3, 8, 16, 16, support=True, g_adj=True, g_w=False)
    for B, sp in ((16, 4), (68, 17)):
        add("bwd", bkey(AGG, 0, NO_BIAS, sp), B, 32, 8, 8, g_x=False, g_b=False)
        add("bwd", bkey(AGG, 0, RIDES, sp), B, 32, 8, 8, g_x=False)
        add("bwd", bkey(AGG, 1, NO_BIAS, sp), B, 32, 8, 8, support=True, g_adj=True, g_b=False)
        add("bwd", bkey(AGG, 1, RIDES, sp), B, 32, 8, 8, support=True, g_adj=True)
    # ---- ragged backward
    add("bwd", _bwd_key(4, 33, 24, 40, g_adj=True, rows=71), 4, 33, 24, 40, support=True, sizes=(1, 5, 32, 33), g_adj=True, neg=True)
    add("bwd", _bwd_key(2, 129, 33, 70, rows=193), 2, 129, 33, 70, support=True, sizes=(129, 64))
    add("bwd", 0, 2, 1, 8, 8, support=True, sizes=(0, 0))
    # ---- stack: (B, n, I, D) and L
    Ls, ns, Ds, Is, Bs = (2, 3, 8), (4, 8, 12, 32), (4, 64, 136, 300, 320), (2, 22, 37, 300, 320), (1, 5, 7)
    for i in range(5):
        add("stack", 0, Bs[i % 3], ns[i % 4], Is[i], Ds[i], L=Ls[i % 3], x_rows=Is[i] % 8 != 0, neg=(i == 1))
    add("stack", 0, 5, 12, 64, 64, L=3, frozen=1)                       # a frozen middle layer
    add("stack", 0, 5, 8, 40, 136, L=3, nobias=1)                       # a layer without bias
    add("stack", 0, 7, 32, 320, 320, L=2, g_x=False)
    add("stack", 0, 6, 16, 24, 20, L=2, ldo=32)                         # pad columns of acts and g_support up to kp(hidden): the widest training stride
    add("stack", 0, 6, 16, 24, 20, L=2, ldo=40, infer_only=True)        # inference: pad columns past kp(hidden)
    add("stack", 0, 5, 12, 384, 64, L=3, infer_only=True)               # the widest input whose activation images fit the LDS ...
    add("stack", 0, 3, 8, 384, 32, L=4, infer_only=True)                # ... beside the bias rows of at most four layers
    # ---- refusals of check(): status, and nothing written
    add("refuse", ERR_INVALID, 3, 8, 16, 16, ldx=17)                    # odd ldx
    add("refuse", ERR_INVALID, 3, 8, 16, 20, ldo=16)                    # ldo < out rounded up to 8
    add("refuse", ERR_INVALID, 3, 8, 16, 16, out_off=4)                 # `out` 8 bytes off a 16-byte boundary
    add("refuse", ERR_INVALID, 2, 33, 16, 16)                           # no `support` at n = 33
    add("refuse", ERR_INVALID, 3, 8, 16, 16, cfg=(("RECON_GCN_FUSED", "0"),))      # no `support` with the fused forward switched off
    add("refuse_bwd", ERR_INVALID, 3, 8, 16, 16, g_adj=True)            # d adj without `support`
    for B, n, I, D, L, infer in ((3, 8, 416, 64, 2, True), (3, 8, 328, 64, 2, False), (3, 6, 16, 16, 2, None), (3, 8, 16, 6, 2, None), (3, 8, 16, 16, 9, None),
                                 (3, 8, 384, 32, 5, True)):             # 384 inputs and the bias rows of five layers do not fit the LDS
        add("refuse_stack", ERR_UNSUPPORTED, B, n, I, D, L=L, infer=infer)
    add("refuse_stack", ERR_UNSUPPORTED, 6, 16, 24, 20, L=2, infer=False, ldo=40)      # training: g_support is written up to kp(hidden) = 32
    return rows


GCN_ROWS = _rows()


def _fmt(k, v):
    if v is True:
        return k
    if isinstance(v, tuple) and v and isinstance(v[0], tuple):          # config switches
        return "_".join(name[6:] + val for name, val in v)
    return "%s%s" % (k, v)


def row_id(r):
    tag = {"fwd": "f", "bwd": "b", "stack": "s", "refuse": "r", "refuse_bwd": "rb", "refuse_stack": "rs"}[r.kind]
    extra = "".join("-" + _fmt(k, v) for k, v in r.opts if v is not False and k != "sizes")
    s = opt(r, "sizes")
    if s is not None:
        extra += "-sizes%dx%d" % (len(s), max(s)) if len(set(s)) == 1 else "-sizes" + "_".join(str(v) for v in s)
    return "%s%d-B%d-n%d-I%d-O%d%s" % (tag, r.key, r.B, r.n, r.I, r.O, extra)


assert len({row_id(r) for r in GCN_ROWS}) == len(GCN_ROWS), "duplicate row ids"


# -------------------------------------------------------------------------------------------------------------------- buffers
class Guarded:
    """`nelem` elements of bf16 (or fp32) at `off` elements into memory filled with one pattern, GUARD elements in front and behind"""

    def __init__(self, nelem, dev, off=0, fp32=False, fill=None):
        self.fp32, self.lo, self.n = fp32, GUARD + off, nelem
        self.fill = (NAN32 if fp32 else NAN16) if fill is None else fill
        self.raw = torch.full((self.lo + nelem + GUARD,), self.fill, dtype=torch.int32 if fp32 else torch.int16, device=dev)
        self.view = self.raw[self.lo:self.lo + nelem].view(torch.float32 if fp32 else torch.bfloat16)

    def put(self, t, ld=None):
        """t [rows, cols] into rows of ld elements (pads keep the fill), or a flat tensor"""
        if ld is None:
            self.view[:t.numel()].copy_(t.reshape(-1))
        else:
            self.view[:t.shape[0] * ld].view(t.shape[0], ld)[:, :t.shape[1]].copy_(t)
        return self

    def guards_intact(self):
        raw = self.raw.cpu()
        return bool((raw[:self.lo] == self.fill).all()) and bool((raw[self.lo + self.n:] == self.fill).all())

    def untouched(self):
        return bool((self.raw.cpu() == self.fill).all())

    def rows(self, nrows, ld):
        return self.view.cpu()[:nrows * ld].view(nrows, ld)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ----------------------------------------------------------------------------------------------------------------------- inputs
def make_adj(n, g, neg):
    m = (torch.rand(n, n, generator=g) < 0.4).float() * (0.2 + torch.rand(n, n, generator=g))
    m = m + torch.diag(0.5 + torch.rand(n, generator=g))
    m = m / m.sum(1, keepdim=True)
    if neg:
        flip = (torch.rand(n, n, generator=g) < 0.3) & ~torch.eye(n, dtype=torch.bool)
        m = torch.where(flip, -m, m)
    return m.to(torch.bfloat16)


def make_inputs(r):
    g = torch.Generator().manual_seed(zlib.crc32(row_id(r).encode()) & 0x7FFFFFFF)
    sizes = _sizes(r)
    rows = sum(sizes)
    bf = torch.bfloat16
    L = opt(r, "L", 1)
    ins = [r.I] + [r.O] * (L - 1)
    Ws = [(torch.randn(i, r.O, generator=g) * i ** -0.5).to(bf) for i in ins]
    bs = []
    for l in range(L):
        b = 0.1 + 0.5 * torch.randn(r.O, generator=g).abs()               # non-zero, two columns of three positive: no row loses every
        b = torch.where(torch.arange(r.O) % 3 == 2, -b, b).to(bf)          # output (and with it every gradient) to the ReLU
        bs.append(None if (not opt(r, "bias", True) or opt(r, "nobias") == l) else b)
    return types.SimpleNamespace(sizes=sizes, rows=rows, x=torch.randn(rows, r.I, generator=g).to(bf), Ws=Ws, bs=bs,
                                 adjs=[make_adj(nb, g, opt(r, "neg", False)) for nb in sizes],
                                 gout=torch.randn(rows, r.O, generator=g).to(bf))


# ---------------------------------------------------------------------------------------------------------- float64 and bands
def agg(adjs, X, transpose=False):
    """per-graph adj_b @ X_b (adj_b^T with transpose) over the concatenated rows of X; adjs: list of [n_b, n_b] float64"""
    if not adjs:
        return X.clone()
    if len({a.shape[0] for a in adjs}) == 1:
        A = torch.stack(adjs)
        return torch.bmm(A.transpose(1, 2) if transpose else A, X.view(len(adjs), adjs[0].shape[0], -1)).reshape(X.shape)
    out, at = [], 0
    for a in adjs:
        out.append((a.t() if transpose else a) @ X[at:at + a.shape[0]])
        at += a.shape[0]
    return torch.cat(out)


def per_row_n(adjs):
    """[rows, 1] float64: the node count of each row's graph"""
    return torch.cat([torch.full((a.shape[0], 1), float(a.shape[0]), dtype=torch.float64) for a in adjs]) if adjs else torch.zeros(0, 1, dtype=torch.float64)


class Report:
    def __init__(self, name):
        self.name, self.ratios, self.failures = name, {}, []

    def within(self, what, got, ref, band):
        band = band * SECOND
        err = (got.double() - ref).abs()
        bad = ~(err <= band)                                            # NaN (an element never written) is bad
        ratio = torch.where(band > 0, err / band.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        ratio = torch.where(torch.isnan(err), torch.full_like(err, math.inf), ratio)
        worst = float(ratio.max()) if ratio.numel() else 0.0
        self.ratios[what] = max(self.ratios.get(what, 0.0), worst)
        if bool(bad.any()):
            idx = [int(v) for v in torch.nonzero(bad)[0]]
            self.failures.append("%s: %d of %d elements outside their band, worst ratio %.3g, first at %s (got %r, float64 %r, band %.3g)" % (
                what, int(bad.sum()), bad.numel(), worst, idx, float(got[tuple(idx)]), float(ref[tuple(idx)]), float(band[tuple(idx)])))

    def alive(self, what, ref):
        """a row whose reference outputs the ReLU clips to zero would check nothing"""
        self.require(ref.numel() == 0 or float((ref > 0).double().mean()) >= 0.125, "%s: fewer than one in eight reference outputs are positive" % what)

    def require(self, cond, what):
        if not cond:
            self.failures.append(what)

    def line(self):
        return "%-58s %s" % (self.name, "  ".join("%s %.3f" % kv for kv in self.ratios.items()))

    def finish(self):
        print(self.line())
        assert not self.failures, "%s:\n  %s" % (self.name, "\n  ".join(self.failures))
        return self.ratios


def band_support(x, W):
    s = x @ W
    return s, U * s.abs() + (x.shape[1] + 2) * V * (x.abs() @ W.abs())


def band_out_given_support(adjs, sd, b):
    """float64 out and its band given the device's support sd"""
    nn = per_row_n(adjs)
    ab = b.abs() if b is not None else 0.0
    pre = agg(adjs, sd) + (b if b is not None else 0.0)
    return torch.relu(pre), U * pre.abs() + (nn + 2) * V * (agg([a.abs() for a in adjs], sd.abs()) + ab)


def band_out_fused(adjs, x, W, b):
    """two roundings: support stays in registers"""
    aabs = [a.abs() for a in adjs]
    s, bs = band_support(x, W)                                          # bs = u |s| + (I + 2) v sum |x| |W|: what reaches the second product
    ref, bo = band_out_given_support(adjs, s, b)
    return ref, agg(aabs, bs) + bo


def band_gsupport(adjs, gpre):
    ref = agg(adjs, gpre, transpose=True)
    return ref, U * ref.abs() + (per_row_n(adjs) + 2) * V * agg([a.abs() for a in adjs], gpre.abs(), transpose=True)


def band_gx(gsd, W):
    ref = gsd @ W.t()
    return ref, U * ref.abs() + (W.shape[1] + 2) * V * (gsd.abs() @ W.abs().t())


def band_gw(x, gsd, splits):
    ref = x.t() @ gsd
    return ref, U * ref.abs() + (x.shape[0] + splits + 2) * V * (x.abs().t() @ gsd.abs())


def band_gb(gpre, carried=None):
    ref = gpre.sum(0)
    return ref, U * ref.abs() + (gpre.shape[0] + 2) * V * gpre.abs().sum(0) + (carried.sum(0) if carried is not None else 0.0)


def band_gadj(sizes, gpre, sd):
    """list of per-graph (ref, band)"""
    out, at = [], 0
    for nb in sizes:
        g, s = gpre[at:at + nb], sd[at:at + nb]
        ref = g @ s.t()
        out.append((ref, U * ref.abs() + (sd.shape[1] + 2) * V * (g.abs() @ s.abs().t())))
        at += nb
    return out


# ------------------------------------------------------------------------------------------------------------------ ctypes
def c_fwd(c):
    from recon_amd import _lib
    p = _lib.ptr
    return _lib.GcnB16Args(c.B, c.n, c.I, c.O, p(c.x), c.ldx, p(c.adj), p(c.W), p(c.bias), p(c.support), c.lds, p(c.out), c.ldo, p(c.planes),
                           c.planes_valid, p(c.node_ptr), p(c.adj_ptr), c.total_rows)


def c_bwd(c):
    from recon_amd import _lib
    p = _lib.ptr
    return _lib.GcnB16BwdArgs(c_fwd(c.fwd), p(c.gout), c.ldg, p(c.g_support), p(c.partial), p(c.g_x), c.ldgx, p(c.g_adj), p(c.g_w), p(c.g_b), p(c.zeros))


def fwd_instance(c):
    from recon_amd import _lib
    return _lib.lib().recon_gcn_b16_fwd_instance(C.byref(c_fwd(c)))


def bwd_instance(c):
    from recon_amd import _lib
    return _lib.lib().recon_gcn_b16_bwd_instance(C.byref(c_bwd(c)))


class Device:
    """the library on the GPU"""

    def __init__(self):
        from recon_amd import _lib
        self._lib, self.L, self.dev = _lib, _lib.lib(), torch.device("cuda")

    def _sync(self, rc):
        """a launch failure or a device error ends the session: nothing more is started on a device that has faulted"""
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit("device error in the GCN instance tests: %s" % e, returncode=3)
        if rc == -3:
            pytest.exit("kernel launch failed in the GCN instance tests", returncode=3)
        return rc

    def _run(self, fn, args):
        return self._sync(fn(C.byref(args), self._lib.current_stream()))

    def fwd(self, c):
        return self._run(self.L.recon_gcn_b16_fwd, c_fwd(c))

    def bwd(self, c):
        return self._run(self.L.recon_gcn_b16_bwd, c_bwd(c))

    def transposed_planes(self, W, I, D, planes):
        return self._sync(self.L.recon_gcn_b16_transposed_planes(W.data_ptr(), I, D, planes.data_ptr(), self._lib.current_stream()))

    def stack_fwd(self, c):
        pa = self._lib.ptr_array
        keep = (pa(c.planes_t), pa(c.bias))
        return self._run(self.L.recon_gcn_b16_stack_fwd, self._lib.GcnB16StackArgs(c.B, c.n, c.I, c.D, c.L, c.x.data_ptr(), c.ldx, c.adj.data_ptr(), keep[0], keep[1],
                                                                                 c.out.data_ptr(), c.ldo))

    def _train_args(self, c, bwd):
        pa, p = self._lib.ptr_array, self._lib.ptr
        arrs = [pa(c.W), pa(c.bias), pa(c.planes), pa(c.acts), pa(c.g_support if bwd else [None] * c.L), pa(c.g_w if bwd else [None] * c.L),
                pa(c.g_b if bwd else [None] * c.L)]
        a = self._lib.GcnB16StackTrainArgs(c.B, c.n, c.I, c.D, c.L, p(c.x), c.ldx, p(c.x_rows), c.ldxr, p(c.adj), arrs[0], arrs[1], arrs[2], arrs[3], c.ldo,
                                           p(c.gout) if bwd else None, c.ldg if bwd else 0, arrs[4], p(c.partial) if bwd else None,
                                           p(c.g_x) if bwd else None, c.ldgx if bwd else 0, arrs[5], arrs[6], p(c.zeros) if bwd else None)
        return a, arrs

    def stack_train_fwd(self, c):
        a, keep = self._train_args(c, False)
        return self._run(self.L.recon_gcn_b16_stack_train_fwd, a)

    def stack_train_bwd(self, c):
        a, keep = self._train_args(c, True)
        return self._run(self.L.recon_gcn_b16_stack_train_bwd, a)


# --------------------------------------------------------------------------------------------------------------------- harness
def _planes_elems(I, O):
    from recon_amd import _lib
    return _lib.lib().recon_gcn_b16_planes_bytes(I, O) // 2


def _flat_adj(inp):
    return torch.cat([a.reshape(-1) for a in inp.adjs]) if inp.adjs and inp.rows else torch.zeros(0, dtype=torch.bfloat16)


def _layer_call(r, inp, dev, x_buf=None, ldx=None, W=None, bias=None, I=None, adj=None):
    """buffers and the call description of one recon_gcn_b16_fwd"""
    I = r.I if I is None else I
    O, rows = r.O, inp.rows
    c = types.SimpleNamespace(B=r.B, n=r.n, I=I, O=O, planes_valid=0, node_ptr=None, adj_ptr=None, total_rows=0)
    ragged = opt(r, "sizes") is not None
    fused = not opt(r, "support", False)
    c.ldx = ldx if ldx is not None else opt(r, "ldx", up8(I))
    c.ldo, c.lds = opt(r, "ldo", up8(O)), opt(r, "lds", up8(O))
    if x_buf is None:
        xfill = {"inf": INF16, "nan": NAN16, None: 0x40E0}[opt(r, "xfill")]               # 7.0 where the pads are multiplied by the planes' zeros
        x_buf = Guarded(max(rows, 1) * max(c.ldx, I), dev, fill=xfill)
        if c.ldx >= I:
            x_buf.put(inp.x.to(dev), c.ldx)
    c.x_buf, c.x = x_buf, x_buf.view
    c.adj_buf = adj if adj is not None else Guarded(max(sum(s * s for s in inp.sizes), 1), dev, off=opt(r, "adj_off", 0)).put(_flat_adj(inp).to(dev))
    c.adj = c.adj_buf.view
    c.W = (inp.Ws[0] if W is None else W).to(dev).contiguous()
    bias = inp.bs[0] if W is None else bias
    c.bias_buf = Guarded(O, dev, off=opt(r, "bias_off", 0)).put(bias.to(dev)) if bias is not None else None
    c.bias = c.bias_buf.view if bias is not None else None
    c.support_buf = None if fused else Guarded(max(rows, 1) * c.lds, dev)
    c.support = None if fused else c.support_buf.view
    c.out_buf = Guarded(max(rows, 1) * max(c.ldo, 8), dev, off=opt(r, "out_off", 0))
    c.out = c.out_buf.view
    c.planes_buf = Guarded(_planes_elems(I, O), dev)
    c.planes = c.planes_buf.view
    if ragged:
        node_ptr = torch.tensor([0] + list(torch.tensor(inp.sizes).cumsum(0)), dtype=torch.int32)
        adj_ptr = torch.tensor([0] + list((torch.tensor(inp.sizes, dtype=torch.int64) ** 2).cumsum(0)), dtype=torch.int64)
        c.node_ptr, c.adj_ptr, c.total_rows = node_ptr.to(dev), adj_ptr.to(dev), rows
    return c


def check_layer_fwd(rep, tag, c, inp, x64, W64, b64, adjs64):
    """guards, pad columns and bands of one forward call's support and out; returns the device's (support, out) in float64"""
    rows, O = inp.rows, c.O
    for name in ("out_buf", "support_buf", "planes_buf"):
        buf = getattr(c, name)
        if buf is not None:
            rep.require(buf.guards_intact(), "%s%s: guard overwritten" % (tag, name[:-4]))
    out = c.out_buf.rows(rows, c.ldo)
    rep.require(bool((_bits(out[:, O:]) == 0).all()), "%sout: pad columns %d .. %d not all zero" % (tag, O, c.ldo))
    outd, sd = out[:, :O].double(), None
    if c.support is not None:
        sup = c.support_buf.rows(rows, c.lds)
        rep.require(bool((_bits(sup[:, O:]) == 0).all()), "%ssupport: pad columns %d .. %d not all zero" % (tag, O, c.lds))
        sd = sup[:, :O].double()
        rep.within(tag + "support", sd, *band_support(x64, W64))
        sdz = torch.nan_to_num(sd, nan=0.0)
        ref, band = band_out_given_support(adjs64, sdz, b64)
    else:
        ref, band = band_out_fused(adjs64, x64, W64, b64)
    rep.alive(tag + "out", ref)
    rep.within(tag + "out", outd, ref, band)
    return sd, outd


def run_layer_row(r, be):
    from recon_amd import _lib
    rep = Report(row_id(r))
    inp = make_inputs(r)
    with _lib.config(**dict(opt(r, "cfg", ()))):
        c = _layer_call(r, inp, be.dev)
        want_fwd = r.key if r.kind == "fwd" else (0 if inp.rows == 0 else (RAGGED if opt(r, "sizes") else GEMM if opt(r, "support") else None))
        got_key = fwd_instance(c)
        if r.kind == "refuse":
            rep.require(got_key == -1, "forward query %d for a call that must be refused" % got_key)
            rc = be.fwd(c)
            rep.require(rc == r.key, "recon_gcn_b16_fwd returned %d, not %d" % (rc, r.key))
            rep.require(c.out_buf.untouched() and c.planes_buf.untouched(), "a refused call wrote")
            return rep.finish()
        if want_fwd is not None:
            rep.require(got_key == want_fwd, "forward query %d, the row names %d" % (got_key, want_fwd))
        else:
            rep.require(got_key in (F4, F2), "forward query %d for a fused forward" % got_key)
        rc = be.fwd(c)
        rep.require(rc == OK, "recon_gcn_b16_fwd returned %d" % rc)
        if rc != OK:
            return rep.finish()
        if inp.rows == 0:
            rep.require(c.out_buf.untouched() and c.support_buf.untouched() and c.planes_buf.untouched(), "a call over no rows wrote")
        x64, W64 = inp.x.double(), inp.Ws[0].double()
        b64 = inp.bs[0].double() if inp.bs[0] is not None else None
        adjs64 = [a.double() for a in inp.adjs]
        sd, outd = check_layer_fwd(rep, "", c, inp, x64, W64, b64, adjs64) if inp.rows else (None, None)
        if r.kind == "fwd":
            return rep.finish()
        # ---- backward on the device's own out (and support)
        rows, I, O = inp.rows, r.I, r.O
        b = types.SimpleNamespace(fwd=c, ldg=opt(r, "ldg", up8(O)), ldgx=opt(r, "ldgx", up8(I)))
        c.planes_valid = 1
        dev = be.dev
        b.gout_buf = Guarded(max(rows, 1) * b.ldg, dev).put(inp.gout.to(dev), b.ldg)
        b.gout = b.gout_buf.view
        b.gs_buf = Guarded(max(rows, 1) * c.lds, dev)
        b.g_support = b.gs_buf.view
        L = _lib.lib()
        ragged = opt(r, "sizes") is not None
        nfl = (L.recon_gcn_b16_bwd_partial_floats(1, rows, I, O) + r.B * O) if ragged else L.recon_gcn_b16_bwd_partial_floats(r.B, r.n, I, O)
        b.partial_buf = Guarded(nfl, dev, fp32=True)
        b.partial = b.partial_buf.view
        want = lambda k, d=True: opt(r, k, d)
        b.gx_buf = Guarded(max(rows, 1) * b.ldgx, dev) if want("g_x") else None
        b.gadj_buf = Guarded(max(sum(s * s for s in inp.sizes), 1), dev) if want("g_adj", False) else None
        b.gw_buf = Guarded(I * O, dev) if want("g_w") else None
        b.gb_buf = Guarded(O, dev) if (want("g_b") and c.bias is not None) else None
        b.g_x, b.g_adj, b.g_w, b.g_b = (v.view if v is not None else None for v in (b.gx_buf, b.gadj_buf, b.gw_buf, b.gb_buf))
        b.zeros = torch.zeros(512, dtype=torch.bfloat16, device=dev)
        bufs = [v for v in (b.gs_buf, b.partial_buf, b.gx_buf, b.gadj_buf, b.gw_buf, b.gb_buf) if v is not None]
        got_key = bwd_instance(b)
        if r.kind == "refuse_bwd":
            rep.require(got_key == -1, "backward query %d for a call that must be refused" % got_key)
            rc = be.bwd(b)
            rep.require(rc == r.key, "recon_gcn_b16_bwd returned %d, not %d" % (rc, r.key))
            rep.require(all(v.untouched() for v in bufs), "a refused call wrote")
            return rep.finish()
        rep.require(got_key == r.key, "backward query %d, the row names %d" % (got_key, r.key))
        rc = be.bwd(b)
        rep.require(rc == OK, "recon_gcn_b16_bwd returned %d" % rc)
        if rc != OK:
            return rep.finish()
        for v, name in zip((b.gs_buf, b.partial_buf, b.gx_buf, b.gadj_buf, b.gw_buf, b.gb_buf, c.out_buf), ("g_support", "partial", "g_x", "g_adj", "g_weight", "g_bias", "out")):
            if v is not None:
                rep.require(v.guards_intact(), "%s: guard overwritten" % name)
        if rows == 0:
            rep.require(all(v.untouched() for v in bufs), "a call over no rows wrote")
            return rep.finish()
        gpre = inp.gout.double() * (outd > 0)
        gs = b.gs_buf.rows(rows, c.lds)
        rep.require(bool((_bits(gs[:, O:]) == 0).all()), "g_support: pad columns %d .. %d not all zero" % (O, c.lds))
        gsd = gs[:, :O].double()
        rep.within("g_support", gsd, *band_gsupport(adjs64, gpre))
        gsz = torch.nan_to_num(gsd, nan=0.0)
        if b.gx_buf is not None:
            rep.within("g_x", b.gx_buf.rows(rows, b.ldgx)[:, :I].double(), *band_gx(gsz, W64))
        if b.gadj_buf is not None:
            flat, at = b.gadj_buf.view.cpu().double(), 0
            for nb, (ref, band) in zip(inp.sizes, band_gadj(inp.sizes, gpre, torch.nan_to_num(sd, nan=0.0))):
                rep.within("g_adj", flat[at:at + nb * nb].view(nb, nb), ref, band)
                at += nb * nb
        if b.gw_buf is not None:
            rep.within("g_weight", b.gw_buf.view.cpu().view(I, O).double(), *band_gw(x64, gsz, r.key % 1000))
        if b.gb_buf is not None:
            rep.within("g_bias", b.gb_buf.view.cpu().double(), *band_gb(gpre))
    return rep.finish()


def run_stack_row(r, be):
    from recon_amd import _lib
    rep = Report(row_id(r))
    inp = make_inputs(r)
    dev, L, B, n, I, D, rows = be.dev, opt(r, "L"), r.B, r.n, r.I, r.O, inp.rows
    lib = _lib.lib()
    ins = [I] + [D] * (L - 1)
    ldo = opt(r, "ldo", up8(D))
    adjs64 = [a.double() for a in inp.adjs]
    W64 = [w.double() for w in inp.Ws]
    b64 = [b.double() if b is not None else None for b in inp.bs]
    adj_buf = Guarded(B * n * n, dev).put(_flat_adj(inp).to(dev))
    Wd = [w.to(dev).contiguous() for w in inp.Ws]
    bias_bufs = [Guarded(D, dev).put(b.to(dev)) if b is not None else None for b in inp.bs]
    bias = [v.view if v is not None else None for v in bias_bufs]
    use_xrows = opt(r, "x_rows", False)
    ldx = (I + (I & 1)) if (use_xrows or opt(r, "infer_only")) else up8(I)
    x_buf = Guarded(rows * ldx, dev, fill=INF16 if ldx % 8 else 0x40E0).put(inp.x.to(dev), ldx)
    # ---- inference: the planes of recon_gcn_b16_transposed_planes, one launch
    pt_bufs = [Guarded(D * kp(i), dev) for i in ins]
    for l in range(L):
        rc = be.transposed_planes(Wd[l], ins[l], D, pt_bufs[l].view)
        rep.require(rc == OK and pt_bufs[l].guards_intact(), "recon_gcn_b16_transposed_planes(%d): %d" % (l, rc))
        pl = pt_bufs[l].view.cpu().view(D, kp(ins[l]))
        rep.require(bool((_bits(pl[:, :ins[l]]) == _bits(inp.Ws[l].t())).all()) and bool((_bits(pl[:, ins[l]:]) == 0).all()), "planes of layer %d are not W^T, zero padded" % l)
    inf = types.SimpleNamespace(B=B, n=n, I=I, D=D, L=L, x=x_buf.view, ldx=ldx, adj=adj_buf.view, planes_t=[v.view for v in pt_bufs], bias=bias, ldo=ldo)
    inf.out_buf = Guarded(rows * ldo, dev)
    inf.out = inf.out_buf.view
    rc = be.stack_fwd(inf)
    rep.require(rc == OK and inf.out_buf.guards_intact(), "recon_gcn_b16_stack_fwd returned %d (or wrote a guard)" % rc)
    if opt(r, "infer_only"):
        # no training form at this width: the chain of fused single-layer calls, each held to float64 from the device's previous
        # activation, and the stack bit-equal to its end (include/recon_hip.h: "bit-equal to L calls of recon_gcn_b16_fwd's fused form")
        prev_buf, prev_ld, prev64 = x_buf, ldx, inp.x.double()
        for l in range(L):
            c = _layer_call(Row("fwd", F4, B, n, ins[l], D, (("ldo", ldo),)), inp, dev, x_buf=prev_buf, ldx=prev_ld, W=inp.Ws[l], bias=inp.bs[l], I=ins[l], adj=adj_buf)
            rep.require(be.fwd(c) == OK, "recon_gcn_b16_fwd of layer %d failed" % l)
            _, outd = check_layer_fwd(rep, "l%d." % l, c, inp, prev64, W64[l], b64[l], adjs64)
            prev_buf, prev_ld, prev64 = c.out_buf, ldo, torch.nan_to_num(outd, nan=0.0)
        rep.require(bool((_bits(inf.out_buf.rows(rows, ldo)) == _bits(prev_buf.rows(rows, ldo))).all()), "the stack differs from the chain of fused layers")
        return rep.finish()
    # ---- training forward
    t = types.SimpleNamespace(B=B, n=n, I=I, D=D, L=L, x=x_buf.view, ldx=ldx, adj=adj_buf.view, W=Wd, bias=bias, ldo=ldo, x_rows=None, ldxr=0)
    xr_buf = Guarded(rows * up8(I), dev) if use_xrows else None
    if use_xrows:
        t.x_rows, t.ldxr = xr_buf.view, up8(I)
    pl_bufs = [Guarded(_planes_elems(i, D), dev) for i in ins]
    act_bufs = [Guarded(rows * ldo, dev) for _ in range(L)]
    t.planes, t.acts = [v.view for v in pl_bufs], [v.view for v in act_bufs]
    rc = be.stack_train_fwd(t)
    rep.require(rc == OK, "recon_gcn_b16_stack_train_fwd returned %d" % rc)
    if rc != OK:
        return rep.finish()
    rep.require(all(v.guards_intact() for v in pl_bufs + act_bufs + ([xr_buf] if use_xrows else [])), "training forward: guard overwritten")
    if use_xrows:
        rep.require(bool((_bits(xr_buf.rows(rows, t.ldxr)[:, :I]) == _bits(inp.x)).all()), "x_rows is not a copy of x")
    acts64, prev = [], inp.x.double()
    for l in range(L):
        a = act_bufs[l].rows(rows, ldo)
        rep.require(bool((_bits(a[:, D:]) == 0).all()), "acts[%d]: pad columns %d .. %d not all zero" % (l, D, ldo))
        ref, band = band_out_fused(adjs64, prev, W64[l], b64[l])
        rep.alive("acts[%d]" % l, ref)
        rep.within("acts[%d]" % l, a[:, :D].double(), ref, band)
        prev = torch.nan_to_num(a[:, :D].double(), nan=0.0)
        acts64.append(prev)
    rep.require(bool((_bits(inf.out_buf.rows(rows, ldo)) == _bits(act_bufs[L - 1].rows(rows, ldo))).all()), "the inference form differs from the training form's last activation")
    # ---- backward
    frozen = opt(r, "frozen")
    t.ldg, t.ldgx = up8(D), (I if I % 4 == 0 else up8(I))
    gout_buf = Guarded(rows * t.ldg, dev).put(inp.gout.to(dev), t.ldg)
    gs_bufs = [Guarded(rows * ldo, dev) for _ in range(L)]
    part_buf = Guarded(lib.recon_gcn_b16_stack_bwd_partial_floats(B, n, I, D, L), dev, fp32=True)
    gx_buf = Guarded(rows * t.ldgx, dev) if opt(r, "g_x", True) else None
    gw_bufs = [Guarded(ins[l] * D, dev) if l != frozen else None for l in range(L)]
    gb_bufs = [Guarded(D, dev) if (l != frozen and inp.bs[l] is not None) else None for l in range(L)]
    t.gout, t.g_support, t.partial = gout_buf.view, [v.view for v in gs_bufs], part_buf.view
    t.g_x = gx_buf.view if gx_buf is not None else None
    t.g_w, t.g_b = [v.view if v is not None else None for v in gw_bufs], [v.view if v is not None else None for v in gb_bufs]
    t.zeros = torch.zeros(512, dtype=torch.bfloat16, device=dev)
    if use_xrows:                                                       # the backward reads the aligned copy the forward left
        t.x, t.ldx, t.x_rows, t.ldxr = xr_buf.view, up8(I), None, 0
    rc = be.stack_train_bwd(t)
    rep.require(rc == OK, "recon_gcn_b16_stack_train_bwd returned %d" % rc)
    if rc != OK:
        return rep.finish()
    rep.require(all(v.guards_intact() for v in gs_bufs + [part_buf] + [v for v in [gx_buf] + gw_bufs + gb_bufs if v is not None] + act_bufs), "backward: guard overwritten")
    aabs = [a.abs() for a in adjs64]
    gs64 = [None] * L
    splits = stack_km_plan(ins, D, rows, [l for l in range(L) if l != frozen])[0]
    for l in range(L - 1, -1, -1):
        gs = gs_bufs[l].rows(rows, ldo)
        rep.require(bool((_bits(gs[:, D:]) == 0).all()), "g_support[%d]: pad columns %d .. %d not all zero" % (l, D, ldo))
        mask = acts64[l] > 0
        if l == L - 1:
            gpre, carried = inp.gout.double() * mask, None
        else:                                                           # g_l = g_support_l+1 W_l+1^T, rounded to bf16 in LDS, then the mask
            tt, tb = band_gx(gs64[l + 1], W64[l + 1])
            gpre, carried = tt * mask, tb * mask
        ref, band = band_gsupport(adjs64, gpre)
        if carried is not None:
            band = band + agg(aabs, carried, transpose=True)
        rep.within("g_support[%d]" % l, gs[:, :D].double(), ref, band)
        gs64[l] = torch.nan_to_num(gs[:, :D].double(), nan=0.0)
        xin = inp.x.double() if l == 0 else acts64[l - 1]
        if gw_bufs[l] is not None:
            rep.within("g_weight[%d]" % l, gw_bufs[l].view.cpu().view(ins[l], D).double(), *band_gw(xin, gs64[l], splits))
        if gb_bufs[l] is not None:
            rep.within("g_bias[%d]" % l, gb_bufs[l].view.cpu().double(), *band_gb(gpre, carried))
    if gx_buf is not None:
        rep.within("g_x", gx_buf.rows(rows, t.ldgx)[:, :I].double(), *band_gx(gs64[0], W64[0]))
    return rep.finish()


def run_refuse_stack_row(r, be):
    rep = Report(row_id(r))
    inp = make_inputs(r)
    dev, L, B, n, I, D, rows = be.dev, opt(r, "L"), r.B, r.n, r.I, r.O, inp.rows
    ins = [I] + [D] * (L - 1)
    ldo, ldx = opt(r, "ldo", up8(D)), up8(I)
    adj_buf = Guarded(B * n * n + 8, dev).put(_flat_adj(inp).to(dev))
    Wd = [w.to(dev).contiguous() for w in inp.Ws]
    bias = [Guarded(D + 8, dev).put(b.to(dev)).view for b in inp.bs]
    x_buf = Guarded(rows * ldx, dev, fill=0).put(inp.x.to(dev), ldx)
    written = []
    if opt(r, "infer") in (True, None):
        planes = [Guarded(D * kp(i), dev, fill=0).view for i in ins]
        c = types.SimpleNamespace(B=B, n=n, I=I, D=D, L=L, x=x_buf.view, ldx=ldx, adj=adj_buf.view, planes_t=planes, bias=bias, ldo=ldo)
        c.out_buf = Guarded(rows * ldo, dev)
        c.out = c.out_buf.view
        rc = be.stack_fwd(c)
        rep.require(rc == r.key, "recon_gcn_b16_stack_fwd returned %d, not %d" % (rc, r.key))
        written.append(c.out_buf)
    if opt(r, "infer") in (False, None):
        t = types.SimpleNamespace(B=B, n=n, I=I, D=D, L=L, x=x_buf.view, ldx=ldx, adj=adj_buf.view, W=Wd, bias=bias, ldo=ldo, x_rows=None, ldxr=0)
        pl = [Guarded(_planes_elems(i, D), dev) for i in ins]
        acts = [Guarded(rows * ldo, dev) for _ in range(L)]
        t.planes, t.acts = [v.view for v in pl], [v.view for v in acts]
        rc = be.stack_train_fwd(t)
        rep.require(rc == r.key, "recon_gcn_b16_stack_train_fwd returned %d, not %d" % (rc, r.key))
        written += pl + acts
    rep.require(all(v.untouched() for v in written), "a refused call wrote")
    return rep.finish()


def run_row(r, be):
    if r.kind == "stack":
        return run_stack_row(r, be)
    if r.kind == "refuse_stack":
        return run_refuse_stack_row(r, be)
    return run_layer_row(r, be)


# ----------------------------------------------------------------------------------------------------------------------- tests
_DEVICE = []


def _device():
    if not _DEVICE:
        _DEVICE.append(Device())
    return _DEVICE[0]


def _of(*kinds):
    rows = [r for r in GCN_ROWS if r.kind in kinds]
    return dict(argvalues=rows, ids=[row_id(r) for r in rows])


@pytest.mark.parametrize("row", **_of("fwd"))
def test_gcn_bf16_forward_instances_vs_float64(row):
    run_row(row, _device())


@pytest.mark.parametrize("row", **_of("bwd"))
def test_gcn_bf16_backward_instances_vs_float64(row):
    run_row(row, _device())


@pytest.mark.parametrize("row", **_of("stack"))
def test_gcn_stack_instances_vs_float64(row):
    run_row(row, _device())


@pytest.mark.parametrize("row", **_of("refuse", "refuse_bwd"))
def test_gcn_bf16_refusals_write_nothing(row):
    run_row(row, _device())


@pytest.mark.parametrize("row", **_of("refuse_stack"))
def test_gcn_stack_refusals_write_nothing(row):
    run_row(row, _device())
