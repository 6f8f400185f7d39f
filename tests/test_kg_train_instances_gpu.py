"""Every instance of the ConvKB training kernels (csrc/kg_train.hip) and every class of the backward's row split against float64,
through the C ABI (recon_convkb_train_fwd / recon_convkb_train_bwd) with buffers the test owns.

KGT_FWD_ROWS: for every NP = ceil(D / 64) = 1 .. 8 (one instance of k_kgt_fwd each, another unroll above NP = 6) the widths
D = 64 (NP - 1) + 1, 64 NP - 27 and 64 NP.  M rotates through {1, 31, 32, 33, 95, 333}; three rows cannot hold M < 32, M % 32 != 0 and
M % 32 == 0 for one NP when 32 is the only multiple in the set, so every width takes two values of the rotation, three apart, and every
NP sees all six.  int32 and int64 indices alternate, the ratio rotates through {1, 3, 40}.  One more row, (37, 2081), has 66 workgroups:
lanes 0 and 1 of the mean's strided sum add two blocks each.

KGT_BWD_ROWS: (D, M) with the split (P parts of rows_per_part rows, rows in the last part) that kgt_bwd_split gives them; the host-only
tests/test_kg_train_instances_cpu.py holds the table to the library's own workspace query.  Classes: P = 1; one 64-row chunk per part;
several chunks with a partial last chunk; every part full; a last part of one row.

Bands (EPS32 = 2^-24, all against float64 on the CPU):
  z, s          those of test_forward_backward_within_fp64_band: 2 (K + 2) EPS32 (|X| |W1|^T + |b1|) and its s band.
  g_scores      32 EPS32 |g64| + 1e-30 against the float64 BCE of the kernel's own s (test_whole_step_within_fp64_band).
  loss          4 (M + 16) EPS32 mean|terms| + 1e-30 (the same test).
  loss_terms    8 EPS32 w (|(1 - y) s| + mx + L + 1), L = log(e^-mx + e^(-s - mx)): the term is w times three summands joined by two
                additions of one rounding each; expf / logf are good to a few ulp; the argument of the log lies in [1, 2], so its relative
                error is an absolute error of L (the + 1); doubled, as the other bands of this file are.
  wide logits   at |s| > 80 sigma(s) - y cancels in fp32 exactly as torch's own fp32 backward does (sigma rounds to 1 or to a denormal
                distance from y), so the band of g_scores is absolute there: (w / M) 8 EPS32 + 32 EPS32 |g64|.
  gradients     2 (M + 4) EPS32 (|delta|^T |X|) + 1e-30 and its kin, with the kernel's own z signs and g_scores, as the existing tests.

Every output is a view inside memory filled with one NaN pattern, which must still surround it afterwards; every workspace is a zeroed
view of the size the query names inside such memory.  The tables and the harness are module-level and touch no device: the CPU file runs
the same harness on a float32 restatement and on subtly wrong ones.
"""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
N_ENT, N_REL, SLOPE = 300, 11, 0.01
GUARD = 64                                     # floats of NaN in front of and behind every view (256 bytes: keeps the alignment)
NAN_BITS = 0x7FC0BEEF
TICKET_WORDS = 256                             # arrival counters at the head of both workspaces
M_ROTATION = (1, 31, 32, 33, 95, 333)
RATIOS = (1, 3, 40)

FwdRow = collections.namedtuple("FwdRow", "D M idx64 ratio")
BwdRow = collections.namedtuple("BwdRow", "D M P rows_per_part last g3")


def _fwd_rows():
    rows = []
    for NP in range(1, 9):
        for j, D in enumerate((64 * (NP - 1) + 1, 64 * NP - 27, 64 * NP)):
            for half in (0, 3):
                i = len(rows)
                rows.append(FwdRow(D, M_ROTATION[(NP - 1 + j + half) % 6], i % 2 == 1, RATIOS[i % 3]))
    rows.append(FwdRow(37, 2081, True, 3))
    return rows


KGT_FWD_ROWS = _fwd_rows()
WIDE_ROW = FwdRow(200, 333, True, 3)
WIDE_W2_SCALE = 300.0                          # s = O(0.3) at unit scale: the extreme rows of 333 then lie past +-100
# expf overflows at 88.7: a term without the mx shift is still finite at |s| = 80, so the case reaches past 90 on both sides
WIDE_SPAN = 90.0

KGT_BWD_ROWS = [
    BwdRow(512, 64, 1, 64, 64, False),         # one full chunk, 192 tiles (the ticket bound)
    BwdRow(1, 17, 1, 64, 17, True),
    BwdRow(384, 449, 8, 64, 1, True),          # one-row last part
    BwdRow(130, 1409, 23, 64, 1, False),
    BwdRow(65, 2305, 37, 64, 1, False),
    BwdRow(512, 385, 4, 128, 1, True),         # two chunks per part, one-row last part
    BwdRow(512, 800, 5, 192, 32, True),        # three chunks, partial last chunk
    BwdRow(512, 768, 6, 128, 128, True),       # every part full
    BwdRow(448, 500, 4, 128, 116, False),
    BwdRow(257, 1100, 9, 128, 76, False),
    BwdRow(200, 2000, 16, 128, 80, False),
    BwdRow(200, 5184, 21, 256, 64, False),     # the workload's own split
    BwdRow(1, 130000, 1016, 128, 80, False),   # the P-term partial sum at its longest
]


def fwd_id(r):
    return "D%d-M%d-%s-r%d" % (r.D, r.M, "i64" if r.idx64 else "i32", r.ratio)


def bwd_id(r):
    return "D%d-M%d-P%d" % (r.D, r.M, r.P)


def split_classes(r):
    """The classes of the backward's split a row stands for."""
    out = set()
    chunks = r.rows_per_part // 64
    if r.P == 1:
        out.add("one part")
    if r.P > 1 and chunks == 1:
        out.add("one chunk per part")
    if chunks > 1 and r.last % 64:
        out.add("several chunks, partial last chunk")
    if r.P > 1 and r.last == r.rows_per_part:
        out.add("every part full")
    if r.P > 1 and r.last == 1:
        out.add("one-row last part")
    return out


SPLIT_CLASSES = ("one part", "one chunk per part", "several chunks, partial last chunk", "every part full", "one-row last part")


# ---------------------------------------------------------------------------------------------------------- inputs and float64
def make_inputs(D, M, w2_scale=1.0):
    """Tables of unit normals and weights at nn.Linear's scale (U(+-fan_in^-1/2), what _model of tests/test_kg_train_gpu.py leaves
    them at), random triples with duplicates and values +-1; float32 / int64 on the CPU, a fixed seed per (D, M)."""
    g = torch.Generator().manual_seed(1000003 * D + M)
    u = lambda *shape: torch.rand(*shape, generator=g) * 2 - 1
    k1, k2 = (3 * D) ** -0.5, D ** -0.5
    inp = dict(D=D, M=M, E=torch.randn(N_ENT, D, generator=g), R=torch.randn(N_REL, D, generator=g), W1=u(D, 3 * D) * k1, b1=u(D) * k1,
               w2=u(D) * k2 * w2_scale, b2=u(1) * k2)
    inp["tri"] = torch.stack([torch.randint(0, N_ENT, (M,), generator=g), torch.randint(0, N_REL, (M,), generator=g),
                              torch.randint(0, N_ENT, (M,), generator=g)], 1)
    inp["val"] = (torch.randint(0, 2, (M,), generator=g) * 2 - 1).float()
    return inp


def gathered(inp, dtype=torch.float64):
    t = inp["tri"]
    return torch.cat([inp["E"][t[:, 0]], inp["R"][t[:, 1]], inp["E"][t[:, 2]]], 1).to(dtype)


def bce64(s, val, ratio):
    """float64 (terms, dL/ds, w, the band of the terms) of the weighted BCE of logits s (main.py:833-840), mean reduction over len(s)."""
    sd, M = s.double(), s.numel()
    y = (val.double() + 1) / 2
    w = y + (1 - y) / (2 * ratio)
    mx = torch.clamp(-sd, min=0)
    L = torch.log(torch.exp(-mx) + torch.exp(-sd - mx))
    terms = w * ((1 - y) * sd + mx + L)
    g = w * torch.where(y == 1, -torch.sigmoid(-sd), torch.sigmoid(sd)) / M          # sigma(s) - y without the cancellation
    band = 8 * EPS32 * w * (((1 - y) * sd).abs() + mx + L + 1)
    return terms, g, w, band


def _held(name, got, ref, band, ratios):
    """Assert |got - ref| <= band elementwise and a finite result; records the worst error / band in ratios[name]."""
    got, ref, band = (torch.as_tensor(t, dtype=torch.float64).reshape(-1) for t in (got, ref, band))
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    q = float(((got - ref).abs() / band).max())
    ratios[name] = max(ratios.get(name, 0.0), q)
    assert q <= 1.0, "%s: error / band = %.3f" % (name, q)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the harness
# A backend answers
#   fwd(inp, row, values, want_z, want_terms) -> dict(z, s, terms, gs, loss) of float32 CPU tensors (None where not asked for)
#   bwd(inp, row, z, gs, g_scale)             -> (dW1, db1, dw2, db2) of float32 CPU tensors; g_scale None or a float
def check_forward(backend, row, w2_scale=1.0, wide=False):
    """One row of KGT_FWD_ROWS (or the wide-logit case) with every assertion it carries; returns {output: worst error / band}."""
    D, M, ratio = row.D, row.M, row.ratio
    inp = make_inputs(D, M, w2_scale)
    out = backend.fwd(inp, row, True, True, True)
    z, s, terms, gs, loss = out["z"], out["s"], out["terms"], out["gs"], out["loss"]
    ratios = {}
    X = gathered(inp)
    W, b1, w2, b2 = inp["W1"].double(), inp["b1"].double(), inp["w2"].double(), inp["b2"].double()
    z64 = X @ W.T + b1
    zb = 2 * (3 * D + 2) * EPS32 * (X.abs() @ W.abs().T + b1.abs())
    _held("z", z, z64, zb, ratios)
    h64 = torch.where(z64 > 0, z64, SLOPE * z64)
    s64 = h64 @ w2 + b2
    sb = 2 * (D + 2) * EPS32 * (h64.abs() @ w2.abs() + b2.abs()) + zb @ w2.abs()
    _held("s", s, s64, sb, ratios)
    if wide:
        assert float(s64.min()) < -WIDE_SPAN and float(s64.max()) > WIDE_SPAN, (float(s64.min()), float(s64.max()))
    t64, g64, w, tband = bce64(s, inp["val"], ratio)
    _held("loss_terms", terms, t64, tband, ratios)
    _held("loss", loss, t64.mean(), 4 * (M + 16) * EPS32 * t64.abs().mean() + 1e-30, ratios)
    gband = 32 * EPS32 * g64.abs() + ((w / M) * 8 * EPS32 if wide else 1e-30)
    _held("g_scores", gs, g64, gband, ratios)
    # the other forms of the call: scoring only, and a loss call that keeps no z and no terms
    sc = backend.fwd(inp, row, False, True, False)
    assert _same_bits(sc["s"], s), "scoring-only call: other bits of scores"
    assert _same_bits(sc["z"], z), "scoring-only call: other bits of z"
    nz = backend.fwd(inp, row, True, False, False)
    assert nz["z"] is None and _same_bits(nz["s"], s), "z = NULL call: other bits of scores"
    assert _same_bits(nz["gs"], gs) and _same_bits(nz["loss"], loss), "z = NULL call: other bits of g_scores / loss"
    return ratios


def check_backward(backend, row):
    """One row of KGT_BWD_ROWS; returns {output: worst error / band}."""
    D, M = row.D, row.M
    inp = make_inputs(D, M)
    out = backend.fwd(inp, FwdRow(D, M, M % 2 == 0, 3), True, True, False)
    z, gs = out["z"], out["gs"]
    g0 = backend.bwd(inp, row, z, gs, None)
    g1 = backend.bwd(inp, row, z, gs, 1.0)
    for name, a, b in zip(("dW1", "db1", "dw2", "db2"), g0, g1):
        assert _same_bits(a, b), "%s: g_scale = [1.0] gives other bits than g_scale = NULL" % name
    # delta with the kernel's own z signs and g_scores (the float64 recomputation's may differ within the z band of zero)
    X = gathered(inp)
    w2 = inp["w2"].double()
    g = gs.double()
    d64 = (g[:, None] * w2[None, :]) * torch.where(z > 0, 1.0, SLOPE).double()
    h32 = torch.where(z > 0, z, z * SLOPE).double()
    c = 2 * (M + 4) * EPS32
    refs = (("dW1", d64.T @ X, c * (d64.abs().T @ X.abs())), ("db1", d64.sum(0), c * d64.abs().sum(0)),
            ("dw2", g @ h32, c * (g.abs() @ h32.abs())), ("db2", g.sum(), c * g.abs().sum()))
    ratios = {}
    for (name, ref, band), got in zip(refs, g0):
        _held(name, got, ref, band + 1e-30, ratios)
    if row.g3:
        g3 = backend.bwd(inp, row, z, gs, 3.0)
        for (name, ref, band), got in zip(refs, g3):
            _held(name + "(g_scale 3)", got, 3 * ref, 3 * band + 1e-30, ratios)
    return ratios


def _report(kind, rid, ratios):
    print("KGT_INST %s %s %s" % (kind, rid, " ".join("%s=%.4f" % kv for kv in sorted(ratios.items()))))


# --------------------------------------------------------------------------------------------------------------- on the device
def _dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


class _View:
    """n floats inside a buffer filled with one NaN pattern, GUARD floats in front and behind."""

    def __init__(self, n, zero=False):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=_dev())
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + 4 * GUARD
        if zero:
            self.words().zero_()

    def words(self):
        return self.buf[GUARD:GUARD + self.n]

    def surroundings_intact(self):
        return bool((self.buf[:GUARD] == NAN_BITS).all()) and bool((self.buf[GUARD + self.n:] == NAN_BITS).all())

    def untouched(self):
        return bool((self.buf == NAN_BITS).all())

    def get(self, shape=None):
        t = self.words().view(torch.float32).cpu().clone()
        return t if shape is None else t.view(shape)


class DeviceBackend:
    """The two library calls.  `ws`: None (a fresh zeroed workspace of the size the query names, inside NaN memory, for every call) or a
    _View every call shares."""

    def __init__(self, ws=None):
        from recon_amd import _lib
        self.L, self._lib, self.ws = _lib.lib(), _lib, ws
        self._up = None

    def _tables(self, inp):
        if self._up is None or self._up[0] is not inp:                   # the inputs of the last call stay on the device
            d = {k: inp[k].to(_dev()) for k in ("E", "R", "W1", "b1", "w2", "b2", "val")}
            d["tri64"], d["tri32"] = inp["tri"].to(_dev()), inp["tri"].int().to(_dev())
            self._up = (inp, d)
        return self._up[1]

    def _workspace(self, floats):
        if self.ws is not None:
            assert self.ws.n >= floats
            return self.ws
        return _View(floats, zero=True)

    def fwd(self, inp, row, values, want_z, want_terms):
        L, d = self.L, self._tables(inp)
        D, M = inp["D"], inp["M"]
        tri = d["tri64"] if row.idx64 else d["tri32"]
        z, s = _View(M * D), _View(M)
        terms, gs, loss = _View(M), _View(M), _View(1)
        floats = L.recon_convkb_train_fwd_workspace_floats(M, D)
        assert floats == TICKET_WORDS + (M + 31) // 32
        ws = self._workspace(floats) if values else None
        rc = L.recon_convkb_train_fwd(tri.data_ptr(), tri.element_size(), M, d["E"].data_ptr(), d["R"].data_ptr(), N_ENT, N_REL, D, d["W1"].data_ptr(),
                                      d["b1"].data_ptr(), d["w2"].data_ptr(), d["b2"].data_ptr(), SLOPE, z.ptr if want_z else None, s.ptr,
                                      d["val"].data_ptr() if values else None, row.ratio if values else 0, terms.ptr if want_terms else None,
                                      gs.ptr if values else None, loss.ptr if values else None, ws.ptr if values else None,
                                      floats if values else 0, self._lib.current_stream())
        assert rc == 0, "recon_convkb_train_fwd returned %d" % rc
        torch.cuda.synchronize()
        for name, v, written in (("z", z, want_z), ("scores", s, True), ("loss_terms", terms, values and want_terms), ("g_scores", gs, values),
                                 ("loss", loss, values)):
            if written:
                assert v.surroundings_intact(), "written outside " + name
            else:
                assert v.untouched(), "%s was written by a call that does not ask for it" % name
        if ws is not None and self.ws is None:
            assert ws.surroundings_intact(), "written outside the workspace"
        return dict(z=z.get((M, D)) if want_z else None, s=s.get(), terms=terms.get() if values and want_terms else None,
                    gs=gs.get() if values else None, loss=loss.get() if values else None)

    def bwd(self, inp, row, z, gs, g_scale):
        L, d = self.L, self._tables(inp)
        D, M = inp["D"], inp["M"]
        tri = d["tri64"] if M % 2 else d["tri32"]
        zd, gd = z.to(_dev()), gs.to(_dev())
        sc = None if g_scale is None else torch.tensor([g_scale], dtype=torch.float32, device=_dev())
        outs = [_View(3 * D * D), _View(D), _View(D), _View(1)]
        floats = L.recon_convkb_train_bwd_workspace_floats(M, D)
        ws = self._workspace(floats)
        rc = L.recon_convkb_train_bwd(tri.data_ptr(), tri.element_size(), M, d["E"].data_ptr(), d["R"].data_ptr(), N_ENT, N_REL, D, d["w2"].data_ptr(),
                                      SLOPE, zd.data_ptr(), gd.data_ptr(), None if sc is None else sc.data_ptr(), outs[0].ptr, outs[1].ptr,
                                      outs[2].ptr, outs[3].ptr, ws.ptr, floats, self._lib.current_stream())
        assert rc == 0, "recon_convkb_train_bwd returned %d" % rc
        torch.cuda.synchronize()
        for name, v in zip(("dW1", "db1", "dw2", "db2"), outs):
            assert v.surroundings_intact(), "written outside " + name
        if self.ws is None:
            assert ws.surroundings_intact(), "written outside the workspace"
        return outs[0].get((D, 3 * D)), outs[1].get(), outs[2].get(), outs[3].get()


@pytest.mark.parametrize("row", KGT_FWD_ROWS, ids=[fwd_id(r) for r in KGT_FWD_ROWS])
def test_kgt_instances_forward_within_fp64_bands(row):
    _report("fwd", fwd_id(row), check_forward(DeviceBackend(), row))


def test_kgt_instances_wide_logits_within_fp64_bands():
    _report("wide", fwd_id(WIDE_ROW), check_forward(DeviceBackend(), WIDE_ROW, w2_scale=WIDE_W2_SCALE, wide=True))


@pytest.mark.parametrize("row", KGT_BWD_ROWS, ids=[bwd_id(r) for r in KGT_BWD_ROWS])
def test_kgt_instances_backward_within_fp64_bands(row):
    _report("bwd", bwd_id(row), check_backward(DeviceBackend(), row))


def test_kgt_instances_one_workspace_serves_every_shape():
    """The header's promise: one zero-filled buffer of the largest size asked for serves every shape, forward and backward alike.  After
    every call the arrival counters read zero again; everything behind them is then NaN for the next call, which must rewrite whatever it
    reads; every result equals, bit for bit, the same call on a fresh zeroed buffer."""
    from recon_amd import _lib
    L = _lib.lib()
    largest = max([L.recon_convkb_train_bwd_workspace_floats(r.M, r.D) for r in KGT_BWD_ROWS] +
                  [L.recon_convkb_train_fwd_workspace_floats(r.M, r.D) for r in KGT_FWD_ROWS])
    shared = _View(largest, zero=True)
    one, fresh = DeviceBackend(shared), DeviceBackend()
    bwd_rows = {(r.D, r.M): r for r in KGT_BWD_ROWS}
    for kind, D, M in (("bwd", 512, 800), ("fwd", 37, 2081), ("bwd", 1, 17), ("bwd", 200, 2000), ("fwd", 200, 333)):
        inp = make_inputs(D, M)
        frow = FwdRow(D, M, True, 3)
        if kind == "fwd":
            a, b = (be.fwd(inp, frow, True, True, True) for be in (one, fresh))
            pairs = [(k, a[k], b[k]) for k in ("z", "s", "terms", "gs", "loss")]
        else:
            saved = fresh.fwd(inp, frow, True, True, False)
            a, b = (be.bwd(inp, bwd_rows[(D, M)], saved["z"], saved["gs"], None) for be in (one, fresh))
            pairs = [(k, x, y) for k, x, y in zip(("dW1", "db1", "dw2", "db2"), a, b)]
        assert shared.surroundings_intact(), "written outside the workspace"
        assert not bool(shared.words()[:TICKET_WORDS].any()), "%s (%d, %d) leaves an arrival counter non-zero" % (kind, D, M)
        shared.words()[TICKET_WORDS:] = NAN_BITS
        for k, x, y in pairs:
            assert bool(torch.isfinite(x).all()) and _same_bits(x, y), "%s (%d, %d): %s differs from the run on a fresh workspace" % (kind, D, M, k)
