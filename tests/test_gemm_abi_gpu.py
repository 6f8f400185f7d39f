"""The stand-alone GEMM entry points of include/recon_hip.h, through the C ABI, at the strides, alignments, tails and splits their
callers use and the tight-stride tests of test_gat_gpu.py never pass: recon_sgemm / recon_sgemm_ex / recon_sgemm_small (exact fp32),
recon_sgemm_bx3 / _bx3_tn (3 x bf16), recon_sgemm_hx2 / _hx2_tn and their _presplit forms (2 x f16).

Every operand and every output is a VIEW inside a larger buffer whose other elements (a guard before and after, the columns from the
logical width up to the leading dimension) hold one NaN bit pattern.  A successful call is held to
  * the elementwise bound of test_sgemm_bx3 against the float64 product, |err| <= 2^-20 (|A| @ |B|) + 1e-30 (the hx2 entries add the
    per-tensor floor of test_sgemm_hx2 / test_sgemm_hx2_tn),
  * an output buffer whose every element outside the M x N view still is that bit pattern, and untouched operand buffers,
  * a finite view,
  * a second call into a second buffer that is bit-identical to the first.
A refused call is held to the code the header documents and to an output buffer nobody wrote.  A case that names a split or a switch
asserts, through the workspace query or recon_config_get, that the library took that path.

The case tables are plain data at module level (importing this file does not touch the device): tests/test_gemm_abi_cpu.py checks
them — the declared matrix has no empty cell, every view fits its buffer, the bound has a factor two of room over a float32 product.
"""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, -1, -2          # RECON_OK, RECON_ERR_INVALID, RECON_ERR_UNSUPPORTED
GUARD = 64                                     # floats of NaN in front of and behind every view (256 bytes: keeps the alignment)
NAN_BITS = 0x7FC0BEEF                          # the quiet NaN every buffer is filled with
SWITCHES = ("RECON_GEMM_CFG", "RECON_GEMM_LIN", "RECON_GEMM_XCD", "RECON_GEMM_SPLITK", "RECON_HX2_RING")
# orientation of the entries that have only one: (a_is_km, b_is_nk)
FIXED_ORIENT = {"bx3": (0, 1), "hx2": (0, 1), "bx3_tn": (1, 0), "hx2_tn": (1, 0)}
ORIENT_NAME = {(0, 0): "nn", (0, 1): "nt", (1, 0): "tn", (1, 1): "tt"}


class Case:
    """One call.  load: "vec4" or "scalar:<reason>" — for ex / small the width of the operand loads, for bx3 / hx2 that of the output
    stores, "scalar" for the k-major split forms (their second pass stores single floats).  split: the call adds partial products in a
    second pass (for the *_tn entries: of more than one split).  query: what the entry's workspace query must answer (floats for ex /
    small) and splits: the split count the *_tn workspace size must encode — the pins of the path.  ws: "query" (the size the query
    names), None (NULL) or "misaligned".  same_as: id of a case whose M x N result must be bit-identical to this one's."""

    def __init__(self, id, entry, M, N, K, akm=0, bnk=0, lda=None, ldb=None, ldc=None, offa=0, offb=0, offc=0, ws="query", cfg=None,
                 expect=OK, load=None, split=False, query=None, splits=None, same_as=None, sa=1.0, sb=1.0):
        if entry in FIXED_ORIENT:
            akm, bnk = FIXED_ORIENT[entry]
        self.id, self.entry, self.M, self.N, self.K, self.akm, self.bnk = id, entry, M, N, K, akm, bnk
        self.lda = self.a_shape()[1] if lda is None else lda
        self.ldb = self.b_shape()[1] if ldb is None else ldb
        self.ldc = N if ldc is None else ldc
        self.offa, self.offb, self.offc, self.ws, self.cfg = offa, offb, offc, ws, dict(cfg or {})
        self.expect, self.load, self.split, self.query, self.splits, self.same_as, self.sa, self.sb = expect, load, split, query, splits, same_as, sa, sb

    def a_shape(self):
        return (self.K, self.M) if self.akm else (self.M, self.K)

    def b_shape(self):
        return (self.N, self.K) if self.bnk else (self.K, self.N)

    @property
    def orient(self):
        return ORIENT_NAME[(self.akm, self.bnk)]

    @property
    def padded(self):
        return self.ldc > self.N

    @property
    def seed(self):
        name = self.same_as or self.id                  # a case compared with another one computes on the same inputs
        return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


def _r4(x):
    return (x + 3) // 4 * 4


def layout(rows, cols, ld, off):
    """(first element of the view, elements of the buffer, row stride the buffer is laid out with).  The stride is `ld` unless a refused
    case passes one below the width: then the rows are laid out tight and the call, were it to run, would still stay inside."""
    ld_alloc = max(ld, cols, 1)
    start = GUARD + off
    return start, start + rows * ld_alloc + GUARD, ld_alloc


def inputs(c):
    """The logical operands A [M,K], B [K,N] (float32, CPU): randn, A's rows scaled by exp(2 randn), a fixed seed per case."""
    g = torch.Generator().manual_seed(c.seed)
    A = torch.randn(c.M, c.K, generator=g) * torch.exp(2.0 * torch.randn(c.M, 1, generator=g)) * c.sa
    B = torch.randn(c.K, c.N, generator=g) * c.sb
    return A, B


def bound_of(c, A, B):
    """(float64 product, elementwise bound) of the logical operands."""
    Ad, Bd = A.double(), B.double()
    Aa, Ba = Ad.abs(), Bd.abs()
    bound = (Aa @ Ba) * (2.0 ** -20) + 1e-30
    if c.entry.startswith("hx2") and c.K > 0:
        # the floor of a per-TENSOR scale, as test_sgemm_hx2 / test_sgemm_hx2_tn write it (there with B given as [N,K] / [K,N])
        bound = bound + (2.0 ** -38) * (Aa.max() * Ba.sum(0)[None, :] + Ba.max() * Aa.sum(1)[:, None])
    return Ad @ Bd, bound


# ---------------------------------------------------------------------------------------------------------------- the case tables
def _ex_cases():
    cs = []
    # orientation x load width x split x ldc.  Operands sit in rows 4 floats wider than their extent (rounded up to 4), so that the
    # named reason is the only one that turns the float4 loads off.
    for (akm, bnk), load, split, pad in itertools.product([(0, 0), (0, 1), (1, 0)], ["vec4", "scalar:base", "scalar:ld", "scalar:extent"],
                                                          [False, True], [False, True]):
        M, N, K = 36, 40, (300 if split else 40)
        if load == "scalar:extent":                    # the contiguous extent of A: K when A is [M,K], M when it is [K,M]
            if akm:
                M += 1
            else:
                K += 1
        c = Case("ex-%s-%s-%s-%s" % (ORIENT_NAME[(akm, bnk)], load.replace("scalar:", "s_"), "split" if split else "unsplit", "ldcpad" if pad else "tight"),
                 "ex", M, N, K, akm, bnk, ldc=N + 4 if pad else N, load=load, split=split, ws="query" if split else None,
                 query=2 * M * N if split else None)
        c.lda, c.ldb = _r4(c.a_shape()[1]) + 4, _r4(c.b_shape()[1]) + 4
        if load == "scalar:ld":
            c.lda += 1
        if load == "scalar:base":
            c.offb = 1
        cs.append(c)
    # tile choice: one 128-wide column tile, two of them, the 208-wide tile, and past it; one and two row tiles; 128 x 128 forced
    for N, M in itertools.product([128, 129, 208, 209], [33, 129]):
        for cfg in (["0", "1"] if N <= 208 else ["0"]):
            cs.append(Case("ex-tile-%d-%d-cfg%s" % (M, N, cfg), "ex", M, N, 20, 0, 1, lda=24, ldb=24, ws=None, cfg={"RECON_GEMM_CFG": cfg}, load="vec4"))
    cs.append(Case("ex-tile-nn-33-208", "ex", 33, 208, 20, 0, 0, lda=24, ldb=212, ws=None, load="vec4"))
    cs.append(Case("ex-tile-tn-36-208", "ex", 36, 208, 20, 1, 0, lda=40, ldb=212, ws=None, load="vec4"))
    # RECON_GEMM_LIN=0 (the general loader in place of the linear one): bit-identical to the default run of the same call
    for o in ("nn", "nt", "tn"):
        twin = "ex-%s-vec4-unsplit-tight" % o
        akm, bnk = {v: k for k, v in ORIENT_NAME.items()}[o]
        c = Case("ex-lin0-" + o, "ex", 36, 40, 40, akm, bnk, ws=None, cfg={"RECON_GEMM_LIN": "0"}, load="vec4", same_as=twin)
        c.lda, c.ldb = _r4(c.a_shape()[1]) + 4, _r4(c.b_shape()[1]) + 4
        cs.append(c)
    # RECON_GEMM_XCD=0 (tiles in launch order) on a 3 x 3 grid
    cs.append(Case("ex-xcd-default", "ex", 300, 300, 40, 0, 1, lda=44, ldb=44, ws=None, load="vec4"))
    cs.append(Case("ex-xcd0", "ex", 300, 300, 40, 0, 1, lda=44, ldb=44, ws=None, cfg={"RECON_GEMM_XCD": "0"}, load="vec4", same_as="ex-xcd-default"))
    # split-K: the natural choice (two splits of 160 and 140), three forced ones (k_per_split = 112: a ragged last split), NULL
    # workspace at the same shape (must run unsplit: bit-identical to the run whose split count the switch holds at 1)
    cs.append(Case("ex-split-natural", "ex", 33, 40, 300, 0, 1, lda=304, ldb=304, load="vec4", split=True, query=2 * 33 * 40))
    cs.append(Case("ex-split-forced3", "ex", 33, 40, 300, 0, 1, lda=304, ldb=304, cfg={"RECON_GEMM_SPLITK": "3"}, load="vec4", split=True, query=3 * 33 * 40))
    cs.append(Case("ex-split-forced3-ldcpad", "ex", 33, 40, 300, 0, 1, lda=304, ldb=304, ldc=47, cfg={"RECON_GEMM_SPLITK": "3"}, load="vec4", split=True,
                   query=3 * 33 * 40))
    cs.append(Case("ex-split-held1", "ex", 33, 40, 300, 0, 1, lda=304, ldb=304, cfg={"RECON_GEMM_SPLITK": "1"}, load="vec4", query=0))
    cs.append(Case("ex-split-null-ws", "ex", 33, 40, 300, 0, 1, lda=304, ldb=304, ws=None, load="vec4", same_as="ex-split-held1"))
    cs.append(Case("ex-split-n41", "ex", 33, 41, 300, 0, 1, lda=304, ldb=304, load="vec4", split=True, query=2 * 33 * 41))
    cs.append(Case("ex-split-n41-ldcpad", "ex", 33, 41, 300, 0, 1, lda=304, ldb=304, ldc=44, load="vec4", split=True, query=2 * 33 * 41))
    cs.append(Case("ex-split-n208", "ex", 33, 208, 300, 0, 1, lda=304, ldb=304, ldc=212, load="vec4", split=True, query=2 * 33 * 208))    # float4 partial stores
    # ldc, and a misaligned C, for the float4 stores of the 208-wide tile and for single-float stores
    for ldc, offc in [(208, 0), (212, 0), (209, 0), (212, 1)]:
        cs.append(Case("ex-ldc-n208-%d-%d" % (ldc, offc), "ex", 33, 208, 20, 0, 1, lda=24, ldb=24, ldc=ldc, offc=offc, ws=None, load="vec4"))
    for ldc in (41, 45, 42):
        cs.append(Case("ex-ldc-n41-%d" % ldc, "ex", 33, 41, 19, 0, 1, lda=24, ldb=24, ldc=ldc, ws=None, load="scalar:extent"))
    # the call of recon_amd/kg_eval.py: P = T W_k^T with W_k the k-th D x D block of W1 [D][3 D]
    for D, k in itertools.product([37, 200], [0, 1, 2]):
        cs.append(Case("ex-kgeval-D%d-k%d" % (D, k), "ex", 50, D, D, 0, 1, lda=D, ldb=3 * D, offb=k * D, ws=None,
                       load="vec4" if D % 4 == 0 else "scalar:mixed"))
    cs.append(Case("ex-refused-tt", "ex", 36, 40, 40, 1, 1, lda=40, ldb=44, ws=None, expect=UNSUPPORTED))
    for (akm, bnk) in [(0, 0), (0, 1), (1, 0)]:
        o = ORIENT_NAME[(akm, bnk)]
        for name, (M, N, K) in [("m1", (1, 40, 24)), ("n1", (36, 1, 24)), ("k1", (36, 40, 1))]:
            c = Case("ex-edge-%s-%s" % (o, name), "ex", M, N, K, akm, bnk, ws=None, load="scalar:mixed")
            c.lda, c.ldb = c.a_shape()[1] + 3, c.b_shape()[1] + 2
            cs.append(c)
    return cs


def _small_loads(akm, bnk):
    """The reasons that can turn recon_sgemm_small's float4 loads off in one orientation."""
    out = ["vec4", "scalar:ld", "scalar:base"]
    if not akm or bnk:
        out.append("scalar:k")             # some operand is contiguous along k
    if akm or not bnk:
        out.append("scalar:mn")            # some operand is contiguous along m / n
    return out


def _small_cases():
    cs = []
    for (akm, bnk) in [(0, 0), (0, 1), (1, 0), (1, 1)]:
        for load, split, pad in itertools.product(_small_loads(akm, bnk), [False, True], [False, True]):
            M, N, K = 20, 36, (1100 if split else 64)
            if load == "scalar:k":
                K += 1
            if load == "scalar:mn":
                if akm:
                    M += 1
                else:
                    N += 1
            c = Case("small-%s-%s-%s-%s" % (ORIENT_NAME[(akm, bnk)], load.replace("scalar:", "s_"), "split" if split else "unsplit", "ldcpad" if pad else "tight"),
                     "small", M, N, K, akm, bnk, ldc=N + 4 if pad else N, load=load, split=split, query=2 * M * N if split else 0)
            c.lda, c.ldb = _r4(c.a_shape()[1]) + 4, _r4(c.b_shape()[1]) + 4
            if load == "scalar:ld":
                c.ldb += 1
            if load == "scalar:base":
                c.offa = 1
            cs.append(c)
        o = ORIENT_NAME[(akm, bnk)]
        for K in (1, 2, 3, 4, 17, 63, 64, 65):         # the per-slice rounding of ks and the tail masks
            c = Case("small-%s-K%d" % (o, K), "small", 20, 36, K, akm, bnk, query=0,
                     load="vec4" if (K % 4 == 0 or (akm and not bnk)) else "scalar:k")
            c.lda, c.ldb = _r4(c.a_shape()[1]) + 4, _r4(c.b_shape()[1]) + 4
            cs.append(c)
    cs.append(Case("small-split-null-ws", "small", 20, 36, 1100, 0, 0, lda=1104, ldb=40, ws=None, load="vec4"))
    cs.append(Case("small-K0-ldcpad", "small", 20, 36, 0, 0, 0, lda=4, ldb=40, ldc=41, query=0))
    cs.append(Case("small-M0", "small", 0, 36, 64, 0, 0, lda=68, ldb=40, query=0))        # RECON_OK, nothing launched
    cs.append(Case("small-N0", "small", 20, 0, 64, 0, 0, lda=68, ldb=4, query=0))
    cs.append(Case("small-refused-lda", "small", 20, 36, 64, 0, 0, lda=63, ldb=40, expect=INVALID))
    cs.append(Case("small-refused-ldb", "small", 20, 36, 64, 0, 0, lda=68, ldb=35, expect=INVALID))
    cs.append(Case("small-refused-ldc", "small", 20, 36, 64, 0, 0, lda=68, ldb=40, ldc=35, expect=INVALID))
    for (akm, bnk) in [(0, 0), (1, 1)]:
        o = ORIENT_NAME[(akm, bnk)]
        for name, (M, N) in [("m1", (1, 36)), ("n1", (20, 1)), ("m17n15", (17, 15))]:
            c = Case("small-edge-%s-%s" % (o, name), "small", M, N, 24, akm, bnk, query=0, load="scalar:mixed")
            c.lda, c.ldb = c.a_shape()[1] + 3, c.b_shape()[1] + 2
            cs.append(c)
    return cs


def _store_load(N, ldc, offc):
    """Width of the output stores of the k-contiguous 16-bit kernels (c_vec4_ok of csrc/gemm_tile16.h), with the reason."""
    if N % 4:
        return "scalar:n"
    if ldc % 4:
        return "scalar:ldc"
    if offc % 4:
        return "scalar:base"
    return "vec4"


def _kc16_cases(entry, shapes, rings):
    """bx3 / hx2: C = A B^T with A [M,K], B [N,K].  B is only read by the split pass, so it may have any stride."""
    cs = []
    for (M, N, K), dlda, dldb, dldc, ring in itertools.product(shapes, [0, 4], [0, 1], [0, 4, 1], rings):
        cfg = {"RECON_HX2_RING": ring} if ring is not None else {}
        cs.append(Case("%s-%d-%d-%d-lda%d-ldb%d-ldc%d%s" % (entry, M, N, K, K + dlda, K + dldb, N + dldc, "" if ring in (None, "1") else "-ring0"),
                       entry, M, N, K, lda=K + dlda, ldb=K + dldb, ldc=N + dldc, cfg=cfg, load=_store_load(N, N + dldc, 0)))
    M, N, K = shapes[0]
    for ring in rings:
        cfg = {"RECON_HX2_RING": ring} if ring is not None else {}
        cs.append(Case("%s-%d-%d-%d-offc1%s" % (entry, M, N, K, "" if ring in (None, "1") else "-ring0"), entry, M, N, K, lda=K + 4, ldb=K + 1, ldc=N + 4,
                       offc=1, cfg=cfg, load="scalar:base"))
    return cs


def _km16_cases(entry):
    """bx3_tn / hx2_tn: C = A^T B with A [K,M], B [K,N]; K = 32, 129, 300, 1000 at 36 x 24 is 1, 1, 2 and 7 splits (whole K tiles of
    32 per split: 160 + 140, and 6 x 160 + 40)."""
    sa, sb = (1e-3, 50.0) if entry == "hx2_tn" else (1.0, 1.0)
    cs = []
    for (K, splits), dlda, dldb, dldc in itertools.product([(32, 1), (129, 1), (300, 2), (1000, 7)], [0, 4], [0, 3], [0, 5]):
        M, N = 36, 24
        cs.append(Case("%s-K%d-lda%d-ldb%d-ldc%d" % (entry, K, M + dlda, N + dldb, N + dldc), entry, M, N, K, lda=M + dlda, ldb=N + dldb, ldc=N + dldc,
                       load="scalar", split=splits > 1, splits=splits, sa=sa, sb=sb))
    # two row tiles, two column tiles, a column tail that is no multiple of 8
    cs.append(Case("%s-132-209-40" % entry, entry, 132, 209, 40, lda=136, ldb=212, ldc=210, load="scalar", splits=1, sa=sa, sb=sb))
    cs.append(Case("%s-36-21-300" % entry, entry, 36, 21, 300, lda=40, ldb=21, ldc=21, load="scalar", split=True, splits=2, sa=sa, sb=sb))
    return cs


def _bx3_cases():
    cs = _kc16_cases("bx3", [(128, 208, 32), (33, 257, 20), (130, 209, 36)], [None])
    cs.append(Case("bx3-refused-K18", "bx3", 33, 40, 18, lda=20, expect=UNSUPPORTED))
    cs.append(Case("bx3-refused-lda21", "bx3", 33, 40, 20, lda=21, expect=UNSUPPORTED))
    cs.append(Case("bx3-refused-offa1", "bx3", 33, 40, 20, lda=24, offa=1, expect=UNSUPPORTED))
    cs += _km16_cases("bx3_tn")
    cs.append(Case("bx3_tn-refused-M37", "bx3_tn", 37, 24, 64, lda=40, expect=UNSUPPORTED))
    cs.append(Case("bx3_tn-refused-M2", "bx3_tn", 2, 24, 64, lda=4, expect=UNSUPPORTED))
    cs.append(Case("bx3_tn-refused-lda38", "bx3_tn", 36, 24, 64, lda=38, expect=UNSUPPORTED))
    return cs


def _hx2_cases():
    cs = _kc16_cases("hx2", [(128, 208, 32), (33, 257, 24), (130, 209, 40)], ["1", "0"])
    for ring in ("1", "0"):                            # the third of the three smallest shapes test_sgemm_hx2 names, at a padded stride
        cs.append(Case("hx2-200-72-56-ring%s" % ring, "hx2", 200, 72, 56, lda=60, ldb=57, ldc=76, cfg={"RECON_HX2_RING": ring}, load="vec4"))
    cs.append(Case("hx2-refused-K20", "hx2", 33, 40, 20, expect=UNSUPPORTED))
    cs.append(Case("hx2-refused-ws", "hx2", 33, 40, 24, ws="misaligned", expect=INVALID))
    cs += _km16_cases("hx2_tn")
    cs.append(Case("hx2_tn-37-21-77", "hx2_tn", 37, 21, 77, lda=39, ldb=22, ldc=23, load="scalar", splits=1, sa=1e-3, sb=50.0))
    cs.append(Case("hx2_tn-1-24-40", "hx2_tn", 1, 24, 40, lda=2, ldb=24, ldc=24, load="scalar", splits=1, sa=1e-3, sb=50.0))
    cs.append(Case("hx2_tn-36-1-40", "hx2_tn", 36, 1, 40, lda=36, ldb=3, ldc=2, load="scalar", splits=1, sa=1e-3, sb=50.0))
    cs.append(Case("hx2_tn-refused-ws", "hx2_tn", 36, 24, 64, ws="misaligned", expect=INVALID))
    return cs


CASES = _ex_cases() + _small_cases() + _bx3_cases() + _hx2_cases()
BY_ID = {c.id: c for c in CASES}


def declared_matrix():
    """The cells (entry, orientation, load, split, padded ldc) that must each hold a case: entry x orientation x {vec4, scalar by each
    reason that exists there} x {unsplit, split} x {tight, padded ldc}."""
    cells = set()
    for o, load, split, pad in itertools.product(["nn", "nt", "tn"], ["vec4", "scalar:base", "scalar:ld", "scalar:extent"], [False, True], [False, True]):
        cells.add(("ex", o, load, split, pad))
    for (akm, bnk), o in ORIENT_NAME.items():
        for load, split, pad in itertools.product(_small_loads(akm, bnk), [False, True], [False, True]):
            cells.add(("small", o, load, split, pad))
    for entry in ("bx3", "hx2"):                       # no split-K in these; "scalar:ldc" needs a padded ldc, a misaligned base is one case
        for load, pad in [("vec4", False), ("vec4", True), ("scalar:ldc", True), ("scalar:n", False), ("scalar:n", True), ("scalar:base", True)]:
            cells.add((entry, "nt", load, False, pad))
    for entry in ("bx3_tn", "hx2_tn"):
        for split, pad in itertools.product([False, True], [False, True]):
            cells.add((entry, "tn", "scalar", split, pad))
    return cells


# ------------------------------------------------------------------------------------------------------------------- on the device
def _dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


class _View:
    """rows x cols floats at row stride `ld`, `off` elements into a NaN-filled buffer (layout())."""

    def __init__(self, rows, cols, ld, off, data=None):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.start, total, self.ld_alloc = layout(rows, cols, ld, off)
        self.host = torch.full((total,), NAN_BITS, dtype=torch.int32)
        self.outside = torch.ones(total, dtype=torch.bool)
        if rows and cols:
            self.outside[self.start:self.start + rows * self.ld_alloc].view(rows, self.ld_alloc)[:, :cols] = False
            if data is not None:
                self.host.view(torch.float32)[self.start:self.start + rows * self.ld_alloc].view(rows, self.ld_alloc)[:, :cols] = data
        self.buf = self.host.to(_dev())
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + 4 * self.start

    def bits(self):
        """(the whole buffer, the rows x cols view) as int32 on the CPU."""
        out = self.buf.cpu()
        if not (self.rows and self.cols):
            return out, out[:0].view(self.rows, self.cols)
        return out, out[self.start:self.start + self.rows * self.ld_alloc].view(self.rows, self.ld_alloc)[:, :self.cols].clone()


def _kp(x):
    return (x + 31) // 32 * 32


def _up256(x):
    return (x + 255) // 256 * 256


def _workspace(c, L):
    """(keep-alive tensor, pointer or None, bytes) of the entry's workspace — 0xFF bytes (NaN patterns) everywhere, 256 more behind
    the size the query names — after asserting what the query must answer for the path the case is named for."""
    M, N, K = c.M, c.N, c.K
    if c.entry in ("ex", "small"):
        q = (L.recon_sgemm_ex_workspace_floats if c.entry == "ex" else L.recon_sgemm_small_workspace_floats)(M, N, K)
        if c.query is not None:
            assert q == c.query, "workspace query answers %d floats, the case is named for %d" % (q, c.query)
        if c.split:
            assert q > M * N and q % (M * N) == 0
        nbytes = 4 * q
    elif c.entry == "bx3":
        nbytes = L.recon_sgemm_bx3_workspace_bytes(N, K)
    elif c.entry == "bx3_tn":
        nbytes = L.recon_sgemm_bx3_tn_workspace_bytes(M, N, K)
        if c.splits is not None:
            assert nbytes == _up256(3 * K * _kp(N) * 2) + c.splits * M * N * 4 + 256, "not %d splits" % c.splits
    elif c.entry == "hx2":
        nbytes = L.recon_sgemm_hx2_workspace_bytes(M, N, K)
    else:
        nbytes = L.recon_sgemm_hx2_tn_workspace_bytes(M, N, K)
        if c.splits is not None:
            hdr = _up256(L.recon_hx2_aux_bytes())
            assert nbytes == hdr + _up256(2 * K * _kp(M) * 2) + _up256(2 * K * _kp(N) * 2) + c.splits * M * N * 4 + 256, "not %d splits" % c.splits
    if c.ws is None:
        return None, None, 0
    t = torch.full((nbytes + 512,), 0xFF, dtype=torch.uint8, device=_dev())
    p = t.data_ptr()
    assert p % 256 == 0
    if c.ws == "misaligned":
        p += 16
    return t, p, nbytes


def _call(c, L, stream, A, B, Cv, wsp):
    M, N, K = c.M, c.N, c.K
    if c.entry == "ex":
        return L.recon_sgemm_ex(M, N, K, A.ptr, c.lda, c.akm, B.ptr, c.ldb, c.bnk, Cv.ptr, c.ldc, wsp, stream)
    if c.entry == "small":
        return L.recon_sgemm_small(M, N, K, A.ptr, c.lda, c.akm, B.ptr, c.ldb, c.bnk, Cv.ptr, c.ldc, wsp, stream)
    fn = {"bx3": L.recon_sgemm_bx3, "bx3_tn": L.recon_sgemm_bx3_tn, "hx2": L.recon_sgemm_hx2, "hx2_tn": L.recon_sgemm_hx2_tn}[c.entry]
    return fn(M, N, K, A.ptr, c.lda, B.ptr, c.ldb, Cv.ptr, c.ldc, wsp, stream)


def _run(c, recon_config):
    """Run one case with every assertion it carries; returns the bits of its M x N result (None for a refused call)."""
    from recon_amd import _lib
    L = _lib.lib()
    stream = _lib.current_stream()
    for name in SWITCHES:
        value = c.cfg.get(name)
        recon_config(name, value)
        got = L.recon_config_get(name.encode())
        assert (got.decode() if got is not None else None) == value, "switch %s is %r" % (name, got)
    Al, Bl = inputs(c)
    A = _View(*c.a_shape(), c.lda, c.offa, Al.t() if c.akm else Al)
    B = _View(*c.b_shape(), c.ldb, c.offb, Bl.t() if c.bnk else Bl)
    C1 = _View(c.M, c.N, c.ldc, c.offc)
    ws1, wsp1, nbytes = _workspace(c, L)
    rc = _call(c, L, stream, A, B, C1, wsp1)
    full1, view1 = C1.bits()
    assert torch.equal(A.buf.cpu(), A.host) and torch.equal(B.buf.cpu(), B.host), "an operand buffer was written"
    if ws1 is not None:
        assert bool((ws1[nbytes + (16 if c.ws == "misaligned" else 0):] == 0xFF).all()), "written behind the workspace"
    if c.expect != OK:
        assert rc == c.expect, "returned %d, the header documents %d" % (rc, c.expect)
        assert bool((full1 == NAN_BITS).all()), "a refused call wrote to its output"
        return None
    assert rc == OK, rc
    assert bool((full1[C1.outside] == NAN_BITS).all()), "%d elements outside the view were written" % int((full1[C1.outside] != NAN_BITS).sum())
    if c.M == 0 or c.N == 0:
        return view1
    got = view1.view(torch.float32)
    ref, bound = bound_of(c, Al, Bl)
    err = (got.double() - ref).abs()
    finite = bool(torch.isfinite(got).all())
    ratio = float((err / bound).max()) if finite else float("nan")
    print("GEMM_ABI %s entry=%s ratio=%.4f" % (c.id, c.entry, ratio))
    assert finite, "non-finite values in the result"
    assert bool((err <= bound).all()), ratio
    # run to run: a second buffer, a second (NaN-filled) workspace
    C2 = _View(c.M, c.N, c.ldc, c.offc)
    ws2, wsp2, _ = _workspace(c, L)
    assert _call(c, L, stream, A, B, C2, wsp2) == OK
    assert torch.equal(C1.buf, C2.buf), "two runs of the same call differ"
    if c.entry == "ex" and not c.akm and c.ws is None:           # the rows recon_sgemm can express: the same kernels, the same bits
        C3 = _View(c.M, c.N, c.ldc, c.offc)
        assert L.recon_sgemm(c.M, c.N, c.K, A.ptr, c.lda, B.ptr, c.ldb, c.bnk, C3.ptr, c.ldc, stream) == OK
        assert torch.equal(C1.buf, C3.buf), "recon_sgemm differs from recon_sgemm_ex"
    if c.entry in ("hx2", "hx2_tn"):                             # the GEMM alone on the planes the first call left in its workspace
        C3 = _View(c.M, c.N, c.ldc, c.offc)
        fn = L.recon_sgemm_hx2_presplit if c.entry == "hx2" else L.recon_sgemm_hx2_tn_presplit
        assert fn(c.M, c.N, c.K, C3.ptr, c.ldc, wsp1, stream) == OK
        assert torch.equal(C1.buf, C3.buf), "the presplit entry differs from the full call"
    return view1


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_sgemm_abi(cid, recon_config):
    c = BY_ID[cid]
    bits = _run(c, recon_config)
    if c.same_as is not None:
        other = _run(BY_ID[c.same_as], recon_config)
        # LIN=0 / XCD=0 / NULL workspace choose other addressing or another tile order, never another order of additions
        assert torch.equal(bits, other), "differs from %s in %d elements" % (c.same_as, int((bits != other).sum()))
