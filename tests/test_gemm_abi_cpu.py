"""The case tables of tests/test_gemm_abi_gpu.py, checked without a device: the declared matrix has no empty cell, every case is what
its tags say (the host-side predicates of csrc/gemm_f32.hip and csrc/gemm_tile16.h, mirrored here, choose the named load / store
width for exactly the named reason), every view fits the buffer the helper allocates, and the bound the device is held to is met
by a plain float32 product of the same inputs with a factor two of room — so a miss on the device is the kernel's."""
import numpy as np

import test_gemm_abi_gpu as G


def _cell(c):
    return (c.entry, c.orient, c.load, c.split, c.padded)


def missing_cells(cases):
    have = {_cell(c) for c in cases if c.expect == G.OK and c.load is not None}
    return sorted(G.declared_matrix() - have, key=str)


def test_sgemm_abi_matrix_has_no_empty_cell():
    missing = missing_cells(G.CASES)
    assert not missing, "no case for: " + "; ".join("%s %s %s %s %s" % (e, o, l, "split" if s else "unsplit", "padded ldc" if p else "tight ldc")
                                                    for e, o, l, s, p in missing)


def test_sgemm_abi_matrix_check_names_an_emptied_cell():
    for cell in [("ex", "tn", "scalar:extent", True, True), ("small", "tt", "scalar:mn", False, False), ("hx2", "nt", "scalar:ldc", False, True),
                 ("bx3_tn", "tn", "scalar", True, False)]:
        assert cell in G.declared_matrix()
        assert missing_cells([c for c in G.CASES if _cell(c) != cell]) == [cell]


def test_sgemm_abi_case_ids_are_unique_and_references_exist():
    assert len(G.BY_ID) == len(G.CASES)
    for c in G.CASES:
        if c.same_as is not None:
            o = G.BY_ID[c.same_as]
            assert (o.entry, o.M, o.N, o.K, o.akm, o.bnk) == (c.entry, c.M, c.N, c.K, c.akm, c.bnk) and o.same_as is None


def _failing(c):
    """The reasons for which the library's host code turns the float4 form of this call off."""
    f = set()
    if c.entry in ("ex", "small"):
        if c.offa % 4 or c.offb % 4:
            f.add("base")
        if c.lda % 4 or c.ldb % 4:
            f.add("ld")
    if c.entry == "ex":                                 # operand_vec4: the contiguous extent of either operand
        if (c.M if c.akm else c.K) % 4 or (c.K if c.bnk else c.N) % 4:
            f.add("extent")
    elif c.entry == "small":                            # the vec4 expression of recon_sgemm_small
        if (not c.akm or c.bnk) and c.K % 4:
            f.add("k")
        if (c.akm and c.M % 4) or (not c.bnk and c.N % 4):
            f.add("mn")
    elif c.entry in ("bx3", "hx2"):                     # c_vec4_ok
        if c.N % 4:
            f.add("n")
        if c.ldc % 4:
            f.add("ldc")
        if c.offc % 4:
            f.add("base")
    return f


def _each(cases, check):
    """Run check(case) over the table and fail once, naming every case that failed."""
    bad = []
    for c in cases:
        try:
            check(c)
        except AssertionError as e:
            bad.append("%s: %s" % (c.id, e))
    assert not bad, "\n".join(bad)


def _takes_the_named_width(c):
    if c.entry in ("bx3_tn", "hx2_tn"):
        assert c.load == "scalar" and c.split == (c.splits > 1)       # the second pass stores single floats
        return
    f = _failing(c)
    if c.load == "vec4":
        assert not f, f
    elif c.load == "scalar:mixed":
        assert f
    elif c.entry in ("ex", "small"):
        assert f == {c.load.split(":")[1]}, f           # the named reason and no other
    else:
        assert c.load.split(":")[1] in f, f
    if c.entry in ("ex", "small") and c.split:
        assert c.ws == "query" and c.query is not None and c.query % (c.M * c.N) == 0 and c.query // (c.M * c.N) > 1


def test_sgemm_abi_cases_take_the_named_width():
    _each([c for c in G.CASES if c.expect == G.OK and c.load is not None], _takes_the_named_width)


def _views_fit(c):
    for (rows, cols), ld, off in [(c.a_shape(), c.lda, c.offa), (c.b_shape(), c.ldb, c.offb), ((c.M, c.N), c.ldc, c.offc)]:
        start, total, ld_alloc = G.layout(rows, cols, ld, off)
        assert off >= 0 and ld >= 0 and start >= G.GUARD
        if c.expect == G.OK:
            assert ld >= cols and ld_alloc == max(ld, 1)            # rows do not overlap
        if rows:
            # the last element the callee may touch with the stride it is GIVEN, and with the stride the buffer is laid out with
            assert start + (rows - 1) * ld + cols <= total - G.GUARD
            assert start + (rows - 1) * ld_alloc + cols <= total - G.GUARD
    if c.entry in ("bx3", "hx2") and c.expect == G.OK:
        assert c.lda % 4 == 0 and c.offa % 4 == 0 and c.K % (8 if c.entry == "hx2" else 4) == 0
    if c.entry == "bx3_tn" and c.expect == G.OK:
        assert c.M % 4 == 0 and c.lda % 4 == 0 and c.offa % 4 == 0


def test_sgemm_abi_views_fit_their_buffers():
    _each(G.CASES, _views_fit)


def _float32_has_margin(c):
    A, B = G.inputs(c)
    ref, bound = G.bound_of(c, A, B)
    f32 = np.matmul(A.numpy(), B.numpy(), dtype=np.float32) if c.K else np.zeros((c.M, c.N), np.float32)
    err = np.abs(f32.astype(np.float64) - ref.numpy())
    assert np.isfinite(f32).all()
    ratio = float((err / bound.numpy()).max())
    assert ratio <= 0.5, ratio


def test_sgemm_abi_bound_holds_for_float32_with_margin():
    _each([c for c in G.CASES if c.expect == G.OK and c.M and c.N], _float32_has_margin)
