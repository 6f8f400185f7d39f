"""The guard of tests/test_stage_a_tail_gpu.py, without a GPU: the inputs meet the conditions the GPU checks rely on, the float32 NumPy
restatement of every kernel (stage_a_tail_checks.Restated, in the kernels' order) passes every check of norm.hip, loss.hip and rel_mm.hip
with the CPU's fp32 torch lines as the chain, and every wrong restatement fails at least one."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stage_a_tail_checks as sa
from stage_a_tail_checks import Guarded, Restated

MARGIN_CASES = [(D, mis, n_pos, reps) for (D, mis) in sa.MARGIN_WIDTHS for (n_pos, reps) in sa.MARGIN_PAIRS]


# ------------------------------------------------------------------------------------------------------------- the inputs
def test_the_norm_grid_holds_every_size_and_the_special_rows():
    assert {n for n, _ in sa.NORM_SHAPES} == {1, 3, 4, 5, 9} and {c for _, c in sa.NORM_SHAPES} == {1, 37, 63, 64, 65, 128, 200, 257}
    assert (9, 200) in sa.NORM_SHAPES and (1, 1) in sa.NORM_SHAPES
    for N, C in sa.NORM_SHAPES:
        c = sa.norm_case(N, C, "skip_mask")
        y, norm, g_t, g_skip = c["ref"]
        assert all(np.isfinite(a).all() for a in c["ref"])
        assert np.abs(c["ew"]).max() < 1e5                              # far from 1e19, where the fp32 sum of squares overflows
        if N >= 3:
            s = c["special"]
            assert norm[s["zero"]] == 0 and not y[s["zero"]].any() and not g_skip[s["zero"]].any() and c["mask"][s["zero"]] == 0
            assert 1e-13 <= norm[s["small"]] <= 5e-13 < sa.EPS          # the clamp branch, far from its threshold
            assert 0 < norm[s["tiny"]] < 1e-18 and (c["ew"][s["tiny"]].astype(np.float32) ** 2 < 2.0 ** -126).all()      # denormal squares
            np.testing.assert_allclose(y[s["small"]], (c["ew"][s["small"]].astype(np.float64) + 0.5 * c["skip"][s["small"]]) / sa.EPS, rtol=1e-12)
            np.testing.assert_allclose(g_t[s["small"]], c["gy"][s["small"]].astype(np.float64) / sa.EPS, rtol=1e-12)       # F.normalize's own backward below eps
            np.testing.assert_allclose(g_t[s["zero"]], c["gy"][s["zero"]].astype(np.float64) / sa.EPS, rtol=1e-12)
        if N >= 9:
            assert {0.0, 1.0, 0.5, 2.0, -1.0} <= set(c["mask"].tolist())
        ordinary = [r for r in range(N) if r not in c["special"].values()]
        assert (norm[ordinary] > 1e-6).all()                            # no ordinary row near eps


@pytest.mark.parametrize("D,mis,n_pos,reps", MARGIN_CASES)
def test_margin_inputs_meet_their_conditions(D, mis, n_pos, reps):
    c = sa.margin_case(D, n_pos, reps, mis)
    assert sa.margin_conditions(c) == []
    assert c["tri"][0, 0] == c["tri"][0, 2] and ((c["tri"][:, 0] == c["tri"][:, 2]).nonzero()[0].tolist() == [0, n_pos])
    assert c["planted_zeros"] == reps * min(4, D - 1)
    assert c["P"] % 4 == {1: 1, 3: 3, 10: 2, 42: 2, 268: 0}[c["P"]]
    assert float(c["margin"]) == float(np.float32(c["margin"]))


def test_margin_widths_select_the_paths_named():
    vec = {D for D, mis in sa.MARGIN_WIDTHS if Restated._vec4(D, mis)}
    assert vec == {4, 64, 252, 256, 260, 508, 512, 200}
    assert not Restated._vec4(200, True) and not Restated._vec4(516, False) and not Restated._vec4(1028, False)
    assert [(n * r) for n, r in sa.MARGIN_PAIRS] == [1, 3, 10, 42, 268]


def test_zero_case_is_exact_and_the_stock_lines_pass_the_gradient_at_zero():
    c = sa.zero_case()
    ent = torch.from_numpy(c["ent"]).requires_grad_(True)
    rel = torch.from_numpy(c["rel"]).requires_grad_(True)
    tri = torch.from_numpy(c["tri"])
    pos, neg = tri[:3].repeat(2, 1), tri[3:]
    pn = torch.norm(ent[pos[:, 0]] + rel[pos[:, 1]] - ent[pos[:, 2]], p=1, dim=1)
    nn = torch.norm(ent[neg[:, 0]] + rel[neg[:, 1]] - ent[neg[:, 2]], p=1, dim=1)
    assert (pn - nn + 1.0).tolist() == [0.0, 2.0, -15.0, -15.0, -14.0, -15.0]      # exact in fp32 too
    g_pn = torch.autograd.grad(F.margin_ranking_loss(pn, nn, -torch.ones(6), margin=1.0, reduction="sum"), pn)[0]
    assert g_pn.tolist() == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]                             # the stock lines pass the gradient at a pre-clamp value of exactly 0
    be = Restated()
    rows = Guarded(6 * 6 * 4, lead=0)
    assert be.margin_bwd(c["ent"], c["rel"], c["tri"], 3, 2, 4, np.array([0.0, 2.0, 0.0, 0.0, 0.0, 0.0], np.float32), np.float32(1.0), rows) == 0
    r = rows.cells().reshape(6, 6, 4)
    assert not r[:, 0].any() and not r[:, 2:].any() and r[:, 1].any()    # the kernels' rule: a term of 0 is inactive


def test_rel_shapes_hold_what_they_are_there_for():
    assert sa.REL_SHAPES[2][1] * 16 * 4 == 48 * 1024 and all(16 * 4 * s[1] > 48 * 1024 for s in sa.BIG_LDS)
    c = sa.rel_case((40, 16, 16, 6))
    assert np.diff(c["seg"]).tolist() == [0, 8, 9, 1, 22, 0] and (np.diff(c["rel"]) < 0).any()
    assert all(np.isfinite(a).all() for s in sa.REL_SHAPES for a in sa.rel_case(s)["ref"])


# ------------------------------------------------------------------------------------------------------------- the restatement passes
@pytest.mark.parametrize("form", sa.NORM_FORMS)
@pytest.mark.parametrize("N,C", sa.NORM_SHAPES)
def test_restated_norm_passes(N, C, form):
    assert sa.norm_failures(Restated(), N, C, form) == []


@pytest.mark.parametrize("D,mis", sa.MARGIN_WIDTHS)
def test_restated_margin_passes(D, mis):
    for n_pos, reps in sa.MARGIN_PAIRS:
        assert sa.margin_failures(Restated(), sa.margin_case(D, n_pos, reps, mis)) == []


def test_restated_margin_propagates_nan():
    assert sa.margin_nan_failures(Restated()) == []


def test_aligned_and_misaligned_tables_agree_within_the_band():
    for n_pos, reps in sa.MARGIN_PAIRS:
        a, m = sa.margin_case(200, n_pos, reps, False), sa.margin_case(200, n_pos, reps, True)
        assert np.array_equal(a["ent"], m["ent"]) and np.array_equal(a["tri"], m["tri"]) and a["margin"] == m["margin"]


@pytest.mark.parametrize("shape", sa.REL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restated_rel_mm_passes(shape):
    assert sa.rel_failures(Restated(), shape) == []


# ------------------------------------------------------------------------------------------------------------- the checks bite
@pytest.mark.parametrize("wrong", Restated.WRONG_NORM)
def test_a_wrong_norm_restatement_fails(wrong):
    bad = [b for N, C in ((9, 200), (5, 64), (3, 37)) for b in sa.norm_failures(Restated(wrong), N, C, "skip_mask")]
    assert bad, wrong
    print(wrong, bad[:3])


@pytest.mark.parametrize("wrong", Restated.WRONG_MARGIN)
def test_a_wrong_margin_restatement_fails(wrong):
    be = Restated(wrong)
    bad = sa.margin_nan_failures(be) + [b for D, n_pos, reps in ((37, 7, 6), (260, 5, 2)) for b in sa.margin_failures(be, sa.margin_case(D, n_pos, reps))]
    assert bad, wrong
    print(wrong, bad[:3])


@pytest.mark.parametrize("wrong", Restated.WRONG_REL)
def test_a_wrong_rel_mm_restatement_fails(wrong):
    bad = [b for shape in ((40, 16, 16, 6), (17, 15, 17, 3))
           if not (wrong == "untransposed" and shape[1] != shape[2]) for b in sa.rel_failures(Restated(wrong), shape)]
    assert bad, wrong
    print(wrong, bad[:3])


def test_one_element_past_an_output_fails_the_guard():
    be = Restated("past_end")
    for bad in (sa.norm_failures(be, 5, 64, "skip_mask"), sa.margin_failures(be, sa.margin_case(37, 5, 2)), sa.rel_failures(be, (17, 15, 17, 3))):
        assert bad and all("guard" in b for b in bad), bad
    g = Guarded(5)
    assert g.intact() and not g.written() and (g.off * 4) % 16 == 4
    g.cells()[:] = 1.0
    assert g.intact() and g.written()
    g.buf[g.off - 1] = 0.0
    assert not g.intact()
