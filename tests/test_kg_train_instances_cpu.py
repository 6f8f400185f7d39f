"""Guard of tests/test_kg_train_instances_gpu.py (host only).

Coverage: KGT_FWD_ROWS holds every instance of k_kgt_fwd at its lowest and highest D and in every class of M; KGT_BWD_ROWS names, for
every row, the split the library's own workspace query gives it, and holds every class of the split.  A change to kgt_bwd_split, or a
deleted row, fails here until the tables follow.

Stand-in: the GPU file's harness with the two library calls replaced by a float32 torch restatement on the CPU (the same formulas, the
same split into parts and 32-row blocks, torch's own order inside a product).  Every row must pass with at least a factor two of room:
no band is tighter than float32 itself.  The same harness must fail for six subtly wrong restatements: no band is vacuous.
"""
import pytest
import torch

from test_kg_train_instances_gpu import (KGT_FWD_ROWS, KGT_BWD_ROWS, WIDE_ROW, WIDE_W2_SCALE, M_ROTATION, SPLIT_CLASSES, SLOPE, TICKET_WORDS, FwdRow,
                                         split_classes, gathered, check_forward, check_backward, fwd_id, bwd_id)

SPLIT = {(r.D, r.M): r for r in KGT_BWD_ROWS}


def test_forward_rows_cover_every_instance_and_row_class():
    for NP in range(1, 9):
        rows = [r for r in KGT_FWD_ROWS if (r.D + 63) // 64 == NP]
        assert any(r.D == 64 * (NP - 1) + 1 for r in rows), "no row at the lowest D of k_kgt_fwd<%d>" % NP
        assert any(r.D == 64 * NP for r in rows), "no row at the highest D of k_kgt_fwd<%d>" % NP
        assert any(r.D % 64 not in (0, 1) and r.D % 2 for r in rows), "no row at an odd D inside k_kgt_fwd<%d>" % NP
        for name, cls in (("M < 32", lambda M: M < 32), ("M % 32 != 0 above 32", lambda M: M > 32 and M % 32), ("M % 32 == 0", lambda M: M % 32 == 0)):
            assert any(cls(r.M) for r in rows), "k_kgt_fwd<%d> has no row with %s" % (NP, name)
        assert {r.M for r in rows} >= set(M_ROTATION), "k_kgt_fwd<%d> misses a value of the M rotation" % NP
        assert {r.idx64 for r in rows} == {False, True} and len({r.ratio for r in rows}) == 3, NP
    assert any((r.M + 31) // 32 > 64 for r in KGT_FWD_ROWS), "no row whose mean adds more than 64 workgroup sums"
    assert len({fwd_id(r) for r in KGT_FWD_ROWS}) == len(KGT_FWD_ROWS)


def test_backward_rows_name_the_split_the_library_takes():
    from recon_amd import _lib
    L = _lib.lib()
    for r in KGT_BWD_ROWS:
        floats = L.recon_convkb_train_bwd_workspace_floats(r.M, r.D)
        per_part = 3 * r.D * r.D + 2 * r.D + 1
        assert (floats - TICKET_WORDS) % per_part == 0, bwd_id(r)
        assert (floats - TICKET_WORDS) // per_part == r.P, "%s: the library splits into %d parts" % (bwd_id(r), (floats - TICKET_WORDS) // per_part)
        assert r.rows_per_part % 64 == 0 and -(-r.M // r.rows_per_part) == r.P, bwd_id(r)
        assert r.last == r.M - (r.P - 1) * r.rows_per_part and 1 <= r.last <= r.rows_per_part, bwd_id(r)
    # rows_per_part itself: the only multiple of 64 with ceil(M / rows_per_part) = P that the rule's ceil(ceil(M / P') / 64) 64 can give is
    # the smallest one
    for r in KGT_BWD_ROWS:
        assert r.rows_per_part == 64 or -(-r.M // (r.rows_per_part - 64)) > r.P, bwd_id(r)
    have = set().union(*(split_classes(r) for r in KGT_BWD_ROWS))
    assert not set(SPLIT_CLASSES) - have, "split classes without a row: %s" % sorted(set(SPLIT_CLASSES) - have)
    for cls in SPLIT_CLASSES:
        assert any(r.g3 for r in KGT_BWD_ROWS if cls in split_classes(r)), "no g_scale = [3.0] row in class " + cls
    assert any(r.D == 200 and r.M == 5184 for r in KGT_BWD_ROWS), "the workload's own shape"
    assert any(-(-r.D // 64) * -(-3 * r.D // 64) == 192 for r in KGT_BWD_ROWS), "no row with 192 tiles"
    assert len({bwd_id(r) for r in KGT_BWD_ROWS}) == len(KGT_BWD_ROWS)


class StandIn:
    """The two calls in float32 torch on the CPU.  `wrong` names one defect."""

    def __init__(self, wrong=None):
        self.wrong = wrong

    def fwd(self, inp, row, values, want_z, want_terms):
        D, M = inp["D"], inp["M"]
        X = gathered(inp, torch.float32)
        acc = X @ inp["W1"].T
        if self.wrong == "last column group":
            acc[:, 64 * ((D + 63) // 64 - 1):] = 0
        z = acc + inp["b1"]
        s = torch.where(z > 0, z, z * SLOPE) @ inp["w2"] + inp["b2"]
        out = dict(z=z if want_z else None, s=s, terms=None, gs=None, loss=None)
        if values:
            one = torch.tensor(1.0)
            y = (inp["val"] + 1) / 2
            w = y + (1 - y) / torch.tensor(2.0 * row.ratio)
            mx = torch.clamp(-s, min=0)
            if self.wrong == "no mx shift":
                terms = w * ((1 - y) * s + torch.log(1 + torch.exp(-s)))
            else:
                terms = w * ((1 - y) * s + mx + torch.log(torch.exp(-mx) + torch.exp(-s - mx)))
            out["gs"] = ((one / (one + torch.exp(-s)) - y) * w) * (one / torch.tensor(float(M)))
            blocks = torch.cat([terms, torch.zeros(-M % 32)]).view(-1, 32).sum(1)        # one sum per workgroup of 32 rows
            if self.wrong == "blocks past 64":
                blocks = blocks[:64]
            out["loss"] = (blocks.sum() / torch.tensor(float(M))).view(1)
            out["terms"] = terms if want_terms else None
        return out

    def bwd(self, inp, row, z, gs, g_scale):
        D, M = inp["D"], inp["M"]
        r = SPLIT[(D, M)]
        X = gathered(inp, torch.float32)
        gm = gs if g_scale is None else gs * torch.tensor(float(g_scale))
        dh = gm[:, None] * inp["w2"][None, :]
        dl = torch.where(z > 0, dh, dh * SLOPE)
        h = torch.where(z > 0, z, z * SLOPE)
        dW1, db1, dw2, db2 = torch.zeros(D, 3 * D), torch.zeros(D), torch.zeros(D), torch.zeros(1)
        parts = r.P - 1 if self.wrong == "P - 1 partials" else r.P
        for p in range(parts):
            lo, hi = p * r.rows_per_part, min((p + 1) * r.rows_per_part, M)
            if self.wrong == "last chunk of each part":
                hi = lo + (hi - lo - 1) // 64 * 64
            if self.wrong == "first chunk only":
                hi = min(hi, lo + 64)
            dW1 += dl[lo:hi].T @ X[lo:hi]
            db1 += dl[lo:hi].sum(0)
            dw2 += gm[lo:hi] @ h[lo:hi]
            db2 += gm[lo:hi].sum()
        return dW1, db1, dw2, db2


def test_float32_stand_in_passes_every_row_at_half_of_every_band():
    be = StandIn()
    worst = {}
    for r in KGT_FWD_ROWS:
        for k, q in check_forward(be, r).items():
            worst[k] = max(worst.get(k, 0.0), q)
    for k, q in check_forward(be, WIDE_ROW, w2_scale=WIDE_W2_SCALE, wide=True).items():
        worst["wide " + k] = q
    for r in KGT_BWD_ROWS:
        for k, q in check_backward(be, r).items():
            worst[k] = max(worst.get(k, 0.0), q)
    print("KGT_INST stand-in worst error / band: " + " ".join("%s=%.4f" % kv for kv in sorted(worst.items())))
    print("KGT_INST stand-in worst of all: %.4f" % max(worst.values()))
    assert max(worst.values()) <= 0.5, worst


def _fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


def test_harness_fails_a_backward_that_drops_each_parts_last_chunk():
    be = StandIn("last chunk of each part")
    for r in KGT_BWD_ROWS:
        assert _fails(check_backward, be, r), bwd_id(r)


def test_harness_fails_a_backward_that_stops_after_each_parts_first_chunk():
    be = StandIn("first chunk only")
    for r in KGT_BWD_ROWS:
        assert _fails(check_backward, be, r) == (r.rows_per_part > 64), bwd_id(r)


def test_harness_fails_a_backward_that_adds_one_partial_too_few():
    """The bands are 2 (M + 4) EPS32 of the sum of magnitudes over M rows, the width of 2 (M + 4) EPS32 M average rows: a dropped last part
    shows wherever it holds more rows than that.  Only the 130 000-row row is past it (80 rows against 2 015); its P = 1 016 partials are
    held by the float64 comparison itself."""
    be = StandIn("P - 1 partials")
    seen = 0
    for r in KGT_BWD_ROWS:
        if r.last > 2 * (r.M + 4) * 2.0 ** -24 * r.M:
            assert _fails(check_backward, be, r), bwd_id(r)
            seen += 1
    assert seen == len(KGT_BWD_ROWS) - 1


def test_harness_fails_a_forward_without_its_last_column_group():
    be = StandIn("last column group")
    for r in KGT_FWD_ROWS:
        assert _fails(check_forward, be, r), fwd_id(r)


def test_harness_fails_a_mean_without_the_blocks_past_64():
    be = StandIn("blocks past 64")
    for r in KGT_FWD_ROWS:
        assert _fails(check_forward, be, r) == ((r.M + 31) // 32 > 64), fwd_id(r)


def test_harness_fails_loss_terms_without_the_mx_shift():
    be = StandIn("no mx shift")
    assert _fails(check_forward, be, WIDE_ROW, w2_scale=WIDE_W2_SCALE, wide=True)
    assert not _fails(check_forward, StandIn(), WIDE_ROW, w2_scale=WIDE_W2_SCALE, wide=True)
