"""Guard of tests/test_proj_instances_gpu.py (host only).

Coverage: a sweep of recon_gat_edge_instance over D = 1 ... 2100 at all three alignments reaches 21 keys; every one has its rows in
PROJ_ROWS (a tail row, the exact upper width, the empty-register-row rows of KR = 4 / 8), every row selects the key it names, every G
has its tall graph and `small` has every degree the unroll tails need.  A change to pick_shape (csrc/gat.hip), or a deleted row, fails
here until the table follows.

Inputs: every row's scores keep 64 score bands away from LeakyReLU's kink, every exp(-leakyrelu(sigma)) stays inside [1e-30, 1e30], and
the hand-written float64 backward the bands are built from agrees with autograd.

Stand-in: the GPU file's harness with the two library calls replaced by a float32 torch restatement on the CPU (torch's own summation
order).  Every row must pass with about a factor two of room: no band is tighter than float32 itself.  The same harness must fail for
nine subtly wrong restatements: no band is vacuous.
"""
import collections

import numpy as np
import torch

from test_proj_instances_gpu import (PROJ_ROWS, KEYS, ALIGN, SMALL_DEGREES, NODE_POS, NODE_NEG, row_id, key_parts, graph_edges, csr,
                                     make_case, check_row, _seg)


def _rows_of(key):
    return [r for r in PROJ_ROWS if r.key == key]


def test_instance_query_follows_pick_shape():
    from recon_amd import _lib
    L = _lib.lib()
    assert L.recon_gat_edge_instance(0, 4) == -1 and L.recon_gat_edge_instance(8, 3) == -1 and L.recon_gat_edge_instance(8, 0) == -1
    assert L.recon_gat_edge_instance(2052, 4) == -1 and L.recon_gat_edge_instance(1026, 2) == -1 and L.recon_gat_edge_instance(513, 1) == -1
    assert L.recon_gat_edge_instance(1026, 4) == -1 and L.recon_gat_edge_instance(513, 4) == -1           # D itself demotes them
    assert L.recon_gat_edge_instance(2048, 4) == 46408 and L.recon_gat_edge_instance(1024, 2) == 26408 and L.recon_gat_edge_instance(512, 1) == 16408
    assert L.recon_gat_edge_instance(50, 4) == 23201 and L.recon_gat_edge_instance(25, 4) == 13201        # the reference's widths
    assert L.recon_gat_edge_instance(64, 4) == 41601 and L.recon_gat_edge_instance(64, 2) == 23201 and L.recon_gat_edge_instance(64, 1) == 16401


def test_every_reachable_instance_has_its_rows():
    from recon_amd import _lib
    L = _lib.lib()
    reached = collections.defaultdict(list)
    for align in (4, 2, 1):
        for D in range(1, 2101):
            key = L.recon_gat_edge_instance(D, align)
            if key >= 0:
                reached[key].append((D, align))
    assert len(reached) == 21 and sorted(reached) == KEYS, sorted(reached)
    missing = sorted(set(reached) - {r.key for r in PROJ_ROWS})
    assert not missing, "instances without a row in PROJ_ROWS: %s (e.g. D, align = %s)" % (missing, [reached[k][0] for k in missing])
    for key in KEYS:
        vec, g, kr = key_parts(key)
        rows, vg = _rows_of(key), vec * g
        assert max(D for D, _ in reached[key]) == vg * kr
        assert any((kr - 1) * vg < r.D < kr * vg and r.D % vg for r in rows), "k%d: no row that ends inside the last register row" % key
        assert any(r.D == kr * vg for r in rows), "k%d: no row at the exact upper width %d" % (key, kr * vg)
        if kr >= 4:
            live = kr // 2 + 1
            assert any((live - 1) * vg < r.D <= live * vg for r in rows), "k%d: no row with %d live register rows" % (key, live)
    assert any(r.D == 25 for r in PROJ_ROWS) and all(r.D % 2 for r in PROJ_ROWS if r.key < 20000 and r.off == 0)
    assert any(r.D % 4 == 2 for r in PROJ_ROWS if 20000 < r.key < 30000)
    assert any(r.D == 2048 and r.H == 3 and r.graph == "small" for r in PROJ_ROWS)


def test_every_row_selects_its_instance():
    from recon_amd import _lib
    L = _lib.lib()
    ids = [row_id(r) for r in PROJ_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    assert len({r.seed for r in PROJ_ROWS}) == len(PROJ_ROWS)
    for r in PROJ_ROWS:
        assert L.recon_gat_edge_instance(r.D, ALIGN[r.off]) == r.key, row_id(r)
        assert r.H in (1, 2, 3)
    demoted = {r.off: r.key for r in PROJ_ROWS if r.D == 64 and r.note.startswith("demoted")}
    assert {off: key // 10000 for off, key in demoted.items()} == {0: 4, 2: 2, 1: 1}
    assert {r.H for r in PROJ_ROWS} == {1, 2, 3} and {r.concat for r in PROJ_ROWS} == {True, False}
    assert {r.alpha for r in PROJ_ROWS} == {0.2, 0.35}
    for vec in (4, 2, 1):                                               # every load width: several heads, both activations, both slopes
        rows = [r for r in PROJ_ROWS if r.key // 10000 == vec]
        assert {r.H for r in rows} == {1, 2, 3} and {r.concat for r in rows} == {True, False} and {r.alpha for r in rows} == {0.2, 0.35}
        assert {r.pad for r in rows if r.off == 0} == {0, 4}, "VEC %d: no row whose leading dimensions differ from H D" % vec
    assert all(r.pad == 0 for r in PROJ_ROWS if r.off) and [r.pad for r in PROJ_ROWS if r.note.startswith("demoted")] == [0, 0, 0]


def test_graphs_hold_what_the_rows_need():
    edge, N = graph_edges("small")
    c = csr("small")
    assert N == 203 and 1100 <= c["E"] <= 1400
    deg, outdeg = c["deg"].numpy(), c["outdeg"].numpy()
    for d in SMALL_DEGREES:
        assert (deg == d).any(), "no destination of in-degree %d" % d
        assert (outdeg == d).any(), "no source of out-degree %d" % d
    assert 140 <= deg.max() <= 170 and 130 <= outdeg.max() <= 170
    assert not deg[195:].any() and deg[0] > 0 and outdeg[202] > 0 and deg[NODE_POS] > 0 and deg[NODE_NEG] > 0
    pairs = collections.Counter(map(tuple, edge.T.tolist()))
    assert sum(1 for v in pairs.values() if v == 2) >= 30 and any(v >= 3 for v in pairs.values())
    assert (np.diff(edge[0]) < 0).any(), "columns are not shuffled"
    for g in (8, 16, 32, 64):
        rows = [r for r in PROJ_ROWS if r.graph == "tall%d" % g]
        assert len(rows) == 1 and key_parts(rows[0].key) == (4, g, 1) and rows[0].H == 1
        assert rows[0].D == (4 if g == 8 else 4 * (g // 2) + 4), "not the narrowest VEC 4 width of G = %d" % g
        ct, gpb = csr(rows[0].graph), 256 // g
        assert ct["N"] == 256 * gpb + gpb // 2 + 1 and ct["N"] > 256 * gpb and ct["N"] % gpb != 0
        assert bool((ct["deg"][256 * gpb:] > 0).all()) and abs(ct["E"] - 2 * ct["N"]) <= 2
        assert 4 * (2 * ct["N"] * rows[0].D * 3 + 3 * ct["N"] * rows[0].D) < 20 << 20
    assert csr("tiny")["N"] == 3 and csr("tiny")["E"] == 5 and csr("none")["E"] == 0
    assert {r.graph for r in PROJ_ROWS} == {"small", "tall8", "tall16", "tall32", "tall64", "tiny", "none"}


# ------------------------------------------------------------------------------------------------------------- the stand-in
WRONG_FWD = ("column D-1", "keep in Z", "alpha on positive", "elu always", "row tails", "a_2 of head 0")
WRONG_BWD = ("no g_Z", "second pass", "duplicates once")


class StandIn:
    """The two calls in float32 torch on the CPU.  `wrong` names one defect."""

    def __init__(self, wrong=None):
        self.wrong = wrong

    def _edges(self, case, h):
        c, inp = case.c, case.inp
        a = inp["a2"][0 if self.wrong == "a_2 of head 0" else h]
        m = (inp["P"][0, h][c["dst"]] + inp["P"][1, h][c["src"]]) + inp["Q"][h]
        return m, a

    def _w(self, case, sigma):
        al = torch.tensor(case.row.alpha, dtype=torch.float32)
        if self.wrong == "alpha on positive":
            return torch.exp(-torch.where(sigma > 0, al * sigma, sigma))
        return torch.exp(-torch.where(sigma > 0, sigma, al * sigma))

    def fwd(self, case, train):
        row, c, inp = case.row, case.c, case.inp
        N, E, D, H = c["N"], c["E"], row.D, row.H
        live = torch.ones(E)
        if self.wrong == "row tails":                                   # the last slot of every row whose length is no multiple of 4
            ends = c["rowptr"][1:][c["deg"] % 4 != 0] - 1
            live[ends] = 0
        out, sig, Zs = [], [], []
        for h in range(H):
            m, a = self._edges(case, h)
            sigma = m[:, :D - 1] @ a[:D - 1] if self.wrong == "column D-1" else m @ a
            w = self._w(case, sigma) * live
            keep = inp["keep"][h] if train else torch.ones(E)
            Z = _seg(c["dst"], w * keep if self.wrong == "keep in Z" else w, N)
            Z = torch.where(Z == 0, torch.tensor(1e-12), Z)
            hh = _seg(c["dst"], (keep * w)[:, None] * m, N) / Z[:, None]
            elu = row.concat or self.wrong == "elu always"
            out.append(torch.where(hh > 0, hh, torch.expm1(hh)) if elu else hh)
            sig.append(sigma)
            Zs.append(Z)
        res = dict(out=torch.cat(out, 1))
        if train:
            res.update(sigma=torch.stack(sig), Z=torch.stack(Zs))
        return res

    def bwd(self, case, out, sigma, Z):
        row, c, inp = case.row, case.c, case.inp
        N, E, D, H = c["N"], c["E"], row.D, row.H
        dst, src = c["dst"], c["src"]
        al = torch.tensor(row.alpha, dtype=torch.float32)
        once = torch.ones(E)
        if self.wrong == "duplicates once":                             # the source gather adds a repeated (destination, source) pair once
            seen = set()
            for k in c["slot_by_src"].tolist():
                pair = (int(dst[k]), int(src[k]))
                once[k] = 0.0 if pair in seen else 1.0
                seen.add(pair)
        Gms, gPd, gPs, ga2 = [], [], [], []
        for h in range(H):
            m, a = self._edges(case, h)
            y, gy = out[:, h * D:(h + 1) * D], inp["gout"][:, h * D:(h + 1) * D]
            if row.concat:
                e = y + 1
                gh = torch.where(y <= 0, gy * e, gy)
                hv = torch.where(y <= 0, torch.where(e > 0, torch.log1p(y), torch.zeros_like(y)), y)
            else:
                gh, hv = gy, y
            gU = gh / Z[h][:, None]
            gZ = -(gh * hv).sum(1) / Z[h]
            if self.wrong == "no g_Z":
                gZ = torch.zeros_like(gZ)
            t = (gU[dst] * m).sum(1)
            w = self._w(case, sigma[h])
            keep = inp["keep"][h]
            gs = -(keep * t + gZ[dst]) * w * torch.where(sigma[h] > 0, torch.tensor(1.0), al)
            Gm = (keep * w)[:, None] * gU[dst] + gs[:, None] * a[None, :]
            if self.wrong == "second pass":                             # the node loop stops after its first pass
                first = (dst < 256 * (256 // key_parts(row.key)[1])).float()
                Gm, gs = Gm * first[:, None], gs * first
            Gms.append(Gm)
            gPd.append(_seg(dst, Gm, N))
            gPs.append(_seg(src, Gm * once[:, None], N))
            ga2.append(gs @ m)
        return dict(Gm=torch.stack(Gms), gP=torch.stack([torch.stack(gPd), torch.stack(gPs)]), g_a_2=torch.stack(ga2))


def _fails(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except AssertionError:
        return True
    return False


def _applies(wrong, row):
    """Whether a defect changes what this row computes."""
    c = csr(row.graph)
    if c["E"] == 0:
        return False
    return {"elu always": not row.concat, "a_2 of head 0": row.H > 1, "second pass": row.graph.startswith("tall"),
            "duplicates once": row.graph in ("small", "tiny")}.get(wrong, True)


def _last_column_in_bands(case):
    """The largest |a_2[D - 1] m[k][D - 1]| over a row's edges and heads in units of that score's band: what "column D-1" changes."""
    c, inp, D = case.c, case.inp, case.row.D
    worst = 0.0
    for h in range(case.row.H if c["E"] else 0):
        m = (inp["P"][0, h][c["dst"], D - 1].double() + inp["P"][1, h][c["src"], D - 1].double()) + inp["Q"][h][:, D - 1].double()
        worst = max(worst, float((m.abs() * abs(float(inp["a2"][h, D - 1])) / case.band["sigma"][h]).max()))
    return worst


_SWEEP = {}


def _sweep():
    """Every row once: its input conditions, the stand-in's error / band per output, and which wrong restatements the harness failed."""
    if not _SWEEP:
        info, worst, caught = {}, {}, collections.defaultdict(dict)
        for r in PROJ_ROWS:
            case = make_case(r)
            info[r] = dict(case.info, last_column=_last_column_in_bands(case))
            for k, q in check_row(StandIn(), r).items():
                worst[k] = max(worst.get(k, (0.0, None)), (q, row_id(r)))
            for wrong in WRONG_FWD + WRONG_BWD:
                if _applies(wrong, r):
                    caught[wrong][r] = _fails(check_row, StandIn(wrong), r, repeat=False)
        _SWEEP.update(info=info, worst=worst, caught=caught)
    return _SWEEP


def test_inputs_keep_their_distance_from_the_kink_and_from_underflow():
    for r, info in _sweep()["info"].items():
        if csr(r.graph)["E"] == 0:
            continue
        assert info["margin"] >= 64.0, "%s: a score lies %.1f score bands from 0" % (row_id(r), info["margin"])
        assert 1e-30 <= info["w_min"] and info["w_max"] <= 1e30, (row_id(r), info["w_min"], info["w_max"])
        if r.graph == "small":
            assert info["w_min"] < 1e-24 and info["w_max"] > 1e12, (row_id(r), info["w_min"], info["w_max"])
        assert info["formula"] <= 1e-3, "%s: the backward the bands are built from is %.2e bands from autograd" % (row_id(r), info["formula"])


def test_float32_stand_in_passes_every_row_at_half_of_every_band():
    worst = _sweep()["worst"]
    print("PROJ_INST stand-in worst error / band: " + " ".join("%s=%.4f (%s)" % (k, q, rid) for k, (q, rid) in sorted(worst.items())))
    assert set(worst) == {"out", "sigma", "Z", "eval", "Gm", "gP", "g_a_2"}
    assert max(q for q, _ in worst.values()) <= 0.5, worst


def test_harness_fails_every_wrong_restatement():
    """Each defect on every row it changes.  One exception, by arithmetic and not by tuning: the score band is (D + 2) u sum |a_2| M, the
    width of a D-term float32 dot, and a single column's term a_2[D - 1] m[D - 1] is about 1 / D of that sum.  Below D ~ 1000 it is tens to
    thousands of bands; at D = 1900 the row's a_2[1899] happens to be small and the term is 0.4 bands on its largest edge: no float32 dot of
    that length can tell.  Its key (46408) is held by the D = 2048 and D = 1100 rows.  So "column D-1" must fail wherever the term is at
    least 1.5 bands on some edge, which is every row but that one."""
    sweep = _sweep()
    caught = sweep["caught"]
    for wrong in WRONG_FWD + WRONG_BWD:
        rows = caught[wrong]
        assert rows, wrong
        if wrong == "column D-1":
            rows = {r: hit for r, hit in rows.items() if sweep["info"][r]["last_column"] >= 1.5}
            assert len(rows) >= len(caught[wrong]) - 1 and {r.key for r in rows} == set(KEYS)
        missed = [row_id(r) for r, hit in rows.items() if not hit]
        assert not missed, "%s stays inside the bands on %s" % (wrong, missed)
    assert all(r.graph.startswith("tall") for r in caught["second pass"]) and len(caught["second pass"]) == 4
    assert {r.key for r in caught["a_2 of head 0"]} == set(KEYS) and {r.key for r in caught["elu always"]} == set(KEYS)
