"""Coverage guard of tests/test_atp_instances_gpu.py (host only): every edge-pass kernel instance the dispatcher can select has a row
of ATP_ROWS, and every row selects the instance it names.  A new instance or a change to atp_shape (csrc/gat_atp.hip) fails here until
the table has a row for it."""
import collections

from test_atp_instances_gpu import ATP_ROWS, row_id

# widths that cross every register-row boundary of both load widths (vec 4: 256 / 512 / 1024 / 2048 columns, vec 2: 128 / 256 / 512 /
# 1024), on both sides of it and at both residues mod 4, plus a coarse sweep of the rest
_EDGES = sorted({b + d for b in (128, 256, 512, 1024, 2048) for d in (-6, -4, -2, 0, 2, 4, 6)} | set(range(2, 17, 2)))
WIDTHS = sorted(w for w in set(_EDGES) | set(range(2, 2049, 26)) | set(range(4, 2049, 60)) if 2 <= w <= 2048)
HEADS = range(1, 33)
D = 16                                        # a multiple of 8: the bf16-I/O query depends on D only through D % 8


def _sweep():
    """{key: [(F, R, H), ...]} over the grid where recon_gat_atp_supported says 1, and the same for recon_gat_atp_bf16_io_supported"""
    from recon_amd import _lib
    L = _lib.lib()
    fp32, bf16 = collections.defaultdict(list), collections.defaultdict(list)
    for F in WIDTHS:
        for R in WIDTHS:
            for H in HEADS:
                key = L.recon_gat_atp_instance(F, R, H)
                if key < 0 or L.recon_gat_atp_supported(100, 1000, F, R, D, H) != 1:
                    continue
                fp32[key].append((F, R, H))
                if L.recon_gat_atp_bf16_io_supported(F, R, D, H) == 1:
                    bf16[key].append((F, R, H))
    return fp32, bf16


def test_instance_query_refuses_what_atp_shape_refuses():
    from recon_amd import _lib
    L = _lib.lib()
    assert L.recon_gat_atp_instance(0, 8, 1) == -1 and L.recon_gat_atp_instance(8, 8, 0) == -1
    assert L.recon_gat_atp_instance(3, 8, 1) == -1                        # odd width: no load width
    assert L.recon_gat_atp_instance(8, 2052, 1) == -1                     # more than 8 register rows
    assert L.recon_gat_atp_instance(2, 1026, 1) == -1
    assert L.recon_gat_atp_instance(200, 200, 8) == 4013 and L.recon_gat_atp_instance(50, 50, 2) == 2011


def test_every_row_selects_its_instance():
    from recon_amd import _lib
    L = _lib.lib()
    ids = [row_id(r) for r in ATP_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    for r in ATP_ROWS:
        assert r.dtype in ("fp32", "bf16")
        assert L.recon_gat_atp_instance(r.F, r.R, r.H) == r.key, row_id(r)
        assert L.recon_gat_atp_supported(200, 2000, r.F, r.R, r.D, r.H) == 1, row_id(r)
        if r.dtype == "bf16":
            assert r.D % 8 == 0 and L.recon_gat_atp_bf16_io_supported(r.F, r.R, r.D, r.H) == 1, row_id(r)
        assert r.ee_grad or r.dtype == "bf16"


def test_every_reachable_instance_has_a_row():
    fp32, bf16 = _sweep()
    assert len(fp32) >= 23 and len(bf16) >= 10                           # the sweep itself reaches what it did when it was written
    have32 = {r.key for r in ATP_ROWS if r.dtype == "fp32"}
    have16 = {r.key for r in ATP_ROWS if r.dtype == "bf16"}
    missing = sorted(set(fp32) - have32)
    assert not missing, "fp32 instances without a row in ATP_ROWS: %s (e.g. F, R, H = %s)" % (missing, [fp32[k][0] for k in missing])
    missing = sorted(set(bf16) - have16)
    assert not missing, "bf16-I/O instances without a row in ATP_ROWS: %s (e.g. F, R, H = %s)" % (missing, [bf16[k][0] for k in missing])
    # a partial and an exact head group for every instance of several heads per wave, wherever the sweep reaches one
    for key, pts in sorted(fp32.items()):
        ht = 1 << (key % 10)
        if ht == 1:
            continue
        rows = [r for r in ATP_ROWS if r.dtype == "fp32" and r.key == key]
        if any(H % ht for _, _, H in pts):
            assert any(r.H % ht for r in rows), "k%d: no row with a partial head group (H %% %d != 0)" % (key, ht)
        if any(H % ht == 0 for _, _, H in pts):
            assert any(r.H % ht == 0 for r in rows), "k%d: no row with whole head groups" % key
    # the last register row partly filled (kr = 4 / 8 also stand for 3 / 5 ... 7 rows: widths just above the previous boundary leave it empty)
    for key in sorted(fp32):
        vec, kr = key // 1000, key // 10 % 100
        if kr > 1:
            assert any((kr - 1) * 64 * vec < max(r.F, r.R) < kr * 64 * vec for r in ATP_ROWS if r.dtype == "fp32" and r.key == key), \
                "k%d: no row whose widest input ends inside the last register row" % key
    # vec 2 with the f16 x 2 planes of odd-quad widths ((2F + R) % 8 == 0 but F or R not a multiple of 8: planes = 1)
    assert any(r.key < 3000 and r.dtype == "fp32" and (2 * r.F + r.R) % 8 == 0 and r.D % 8 == 0 for r in ATP_ROWS)
    # both K2' ring instances of the bf16 rows at kr = 1: with the bf16 g_edge_embed store and without it
    assert {r.ee_grad for r in ATP_ROWS if r.dtype == "bf16" and r.key // 10 == 401} == {True, False}


def test_switch_dependent_answers_are_not_kept_across_a_switch():
    """gat_layers caches whether the backward may store bf16 g_edge_embed; the library says no once RECON_K2_LDS_RING=0 (that store is an
    instance of the ring kernel only).  A stale yes made every later bf16 backward of the shape fail with RECON_ERR_UNSUPPORTED."""
    from recon_amd import _lib, gat_layers
    shape = (200, 200, 32, 8)
    before = gat_layers._gee_bf16_ok(*shape)
    with _lib.config(RECON_K2_LDS_RING="0"):
        assert not gat_layers._gee_bf16_ok(*shape)
    assert gat_layers._gee_bf16_ok(*shape) == before
