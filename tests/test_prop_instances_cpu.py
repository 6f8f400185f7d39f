"""Coverage guard of tests/test_prop_instances_gpu.py (host only): every propagation kernel instance the launchers can select has a row of
PROP_ROWS, and every row selects the instances it names.  A new instance, or a change to the selection in csrc/prop.hip, prop_h.hip,
prop_hl.hip or prop_b16.hip, fails here until the table has a row for it.

The sweep asks recon_propagate_instance / recon_propagate_bwd_instance / recon_propagate_b16_instance through the table's own probe()
(the argument structures of recon_amd/propagation.py with placeholder addresses) over state sizes, channel counts, gather widths, hop
counts, both modes, both dtypes, both index kinds, aligned and offset adjacencies and every RECON_PROP_* setting the table uses.

bfloat16: the table's scope is the small fused kernel (family 11).  The wide fused kernel, the batched-GEMM forward and the backward
(families 12 - 14, k_bgemm_b16) have their shapes in tests/test_prop_b16_gpu.py; the sweep reports them and the guard does not ask for rows."""
import collections
import ctypes as C

import pytest
import torch

from test_prop_instances_gpu import (SCATTER_BWD, collides, collision_free, PROP_ROWS, FAMILY, row_id, probe, _probe, _r, make_inputs, key, H, HL, CHAIN8, CHAIN16, WAVE, BLOCK, HOP, GEMM, B16,
                                     B16_WIDE, B16_GEMM, B16_BWD, W_F, B_F)

# state sizes around every boundary of the selection: multiples of 16 (MFMA tiles, the f16 forms), of 32 (K steps), 96, 160 (the small forms' limit),
# 192 .. 512 in steps of 64 (the wide forms' K steps / row tiles), +- 4 around each, and the limits themselves
_S_EDGES = set(range(16, 513, 16)) | {96, 160} | set(range(192, 513, 64))
S_GRID = sorted(s for s in {b + d for b in _S_EDGES for d in (-4, -2, -1, 0, 1, 4)} | {4, 5, 6, 7, 8} if 4 <= s <= 512)
# channel counts around the channel tiles (16), the small forms' limit (96), the chunk sizes (64, 80, 128), the d A kernel's pass sizes (256, 512)
C_GRID = sorted(c for c in {b + d for b in list(range(16, 129, 16)) + [80, 96, 160, 256, 512, 1000] for d in (-1, 0, 1)} | {1, 2, 3, 7, 330, 700} if 1 <= c <= 1000)
SETTINGS = [(), W_F, B_F, (("RECON_PROP_FWD", "b"),), (("RECON_PROP_BWD", "f"),), (("RECON_PROP_BWD_WIDE", "0"),), (("RECON_PROP_BWD_CHAIN", "0"),),
            B_F + (("RECON_PROP_LDS_KB", "48"),), (("RECON_PROP_BWD", "f"), ("RECON_PROP_BWD_WIDE", "0"))]


def _points():
    """(dtype, mode, S, C, dd, L, idx, offset) of the sweep: the full S x C grid at dd = 16, L = 3 in both index kinds, the other gather widths
    and hop counts on every third channel count, offset adjacencies on the same; block mode n = 2 .. 32 for every hop count"""
    for dtype in ("fp32", "bf16"):
        for S in S_GRID:
            for i, Cn in enumerate(C_GRID):
                yield dtype, "dense", S, Cn, 16, 3, "rand", False
                if S % 16 == 0 and S > 160:
                    yield dtype, "dense", S, Cn, 16, 3, "blocks", False
                if i % 3 == 0:
                    for dd in (2, 8, 16):
                        for L in (1, 3, 8):
                            if (dd, L) != (16, 3):
                                yield dtype, "dense", S, Cn, dd, L, "rand", False
                    if dtype == "fp32":
                        yield dtype, "dense", S, Cn, 16, 3, "rand", True
        for n in range(2, 33):
            for L in (1, 3, 8):
                yield dtype, "blocks", 16 * n, n * (n - 1), 16, L, "blocks", False


def _sweep():
    """{(dtype, direction): {key: first point that returned it}}; direction "fwd" (training and no_grad forwards) or "bwd" """
    from recon_amd import _lib
    seen = collections.defaultdict(dict)
    pts = list(_points())
    for cfg in SETTINGS:
        with _lib.config(**dict(cfg)):
            for dtype, mode, S, Cn, dd, L, idx, offset in pts:
                if dtype == "bf16" and cfg:
                    continue                                            # the RECON_PROP_* switches of the table do not reach the bf16 kernels
                r = _r(0, 0, S, Cn, dd=dd, L=L, B=2, dtype=dtype, idx=idx, cfg=cfg, offset=offset, mode=mode)
                fwd, bwd, infer = _probe(r)
                for d, k in (("fwd", fwd), ("fwd", infer), ("bwd", bwd)):
                    if k > 0:
                        seen[(dtype, d)].setdefault(k, row_id(r))
    return seen


def test_every_row_selects_its_instances():
    ids = [row_id(r) for r in PROP_ROWS]
    assert len(ids) == len(set(ids)), "duplicate row ids"
    for r in PROP_ROWS:
        assert r.dtype in ("fp32", "bf16") and r.mode in ("dense", "blocks") and r.B >= 2
        assert probe(r) == (r.fwd, r.bwd, r.infer), row_id(r)


def test_scatter_backward_instances_all_get_a_bit_equality_pass():
    """check (b) of the GPU test compares every gradient bit for bit on the row's own indices or, where these collide, on collision-free ones:
    those must exist (2 dd <= S) for every row of the backward families that scatter with float atomics"""
    for r in PROP_ROWS:
        if r.dtype == "fp32" and r.bwd // 10000 in SCATTER_BWD:
            inp = make_inputs(r)
            if collides(inp["head"], inp["tail"]):
                assert not collides(*collision_free(r)), row_id(r)


def test_every_reachable_instance_has_a_row():
    seen = _sweep()
    count = {k: len(v) for k, v in seen.items()}
    # the sweep itself reaches what it did when it was written
    assert count[("fp32", "fwd")] >= N_FP32_FWD and count[("fp32", "bwd")] >= N_FP32_BWD, count
    assert count[("bf16", "fwd")] >= N_BF16_FWD and count[("bf16", "bwd")] >= 2, count
    for (dtype, d), keys in sorted(seen.items()):
        have = {k for r in PROP_ROWS if r.dtype == dtype for k in ((r.fwd, r.infer) if d == "fwd" else (r.bwd,))}
        want = {k for k in keys if dtype == "fp32" or k // 10000 == B16}
        missing = sorted(want - have)
        assert not missing, "%s %s instances without a row in PROP_ROWS: %s" % (dtype, d, ["%d (%s, e.g. %s)" % (k, FAMILY[k // 10000], keys[k]) for k in missing])
    rows = [r for r in PROP_ROWS if r.dtype == "fp32"]
    # what a key does not say: the d A kernel in two passes (C > 512), the per-hop backward above 64 KiB of LDS, a lowered LDS budget that
    # changes the chunk count, adjacencies at a 4-byte offset, a shared h0 per family
    assert any(r.bwd // 10000 == CHAIN16 and r.C > 512 for r in rows)
    assert any(r.bwd // 10000 == HOP and r.S > 160 for r in rows)
    assert any(dict(r.cfg).get("RECON_PROP_LDS_KB") for r in rows)
    assert any(r.offset and r.fwd // 10000 == WAVE for r in rows) and any(r.offset and r.fwd // 10000 == BLOCK for r in rows)
    for fam in (H, HL, CHAIN8, CHAIN16, WAVE, BLOCK, HOP, GEMM):
        assert any(r.shared for r in rows if fam in (r.fwd // 10000, r.bwd // 10000)), "no row with a shared h0 in family " + FAMILY[fam]
        assert any(r.act == "relu" for r in rows if fam in (r.fwd // 10000, r.bwd // 10000)), "no ReLU row in family " + FAMILY[fam]
    # tails: S % 32 == 16 and C % 16 != 0 for every dense two-term instance
    for nks in range(1, 6):
        for ntc in range(1, 7):
            assert any(r.fwd == key(H, nks, ntc) and r.S % 32 == 16 and r.C % 16 for r in PROP_ROWS if r.dtype == "fp32"), (nks, ntc)
            assert any(r.fwd == key(B16, nks, ntc) and r.S % 32 == 16 and r.C % 16 for r in PROP_ROWS if r.dtype == "bf16"), (nks, ntc)


# keys the sweep returned when it was written: fp32 forward 30 + 7 (h dense / block) + 6 + 6 (hl dense / block) + 18 (wave) + 10 (block);
# fp32 backward 30 + 6 (h) + 12 + 6 (chain dense / block) + 10 (bwd_hop) + 1 (GEMMs); bf16 forward 30 + 7 fused + 12 wide + 2 GEMM
N_FP32_FWD, N_FP32_BWD, N_BF16_FWD = 77, 65, 51


def test_instance_query_refuses_what_the_launchers_refuse():
    from recon_amd import _lib
    L = _lib.lib()
    assert probe(_r(None, None, 64, 20, L=9))[0] == -1                                      # more than kMaxHops hops
    assert probe(_r(None, None, 64, 20, L=8))[0] == key(H, 2, 2)
    assert probe(_r(None, None, 528, 20, L=2))[0] == key(BLOCK, 2, 0, 1)                    # S > 512: no f16 form, the fp32 form answers
    with _lib.config(RECON_PROP_FWD="h"):
        assert probe(_r(None, None, 528, 20, L=2))[0] == key(BLOCK, 2, 0, 1)
    assert probe(_r(None, None, 2000, 20, L=2))[0] == -1                                    # 16 channels of S = 2000 do not fit the LDS
    # block mode: C != n (n - 1), and wide states without the split workspace (no fp32 form reads the transition tensors)
    one = (C.c_void_p * 2)(1 << 20, 1 << 20)
    for S, Cn, ws, want in ((64, 12, None, key(H, 2, 1, 1)), (64, 11, None, -1), (192, 132, None, -1), (192, 132, 1 << 20, key(HL, 6, 2, 1)), (72, 12, None, -1)):
        a = _lib.PropArgs(2, Cn, S, 2, 16, 2, None, 1 << 20, 0, 1 << 20, 1 << 20, 0, 1 << 20, None, one, 1 << 20, None, None, 0)
        if ws:
            a.split_ws, a.split_ws_bytes = ws, L.recon_propagate_ws_bytes(C.byref(a))
        assert L.recon_propagate_instance(C.byref(a)) == want, (S, Cn)
    a = _lib.PropArgs(2, 12, 64, 2, 16, 2, one, None, 0, 1 << 20, 1 << 20, 0, 1 << 20, None, None, None, None, None, 0)
    assert L.recon_propagate_instance(C.byref(a)) == -1 and L.recon_propagate_instance(None) == -1      # no h0; no arguments
    a.h0, a.B = 1 << 20, 0
    assert L.recon_propagate_instance(C.byref(a)) == 0                                       # no graphs: nothing is launched
    b = _lib.PropBwdArgs(a, None, None, None, None, None, None, None, None, None, None)
    assert L.recon_propagate_bwd_instance(C.byref(b)) == -1 and L.recon_propagate_bwd_instance(None) == -1
    q = _lib.PropB16Args(2, 12, 68, 2, 16, 2, one, 1 << 20, 0, 1 << 20, 1 << 20, 0, 1 << 20, None, None, None, 1 << 20)
    assert L.recon_propagate_b16_instance(C.byref(q), 0) == -1 and L.recon_propagate_b16_instance(C.byref(q), 1) == -1   # S % 8 != 0
    q.S = 64
    assert L.recon_propagate_b16_instance(C.byref(q), 0) == key(B16, 2, 1) and L.recon_propagate_b16_instance(C.byref(q), 1) == -1   # no saved states
    q.h_saved = 1 << 20
    assert L.recon_propagate_b16_instance(C.byref(q), 1) == key(B16_BWD, 0)


RELU_ROWS = [r for r in PROP_ROWS if r.act == "relu" and r.dtype == "fp32"]


@pytest.mark.parametrize("row", RELU_ROWS, ids=[row_id(r) for r in RELU_ROWS])
def test_relu_rows_keep_every_preactivation_outside_its_band(row):
    """A ReLU row is comparable with the float64 oracle element by element only if no pre-activation is so close to zero that the kernels'
    rounding can put it on the other side.  The forward's products are two-term f16 (or fp32) sums held elementwise to 2^-20 (|A| . |H|)
    (tests/test_sgemm_hx2.py, test_sgemm_bx3.py), and an error of the previous state passes through |A_l| (the activations are 1-Lipschitz):
        band_l = 2^-20 (|A_l| . |H_l-1|) + |A_l| . band_l-1,   band_0 = 0.
    The row's seed is chosen (searched on the host) so that |Z_l| > band_l everywhere; the GPU test then skips nothing."""
    from oracle import recon_oracle as O
    r = row
    assert r.B <= 3 and r.B * r.C * r.S <= 100000, "ReLU rows stay small: B <= 3, below 10^5 states (C > 256 at S > 160, two graphs: 9 x 10^4)"
    inp = make_inputs(r)
    if r.mode == "blocks":
        adjs = [O.build_block_adjacency(t.double(), inp["ident"].double(), r.S // 16) for t in inp["Ts"]]
    else:
        adjs = [a.double() for a in inp["adjs"]]
    h = inp["h0"].double().squeeze(-1)
    Hm = (h if h.dim() == 3 else h[None].expand(r.B, -1, -1)).transpose(1, 2)            # [B, S, C]
    band = torch.zeros_like(Hm)
    worst = float("inf")
    for A in adjs:
        Z = torch.bmm(A, Hm)
        band = 2.0 ** -20 * torch.bmm(A.abs(), Hm.abs()) + torch.bmm(A.abs(), band)
        margin = (Z.abs() - band)
        worst = min(worst, float((Z.abs() / band.clamp_min(1e-300)).min()))
        assert bool((margin > 0).all()), "%s: %d pre-activations within their band of zero (closest |Z| / band = %.3f): pick another seed" % (
            row_id(r), int((margin <= 0).sum()), worst)
        Hm = torch.relu(Z)
