"""Host side of tests/test_atp_tail_ride_gpu.py (no GPU): recon_gat_atp_bwd_ride_plan — the slices and reduce blocks of the three skinny
products, the weight gradient's splits and tile workgroups and the grid layers its rider adds — against
the same arithmetic written out in Python, at that file's shapes and at the benchmark's."""
import ctypes

from test_atp_tail_ride_gpu import CASES, SPLITS, edges_of, plan_of

BM, BN, BK = 128, 208, 32                    # the k-major product's tile (csrc/gemm_tile16.h)
SLICES = 1024                                # kSkinnySlices (csrc/gat_atp.hip)


def cdiv(a, b):
    return -(-a // b)


def model(NR, N, E, F, R, D, H):
    W = 2 * F + R
    rows, K = (NR, N, E), (F, F, R)
    slices = [cdiv(r, max(32, cdiv(r, SLICES))) if r > 0 else 0 for r in rows]
    blocks = [cdiv(H * k, 16) if r > 0 else 0 for r, k in zip(rows, K)]
    tiles_xy = cdiv(W, BM) * cdiv(D, BN)
    tiles = tiles_xy * H
    max_s = min(64, max(1, NR // (4 * BK)))
    if tiles >= 256:
        best, best_score = 1, -1.0
        for s in range(1, min(max_s, 8) + 1):
            wg = tiles * s
            score = wg / (cdiv(wg, 512) * 512) - 0.01 * (s - 1)
            if score > best_score + 1e-9:
                best, best_score = s, score
        want = best
    else:
        want = max(1, min(512 // tiles, max_s))
    kps = cdiv(cdiv(max(NR, 1), want), BK) * BK                    # whole K tiles per split: fewer splits than asked for may come out
    sk = cdiv(max(NR, 1), kps)
    total = sum(blocks)
    return slices + blocks + [sk, tiles * sk, H * sk + (cdiv(total, tiles_xy) if total else 0), total]


def blocks_of(plan):
    """(job, first element) of every rider block in launch order: job after job, 16 elements a block (skinny_reduce_block)"""
    out = []
    for b in range(plan[9]):
        job = 0 if b < plan[3] else (1 if b < plan[3] + plan[4] else 2)
        out.append((job, 16 * (b - sum(plan[3:3 + job]))))
    return out


def test_plan_is_the_written_out_arithmetic():
    for name, (N, _, F, R, D, H, kind, rides) in CASES.items():
        E = edges_of(name).shape[1]
        for NR in (N, N // 2):
            says, plan = plan_of(name, NR)
            assert plan == model(NR, N, E, F, R, D, H), name
        says, plan = plan_of(name)
        if kind != "hub":
            assert says == (1 if rides else 0), name
        if name in SPLITS:
            assert plan[6] == SPLITS[name], name


def test_plan_at_the_benchmarked_shape():
    from recon_amd import _lib
    plan = (ctypes.c_int32 * 10)()
    # cfg 2: 512 graphs x 16 nodes x 64 edges, F = R = D = 200, 8 heads
    assert _lib.lib().recon_gat_atp_bwd_ride_plan(8192, 8192, 32768, 200, 200, 200, 8, plan) == 1
    assert list(plan) == model(8192, 8192, 32768, 200, 200, 200, 8)
    assert list(plan) == [256, 256, 1024, 100, 100, 100, 12, 480, 96 + 60, 300]


def test_every_element_has_one_rider_block_and_every_block_a_grid_slot():
    for name, (N, _, F, R, D, H, _, _) in CASES.items():
        _, plan = plan_of(name)
        K = (F, F, R)
        seen = [set(), set(), set()]
        for job, first in blocks_of(plan):
            assert first < H * K[job], "%s: a block without elements" % name
            assert first not in seen[job]
            seen[job].add(first)
        for job in range(3):
            want = set(range(0, H * K[job], 16)) if plan[job] else set()
            assert seen[job] == want, "%s: job %d" % (name, job)
        tiles_xy = cdiv(2 * F + R, BM) * cdiv(D, BN)
        tile_layers = plan[7] // tiles_xy
        assert plan[7] == tile_layers * tiles_xy and plan[8] >= tile_layers
        room = (plan[8] - tile_layers) * tiles_xy
        assert room >= plan[9] > room - tiles_xy or (plan[9] == 0 and room == 0), name


def test_plan_refuses_nonsense():
    from recon_amd import _lib
    L = _lib.lib()
    plan = (ctypes.c_int32 * 10)()
    assert L.recon_gat_atp_bwd_ride_plan(8, 8, 8, 8, 8, 8, 8, None) == 0
    assert L.recon_gat_atp_bwd_ride_plan(8, 0, 8, 8, 8, 8, 8, plan) == 0
    assert L.recon_gat_atp_bwd_ride_plan(64, 64, 64, 8, 8, 8, 9, plan) == 0           # more than 8 heads
    assert L.recon_gat_atp_bwd_ride_plan(64, 64, 64, 8, 8, 264, 8, plan) == 0         # heads wider than 256 columns: no per-row scales
