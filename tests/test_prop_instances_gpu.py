"""Every kernel instance of the GP-GNN propagation (csrc/prop.hip, prop_h.hip, prop_hl.hip, prop_b16.hip) against the float64 oracle.

The launchers pick a template instance from the shape, the pointers' alignment and the RECON_PROP_* switches; recon_propagate_instance /
recon_propagate_bwd_instance / recon_propagate_b16_instance return the key of that choice (include/recon_hip.h: family * 10000 + p1 * 100 +
p2 * 10 + flag), computed by the code the launchers switch on.  Each instance has its own tails, pitches and register layout, so each gets
a row of PROP_ROWS at a shape that selects it; tests/test_prop_instances_cpu.py fails when a reachable key has no row.

A row names the key of its training forward, of its backward and (where it differs) of its forward under no_grad.  The test asserts that
the query answers exactly these for the arguments propagation.py builds (probe(): the same structures with placeholder addresses of the
tensors' alignment, before anything runs; propagation.trace_instances(): the query on the very arguments of each launch), then checks
  (a) the output and every gradient against oracle.recon_oracle in float64 on the float32 inputs,
  (b) a second identical call bit for bit (gradients that pass through colliding float atomics: see SCATTER_BWD),
  (c) the no_grad call bit for bit against the training forward where one instance serves both,
  (d) bfloat16 rows as tests/test_prop_b16_gpu.py::_check_b16 does (the oracle rounding its states hop by hop).
Dense rows go through propagate() on arbitrary adjacencies with per-row and per-column factors, one row of A three orders of magnitude
below the rest, gather indices with duplicates ("rand") or GP-GNN's blocks of 16 columns ("blocks": what the wide backward's chain form
needs), B >= 2 graphs, one channel without output gradient; block-mode rows go through propagate_blocks().

Instance rows use tanh or linear: smooth, so two-term rounding cannot flip a mask against float64.  The ReLU rows (a few per family) are
bound by tests/test_prop_instances_cpu.py::test_relu_rows_keep_every_preactivation_outside_its_band: their seeds are chosen so that no
pre-activation lies within the forward's error band of zero, hence no element is skipped here either.

Bars: float32 output 1e-4 + 1e-5 max|ref|, gradients 1e-5 + 1e-4 max|ref| (tests/test_prop_gpu.py's wide-state tests); bfloat16 rows
_check_b16's defaults."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import recon_oracle as O

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

Row = collections.namedtuple("Row", "fwd bwd mode S C dd L B act dtype shared idx cfg offset infer seed note")


def key(fam, p1, p2=0, flag=0):
    """include/recon_hip.h: recon_propagate_instance"""
    return fam * 10000 + p1 * 100 + p2 * 10 + int(flag)


H, HL, CHAIN8, CHAIN16, WAVE, BLOCK, HOP, GEMM, B16, B16_WIDE, B16_GEMM, B16_BWD = 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14
FAMILY = {H: "h", HL: "hl", CHAIN8: "hl-chain+gadj8", CHAIN16: "hl-chain+gadj16", WAVE: "wave", BLOCK: "block", HOP: "bwd_hop", GEMM: "bwd-gemm",
          B16: "b16-fused", B16_WIDE: "b16-wide", B16_GEMM: "b16-gemm", B16_BWD: "b16-bwd"}
W_F = (("RECON_PROP_FWD", "w"), ("RECON_PROP_BWD", "f"))      # fp32 MFMA forms: per-wave forward, per-hop backward
B_F = (("RECON_PROP_FWD", "b"), ("RECON_PROP_BWD", "f"))      # per-workgroup forward, per-hop backward


def _r(fwd, bwd, S, C, dd=16, L=2, B=2, act="tanh", dtype="fp32", shared=False, idx="rand", cfg=(), offset=False, infer=None, seed=1, note="", mode="dense"):
    return Row(fwd, bwd, mode, S, C, dd, L, B, act, dtype, shared, idx, tuple(cfg), offset, fwd if infer is None else infer, seed, note)


def _blocks(fwd, bwd, n, **kw):
    kw.setdefault("idx", "blocks")
    return _r(fwd, bwd, 16 * n, n * (n - 1), mode="blocks", **kw)


# (NKS, NTC) of the two-term f16 kernels in block mode, per n (csrc/prop_h.hip: h_key)
_BLK_KN = {2: (1, 1), 3: (2, 1), 4: (2, 1), 5: (3, 2), 6: (3, 2), 7: (4, 3), 8: (4, 4), 9: (5, 5), 10: (5, 6)}
_DD = (2, 6, 8, 16, 20, 4)


def _dd(i, S):
    """gather width number i, not above S / 2: a channel's 2 dd gather indices can then be chosen without a collision (check (b))"""
    return _DD[i % 6] if 2 * _DD[i % 6] <= S else max(d for d in _DD if 2 * d <= S)


PROP_ROWS = []

# ---- k_propagate_fwd_h / k_propagate_bwd_h <NKS, NTC, false>: S ends half way into the last K step (S % 32 == 16), C inside the last
#      channel tile; the diagonal again with whole tiles
for nks in range(1, 6):
    for ntc in range(1, 7):
        PROP_ROWS.append(_r(key(H, nks, ntc), key(H, nks, ntc), 32 * nks - 16, 16 * ntc - 1 - (3 * nks + ntc) % 13, dd=_dd(nks + ntc, 32 * nks - 16), L=1 + (nks + ntc) % 3,
                            B=2 + (nks * ntc) % 2, act=("tanh", "linear")[(nks + ntc) % 2], shared=(nks == ntc), seed=100 * nks + ntc,
                            note="S %% 32 == 16, C %% 16 == %d" % ((16 * ntc - 1 - (3 * nks + ntc) % 13) % 16)))
    PROP_ROWS.append(_r(key(H, nks, nks), key(H, nks, nks), 32 * nks, 16 * nks, dd=16, L=2, B=3, seed=150 + nks, note="whole tiles both ways"))
PROP_ROWS += [
    _r(key(H, 5, 6), key(HOP, 5, 0, 1), 160, 96, dd=16, L=2, B=2, idx="blocks", seed=7, note="the largest fused shape: the backward's LDS image does not fit, per-hop fp32 backward"),
    _r(key(H, 3, 2), key(H, 3, 2), 80, 20, dd=8, L=8, B=2, seed=8, note="eight hops: the state images swap roles four times"),
    _r(key(H, 2, 3), key(H, 2, 3), 48, 40, dd=6, L=3, B=3, act="relu", seed=1, note="ReLU"),
    _r(key(H, 5, 5), key(H, 5, 5), 144, 72, dd=16, L=2, B=2, act="relu", idx="blocks", seed=1,
       note="ReLU at model_params.json sizes, GP-GNN's indices (two hops: no seed below 60 keeps a third hop's 20 736 pre-activations outside their bands)"),
]
# ---- the same kernels in block mode (propagate_blocks): one instance per n (n = 3 / 4 and 5 / 6 share one)
for n, (nks, ntc) in sorted(_BLK_KN.items()):
    if n < 10:
        PROP_ROWS.append(_blocks(key(H, nks, ntc, 1), key(H, nks, ntc, 1), n, L=1 + n % 3, B=2 + n % 2, act=("tanh", "linear")[n % 2], shared=(n == 4), seed=200 + n,
                                 note="block mode n = %d" % n))
PROP_ROWS += [
    _blocks(key(H, 5, 6), key(HOP, 5, 0, 1), 10, infer=key(H, 5, 6, 1), L=2, B=2, seed=210,
            note="n = 10: inference in block mode, training through the materialised adjacency (no backward instance in block mode)"),
    _blocks(key(H, 3, 2, 1), key(H, 3, 2, 1), 6, L=3, B=3, act="relu", seed=7, note="ReLU in block mode"),
]
# ---- fp32 MFMA forms (RECON_PROP_FWD = w | b, RECON_PROP_BWD = f): k_propagate_fwd_w <NTn, V4>, k_propagate_fwd <MT, V4>,
#      k_propagate_bwd_hop <MT, V4>.  V4: S % 4 == 0 and 16-byte aligned adjacencies (forward) / states (backward)
for ntn in range(1, 10):
    mt = 1 + (ntn - 1) % 5
    PROP_ROWS.append(_r(key(WAVE, ntn, 0, 1), key(HOP, mt, 0, 1), 16 * ntn - 4, 16 * mt - 3, dd=_dd(ntn, 16 * ntn - 4), L=1 + ntn % 3, B=2 + ntn % 2, cfg=W_F,
                        act=("tanh", "linear")[ntn % 2], shared=(ntn == 3), seed=300 + ntn, note="float4 loads, S ends inside the last tile"))
    PROP_ROWS.append(_r(key(WAVE, ntn, 0, 0), key(HOP, mt, 0, 0), 16 * ntn - 2 - ntn % 2, 16 * mt - 7, dd=_dd(ntn + 1, 16 * ntn - 3), L=1 + (ntn + 1) % 3, B=2, cfg=W_F,
                        seed=320 + ntn, note="S %% 4 != 0: scalar loads"))
for mt in range(1, 6):
    PROP_ROWS.append(_r(key(BLOCK, mt, 0, 1), key(HOP, mt, 0, 1), (36, 100, 64, 148, 120)[mt - 1], 16 * mt - 5, dd=_dd(mt, 36), L=2 + mt % 2, B=2 + mt % 2, cfg=B_F,
                        act=("tanh", "linear")[mt % 2], shared=(mt == 2), seed=340 + mt, note="state in LDS per workgroup, float4 loads"))
    PROP_ROWS.append(_r(key(BLOCK, mt, 0, 0), key(HOP, mt, 0, 0), (30, 70, 141, 19, 98)[mt - 1], 16 * mt - 9, dd=_dd(mt + 1, 19), L=1 + mt % 3, B=2, cfg=B_F,
                        seed=350 + mt, note="S %% 4 != 0"))
PROP_ROWS += [
    _r(key(WAVE, 4, 0, 0), key(HOP, 2, 0, 1), 64, 30, dd=8, L=2, B=2, offset=True, seed=361,
       note="adjacencies at a 4-byte offset, no switch: the f16 forms decline, scalar loads at S % 4 == 0; the states stay aligned"),
    _r(key(BLOCK, 3, 0, 0), key(HOP, 3, 0, 1), 148, 44, dd=6, L=2, B=2, offset=True, cfg=(("RECON_PROP_FWD", "b"),), seed=362,
       note="adjacencies at a 4-byte offset, state in LDS"),
    # two channel chunks: their d A contributions meet in float atomics, and a sum of two terms does not depend on their order (check (b))
    _r(key(BLOCK, 5, 0, 1), key(HOP, 5, 0, 1), 96, 150, dd=8, L=2, B=2, cfg=B_F, seed=363, note="C = 150: two channel chunks, the second of 70 channels"),
    _r(key(BLOCK, 2, 0, 1), key(HOP, 2, 0, 1), 144, 60, dd=16, L=2, B=2, cfg=B_F + (("RECON_PROP_LDS_KB", "48"),), seed=364,
       note="RECON_PROP_LDS_KB lowered: two chunks of 32 channels instead of one of 64"),
    _r(key(WAVE, 3, 0, 1), key(HOP, 2, 0, 1), 48, 24, dd=6, L=3, B=3, act="relu", cfg=W_F, seed=2, note="ReLU, per wave"),
    _r(key(BLOCK, 2, 0, 1), key(HOP, 2, 0, 1), 40, 30, dd=8, L=2, B=2, act="relu", cfg=B_F, seed=4, note="ReLU, per workgroup"),
]
# ---- wide states (160 < S <= 512): k_propagate_fwd_hl <RT, NKS>; backward by the gather indices: blocks of 16 columns -> the chain form
#      k_propagate_fwd_hl <.., true> + k_prop_gadj_hl <RT, 8 | 16> (8: C <= 256), arbitrary indices -> batched fp32 GEMMs
for nks, rt, S in ((6, 2, 176), (8, 2, 240), (10, 3, 304), (12, 3, 368), (14, 4, 432), (16, 4, 496)):
    c8, c16 = (40, 300) if nks % 4 == 2 else (130, 270)
    PROP_ROWS.append(_r(key(HL, nks, rt), key(CHAIN8, nks, rt), S, c8, L=2 + nks % 3 % 2, B=2 + (nks == 8), idx="blocks", shared=(nks == 10), seed=400 + nks,
                        act=("tanh", "linear")[nks // 2 % 2], note="chain form, d A in one pass of 8 K steps; S %% 32 == 16"))
    PROP_ROWS.append(_r(key(HL, nks, rt), key(CHAIN16, nks, rt), S, c16, L=2, B=2, idx="blocks", seed=420 + nks, note="chain form, d A in 16 K steps per pass"))
PROP_ROWS += [
    _r(key(HL, 16, 4), key(CHAIN16, 16, 4), 512, 530, L=2, B=2, idx="blocks", seed=440, note="C > 512: d A in two passes, RT = 4"),
    _r(key(HL, 12, 3), key(GEMM, 0), 340, 50, dd=8, L=2, B=2, seed=441, note="S % 16 != 0, arbitrary indices: batched-GEMM backward"),
    _r(key(HL, 6, 2), key(GEMM, 0), 164, 3, dd=2, L=3, B=3, shared=True, seed=442, note="a partial row tile and a partial K step; shared h0"),
    _r(key(HL, 8, 2), key(GEMM, 0), 240, 70, L=2, B=2, idx="blocks", cfg=(("RECON_PROP_BWD_CHAIN", "0"),), seed=443, note="RECON_PROP_BWD_CHAIN=0: batched GEMMs at a chain shape"),
    _r(key(HL, 8, 2), key(HOP, 4, 0, 1), 256, 70, L=2, B=2, idx="blocks", cfg=(("RECON_PROP_BWD_WIDE", "0"),), seed=444,
       note="RECON_PROP_BWD_WIDE=0: per-hop kernel at a wide shape, two 64-channel chunks, 130 KiB of LDS"),
    _r(key(BLOCK, 4, 0, 1), key(GEMM, 0), 272, 60, dd=8, L=2, B=2, cfg=B_F, seed=445, note="RECON_PROP_FWD=b at S > 256: two state buffers, several passes per hop"),
    _r(key(HL, 10, 3), key(CHAIN8, 10, 3), 320, 80, L=2, B=2, act="relu", idx="blocks", seed=19, note="ReLU, chain form"),
    _r(key(HL, 6, 2), key(GEMM, 0), 192, 20, dd=4, L=2, B=2, act="relu", seed=5, note="ReLU, batched-GEMM backward"),
    _r(key(HL, 6, 2), key(CHAIN16, 6, 2), 176, 260, L=1, B=2, act="relu", idx="blocks", seed=1,
       note="ReLU, chain form with d A in 16 K steps (one hop: no seed below 40 keeps a second hop's 91 520 pre-activations outside their bands)"),
]
# ---- wide states in block mode (propagate_blocks, 10 < n <= 32)
for n, nks, rt, fam in ((12, 6, 2, CHAIN8), (16, 8, 2, CHAIN8), (20, 10, 3, CHAIN16), (24, 12, 3, CHAIN16), (28, 14, 4, CHAIN16), (32, 16, 4, CHAIN16)):
    PROP_ROWS.append(_blocks(key(HL, nks, rt, 1), key(fam, nks, rt, 1), n, L=2, B=2, act=("tanh", "linear")[n // 4 % 2], shared=(n == 20), seed=500 + n,
                             note="block mode n = %d" % n))
PROP_ROWS.append(_blocks(key(HL, 6, 2, 1), key(CHAIN8, 6, 2, 1), 11, L=2, B=2, act="relu", seed=1, note="ReLU, wide block mode, partial last row tile"))
# ---- bfloat16 small fused kernel k_prop_b16_fwd <NKS, NTC, BLK> (the backward is the batched-GEMM form for every shape)
for nks in range(1, 6):
    for ntc in range(1, 7):
        PROP_ROWS.append(_r(key(B16, nks, ntc), key(B16_BWD, 0), 32 * nks - 16, 16 * ntc - 2 * ((nks + ntc) % 7) - 2, dd=(2, 6, 8, 16, 20, 4)[(nks + ntc) % 6],
                            L=1 + (nks + ntc) % 3, B=2 + (nks * ntc) % 2, act=("tanh", "linear", "relu")[(nks + ntc) % 3], dtype="bf16", shared=(nks == ntc),
                            seed=600 + 10 * nks + ntc, note="bf16, S %% 32 == 16"))
for n, (nks, ntc) in sorted(_BLK_KN.items()):
    PROP_ROWS.append(_blocks(key(B16, nks, ntc, 1), key(B16_BWD, 0, 0, 1), n, L=1 + n % 3, B=2 + n % 2, act=("tanh", "relu")[n % 2], dtype="bf16", seed=700 + n,
                             note="bf16 block mode n = %d" % n))


# Backward kernels that scatter the relation gradient d (h[head] h[tail]) with LDS float atomics, many waves per channel row (k_propagate_bwd_h:
# scatter_commit, k_propagate_bwd_hop): where two of a channel's 2 dd gather indices coincide, the additions meet in the hardware's order and
# d h0 / d A may differ in the last place from call to call.  Check (b) for a row of these families whose indices
# really collide (collides()): the output bit for bit and the gradients of both calls at the oracle's bar on the colliding indices, then the
# same tensors with collision-free indices (collision_free()) twice, every gradient bit for bit — so every instance of both kernels has a
# run-to-run check of all its gradients.  Rows without a collision are held to bit-equality as they are.
SCATTER_BWD = (H, HOP)


def collides(head, tail):
    """whether two of the 2 dd gather indices of some channel coincide"""
    both = torch.cat([head, tail], dim=-1).sort(dim=-1).values
    return bool((both[..., 1:] == both[..., :-1]).any())


def collision_free(r):
    """(head, tail) [C, dd] with 2 dd distinct columns per channel, from the row's seed"""
    assert 2 * r.dd <= r.S, "%s: 2 dd > S, no collision-free indices exist" % row_id(r)
    g = torch.Generator().manual_seed(r.seed + 9000)
    perm = torch.stack([torch.randperm(r.S, generator=g)[:2 * r.dd] for _ in range(r.C)])
    return perm[:, :r.dd].contiguous(), perm[:, r.dd:].contiguous()


def row_id(r):
    tag = "".join("-%s=%s" % (k.replace("RECON_PROP_", ""), v) for k, v in r.cfg)
    return "k%d-k%d-%s-S%dC%d-%s-%s%s%s" % (r.fwd, r.bwd, r.mode, r.S, r.C, r.act, r.dtype, tag, "-off4" if r.offset else "")


# ------------------------------------------------------------------------------- what propagation.py asks the library (host only)
_FAKE = 1 << 20                                   # a placeholder address, 16-byte aligned: the queries look at null-ness and alignment only


def _prop_args(r, blocks, need):
    """recon_prop_args as _Propagate.forward / _PropagateBlocks.forward fill it (propagation.py), with placeholder addresses"""
    from recon_amd import _lib
    L = _lib.lib()
    arr = (C.c_void_p * r.L)(*([_FAKE + (4 if r.offset and not blocks else 0)] * r.L))
    a = _lib.PropArgs(r.B, r.C, r.S, r.L, r.dd, _lib.ACT[r.act], None if blocks else arr, _FAKE, 0 if r.shared else r.C * r.S, _FAKE, _FAKE, 0, _FAKE,
                      _FAKE if need else None, arr if blocks else None, _FAKE if blocks else None, None, None, 0)
    nbytes = L.recon_propagate_ws_bytes(C.byref(a))
    if nbytes:
        a.split_ws, a.split_ws_bytes = _FAKE, nbytes
    if need and (r.S <= 160 if blocks else L.recon_propagate_form(C.byref(a)) & 1):
        a.stats = _FAKE
    return a, arr


def _blocks_fused(r, need_grad):
    """propagate_blocks(): whether the call runs in block mode (blocks_mode_available / _blocks_wide_trainable) or through the adjacency"""
    from recon_amd import _lib
    L = _lib.lib()
    n = r.S // 16
    if r.dd != 16 or n < 2 or n > 32:
        return False
    p = _lib.PropArgs(r.B, r.C, r.S, r.L, 16, 1, None, _FAKE, 0 if r.shared else r.C * r.S, None, None, 0, None, None, None, None, None, None, 0)
    if n <= 10:
        form = L.recon_propagate_form(C.byref(p))
        return form == 3 or (form == 1 and not need_grad)
    nbytes = L.recon_propagate_ws_bytes(C.byref(p))
    if not nbytes or not need_grad:
        return bool(nbytes)
    one = (C.c_void_p * 1)()
    q = _lib.PropArgs(r.B, r.C, r.S, r.L, 16, 1, None, _FAKE, 0 if r.shared else r.C * r.S, None, None, 0, None, None, one, 16, None, 1, nbytes)
    return r.idx == "blocks" and L.recon_propagate_bwd_chain_ws_floats(C.byref(q)) > 0


def probe(r):
    """(training forward key, backward key, no_grad forward key) of the row as recon_propagate_instance & co. answer for the arguments
    propagation.py passes under the row's switches — no device needed"""
    from recon_amd import _lib
    with _lib.config(**dict(r.cfg)):
        return _probe(r)


def _probe(r):
    from recon_amd import _lib
    L = _lib.lib()
    if r.dtype == "bf16":
        blocks = r.mode == "blocks"
        arr = (C.c_void_p * r.L)(*([_FAKE] * r.L))
        a = _lib.PropB16Args(r.B, r.C, r.S, r.L, r.dd, _lib.ACT[r.act], None if blocks else arr, _FAKE, 0 if r.shared else r.C * r.S, _FAKE, _FAKE, 0, _FAKE, None,
                             arr if blocks else None, _FAKE if blocks else None, _FAKE)
        infer = L.recon_propagate_b16_instance(C.byref(a), 0)
        a.h_saved = _FAKE
        return L.recon_propagate_b16_instance(C.byref(a), 0), L.recon_propagate_b16_instance(C.byref(a), 1), infer
    res = []
    for need in (True, False):
        blocks = r.mode == "blocks" and _blocks_fused(r, need)
        a, keep = _prop_args(r, blocks, need)
        res.append(L.recon_propagate_instance(C.byref(a)))
        if not need:
            break
        garr = (C.c_void_p * r.L)(*([_FAKE] * r.L))
        f, keep2 = _prop_args(r, blocks, True)
        f.split_ws, f.split_ws_bytes = None, 0
        if blocks:
            if r.S > 160:
                f.split_ws_bytes = L.recon_propagate_ws_bytes(C.byref(f))
                f.split_ws = _FAKE
                b = _lib.PropBwdArgs(f, _FAKE, None, _FAKE, garr, _FAKE, None, None, _FAKE, _FAKE, _FAKE)
            else:
                b = _lib.PropBwdArgs(f, _FAKE, None, _FAKE, garr, _FAKE, _FAKE, None)
        else:
            chain = wide = None
            if r.S > 160 and r.dd == 16 and not r.offset and r.idx == "blocks" and r.S % 16 == 0:
                nbytes = L.recon_propagate_ws_bytes(C.byref(f))
                if nbytes:
                    f.split_ws, f.split_ws_bytes = _FAKE, nbytes
                    chain = _FAKE if L.recon_propagate_bwd_chain_ws_floats(C.byref(f)) else None
            if chain is None and L.recon_propagate_bwd_ws_floats(C.byref(f)):
                wide = _FAKE
            b = _lib.PropBwdArgs(f, _FAKE, garr, _FAKE, None, None, None, wide, chain, chain, chain)
        res.append(L.recon_propagate_bwd_instance(C.byref(b)))
    return res[0], res[1], res[2]


# ------------------------------------------------------------------------------- inputs
def _scale(n, a, b, lo, hi):
    """n factors in [lo, hi] with period b: an element read in place of its neighbour, or twice, is far outside the bar"""
    return lo + (hi - lo) * torch.from_numpy(((np.arange(n) * a) % b) / float(b - 1)).float()


def make_inputs(r):
    """float32 CPU tensors of the row (bf16 rows: bf16 values): dense rows dict(adjs, h0, head, tail, Gr), block-mode rows dict(Ts, ident, ...)"""
    g = torch.Generator().manual_seed(r.seed)
    S, Cn, dd, L, B = r.S, r.C, r.dd, r.L, r.B
    inp = {}
    if r.mode == "blocks":
        n = S // 16
        from recon_amd.propagation import make_start_embedding
        Ts = [torch.relu(torch.randn(B, Cn, 256, generator=g)) * (0.6 / n) * _scale(256, 7, 13, 0.5, 1.5) for _ in range(L)]
        for t in Ts:
            t[:, ::5] *= 6.0                                           # blocks of very different magnitude
            t[:, :, 5 * 16:6 * 16] *= 1e-3                             # row 5 of every block three orders of magnitude below the rest
        inp["Ts"] = Ts
        inp["ident"] = torch.eye(16) + 0.02 * torch.randn(16, 16, generator=g)
        tmpl = torch.from_numpy(make_start_embedding(n, 8)).float()
        h0 = (torch.randn(Cn, S, 1, generator=g) if r.shared else torch.randn(B, Cn, S, 1, generator=g)) * tmpl
    else:
        adjs = []
        for l in range(L):
            a = (torch.rand(B, S, S, generator=g) - 0.45) * (2.0 / S ** 0.5) * (1.0 + 0.5 * l if L <= 3 else 1.0)
            a = a * _scale(S, 7, 13, 0.5, 1.5) * _scale(S, 5, 11, 0.6, 1.4)[:, None]      # every column and every row its own factor
            a[:, :, ::7] *= 4.0
            a[:, min(5, S - 1)] *= 1e-3                                # one row three orders of magnitude below the rest
            adjs.append(a.contiguous())
        inp["adjs"] = adjs
        h0 = (torch.randn(Cn, S, 1, generator=g) if r.shared else torch.randn(B, Cn, S, 1, generator=g)) * _scale(S, 3, 7, 0.5, 1.5)[:, None]
    if r.idx == "blocks":                                               # GP-GNN's: 16 consecutive columns from a multiple of 16, head != tail
        nb = S // 16
        if r.mode == "blocks":
            from recon_amd.propagation import get_head_indices, get_tail_indices
            head, tail = torch.from_numpy(get_head_indices(nb, 8, bs=1)[0]), torch.from_numpy(get_tail_indices(nb, 8, bs=1)[0])
        else:
            hb = torch.randint(0, nb, (Cn,), generator=g)
            tb = (hb + 1 + torch.randint(0, nb - 1, (Cn,), generator=g)) % nb
            head, tail = 16 * hb[:, None] + torch.arange(16), 16 * tb[:, None] + torch.arange(16)
    else:
        head, tail = torch.randint(0, S, (Cn, dd), generator=g), torch.randint(0, S, (Cn, dd), generator=g)
    Gr = torch.randn(B, Cn, dd * L, generator=g) * _scale(dd * L, 3, 5, 0.5, 1.5)
    if Cn > 1:
        Gr[:, min(3, Cn - 1)] = 0.0                                     # a channel without output gradient
    inp.update(h0=h0, head=head.contiguous(), tail=tail.contiguous(), Gr=Gr)
    if r.dtype == "bf16":
        inp = {k: ([t.to(BF) for t in v] if isinstance(v, list) else v.to(BF) if v.is_floating_point() else v) for k, v in inp.items()}
    return inp


def reference(r, inp):
    """float64 oracle on the float32 inputs: out and every gradient (autograd of oracle.recon_oracle.propagate)"""
    h = inp["h0"].double().requires_grad_(True)
    if r.mode == "blocks":
        Tl = [t.double().requires_grad_(True) for t in inp["Ts"]]
        I = inp["ident"].double().requires_grad_(True)
        adjs = [O.build_block_adjacency(t, I, r.S // 16) for t in Tl]
    else:
        adjs = [a.double().requires_grad_(True) for a in inp["adjs"]]
    out = O.propagate(adjs, h, r.act, inp["head"], inp["tail"], as_gemm=True)
    out.backward(inp["Gr"].double())
    ref = dict(out=out.detach(), g_h0=h.grad)
    if r.mode == "blocks":
        ref["g_identity"] = I.grad
        ref.update(("g_T[%d]" % l, t.grad) for l, t in enumerate(Tl))
    else:
        ref.update(("g_adj[%d]" % l, a.grad) for l, a in enumerate(adjs))
    return ref


# ------------------------------------------------------------------------------- the GPU side
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


def _to_dev(t, offset=False):
    if not offset:
        return t.to(dev())
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev())       # the same values one element into a buffer: a contiguous view at a 4-byte offset
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v.detach()


def run(r, inp, train):
    """one call through propagate() / propagate_blocks() (train: then the backward of Gr).  Returns (results on the host, [keys of the launches],
    the states the forward saved (bf16 rows) or None)"""
    from recon_amd import propagation as P
    d = dev()
    blocks = r.mode == "blocks"
    h = inp["h0"].to(d).requires_grad_(train)
    head, tail = inp["head"].to(d), inp["tail"].to(d)
    A = [_to_dev(a, r.offset).requires_grad_(train) for a in (inp["Ts"] if blocks else inp["adjs"])]
    I = inp["ident"].to(d).requires_grad_(train) if blocks else None
    states = None
    with P.trace_instances() as trace, torch.set_grad_enabled(train):
        want_states = r.dtype == "bf16" and train
        if blocks:
            out = P.propagate_blocks(A, I, r.S // 16, h, r.act, head, tail, return_states=want_states)
        else:
            out = P.propagate(A, h, r.act, head, tail, return_states=want_states)
        if want_states:
            out, states = out
        if train:
            out.backward(inp["Gr"].to(d))
    res = dict(out=out.detach())
    if train:
        res["g_h0"] = h.grad
        if blocks:
            res["g_identity"] = I.grad
        res.update((("g_T[%d]" if blocks else "g_adj[%d]") % l, a.grad) for l, a in enumerate(A))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}, [k for _, k in trace], states


def _close(actual, desired, atol, rel_to_max, what):
    """test_gat_gpu.close(), returning max |error| / max |desired|"""
    actual, desired = actual.double().numpy(), desired.double().numpy()
    assert actual.shape == desired.shape, "%s: shape %s, oracle %s" % (what, actual.shape, desired.shape)
    assert np.isfinite(actual).all(), what + ": non-finite values"
    mx = np.abs(desired).max() if desired.size else 0.0
    err = np.abs(actual - desired).max() if desired.size else 0.0
    print("%s: max abs err %.3e, max |ref| %.3e, tol %.3e" % (what, err, mx, atol + rel_to_max * mx))
    assert err <= atol + rel_to_max * mx, "%s: max abs err %.3e > tol %.3e" % (what, err, atol + rel_to_max * mx)
    return err / mx if mx > 0 else err


def _check_b16_row(r, inp, got, states, worst):
    """(d): the oracle on the bf16 operands with its states rounded hop by hop; gradients from the states the forward saved (test_prop_b16_gpu._check_b16;
    block mode: d A cut into the transition tensors' layout, its diagonal blocks summed into d identity)"""
    from test_prop_b16_gpu import _check_b16
    what = row_id(r)
    L = r.L
    if r.mode != "blocks":
        _check_b16(got["out"], ([got["g_adj[%d]" % l] for l in range(L)], got["g_h0"]), inp["adjs"], inp["h0"], inp["head"], inp["tail"], r.act, inp["Gr"],
                   states, not r.shared, what)
        return
    n = r.S // 16
    adjs = [O.build_block_adjacency(t.float(), inp["ident"].float(), n).to(BF) for t in inp["Ts"]]
    _check_b16(got["out"], None, adjs, inp["h0"], inp["head"], inp["tail"], r.act, inp["Gr"], None, not r.shared, what)
    adjs_f, h0_f = [a.float() for a in adjs], inp["h0"].float()
    _, ref_states = O.propagate(adjs_f, h0_f, r.act, inp["head"], inp["tail"], as_gemm=True, storage=BF, return_states=True)
    st = [states[l].float().cpu() for l in range(L)]
    for l in range(L):
        worst["state"] = max(worst.get("state", 0.0), _close(st[l], ref_states[l], 1e-3, 1.5e-2, what + " state %d" % (l + 1)))
    g_adj_r, g_h_r = O.propagate_backward(adjs_f, h0_f, st, r.act, inp["head"], inp["tail"], inp["Gr"].float(), storage=BF)
    g_I = torch.zeros(16, 16, dtype=torch.float64)
    for l in range(L):
        blk = g_adj_r[l].reshape(r.B, n, 16, n, 16).permute(0, 1, 3, 2, 4)                 # [B, i, j, 16, 16]
        off = ~torch.eye(n, dtype=torch.bool)
        worst["g_T"] = max(worst.get("g_T", 0.0), _close(got["g_T[%d]" % l].float(), blk[:, off].reshape(r.B, r.C, 256), 1e-3, 2e-2, what + " g_T[%d]" % l))
        g_I += blk[:, torch.eye(n, dtype=torch.bool)].double().sum((0, 1))
    worst["g_identity"] = max(worst.get("g_identity", 0.0), _close(got["g_identity"].float(), g_I, 1e-3, 2e-2, what + " g_identity"))
    ref_h = g_h_r if not r.shared else g_h_r.sum(0)
    worst["g_h0"] = max(worst.get("g_h0", 0.0), _close(got["g_h0"].float().reshape(ref_h.shape), ref_h, 1e-3, 2e-2, what + " g_h0"))


def pytest_generate_tests(metafunc):
    if "row" in metafunc.fixturenames:
        metafunc.parametrize("row", PROP_ROWS, ids=[row_id(r) for r in PROP_ROWS])


def test_propagation_instance_vs_oracle(row, recon_config, record_property):
    r = row
    for name, value in r.cfg:
        recon_config(name, value)
    assert probe(r) == (r.fwd, r.bwd, r.infer), "the row's shape and switches select other instances than it names"
    inp = make_inputs(r)
    got, keys, states = run(r, inp, True)
    assert keys == [r.fwd, r.bwd], "the launches of this call ran other instances than the row names"
    worst = {}
    if r.dtype == "bf16":
        _check_b16_row(r, inp, got, states, worst)                      # (d)
    else:
        ref = reference(r, inp)
        for name, v in got.items():                                     # (a)
            atol, rel = (1e-4, 1e-5) if name == "out" else (1e-5, 1e-4)
            worst[name] = _close(v, ref[name].reshape(v.shape), atol, rel, "%s %s" % (row_id(r), name))
    again, keys2, _ = run(r, inp, True)                                 # (b)
    assert keys2 == keys
    scatter = r.dtype == "fp32" and r.bwd // 10000 in SCATTER_BWD and collides(inp["head"], inp["tail"])
    for name, v in got.items():
        if scatter and name != "out":                                   # colliding float atomics: the second call meets the oracle's bar again
            worst[name] = max(worst[name], _close(again[name], ref[name].reshape(v.shape), 1e-5, 1e-4, "%s %s, second call" % (row_id(r), name)))
        else:
            assert torch.equal(v, again[name]), "%s: %s differs between two identical calls" % (row_id(r), name)
    if scatter:                                                         # the same instance on collision-free indices: every gradient bit for bit
        head, tail = collision_free(r)
        assert not collides(head, tail)
        inp2 = dict(inp, head=head, tail=tail)
        one, k1, _ = run(r, inp2, True)
        two, k2, _ = run(r, inp2, True)
        assert k1 == keys and k2 == keys
        for name, v in one.items():
            assert torch.isfinite(v).all() and torch.equal(v, two[name]), "%s: %s differs between two identical calls (collision-free indices)" % (row_id(r), name)
    infer, keys3, _ = run(r, inp, False)                                # (c)
    assert keys3 == [r.infer], "the no_grad call ran another instance than the row names"
    if r.infer == r.fwd:
        assert torch.equal(infer["out"], got["out"]), "%s: the no_grad forward differs from the training forward of the same instance" % row_id(r)
    elif r.dtype != "bf16":
        worst["out_no_grad"] = _close(infer["out"], ref["out"], 1e-4, 1e-5, "%s no_grad out" % row_id(r))
    for name, v in sorted(worst.items()):
        record_property("worst_rel_" + name, "%.3e" % v)
