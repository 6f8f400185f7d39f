"""Coverage guard and self-test of tests/test_gcn_instances_gpu.py (host only: the built library, no GPU).

1. Every path the launchers of csrc/gcn_b16.hip can select has a row of GCN_ROWS, and every row selects the key it names.  The sweep asks
   recon_gcn_b16_fwd_instance / recon_gcn_b16_bwd_instance (argument structures with placeholder addresses: the queries look at pointers
   for null and alignment only) over node counts, feature counts, aligned and offset pointers, each gradient wanted or not, and both
   RECON_GCN_FUSED* switches.  The forward is asked over the whole n x out grid at in = 16, the n x in grid at out = 16 (every third n, 32 and
   33) and a coarser in x out grid at n = 8 and 33; the backward over a REDUCED grid — out = 16 or n in (8, 32, 33), aligned pointers, and
   16 / 68 graphs (the split regimes) only at in = out = 16: its choice depends on n <= 32, on in and out rounded up to 8 against 320 and
   on what is wanted, which the n = 8 and n = 33 lines cross with every in and out.  A backward key carries the weight gradient's split count; the guard asks for a row per REGIME of it (none,
   one split, 2 .. 16, more than 16: k_b16_reduce's second level), the rows themselves name exact counts.
2. The GPU file's harness, run on the CPU against a float32-accumulate, bf16-round-to-nearest restatement of every stage, passes every
   band of every row: the bands are satisfiable by a faithful implementation.
3. The same harness rejects nine subtly wrong restatements, each on at least one row: the bands are sharp."""
import ctypes as C

import pytest
import torch

import test_gcn_instances_gpu as G
from test_gcn_instances_gpu import GCN_ROWS, row_id, opt, F4, F2, GEMM, RAGGED, FUSED, AGG, OK, ERR_INVALID, ERR_UNSUPPORTED, km_plan, kp, agg

BF = torch.bfloat16
PH = 1 << 20                                    # a placeholder address, 16-byte aligned


def rn(t):
    return t.to(BF)


def trunc(t):
    """float32 -> bf16 by dropping the low 16 bits"""
    return (t.contiguous().view(torch.int32) >> 16).to(torch.int16).view(BF)


class Restatement:
    """The family's arithmetic in float32 torch on the CPU with bf16 round-to-nearest stores, writing into the harness's buffers as the
    library does.  `mutant` names one deliberate error."""
    dev = torch.device("cpu")

    def __init__(self, mutant=None):
        self.mutant = mutant

    # ---- one layer
    def _sizes(self, c):
        if c.node_ptr is not None:
            return [int(v) for v in (c.node_ptr[1:] - c.node_ptr[:-1])]
        return [c.n] * c.B

    def _adjs(self, flat, sizes):
        out, at = [], 0
        for nb in sizes:
            out.append(flat[at:at + nb * nb].view(nb, nb).float())
            at += nb * nb
        return out

    def _layer(self, x, W, bias, adjs, B):
        """(support bf16, out bf16) of relu(adj @ (x @ W) + b); x float32 [rows, I]"""
        m, I, O = self.mutant, x.shape[1], W.shape[1]
        if m == "ktail" and I % 32:
            x = x.clone()
            x[:, I - 1] = 0
        s = rn(x @ W.float())
        adjs = [a.clone() for a in adjs]
        if m == "adjterm" and adjs:
            adjs[-1][-1, -1] = 0
        if m == "adjT":
            adjs = [a.t().contiguous() for a in adjs]
        pre = agg(adjs, s.float())
        if bias is not None:
            b = bias.float().clone()
            if m == "bias4" and O >= 164:
                b[80:160] = bias.float()[84:164]
            pre = pre + b
        out = torch.relu(pre)
        out = trunc(out) if m == "trunc" else rn(out)
        if m == "swap" and len({a.shape[0] for a in adjs}) == 1 and B % 4 >= 2:
            n, b0 = adjs[0].shape[0], 4 * (B // 4)
            out = out.clone()
            out[b0 * n:(b0 + 1) * n], out[(b0 + 1) * n:(b0 + 2) * n] = out[(b0 + 1) * n:(b0 + 2) * n].clone(), out[b0 * n:(b0 + 1) * n].clone()
        return s, out

    def _store(self, view, rows, ld, cols, val, zero_pads=True):
        v = view[:rows * ld].view(rows, ld)
        v[:, :cols] = val
        if zero_pads:
            v[:, cols:] = 1.0 if self.mutant == "padnz" else 0.0

    def fwd(self, c):
        key = G.fwd_instance(c)
        if key <= 0:
            return ERR_INVALID if key < 0 else OK
        sizes = self._sizes(c)
        rows = sum(sizes)
        x = c.x[:rows * c.ldx].view(rows, c.ldx)[:, :c.I].float()
        s, out = self._layer(x, c.W, c.bias, self._adjs(c.adj, sizes), c.B)
        if c.support is not None:
            pad, self.mutant = self.mutant, None                        # (padnz is about `out`)
            self._store(c.support, rows, c.lds, c.O, s)
            self.mutant = pad
        self._store(c.out, rows, c.ldo, c.O, out)
        return OK

    def bwd(self, b):
        key = G.bwd_instance(b)
        if key <= 0:
            return ERR_INVALID if key < 0 else OK
        c, m = b.fwd, self.mutant
        sizes = self._sizes(c)
        rows, I, O = sum(sizes), c.I, c.O
        out = c.out[:rows * c.ldo].view(rows, c.ldo)[:, :O].float()
        gout = b.gout[:rows * b.ldg].view(rows, b.ldg)[:, :O].float()
        gpre = gout * ((out >= 0) if m == "maskge" else (out > 0))
        adjs = self._adjs(c.adj, sizes)
        gs = rn(agg(adjs, gpre, transpose=True))
        pad, self.mutant = self.mutant, None
        self._store(b.g_support, rows, c.lds, O, gs)
        self.mutant = pad
        W = c.W.float()
        if b.g_x is not None:
            self._store(b.g_x, rows, b.ldgx, I, rn(gs.float() @ W.t()), zero_pads=False)
        if b.g_adj is not None:
            s = c.support[:rows * c.lds].view(rows, c.lds)[:, :O].float()
            at = r0 = 0
            for nb in sizes:
                b.g_adj[at:at + nb * nb] = rn(gpre[r0:r0 + nb] @ s[r0:r0 + nb].t()).reshape(-1)
                at, r0 = at + nb * nb, r0 + nb
        if b.g_w is not None:
            x = c.x[:rows * c.ldx].view(rows, c.ldx)[:, :I].float()
            b.g_w[:] = rn(self._split_k(x, gs.float(), *km_plan(I, O, rows))).reshape(-1)
        if b.g_b is not None:
            b.g_b[:] = rn(gpre.sum(0))
        return OK

    def _split_k(self, x, gs, splits, kps):
        parts = [x[z * kps:(z + 1) * kps].t() @ gs[z * kps:(z + 1) * kps] for z in range(splits)]
        if self.mutant == "splitk" and splits > 1:
            parts = parts[:-1]
        acc = parts[0]
        for p in parts[1:]:
            acc = acc + p
        return acc

    # ---- the stack
    @staticmethod
    def _stack_refused(c, train):
        if c.L > 8 or c.n > 32 or c.n % 4 or c.D % 4 or c.ldo > 320:
            return True
        if train:
            return c.I > 320 or c.ldo > kp(c.D)
        base = 3 * 20 * 16 * 64 + 4 * (-(-max(c.I, c.D) // 32)) * 2048 + 1024      # slabs, activation images, scratch; + the bias rows
        return base + 8 * 640 > 160 * 1024 and base + c.L * 640 > 160 * 1024

    def transposed_planes(self, W, I, D, planes):
        pl = planes[:D * kp(I)].view(D, kp(I))
        pl.zero_()
        pl[:, :I] = W.t()
        return OK

    def _stack(self, c, Ws):
        rows = c.B * c.n
        adjs = self._adjs(c.adj, [c.n] * c.B)
        h = c.x[:rows * c.ldx].view(rows, c.ldx)[:, :c.I].float()
        acts = []
        for l in range(c.L):
            _, out = self._layer(h, Ws[l], c.bias[l], adjs, c.B)
            acts.append(out)
            h = out.float()
        return acts

    def stack_fwd(self, c):
        if self._stack_refused(c, False):
            return ERR_UNSUPPORTED
        ins = [c.I] + [c.D] * (c.L - 1)
        Ws = [c.planes_t[l][:c.D * kp(ins[l])].view(c.D, kp(ins[l]))[:, :ins[l]].t() for l in range(c.L)]
        self._store(c.out, c.B * c.n, c.ldo, c.D, self._stack(c, Ws)[-1])
        return OK

    def stack_train_fwd(self, c):
        if self._stack_refused(c, True):
            return ERR_UNSUPPORTED
        rows = c.B * c.n
        for l, a in enumerate(self._stack(c, c.W)):
            self._store(c.acts[l], rows, c.ldo, c.D, a)
        if c.x_rows is not None:
            c.x_rows[:rows * c.ldxr].view(rows, c.ldxr)[:, :c.I] = c.x[:rows * c.ldx].view(rows, c.ldx)[:, :c.I]
        return OK

    def stack_train_bwd(self, c):
        m, rows, D = self.mutant, c.B * c.n, c.D
        adjs = self._adjs(c.adj, [c.n] * c.B)
        act = [c.acts[l][:rows * c.ldo].view(rows, c.ldo)[:, :D].float() for l in range(c.L)]
        mask = lambda a: (a >= 0) if m == "maskge" else (a > 0)
        g = c.gout[:rows * c.ldg].view(rows, c.ldg)[:, :D].float()
        for l in range(c.L - 1, -1, -1):
            gpre = g * mask(act[l])
            gs = rn(agg(adjs, gpre, transpose=True))
            pad, self.mutant = self.mutant, None
            self._store(c.g_support[l], rows, c.ldo, D, gs)
            self.mutant = pad
            I = c.I if l == 0 else D
            xin = c.x[:rows * c.ldx].view(rows, c.ldx)[:, :I].float() if l == 0 else act[l - 1]
            if c.g_w[l] is not None:
                wanted = [k for k in range(c.L) if c.g_w[k] is not None]
                c.g_w[l][:] = rn(self._split_k(xin, gs.float(), *G.stack_km_plan([c.I] + [D] * (c.L - 1), D, rows, wanted))).reshape(-1)
            if c.g_b[l] is not None:
                c.g_b[l][:] = rn(gpre.sum(0))
            g = rn(gs.float() @ c.W[l].float().t()).float()
        if c.g_x is not None:
            self._store(c.g_x, rows, c.ldgx, c.I, rn(g), zero_pads=False)
        return OK


# ------------------------------------------------------------------------------------------------- the harness on the restatement
@pytest.mark.parametrize("row", GCN_ROWS, ids=[row_id(r) for r in GCN_ROWS])
def test_float32_restatement_is_inside_every_band(row):
    ratios = G.run_row(row, Restatement())
    assert all(v <= 1.0 for v in ratios.values())


# mutant -> the rows it is tried on (the first that rejects it ends the search)
MUTANTS = {
    "ktail": lambda r: r.kind == "fwd" and r.I % 32,                    # the last feature of a K tail dropped
    "adjterm": lambda r: r.kind == "fwd" and r.key in (F4, F2, GEMM),   # one adjacency term dropped
    "adjT": lambda r: r.kind == "fwd" and r.n > 1,                      # the adjacency transposed
    "bias4": lambda r: r.kind == "fwd" and r.O >= 164 and opt(r, "bias", True),      # the bias of one column part shifted by four columns
    "trunc": lambda r: r.kind == "fwd" and r.key == GEMM,               # a truncating store (single-rounding band)
    "swap": lambda r: r.kind == "fwd" and r.B % 4 >= 2 and opt(r, "sizes") is None,  # graphs b, b + 1 swapped in a partly filled workgroup
    "maskge": lambda r: r.kind in ("bwd", "stack"),                     # the mask taken as out >= 0
    "splitk": lambda r: r.kind == "bwd" and r.key % 1000 > 1,           # the last split-K partial dropped
    "padnz": lambda r: r.kind == "fwd" and opt(r, "ldo", G.up8(r.O)) > r.O,          # the pad columns of out left non-zero
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_harness_rejects_the_wrong_restatement(mutant, capsys):
    tried = 0
    for r in GCN_ROWS:
        if MUTANTS[mutant](r) and r.B * r.n > 0:
            tried += 1
            try:
                G.run_row(r, Restatement(mutant))
            except AssertionError:
                return
    raise AssertionError("no row of GCN_ROWS rejects the restatement `%s` (%d rows tried)" % (mutant, tried))


def test_truncating_store_fails_the_fused_band_too():
    """the two-rounding band of the fused forward is wider than the single-rounding one; a truncated store still has to fall outside it
    on some fused row"""
    for r in GCN_ROWS:
        if r.kind == "fwd" and r.key in (F4, F2):
            try:
                G.run_row(r, Restatement("trunc"))
            except AssertionError:
                return
    pytest.fail("no fused row rejects a truncating store")


# ------------------------------------------------------------------------------------------------------------- coverage guard
N_GRID = list(range(1, 41)) + [64, 100, 256]
F_GRID = sorted({v for v in list(range(1, 9)) + [k * 16 + d for k in range(1, 22) for d in (-4, -1, 0, 1, 4)] if 1 <= v <= 336})
SWITCHES = [{}, {"RECON_GCN_FUSED": "0"}, {"RECON_GCN_FUSED_BWD": "0"}]


def regime(splits):
    return 0 if splits == 0 else 1 if splits == 1 else 2 if splits <= 16 else 3


def key_class(k):
    return k if k < 100000 else k - k % 1000 + regime(k % 1000)


def _placeholder(B, n, I, O, support, adj_off, bias, ragged):
    from recon_amd import _lib
    i8, o8 = G.up8(I), G.up8(O)
    return _lib.GcnB16Args(B, n, I, O, PH, i8, PH + adj_off, PH, None if bias is None else PH + bias, PH if support else None, o8, PH, o8, PH, 0,
                           PH if ragged else None, PH if ragged else None, B * n if ragged else 0)


def _sweep():
    from recon_amd import _lib
    L = _lib.lib()
    fwd_seen, bwd_seen = {}, {}
    pts = [(n, 16, O) for n in N_GRID for O in F_GRID] + [(n, I, 16) for n in N_GRID[::3] + [32, 33] for I in F_GRID] + [(n, I, O) for n in (8, 33) for I in F_GRID[::4] for O in F_GRID[::4]]
    for sw in SWITCHES:
        with _lib.config(**sw):
            for n, I, O in pts:
                for support, adj_off, bias, ragged in ((False, 0, 0, False), (False, 2, 0, False), (False, 0, 2, False), (False, 0, None, False),
                                                       (True, 0, 0, False), (True, 2, 2, False), (True, 0, 0, True)):
                    a = _placeholder(2, n, I, O, support, adj_off, bias, ragged)
                    k = L.recon_gcn_b16_fwd_instance(C.byref(a))
                    fwd_seen.setdefault(k, (n, I, O, support, adj_off, bias, ragged, sw))
                    if k <= 0 or adj_off or bias == 2 or (O != 16 and n not in (8, 32, 33)):
                        continue
                    for B in (2, 16, 68):
                        if B != 2 and (I, O) != (16, 16):
                            continue
                        a.B, a.total_rows = B, (B * n if ragged else 0)
                        for flags in range(16):
                            g_x, g_adj, g_w, g_b = (PH if flags & bit else None for bit in (1, 2, 4, 8))
                            b = _lib.GcnB16BwdArgs(a, PH, G.up8(O), PH, PH, g_x, G.up8(I), g_adj, g_w, g_b if bias is not None else None, PH)
                            kb = L.recon_gcn_b16_bwd_instance(C.byref(b))
                            bwd_seen.setdefault(key_class(kb), (B, n, I, O, support, ragged, flags, sw))
    return fwd_seen, bwd_seen


def _row_keys():
    fwd = {r.key for r in GCN_ROWS if r.kind == "fwd"}
    bwd = {key_class(r.key) for r in GCN_ROWS if r.kind == "bwd"}
    return fwd, bwd


def test_every_reachable_instance_has_a_row():
    fwd_seen, bwd_seen = _sweep()
    fwd_rows, bwd_rows = _row_keys()
    # the sweep itself reaches every forward path and refusals, both backward paths with and without d adj, every bias mode and split regime
    assert set(fwd_seen) >= {-1, F4, F2, GEMM, RAGGED}, sorted(fwd_seen)
    assert -1 in bwd_seen and len([k for k in bwd_seen if k > 0]) >= N_BWD_CLASSES, sorted(bwd_seen)
    missing = sorted(k for k in fwd_seen if k > 0 and k not in fwd_rows)
    assert not missing, "forward paths without a row in GCN_ROWS: %s" % [(k, fwd_seen[k]) for k in missing]
    missing = sorted(k for k in bwd_seen if k > 0 and k not in bwd_rows)
    assert not missing, "backward instances without a row in GCN_ROWS: %s" % [(k, bwd_seen[k]) for k in missing]


# what the launcher can select: {no g_W: bias none / alone; g_W in three regimes: bias none / rides} = 8 combinations, for the fused path
# (never with d adj) and for the aggregate path with and without d adj
N_BWD_CLASSES = 8 + 2 * 8


def test_every_row_selects_its_key():
    """with the row's own buffers on the host: what the GPU test asserts before it launches"""
    from recon_amd import _lib
    for r in GCN_ROWS:
        if r.kind not in ("fwd", "bwd"):
            continue
        inp = G.make_inputs(r)
        with _lib.config(**dict(opt(r, "cfg", ()))):
            c = G._layer_call(r, inp, torch.device("cpu"))
            k = G.fwd_instance(c)
            if r.kind == "fwd":
                assert k == r.key, row_id(r)
            elif inp.rows == 0 or opt(r, "sizes") or opt(r, "support"):
                assert k == (0 if inp.rows == 0 else RAGGED if opt(r, "sizes") else GEMM), row_id(r)
            else:
                assert k in (F4, F2), row_id(r)


def test_the_named_tails_each_have_a_row():
    rows = GCN_ROWS
    fwd = lambda key: [r for r in rows if r.kind == "fwd" and r.key == key]
    have = lambda rs, field, values: not (set(values) - {getattr(r, field) for r in rs})
    f4, f2, gm, rg = fwd(F4), fwd(F2), fwd(GEMM), fwd(RAGGED)
    assert any((r.B, r.n, r.I, r.O) == (1, 4, 8, 4) for r in f4)
    assert have(f4, "n", (12, 16, 20, 28, 32)) and have(f4, "B", (1, 4, 5, 7)) and have(f4, "I", (2, 30, 32, 34, 64, 300, 320, 520))
    assert have(f4, "O", (76, 80, 84, 156, 160, 164, 236, 240, 244, 300, 316, 320))
    assert any(not opt(r, "bias", True) for r in f4)
    assert any(opt(r, "ldx") == r.I and r.I % 2 == 0 and r.I % 8 and opt(r, "xfill") == "inf" for r in f4)
    assert any(opt(r, "ldx", 0) > G.up8(r.I) and opt(r, "xfill") == "nan" for r in f4)
    assert have(f2, "n", (1, 2, 9, 17, 31)) and have(f2, "O", (5, 130, 158, 162, 318))
    assert any(opt(r, "adj_off") and r.n % 4 == 0 and r.O % 4 == 0 for r in f2) and any(opt(r, "bias_off") and r.n % 4 == 0 and r.O % 4 == 0 for r in f2)
    assert have(gm, "n", (1, 2, 9, 12, 16, 17, 20, 28, 31, 32, 33, 64, 65, 100)) and have(gm, "O", (5, 63, 64, 65, 80, 160, 300, 320, 328))
    assert any(dict(opt(r, "cfg", ())).get("RECON_GCN_FUSED") == "0" and r.n <= 32 and r.O <= 320 for r in gm)
    sizes = [opt(r, "sizes") for r in rg]
    assert (1, 5, 32, 33, 256) in sizes and (3,) * 70 in sizes and any(s == (129, 64) and r.I == 33 for r, s in zip(rg, sizes))
    assert any(r.kind == "fwd" and r.key == 0 and sum(opt(r, "sizes")) == 0 for r in rows)
    bw = [r for r in rows if r.kind == "bwd"]
    fb = [r for r in bw if r.key // 100000 == FUSED]
    ag = [r for r in bw if r.key // 100000 == AGG]
    assert have(fb, "n", (2, 4, 9, 16, 17, 31, 32)) and have(fb, "B", (1, 5, 7)) and have(fb, "I", (7, 8, 33, 300, 320)) and have(fb, "O", (5, 16, 136, 300, 320))
    for mode in (0, 1, 2):
        assert any(r.key // 1000 % 10 == mode for r in fb), mode
    assert any(r.key % 1000 == 0 for r in fb) and any(r.key % 1000 > 0 for r in fb)
    assert any(not opt(r, "g_x", True) for r in ag) and any(G.up8(r.I) == 328 for r in ag) and any(opt(r, "g_adj") for r in ag)
    assert any(dict(opt(r, "cfg", ())).get("RECON_GCN_FUSED_BWD") == "0" for r in ag) and any(r.n == 33 for r in ag)
    assert any(r.B == 70 and r.n == 2 and r.key // 1000 % 10 == 2 for r in bw)
    assert have([r for r in ag if opt(r, "g_adj")], "n", (1, 17, 33))
    eights = [r for r in bw if (r.I, r.O) == (8, 8) and r.key > 0]
    assert {regime(r.key % 1000) for r in eights} == {1, 2, 3} and any(r.B * r.n == 68 * 32 and r.key % 1000 > 16 for r in eights)
    st = [r for r in rows if r.kind == "stack"]
    assert not (set((2, 3, 8)) - {opt(r, "L") for r in st}) and have(st, "n", (4, 8, 12, 32)) and have(st, "O", (4, 64, 136, 300, 320))
    assert have(st, "I", (2, 22, 37, 300, 320, 384)) and have(st, "B", (1, 5, 7))
    assert any(opt(r, "x_rows") and r.I == 37 for r in st) and any(opt(r, "frozen") is not None for r in st) and any(opt(r, "nobias") is not None for r in st)
    assert any(opt(r, "g_x") is False for r in st) and any(opt(r, "infer_only") and r.I == 384 for r in st)
    rs = [r for r in rows if r.kind == "refuse_stack"]
    assert all(r.key == ERR_UNSUPPORTED for r in rs)
    assert any(r.I == 416 and opt(r, "infer") for r in rs) and any(r.I == 328 and opt(r, "infer") is False for r in rs)
    assert any(r.n == 6 for r in rs) and any(r.O == 6 for r in rs) and any(opt(r, "L") == 9 for r in rs)
    rf = [r for r in rows if r.kind == "refuse"]
    assert any(opt(r, "ldx", 0) % 2 for r in rf) and any(opt(r, "ldo", 1 << 30) < G.up8(r.O) for r in rf) and any(opt(r, "out_off") for r in rf) and any(r.n == 33 for r in rf)


def test_split_rule_restated_matches_the_library():
    """km_plan() (the bands' split counts, the restatement's partition of the rows) is the library's rule"""
    from recon_amd import _lib
    L = _lib.lib()
    for B, n, I, O in ((4, 32, 8, 8), (16, 32, 8, 8), (68, 32, 8, 8), (7, 32, 320, 320), (5, 31, 300, 136), (70, 2, 8, 12), (1, 2, 7, 5), (2, 100, 24, 65)):
        a = _placeholder(B, n, I, O, True, 0, 0, False)
        b = _lib.GcnB16BwdArgs(a, PH, G.up8(O), PH, PH, None, G.up8(I), None, PH, None, PH)
        assert L.recon_gcn_b16_bwd_instance(C.byref(b)) % 1000 == km_plan(I, O, B * n)[0], (B, n, I, O)


def test_stack_split_rule_restated_matches_the_library():
    """the stack's weight gradients have no query: recon_gcn_b16_stack_bwd_partial_floats sizes the partials by the split counts of
    b16_kmajor_splits / _multi over every number of products, which pins km_plan()'s `count` and with it stack_km_plan() (the stack rows'
    g_weight bands, the restatement's partition)"""
    from recon_amd import _lib
    L = _lib.lib()
    shapes = [(r.B, r.n, r.I, r.O, opt(r, "L")) for r in GCN_ROWS if r.kind == "stack" and not opt(r, "infer_only")]
    shapes += [(64, 32, 8, 8, 2), (68, 32, 8, 8, 8), (16, 32, 8, 8, 3), (1024, 32, 300, 300, 3), (40, 32, 64, 320, 8), (256, 32, 320, 4, 5)]
    for B, n, I, D, nl in shapes:
        assert L.recon_gcn_b16_stack_bwd_partial_floats(B, n, I, D, nl) == G.stack_partial_floats(B, n, I, D, nl), (B, n, I, D, nl)
    # the counts differ with the number of products where rows allow many splits: the check above is not vacuous
    assert km_plan(320, 320, 1024 * 32, 1)[0] != km_plan(320, 320, 1024 * 32, 8)[0]


def test_instance_queries_refuse_what_the_launchers_refuse():
    from recon_amd import _lib
    L = _lib.lib()
    assert L.recon_gcn_b16_fwd_instance(None) == -1 and L.recon_gcn_b16_bwd_instance(None) == -1
    a = _placeholder(0, 8, 16, 16, False, 0, 0, False)
    assert L.recon_gcn_b16_fwd_instance(C.byref(a)) == 0                                     # no graphs: nothing is launched
    a = _placeholder(3, 33, 16, 16, False, 0, 0, False)
    assert L.recon_gcn_b16_fwd_instance(C.byref(a)) == -1                                    # the fused forward stops at 32 nodes
    a = _placeholder(3, 8, 16, 16, False, 0, 0, False)
    assert L.recon_gcn_b16_fwd_instance(C.byref(a)) == F4
    a.ldx = 17
    assert L.recon_gcn_b16_fwd_instance(C.byref(a)) == -1
    a.ldx, a.out = 18, PH + 8
    assert L.recon_gcn_b16_fwd_instance(C.byref(a)) == -1
    a.out = PH
    assert L.recon_gcn_b16_fwd_instance(C.byref(a)) == F4                                    # any even ldx >= in: the K tail is masked
    mk = lambda **kw: _lib.GcnB16BwdArgs(a, PH, 16, PH, PH, PH, 16, kw.get("g_adj"), kw.get("g_w"), None, PH)
    assert L.recon_gcn_b16_bwd_instance(C.byref(mk())) == G.bkey(FUSED, 0, 0, 0)
    assert L.recon_gcn_b16_bwd_instance(C.byref(mk(g_adj=PH))) == -1                         # d adj reads `support`
    assert L.recon_gcn_b16_bwd_instance(C.byref(mk(g_w=PH))) == -1                           # the weight gradient reads x in rows of 8
    a.ldx = 16
    assert L.recon_gcn_b16_bwd_instance(C.byref(mk(g_w=PH))) == G.bkey(FUSED, 0, 0, 1)
    b = mk()
    b.ldgx = 12
    assert L.recon_gcn_b16_bwd_instance(C.byref(b)) == -1
    b.ldgx, b.fwd.lds = 16, 8
    assert L.recon_gcn_b16_bwd_instance(C.byref(b)) == -1                                    # g_support has rows of fwd.lds >= out rounded up to 8
