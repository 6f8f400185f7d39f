"""recon_amd.pair_groups (csrc/pair_groups.hip) on the GPU: the maps and the compact copies against the plain-loop restatement through the
Python entry and through the C ABI, inside sentinel-filled guards; `expand` and its backward against float64; `pair_sentence_states(...,
groups=)` against the DENSE stock chain in float64 inside the band tests/test_sent_lstm_gpu.py uses; the saved state's size; and GPGNN,
RECON and ContextAware under `run_epoch` with `distinct_pair_sequences` off and on.  DESIGN.md section 35.

Figures measured on an MI355X are in DESIGN.md section 35."""
import copy

import numpy as np
import pytest
import torch

from op_checks import band_failures, bound, calls_of, close, dev, peak_bytes, rel_err, same
from pair_groups_checks import (CASE_NAMES, KERNEL_REFUSES, case, compact_differences, dense_reference, differences, entity_markers, op_inputs, tile_case,
                                wide_case)
from test_sent_lstm_gpu import NAMES, kernels_ran, run

pytestmark = pytest.mark.gpu
SENTINEL = {torch.int64: -7777, torch.int32: -7777, torch.float32: 12345.678}
GUARD = 64                                      # elements: the guarded bases stay 16-byte aligned, as torch's own allocations are
DTYPES = [(torch.int64, torch.int64), (torch.int32, torch.int32), (torch.int64, torch.int8), (torch.int32, torch.int8), (torch.int64, torch.int32)]


class Guards:
    """Buffers inside sentinel-filled memory, a guard in front and another behind."""

    def __init__(self):
        self.held = []

    def new(self, shape, dtype, device):
        n = int(np.prod(shape))
        flat = torch.full((n + 2 * GUARD,), SENTINEL[dtype], dtype=dtype, device=device)
        self.held.append((flat, n, dtype))
        return flat[GUARD:GUARD + n].view(shape)

    def intact(self):
        assert self.held
        for flat, n, dtype in self.held:
            sentinel = torch.full((GUARD,), SENTINEL[dtype], dtype=dtype, device=flat.device)
            assert torch.equal(flat[:GUARD], sentinel) and torch.equal(flat[GUARD + n:], sentinel), (dtype, n)


def _guarded(monkeypatch):
    from recon_amd import pair_groups
    g = Guards()
    monkeypatch.setattr(pair_groups, "_new", g.new)
    return g


def _abi_build(sentence, markers, total, guards):
    """recon_pair_groups_build through ctypes into guarded buffers -> (rc, seq_pair, pair_seq, seq_ptr, sentence_d, markers_d, status)."""
    from recon_amd import _lib
    L = _lib.lib()
    B, C, T = markers.shape
    d = dev()
    rows = max(total, 0)
    seq_pair, pair_seq, seq_ptr = guards.new((rows,), torch.int32, d), guards.new((B * C,), torch.int32, d), guards.new((B + 1,), torch.int32, d)
    sentence_d, markers_d = guards.new((rows, T), sentence.dtype, d), guards.new((rows, 1, T), sentence.dtype, d)
    status = torch.zeros(1, dtype=torch.int32, device=d)
    ws = _lib.workspace(L.recon_pair_groups_workspace_bytes(B, C, T), d)
    rc = L.recon_pair_groups_build(sentence.data_ptr(), sentence.element_size(), markers.data_ptr(), markers.element_size(), B, C, T, total,
                                   seq_pair.data_ptr(), pair_seq.data_ptr(), seq_ptr.data_ptr(), sentence_d.data_ptr(), markers_d.data_ptr(),
                                   status.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, seq_pair, pair_seq, seq_ptr, sentence_d, markers_d, status


# ------------------------------------------------------------------------------------------------------------- maps and status
@pytest.mark.parametrize("name", CASE_NAMES)
def test_maps_and_compact_copies_are_the_restatement(name, monkeypatch):
    from recon_amd import PairGroups, _lib, pair_groups
    sentence, markers, want = case(name)
    s, m = sentence.to(dev()), markers.to(dev())
    B, C, T = m.shape
    taken = bool(_lib.lib().recon_pair_groups_supported(B, C, T))
    assert taken == (name not in KERNEL_REFUSES)
    guards = _guarded(monkeypatch)
    kernel = calls_of(monkeypatch, pair_groups._lib, "check")
    g = PairGroups.from_markers(s, m)
    assert bool(kernel) == taken                                           # above the limits the torch path runs, and nothing else
    assert g.total == want["total"] and not differences(g, want) and not compact_differences(g, s, m, want)
    again = PairGroups.from_markers(s, m, total=want["total"])
    for a, b in ((g.seq_pair, again.seq_pair), (g.pair_seq, again.pair_seq), (g.seq_ptr, again.seq_ptr), (g.sentence_d, again.sentence_d),
                 (g.markers_d, again.markers_d)):
        assert torch.equal(a, b)                                           # two runs, bit for bit
    if taken:
        guards.intact()
        abi = Guards()
        rc, seq_pair, pair_seq, seq_ptr, sentence_d, markers_d, status = _abi_build(s, m, want["total"], abi)
        assert rc == 0 and int(status) == 0
        got = {"seq_pair": seq_pair, "pair_seq": pair_seq, "seq_ptr": seq_ptr, "total": int(seq_ptr[B])}
        assert not differences(got, want)
        assert torch.equal(sentence_d, g.sentence_d) and torch.equal(markers_d, g.markers_d)
        abi.intact()
    else:
        rc = _abi_build(s, m, want["total"], Guards())[0]
        assert rc == -2                                                    # RECON_ERR_UNSUPPORTED, before any launch


@pytest.mark.parametrize("index_dtype,marker_dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_all_index_dtypes(index_dtype, marker_dtype, monkeypatch):
    from recon_amd import PairGroups
    from recon_amd.pair_groups import distinct_counts
    guards = _guarded(monkeypatch)
    for name in ("zero_and_distinct", "T37", "T1", "C72_k3", "tile_17", "last_element", "first_element"):
        sentence, markers, want = case(name)
        s, m = sentence.to(dev(), index_dtype), markers.to(dev(), marker_dtype)
        g = PairGroups.from_markers(s, m)
        assert not differences(g, want) and not compact_differences(g, s, m, want)
        assert g.sentence_d.dtype == g.markers_d.dtype == index_dtype
        assert torch.equal(distinct_counts(m).cpu().long(), torch.from_numpy(np.diff(want["seq_ptr"])))
        assert torch.equal(distinct_counts(m, chunk=2).cpu().long(), torch.from_numpy(np.diff(want["seq_ptr"])))
    guards.intact()


def test_unaligned_marker_rows_take_the_narrow_word_kernels():
    """A markers view whose base is 1, 2 and 4 bytes off an 8-byte boundary (int8; T = 37, 6 and 4): the word width follows the address."""
    from recon_amd import _lib
    L = _lib.lib()
    for name in ("T37", "last_element", "far_equal_nonzero"):
        _, markers, want = case(name)
        B, C, T = markers.shape
        for off in (0, 1, 2, 4):
            flat = torch.zeros(B * C * T + 8, dtype=torch.int8, device=dev())
            flat[off:off + B * C * T] = markers.to(torch.int8).reshape(-1).to(dev())
            first, lrank, counts = (torch.full((n,), -7777, dtype=torch.int32, device=dev()) for n in (B * C, B * C, B))
            assert L.recon_pair_groups_local(flat[off:].data_ptr(), 1, B, C, T, first.data_ptr(), lrank.data_ptr(), counts.data_ptr(),
                                             _lib.current_stream()) == 0
            assert torch.equal(counts.cpu().long(), torch.from_numpy(np.diff(want["seq_ptr"]))), (name, off)


@pytest.mark.parametrize("name", ["C72_k3", "tile_17", "zero_and_distinct"])
def test_a_wrong_total_sets_the_status_word_and_writes_nothing_behind_the_guard(name, monkeypatch):
    from recon_amd import PairGroups
    from recon_amd.pair_groups import known_total
    sentence, markers, want = case(name)
    s, m = sentence.to(dev()), markers.to(dev())
    B, C, T = m.shape
    guards = _guarded(monkeypatch)
    for wrong in (want["total"] - 1, want["total"] + 1):
        abi = Guards()
        rc, seq_pair, pair_seq, seq_ptr, sentence_d, markers_d, status = _abi_build(s, m, wrong, abi)
        assert rc == 0 and int(status) == 1
        abi.intact()
        assert int(seq_ptr[B]) == want["total"]                            # the scan's own total
        assert int(pair_seq.max()) < wrong and int(pair_seq.min()) >= 0 and int(seq_pair.min()) >= 0 and int(seq_pair.max()) < B * C
        with pytest.raises(ValueError, match="not the %d given" % wrong):
            PairGroups.from_markers(s, m, total=wrong)
        guards.intact()
        with pytest.raises(ValueError, match="not the %d given" % wrong):
            with known_total(wrong):
                g = PairGroups.from_markers(s, m)                          # nothing is read here
                assert g.total == wrong
        guards.intact()
    assert PairGroups.from_markers(s, m, total=want["total"]).total == want["total"]       # the word was cleared
    # outside [B, B C]: refused before any launch, by the entry and by the class
    assert _abi_build(s, m, B - 1, Guards())[0] == -1 and _abi_build(s, m, B * C + 1, Guards())[0] == -1


def test_the_torch_path_on_the_gpu_defers_its_mismatch_too():
    from recon_amd import PairGroups
    from recon_amd.pair_groups import known_total
    sentence, markers, want = case("C257")
    s, m = sentence.to(dev()), markers.to(dev())
    with pytest.raises(ValueError, match="not the"):
        with known_total(want["total"] + 2):
            g = PairGroups.from_markers(s, m)
            assert g.total == want["total"] + 2 and int(g.pair_seq.max()) < g.total
    with known_total(want["total"]):
        assert not differences(PairGroups.from_markers(s, m), want)


# ------------------------------------------------------------------------------------------------------------- expansion
def _sized_groups():
    """B = 4, C = 72, T = 2: group sizes 1 (sentence 0), 2 (sentence 1), 66 beside six of 1 (sentence 2) and 72 (sentence 3)."""
    from recon_amd import PairGroups
    m = torch.zeros(4, 72, 2, dtype=torch.int64)
    m[0, :, 0] = torch.arange(72)
    m[0, :, 1] = 1
    m[1, :, 0] = torch.arange(72) % 36
    m[1, :, 1] = 2
    m[2, [3, 9, 20, 33, 50, 71], 0] = torch.arange(1, 7)
    g = PairGroups.from_markers(torch.zeros(4, 2, dtype=torch.int64, device=dev()), m.to(dev()))
    sizes = torch.bincount(g.pair_seq.cpu().long())
    assert sorted(set(sizes.tolist())) == [1, 2, 66, 72] and g.total == 72 + 36 + 7 + 1
    return g


@pytest.mark.parametrize("F", [1, 32, 512, 513])
def test_expand_is_exact_and_its_backward_stays_inside_the_stock_chains_band(F, monkeypatch):
    g = _sized_groups()
    guards = _guarded(monkeypatch)
    gen = torch.Generator().manual_seed(F)
    rows = torch.randn(g.total, F, generator=gen)
    g_out = torch.randn(g.B, g.C, F, generator=gen)
    ps = g.pair_seq.cpu().long()

    def run_op():
        r = rows.to(dev()).requires_grad_(True)
        out = g.expand(r)
        out.backward(g_out.to(dev()))
        return [out.detach(), r.grad]
    out, grad = run_op()
    guards.intact()
    assert torch.equal(out.cpu().reshape(-1, F), rows[ps])                # the forward is a copy
    ref = torch.zeros(g.total, F, dtype=torch.float64).index_add_(0, ps, g_out.double().reshape(-1, F))
    r_cpu = rows.clone().requires_grad_(True)                              # the stock chain: index_select's backward on the CPU, one order
    r_cpu.index_select(0, ps).backward(g_out.reshape(-1, F))
    e_op, e_chain = rel_err(grad, ref), rel_err(r_cpu.grad, ref)
    print("expand backward F=%d: op %.3e chain %.3e bound %.3e" % (F, e_op, e_chain, bound(e_chain)))
    assert e_op <= bound(e_chain)
    same([out, grad], run_op())                                            # two runs agree bit for bit


def test_expand_takes_unaligned_rows_and_any_number_of_backwards():
    g = _sized_groups()
    flat = torch.randn(g.total * 8 + 1, device=dev())
    rows = flat[1:].view(g.total, 8).requires_grad_(True)                 # 4 bytes off a 16-byte boundary: the element-store instance
    out = g.expand(rows)
    assert torch.equal(out.reshape(-1, 8), rows.detach()[g.pair_seq.long()])
    g_out = torch.randn_like(out)
    a, = torch.autograd.grad(out, rows, g_out, retain_graph=True)
    b, = torch.autograd.grad(out, rows, g_out)
    assert torch.equal(a, b)
    ref = torch.zeros(g.total, 8, dtype=torch.float64).index_add_(0, g.pair_seq.cpu().long(), g_out.cpu().double().reshape(-1, 8))
    assert rel_err(a, ref) <= 1e-5


# ------------------------------------------------------------------------------------------------------------- the op
def _k_markers(B, ks, T, seed):
    return torch.from_numpy(entity_markers(B, ks, T, seed=seed))


OP_CASES = {                                                               # markers, Dw, P, H
    "zero_and_distinct_H16": (lambda: case("zero_and_distinct")[1], 4, 3, 16),
    "k3_H100": (lambda: _k_markers(3, 3, 8, 11), 50, 3, 100),
    "k2_H256": (lambda: _k_markers(2, 2, 6, 12), 7, 3, 256),
    "tile_15": (lambda: torch.from_numpy(tile_case(15)), 5, 3, 16),
    "tile_16": (lambda: torch.from_numpy(tile_case(16)), 5, 3, 16),
    "tile_17": (lambda: torch.from_numpy(tile_case(17)), 5, 3, 16),
    "tile_33": (lambda: torch.from_numpy(tile_case(33)), 5, 3, 16),
    "wide_2048": (lambda: torch.from_numpy(wide_case(2048)), 4, 3, 16),
    "wide_2049": (lambda: torch.from_numpy(wide_case(2049)), 4, 3, 16),
    "reference_widths_B5": (lambda: _k_markers(5, [2, 3, 5, 3, 2], 36, 13), 50, 3, 256),
}
EXPECTED_S_D = {"tile_15": 15, "tile_16": 16, "tile_17": 17, "tile_33": 33, "wide_2048": 2048, "wide_2049": 2049, "k3_H100": 21, "k2_H256": 6,
                "reference_widths_B5": 3 + 7 + 21 + 7 + 3}
_OP = {}


def op_case(name, packed):
    """Inputs, the restated pair_seq, the S_d-row draw and the float64 DENSE reference of a case, computed once and left unchanged."""
    from pair_groups_checks import restate
    from recon_amd.char_features import pack_keep
    if (name, packed) not in _OP:
        make, Dw, P, H = OP_CASES[name]
        rnn, sentence, markers, word_table, pos_table, g_out = op_inputs(make(), Dw, P, H)
        B, C, T = markers.shape
        want = restate(markers.numpy())
        keep = factors = None
        if packed:
            keep = pack_keep((torch.rand(want["total"], T, Dw, generator=torch.Generator().manual_seed(9)) >= 0.5).float() * 2.0, 2.0)      # p = 0.5
            factors = keep.factors()[torch.from_numpy(want["pair_seq"])].view(B, C, T, Dw)     # pair (b, c) takes row pair_seq[b, c]
        ref = dense_reference(rnn, sentence, markers, word_table, pos_table, g_out, factors)
        _OP[(name, packed)] = (rnn, sentence, markers, word_table, pos_table, g_out, keep, factors, want, ref)
    return _OP[(name, packed)]


def _keep_on_gpu(keep):
    from recon_amd.char_features import PackedKeep
    return None if keep is None else PackedKeep(keep.bits.to(dev()), keep.scale, keep.C)


def grouped(m, s, k, wt, pt, keep):
    from recon_amd import PairGroups, pair_sentence_states
    return pair_sentence_states(m, s, k, wt, pt, keep, groups=PairGroups.from_markers(s, k))


@pytest.mark.parametrize("packed", [False, True], ids=["nokeep", "packed"])
@pytest.mark.parametrize("name", list(OP_CASES))
def test_value_and_gradients_against_the_dense_float64_chain(name, packed, monkeypatch):
    from recon_amd.sentence_lstm import _chain
    rnn, sentence, markers, word_table, pos_table, g_out, keep, factors, want, ref = op_case(name, packed)
    if name in EXPECTED_S_D:
        assert want["total"] == EXPECTED_S_D[name]
    calls = kernels_ran(monkeypatch)
    got = run(grouped, rnn, sentence, markers, word_table, pos_table, g_out, _keep_on_gpu(keep))
    assert calls, "the kernels take this shape: the op must not run the chain"
    f = None if factors is None else factors.to(dev())
    chain = run(lambda m, s, k, wt, pt, _: _chain(m, s, k, wt, pt, f), rnn, sentence, markers, word_table, pos_table, g_out, None)
    assert got[0].shape == tuple(markers.shape[:2]) + (2 * rnn.hidden_size,)
    assert torch.count_nonzero(got[1][0]) == 0                             # the padding row's gradient
    failures = band_failures(NAMES, got, chain, ref, "pair_groups %s %s" % (name, "packed" if packed else "nokeep"))
    assert not failures, failures


@pytest.mark.parametrize("name", ["zero_and_distinct_H16", "k3_H100", "tile_17"])
def test_identity_groups_give_the_dense_calls_bits(name):
    from recon_amd import PairGroups, pair_sentence_states
    from recon_amd.char_features import pack_keep
    rnn, sentence, markers, word_table, pos_table, g_out = op_case(name, False)[:6]
    B, C, T = markers.shape
    full = pack_keep((torch.rand(B * C, T, word_table.shape[1], generator=torch.Generator().manual_seed(4)) >= 0.5).float() * 2.0, 2.0)
    ident = lambda m, s, k, wt, pt, keep: pair_sentence_states(m, s, k, wt, pt, keep, groups=PairGroups.identity(B, C, dev()))
    for keep in (None, full):
        args = (rnn, sentence, markers, word_table, pos_table, g_out, _keep_on_gpu(keep))
        same(run(pair_sentence_states, *args), run(ident, *args))


@pytest.mark.parametrize("name", ["k3_H100", "tile_16", "tile_17", "wide_2049"])
def test_out_is_expand_of_a_dense_call_over_the_gathered_rows(name):
    """Pins the maps, not the LSTM: the rows are gathered here from the restatement, on the host."""
    from recon_amd import PairGroups, pair_sentence_states
    rnn, sentence, markers, word_table, pos_table, g_out, keep, _, want, _ = op_case(name, True)
    C = markers.shape[1]
    p = torch.from_numpy(want["seq_pair"])
    s_d, m_d = sentence[p // C].to(dev()), markers.reshape(-1, markers.shape[2])[p].unsqueeze(1).to(dev())
    m = copy.deepcopy(rnn).to(dev())
    wt, pt, kp = word_table.to(dev()), pos_table.to(dev()), _keep_on_gpu(keep)
    with torch.no_grad():
        groups = PairGroups.from_markers(sentence.to(dev()), markers.to(dev()))
        rows = pair_sentence_states(m, s_d, m_d, wt, pt, kp)
        out = pair_sentence_states(m, sentence.to(dev()), markers.to(dev()), wt, pt, kp, groups=groups)
        assert torch.equal(out, groups.expand(rows.view(want["total"], -1)))
        assert torch.equal(out.reshape(-1, out.shape[2]), rows.view(want["total"], -1)[torch.from_numpy(want["pair_seq"]).to(dev())])
        # hand-built groups without compact copies (the gather by seq_pair) give the same bits
        bare = PairGroups(groups.seq_pair, groups.pair_seq, groups.seq_ptr, groups.B, groups.C, groups.total)
        assert torch.equal(out, pair_sentence_states(m, sentence.to(dev()), markers.to(dev()), wt, pt, kp, groups=bare))


def test_fallback_chain_takes_the_same_gather_and_expand(monkeypatch):
    """fp32 factors send the call to `_chain`: over the S_d compact rows, then `expand`."""
    from recon_amd import PairGroups, pair_sentence_states, sentence_lstm
    rnn, sentence, markers, word_table, pos_table, g_out, keep, factors, want, ref = op_case("k3_H100", True)
    T, Dw = markers.shape[2], word_table.shape[1]
    chain_calls = calls_of(monkeypatch, sentence_lstm, "_chain")
    f = keep.factors().view(want["total"], 1, T, Dw).to(dev())
    got = run(lambda m, s, k, wt, pt, kp: pair_sentence_states(m, s, k, wt, pt, kp, groups=PairGroups.from_markers(s, k)), rnn, sentence, markers,
              word_table, pos_table, g_out, f)
    assert len(chain_calls) == 1
    for a, r in zip(got, ref):
        assert rel_err(a, r) <= 2e-5


def test_saved_state_scales_with_the_distinct_sequences():
    """k = 3 of n = 9: 7 of 72 sequences per sentence.  Forward + backward of the mapped call peaks below the dense call's."""
    from recon_amd import PairGroups, pair_sentence_states
    markers = _k_markers(5, 3, 12, 21)
    rnn, sentence, markers, word_table, pos_table, g_out = op_inputs(markers, 50, 3, 100)
    m = copy.deepcopy(rnn).to(dev())
    s, k, wt, pt, g = sentence.to(dev()), markers.to(dev()), word_table.to(dev()), pos_table.to(dev()).requires_grad_(True), g_out.to(dev())
    groups = PairGroups.from_markers(s, k)
    assert groups.total == 35

    def step(gr):
        m.zero_grad(set_to_none=True)
        pt.grad = None
        pair_sentence_states(m, s, k, wt, pt, groups=gr).backward(g)
    mapped_peak, _ = peak_bytes(lambda: step(groups))
    dense_peak, _ = peak_bytes(lambda: step(None))
    print("pair_sentence_states forward + backward peak: mapped %d bytes, dense %d bytes (S_d / S = 35 / 360)" % (mapped_peak, dense_peak))
    assert 0 < mapped_peak < dense_peak


# ------------------------------------------------------------------------------------------------------------- whole models
def _absent_pairs_zeroed(as_indices):
    """The dataset with the marker rows of the pairs without a label zeroed, as the preprocessing leaves them."""
    a = list(as_indices)
    a[1] = np.where((np.asarray(a[2]) != 0)[:, :, None], a[1], 0).astype(np.int8)
    return tuple(a)


def _model_case(which):
    from pair_attention_checks import context_aware_for_epochs
    from test_stage_b_gpu import _gpgnn, _recon
    if which == "ContextAware":
        make, as_indices = context_aware_for_epochs(dev())
        return make, as_indices, None, None
    return _gpgnn(False) if which == "GPGNN" else _recon(False)


@pytest.mark.parametrize("which", ("GPGNN", "RECON", "ContextAware"))
def test_run_epoch_with_the_switch_off_and_on(which, monkeypatch):
    """N = 7, dropout 0: three training steps under Adam (an epoch of two batches of 3, then one batch of 6), then an evaluation pass
    with rows, with `distinct_pair_sequences` off and on.  Eval: predictions and result rows equal, the
    loss within 1e-4; training: every parameter within 1e-4 after the three steps.  Off: `from_markers` is never called."""
    from recon_amd import EpochRows, PairGroups, RelationMetrics, StageBData, run_epoch, stage_b
    from recon_amd.optim import Adam
    from stage_b_checks import permutation
    make, as_indices, surface_ids, batcher = _model_case(which)
    data = StageBData.from_indices(_absent_pairs_zeroed(as_indices), surface_ids).to(dev())
    order = torch.from_numpy(permutation(7, 3)).to(dev())
    adam = lambda m: Adam(filter(lambda p: p.requires_grad, m.parameters()), lr=1e-2, weight_decay=1e-4, max_grad_norm=0.25)
    losses, real = [], stage_b.relation_objective

    def recorded(*a, **k):
        res = real(*a, **k)
        losses[-1].append(res.loss.detach().clone())
        return res
    monkeypatch.setattr(stage_b, "relation_objective", recorded)
    built = []
    real_from = PairGroups.from_markers.__func__

    def counted(cls, *a, **k):
        g = real_from(cls, *a, **k)
        built.append(g.total)
        return g
    monkeypatch.setattr(PairGroups, "from_markers", classmethod(counted))
    results = []
    for on in (False, True):
        m = make().train()
        m.distinct_pair_sequences = on
        opt = adam(m)
        train, test, rows = RelationMetrics(dev()), RelationMetrics(dev()), EpochRows.for_data(data)
        losses.append([])
        run_epoch(m, data, 3, order=order, optimizer=opt, batcher=batcher, metrics=train)          # two steps
        run_epoch(m, data, 6, order=order, optimizer=opt, batcher=batcher, metrics=train)          # the third
        m.eval()
        run_epoch(m, data, 3, batcher=batcher, metrics=test, rows=rows)
        results.append((m, train.result(), test.result(), rows.result()))
        assert len(built) == (5 if on else 0)
    assert all(t < n * data.C for t, n in zip(built, (3, 3, 6, 3, 3)))    # the zeroed rows are shared
    (ma, train_a, test_a, rows_a), (mb, train_b, test_b, rows_b) = results
    assert len(losses[0]) == len(losses[1]) == 5
    for x, y in zip(losses[0], losses[1]):
        assert abs(float(x) - float(y)) <= 1e-4
    changed = 0
    for (k, p), q, fresh in zip(ma.named_parameters(), mb.parameters(), make().parameters()):
        assert (p - q).abs().max().item() <= 1e-4, k
        changed += int(p.requires_grad and not torch.equal(p, fresh))
    assert changed > 0
    assert test_a[:4] == test_b[:4] and test_a.batches == 2
    assert rows_a.pair.numel() == test_a.kept > 0
    for f in ("pair", "predicted", "gold"):
        assert torch.equal(getattr(rows_a, f), getattr(rows_b, f)), f
    close(rows_b.confidence, rows_a.confidence, what="confidence")


def test_packed_dropout_draws_one_row_per_distinct_sequence(monkeypatch):
    from recon_amd import gpgnn
    from test_stage_b_gpu import _gpgnn
    make, as_indices, _, _ = _gpgnn(True)
    m = make().train()
    m.distinct_pair_sequences = True
    m.dropout2.p = 0.0
    a = _absent_pairs_zeroed(as_indices)
    sent, mark = torch.from_numpy(a[0][:3].astype(np.int64)).to(dev()), torch.from_numpy(a[1][:3].astype(np.int64)).to(dev())
    drawn = []
    real = gpgnn.draw_packed_keep
    monkeypatch.setattr(gpgnn, "draw_packed_keep", lambda rows, *r, **k: (drawn.append(rows), real(rows, *r, **k))[1])
    calls = kernels_ran(monkeypatch)
    out = m.encode(sent, mark)
    from pair_groups_checks import restate
    want = restate(a[1][:3].astype(np.int64))
    assert drawn == [want["total"]] and len(calls) == 1 and want["total"] < 3 * mark.shape[1]
    rows = out.reshape(-1, out.shape[2])
    ps = torch.from_numpy(want["pair_seq"]).to(dev())
    assert torch.equal(rows, rows[torch.from_numpy(want["seq_pair"]).to(dev())][ps])          # the slots of a group share the draw
