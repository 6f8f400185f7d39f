"""recon_amd.pair_groups on CPU tensors (the torch path) against the plain-loop restatement of tests/pair_groups_checks.py, the
restatement's wrong variants, `expand` against float64, the grouped `pair_sentence_states` against the dense call on the reference's
fixtures, `known_total`, and every rejection.  DESIGN.md section 35."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from op_checks import entries_declared_and_bound, state_dict_of
from pair_groups_checks import (CASE_NAMES, EXPECTED_TOTAL, VARIANTS, case, compact_differences, dense_reference, differences, entity_markers,
                                op_inputs, restate)

ENTRIES = ("recon_pair_groups_supported", "recon_pair_groups_workspace_bytes", "recon_pair_groups_local", "recon_pair_groups_build",
           "recon_pair_groups_expand", "recon_pair_groups_reduce")
DTYPES = [(torch.int64, torch.int64), (torch.int32, torch.int32), (torch.int64, torch.int8), (torch.int32, torch.int8), (torch.int64, torch.int32)]


def test_header_declares_and_lib_binds_the_entries():
    entries_declared_and_bound(ENTRIES[2:], "models/models.py:160-184")
    entries_declared_and_bound(ENTRIES[:4], "parsing/legacy_sp_models.py:294-326")
    assert "pair_groups.hip" in open(os.path.join(ROOT, "recon_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_torch_path_is_the_restatement(name):
    from recon_amd import PairGroups
    sentence, markers, want = case(name)
    if name in EXPECTED_TOTAL:
        assert want["total"] == EXPECTED_TOTAL[name]
    g = PairGroups.from_markers(sentence, markers)
    assert (g.B, g.C) == tuple(markers.shape[:2])
    assert not differences(g, want) and not compact_differences(g, sentence, markers, want)
    for t in (g.seq_pair, g.pair_seq, g.seq_ptr):
        assert t.dtype == torch.int32
    again = PairGroups.from_markers(sentence, markers, total=want["total"])
    assert not differences(again, want) and not compact_differences(again, sentence, markers, want)


@pytest.mark.parametrize("index_dtype,marker_dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_all_index_dtypes(index_dtype, marker_dtype):
    from recon_amd import PairGroups
    from recon_amd.pair_groups import distinct_counts
    for name in ("zero_and_distinct", "T37", "C72_k3", "tile_17"):
        sentence, markers, want = case(name)
        s, m = sentence.to(index_dtype), markers.to(marker_dtype)
        g = PairGroups.from_markers(s, m)
        assert not differences(g, want) and not compact_differences(g, s, m, want)
        assert g.sentence_d.dtype == g.markers_d.dtype == index_dtype
        assert torch.equal(distinct_counts(m).long(), torch.from_numpy(np.diff(want["seq_ptr"])))


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_wrong_variant_is_reported(variant):
    """Each wrong reading of the rule differs from the rule on at least one case, in a field `differences` names; the right reading on none."""
    seen = {}
    for name in CASE_NAMES[:12]:
        _, markers, want = case(name)
        assert not differences(restate(markers.numpy()), want)
        bad = differences(restate(markers.numpy(), variant), want)
        if bad:
            seen[name] = bad
    assert seen, variant
    field = {"across_sentences": "pair_seq", "highest_c": "seq_pair", "zero_only": "total", "ptr_off_by_one": "seq_ptr", "short_rows": "total"}[variant]
    assert any(field in bad for bad in seen.values()), (variant, seen)


def test_identity_and_to():
    from recon_amd import PairGroups
    g = PairGroups.identity(3, 4)
    assert g.total == 12 and torch.equal(g.seq_pair, torch.arange(12, dtype=torch.int32)) and torch.equal(g.pair_seq, g.seq_pair)
    assert g.seq_ptr.tolist() == [0, 4, 8, 12] and g.sentence_d is None
    rows = torch.randn(12, 5)
    assert torch.equal(g.expand(rows), rows.view(3, 4, 5))
    h = g.to("cpu")
    assert not differences(h, {"seq_pair": g.seq_pair.numpy().astype(np.int64), "pair_seq": g.pair_seq.numpy().astype(np.int64),
                               "seq_ptr": g.seq_ptr.numpy().astype(np.int64), "total": 12})
    assert "total=12" in repr(g)


@pytest.mark.parametrize("name,F", [("C72_k2", 1), ("C72_k3", 32), ("far_equal_nonzero", 513), ("tile_17", 7)])
def test_expand_and_its_backward_against_float64(name, F):
    from recon_amd import PairGroups
    sentence, markers, want = case(name)
    g = PairGroups.from_markers(sentence, markers)
    B, C = markers.shape[:2]
    gen = torch.Generator().manual_seed(F)
    rows = torch.randn(g.total, F, generator=gen, requires_grad=True)
    g_out = torch.randn(B, C, F, generator=gen)
    out = g.expand(rows)
    out.backward(g_out)
    ps = want["pair_seq"]
    assert torch.equal(out.detach().reshape(B * C, F), rows.detach()[torch.from_numpy(ps)])
    ref = torch.zeros(g.total, F, dtype=torch.float64)
    for p in range(B * C):                                               # plain loop, c ascending
        ref[ps[p]] += g_out.reshape(B * C, F)[p].double()
    err = (rows.grad.double() - ref).abs().max().item()
    print("expand backward %s F=%d: max abs err %.3e" % (name, F, err))
    assert err <= 72 * 2.0 ** -23 * ref.abs().max().item()            # at most 72 fp32 adds per element


def _gpgnn(name):
    from recon_amd.gpgnn import GPGNN
    g = load_golden(name)
    p = {"max_num_nodes": int(g["n"]), "embedding_dim": int(g["d"]), "layer_number": int(g["L"]), "projection_style": str(g["style"]),
         "non-linear1": "relu", "non-linear": "tanh", "dropout1": 0.0, "position_emb": 3, "units1": 4, "rnn1_layers": 1, "bidirectional": 1,
         "batch_size": int(g["B"])}
    m = GPGNN(p, g["emb"], max_sent_len=4, n_out=3)
    m.load_state_dict(state_dict_of(g), strict=False)
    return m.eval(), torch.from_numpy(g["sent"]), torch.from_numpy(g["mark"])


@pytest.mark.parametrize("name", ["gpgnn1_untied", "gpgnn2_tied_n9"])
def test_grouped_op_on_cpu_tensors_equals_the_dense_call_on_the_fixtures(name, monkeypatch):
    from recon_amd import PairGroups, pair_sentence_states, sentence_lstm
    from op_checks import calls_of
    m, sent, mark = _gpgnn(name)
    # the fixture's markers, and the same sentences with only the first pairs' rows kept (absent pairs: all-zero rows)
    sparse = mark.clone()
    sparse[:, 2:] = 0
    for markers in (mark, sparse):
        args = (m.rnn1, sent, markers, m.word_embedding.weight, m.pos_embedding.weight)
        with torch.no_grad():
            dense = pair_sentence_states(*args)
            g = PairGroups.from_markers(sent, markers)
            calls = calls_of(monkeypatch, sentence_lstm, "_chain")
            mapped = pair_sentence_states(*args, groups=g)
        assert calls == [1]                                              # the stock chain, over the compact copies
        assert mapped.shape == dense.shape
        assert g.total < markers.shape[0] * markers.shape[1] or markers is mark
        torch.testing.assert_close(mapped, dense, rtol=0, atol=1e-6)     # the same fp32 ops per row; MKL may block S_d rows otherwise than B C
        monkeypatch.undo()
    # the model: the switch changes nothing where the fused encoder does not apply (CPU tensors are outside `_fused`, inside the wiring)
    with torch.no_grad():
        off = m.encode(sent, sparse)
        m.distinct_pair_sequences = True
        on = m.encode(sent, sparse)
    torch.testing.assert_close(on, off, rtol=0, atol=1e-6)


def test_grouped_op_against_the_dense_float64_reference_with_gradients_and_factors():
    from recon_amd import PairGroups, pair_sentence_states
    markers = torch.from_numpy(entity_markers(2, 3, 8, seed=5))
    rnn, sentence, markers, word_table, pos_table, g_out = op_inputs(markers, 5, 3, 6)
    B, C, T = markers.shape
    g = PairGroups.from_markers(sentence, markers)
    assert g.total == 14
    factors = (torch.rand(g.total, 1, T, 5, generator=torch.Generator().manual_seed(2)) >= 0.5).float() * 2.0
    per_pair = factors[:, 0][g.pair_seq.long()].view(B, C, T, 5)
    for keep, dense_keep in ((None, None), (factors, per_pair)):
        ref = dense_reference(rnn, sentence, markers, word_table, pos_table, g_out, dense_keep)
        rnn.zero_grad()
        pt = pos_table.clone().requires_grad_(True)
        out = pair_sentence_states(rnn, sentence, markers, word_table, pt, keep, groups=g)
        out.backward(g_out)
        got = [out.detach(), pt.grad] + [p.grad for p in rnn.parameters()]
        for a, r in zip(got, ref):
            assert ((a.double() - r).abs().max() / r.abs().max()).item() <= 2e-5


def test_known_total():
    from recon_amd import PairGroups
    from recon_amd.pair_groups import known_total
    sentence, markers, want = case("C72_k3")
    with known_total(want["total"]):
        g = PairGroups.from_markers(sentence, markers)
        with known_total(None):                                          # an inner context overrides n; the outer one still reads
            assert PairGroups.from_markers(sentence, markers).total == want["total"]
        assert PairGroups.from_markers(sentence, markers).total == want["total"]
    assert not differences(g, want)
    with pytest.raises(ValueError, match="not the %d given" % (want["total"] + 1)):
        with known_total(want["total"] + 1):
            g = PairGroups.from_markers(sentence, markers)               # no raise here: the context's end reports it
            assert g.total == want["total"] + 1 and int(g.pair_seq.max()) < g.total and int(g.seq_pair.max()) < markers.shape[0] * markers.shape[1]
    with pytest.raises(ValueError, match="not the"):
        with known_total(want["total"] - 1):
            g = PairGroups.from_markers(sentence, markers)
            assert int(g.pair_seq.max()) < g.total
    with pytest.raises(ValueError, match="not the"):                     # outside a context: at once
        PairGroups.from_markers(sentence, markers, total=want["total"] - 1)
    with pytest.raises(KeyError):                                        # another exception goes on, and the context is left clean
        with known_total(want["total"] + 1):
            PairGroups.from_markers(sentence, markers)
            raise KeyError("x")
    assert PairGroups.from_markers(sentence, markers).total == want["total"]


class _EncoderAndHead(torch.nn.Module):
    """GPGNN's encoder with a linear head: what of the model runs on CPU tensors (the propagation has no CPU path)."""

    def __init__(self, gpgnn):
        super().__init__()
        self.gpgnn, self.head = gpgnn, torch.nn.Linear(8, 3)

    @property
    def distinct_pair_sequences(self):
        return self.gpgnn.distinct_pair_sequences

    def forward(self, sentence_input, entity_markers, num_entities=None):
        return self.head(self.gpgnn.encode(sentence_input, entity_markers)).view(-1, 3)


def test_run_epoch_enters_known_total_per_batch_and_not_at_all_with_the_switch_off(monkeypatch):
    from recon_amd import PairGroups, StageBData, run_epoch
    from recon_amd import pair_groups
    gp, sent, mark = _gpgnn("gpgnn1_untied")
    m = _EncoderAndHead(gp)
    B, C, T = mark.shape
    sparse = mark.clone()
    sparse[:, 2:] = 0
    N = 3 * B
    data = StageBData.from_indices((sent.repeat(3, 1).numpy(), sparse.repeat(3, 1, 1).numpy(), np.ones((N, C), dtype=np.int64), np.full(N, 2)))
    seen = []
    real = pair_groups.known_total
    monkeypatch.setattr(pair_groups, "known_total", lambda n: (seen.append(n), real(n))[1])
    calls = []
    real_from = PairGroups.from_markers.__func__
    monkeypatch.setattr(PairGroups, "from_markers", classmethod(lambda cls, *a, **k: (calls.append(1), real_from(cls, *a, **k))[1]))
    run_epoch(m, data, B)
    assert not seen and not calls and data._distinct_counts is None
    gp.distinct_pair_sequences = True
    run_epoch(m, data, B)
    per_batch = int(data.distinct_counts()[:B].sum())
    assert seen == [None] + [per_batch] * 3
    order = torch.arange(N - 1, -1, -1)
    run_epoch(m, data, B, order=order)
    assert seen[4:] == [None] + [per_batch] * 3


def test_rejections():
    from recon_amd import PairGroups, pair_sentence_states
    from recon_amd.pair_groups import distinct_counts, known_total
    sentence, markers, want = case("zero_and_distinct")
    B, C, T = markers.shape
    bad_calls = [
        lambda: PairGroups.from_markers(sentence, markers.float()),
        lambda: PairGroups.from_markers(sentence, markers[0]),
        lambda: PairGroups.from_markers(sentence, markers.to(torch.int16)),
        lambda: PairGroups.from_markers(sentence.to(torch.int8), markers),
        lambda: PairGroups.from_markers(sentence[:, :-1], markers),
        lambda: PairGroups.from_markers(sentence[:1], markers),
        lambda: PairGroups.from_markers(sentence, markers[:, :0]),
        lambda: PairGroups.from_markers(sentence, markers, total=B - 1),
        lambda: PairGroups.from_markers(sentence, markers, total=B * C + 1),
        lambda: PairGroups.from_markers(sentence, markers, total=7.0),
        lambda: PairGroups.from_markers(sentence, markers, total=True),
        lambda: distinct_counts(markers.float()),
        lambda: known_total(-1).__enter__(),
        lambda: known_total(2.5).__enter__(),
        lambda: PairGroups.identity(2, 0),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was accepted" % i)
    g = PairGroups.from_markers(sentence, markers)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    for make in (lambda: PairGroups(g.seq_pair.long(), g.pair_seq, g.seq_ptr, B, C, g.total),
                 lambda: PairGroups(g.seq_pair, g.pair_seq[:-1], g.seq_ptr, B, C, g.total),
                 lambda: PairGroups(g.seq_pair, g.pair_seq, g.seq_ptr[:-1], B, C, g.total),
                 lambda: PairGroups(g.seq_pair, g.pair_seq, g.seq_ptr, B, C, g.total + 1),
                 lambda: PairGroups(i32(0), i32(0, 0), i32(0, 1), 1, 2, 1, sentence_d=torch.zeros(1, 3, dtype=torch.int64)),
                 lambda: PairGroups(i32(0), i32(0, 0), i32(0, 1), 1, 2, 1, torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 3, dtype=torch.int64)),
                 lambda: g.expand(torch.zeros(g.total + 1, 3)),
                 lambda: g.expand(torch.zeros(g.total)),
                 lambda: g.compact(sentence[:1], markers[:1]),
                 lambda: g.compact(sentence, markers[:, :-1])):
        with pytest.raises(ValueError):
            make()
    rnn, s, mk, wt, pt, _ = op_inputs(markers, 5, 3, 4)
    with pytest.raises(ValueError, match="PairGroups or None"):
        pair_sentence_states(rnn, s, mk, wt, pt, groups="yes")
    with pytest.raises(ValueError, match="groups are over"):
        pair_sentence_states(rnn, s, mk, wt, pt, groups=PairGroups.identity(B, C + 1))
    with pytest.raises(ValueError, match="one draw"):
        pair_sentence_states(rnn, s, mk, wt, pt, torch.ones(B, C, T, 5), groups=g)
    from recon_amd.char_features import pack_keep
    with pytest.raises(ValueError, match="PackedKeep"):                  # B C rows where S_d are due
        pair_sentence_states(rnn, s, mk, wt, pt, pack_keep(torch.ones(B * C, T, 5) * 2.0, 2.0), groups=g)
    # an empty batch: nothing to group
    e = PairGroups.from_markers(sentence[:0], markers[:0])
    assert e.total == 0 and e.expand(torch.zeros(0, 4)).shape == (0, C, 4)
    assert pair_sentence_states(rnn, s[:0], mk[:0], wt, pt, groups=e).shape == (0, C, 8)
    assert distinct_counts(markers[:0]).shape == (0,)
