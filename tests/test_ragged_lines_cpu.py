"""Ragged stage-B batches without a GPU: `recon_amd.RaggedLines`, the torch path of
`ContextBatcher.batch(..., ragged_lines=True)` on the fixture recorded from the reference's own functions, `entity_line_pool_ragged` on
CPU tensors against `entity_line_pool` on the padded form bit for bit, `EntityEmbedding.forward` with a RaggedLines, the argument
errors, the status codes and shape queries of the C ABI, the header / `_lib.SYMBOLS` check, and the guard of the comparison that
tests/test_ragged_lines_gpu.py holds the kernels to (tests/ragged_lines_checks.py has the cases and the rules)."""
import numpy as np
import pytest
import torch

from context_batch_checks import as_numpy, build, expected, fixture
from op_checks import close, entries_declared_and_bound
from ragged_lines_checks import (CASES, CITES, ENCODER_COUNTS, ENTRIES, FILL_CITES, FILL_ENTRY, MAX_TIE_SHARE, REFUSED, WRONG, applies, case, encoder,
                                 encoder_inputs, failures, groups_of, line_ptr_of, mask_of, pad_rows, restate, run, tie_case)


def test_import():
    from recon_amd import RaggedLines, entity_line_pool_ragged
    from recon_amd.line_pool import entity_line_pool_ragged as same
    from recon_amd.ragged_lines import RaggedLines as same_class
    assert entity_line_pool_ragged is same and RaggedLines is same_class


# ------------------------------------------------------------------------------------------------------------- the holder
@pytest.mark.parametrize("counts", ([1], [0], [0, 3, 1, 0], [5, 1, 32, 2], [], [0, 0]), ids=str)
def test_ragged_lines_round_trips(counts):
    from recon_amd import RaggedLines
    lines = RaggedLines.from_counts(counts)
    U, L, n_max = len(counts), sum(counts), max(counts) if counts else 0
    assert (lines.U, lines.total, lines.n_max) == (U, L, n_max)
    assert lines.line_ptr.dtype == torch.int32 and lines.line_ptr.tolist() == line_ptr_of(counts)
    assert lines.counts().tolist() == counts
    also = RaggedLines.from_counts(torch.tensor(counts, dtype=torch.int64))
    assert also.line_ptr.tolist() == lines.line_ptr.tolist() and (also.U, also.total, also.n_max) == (U, L, n_max)
    for P in (n_max, n_max + 3):
        mask = lines.to_mask(P)
        assert mask.dtype == torch.bool and torch.equal(mask, mask_of(counts, P))
        back = RaggedLines.from_mask(mask)
        assert back.line_ptr.tolist() == lines.line_ptr.tolist() and (back.U, back.total, back.n_max) == (U, L, n_max)
        rows = torch.arange(1, L * 6 + 1, dtype=torch.float32).view(L, 2, 3)
        padded = lines.pad(rows, P)
        assert padded.shape == (U, P, 2, 3) and torch.equal(padded, pad_rows(counts, rows, P))
        if U:
            assert torch.equal(padded[~mask], rows) and torch.count_nonzero(padded[mask]) == 0      # the rows under ~mask, in order; zeros elsewhere
        for k in (1, 2, 3):
            if P - k + 1 >= 0:
                assert torch.equal(lines.to_mask(P, k), mask_of(counts, P, k))
    ids = torch.arange(L, dtype=torch.int64).view(L, 1)                  # integer rows pad too (the stock-op fallbacks pad ids)
    assert torch.equal(lines.pad(ids, n_max), pad_rows(counts, ids, n_max))


def test_pad_is_differentiable():
    from recon_amd import RaggedLines
    lines = RaggedLines.from_counts([2, 0, 1])
    rows = torch.randn(3, 4, requires_grad=True)
    w = torch.randn(3, 5, 4)
    (lines.pad(rows, 5) * w).sum().backward()
    assert torch.equal(rows.grad, torch.stack([w[0, 0], w[0, 1], w[2, 0]]))


def test_ragged_lines_errors():
    from recon_amd import RaggedLines
    mask = torch.tensor([[False, False, True], [False, True, False]])   # a present line behind a padding line
    with pytest.raises(ValueError, match="prefix"):
        RaggedLines.from_mask(mask)
    with pytest.raises(ValueError, match="prefix"):
        RaggedLines.from_mask(torch.tensor([[True, False]]))
    for bad in (lambda: RaggedLines.from_mask(mask.float()), lambda: RaggedLines.from_mask(mask[0]), lambda: RaggedLines.from_counts([1, -1]),
                lambda: RaggedLines.from_counts(torch.tensor([1.0])), lambda: RaggedLines(torch.zeros(3, dtype=torch.int64), 2, 0, 0),
                lambda: RaggedLines(torch.zeros(3, dtype=torch.int32), 3, 0, 0), lambda: RaggedLines(torch.zeros(3, dtype=torch.int32), 2, 5, 2),
                lambda: RaggedLines.from_counts([2, 1]).pad(torch.zeros(4, 2), 2), lambda: RaggedLines.from_counts([2, 1]).pad(torch.zeros(3, 2), 1),
                lambda: RaggedLines.from_counts([2, 1]).to_mask(1, 3)):
        with pytest.raises(ValueError, match="RaggedLines"):
            bad()


# ------------------------------------------------------------------------------------------------------------- the batcher's torch path
def _torch_path(batcher, *args, **kw):
    from recon_amd import context_batch
    prev, context_batch._KERNELS = context_batch._KERNELS, False
    try:
        return batcher.batch(*args, **kw)
    finally:
        context_batch._KERNELS = prev


def ragged_differences(ragged, padded, index_dtype=np.int64):
    """What a ragged batch (as_numpy + its RaggedLines) must be beside the padded arrays of the same ids: the rows under ~mask, exactly,
    line_ptr the cumulative sum of the mask's row counts, L = line_ptr[U], every other field equal.  `padded` is a dict over FIELDS."""
    got, lines = ragged
    bad = []
    mask = np.asarray(padded["mask"])
    counts = (~mask).sum(1)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    if lines.line_ptr.dtype != torch.int32 or lines.line_ptr.cpu().numpy().tolist() != ptr.tolist():
        bad.append("line_ptr")
    if (lines.U, lines.total, lines.n_max) != (mask.shape[0], int(ptr[-1]), int(counts.max())):
        bad.append("sizes")
    for f in ("words", "chars"):
        want = np.asarray(padded[f])[~mask].astype(index_dtype)
        a = np.asarray(got[f])
        if a.shape != want.shape or a.dtype != want.dtype or a.tobytes() != want.tobytes():
            bad.append(f)
    for f in ("unique", "pos", "gat", "nz", "nz_pos"):
        a, b = got[f], padded[f]
        if (a is None) != (b is None) or (a is not None and (np.asarray(a).shape != np.asarray(b).shape or np.asarray(a).tobytes() != np.asarray(b).tobytes())):
            bad.append(f)
    if got["max_pos"] != padded["max_pos"]:
        bad.append("max_pos")
    return bad


def ragged_numpy(batch):
    """(as_numpy of the batch with its mask left out, the RaggedLines)."""
    lines, batch.context_mask = batch.context_mask, None
    try:
        return as_numpy(batch), lines
    finally:
        batch.context_mask = lines


@pytest.mark.parametrize("layout", ("wikidata", "nyt"))
@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32), ids=("int64", "int32"))
def test_the_torch_path_on_the_fixture(layout, index_dtype):
    from recon_amd import ContextBatcher, RaggedLines
    ds, g = fixture()
    all_sf = np.concatenate([sf for _, sf in ds["batches"]], axis=0)
    np_dtype = np.int32 if index_dtype == torch.int32 else np.int64
    seen = 0
    for mode in (None, "selected"):
        tables, surface_ids = build(ds, layout, all_sf, mode)
        batcher = ContextBatcher(tables)
        for b, (ids, _) in enumerate(ds["batches"]):
            args = (torch.from_numpy(np.ascontiguousarray(ids)), torch.from_numpy(np.ascontiguousarray(surface_ids[3 * b:3 * b + 3])))
            batch = _torch_path(batcher, *args, index_dtype=index_dtype, ragged_lines=True)
            assert isinstance(batch.context_mask, RaggedLines) and batch.model_args()[4] is batch.context_mask
            assert batch.context_words.dim() == 2 and batch.context_chars.dim() == 2 and batch.context_words.dtype == index_dtype
            assert batch.context_words.shape[0] == batch.context_chars.shape[0] == batch.context_mask.total == int(batch.context_mask.line_ptr[-1])
            assert ragged_differences(ragged_numpy(batch), expected(g, layout, b, mode), np_dtype) == [], (layout, mode, b)
            padded = _torch_path(batcher, *args, index_dtype=index_dtype)                    # the default is the padded form, as before
            assert padded.context_mask.dtype == torch.bool and padded.context_words.dim() == 3
            seen += int((~padded.context_mask).sum() < padded.context_mask.numel())
    assert seen > 0                                                      # the fixture has padding lines to leave out


def test_the_comparison_of_ragged_batches_bites():
    from recon_amd import ContextBatcher, RaggedLines
    ds, g = fixture()
    ids, sf = ds["batches"][0]
    tables, surface_ids = build(ds, "wikidata", sf, None)
    args = (torch.from_numpy(np.ascontiguousarray(ids)), torch.from_numpy(np.ascontiguousarray(surface_ids)))
    batch = _torch_path(ContextBatcher(tables), *args, ragged_lines=True)
    want = expected(g, "wikidata", 0, None)
    got, lines = ragged_numpy(batch)
    assert ragged_differences((got, lines), want) == []
    rolled = dict(got, words=np.roll(got["words"], 1, axis=0))
    assert ragged_differences((rolled, lines), want) == ["words"]
    short = dict(got, chars=got["chars"][:-1])
    assert ragged_differences((short, lines), want) == ["chars"]
    ptr = lines.line_ptr.clone()
    ptr[1] += 1
    assert ragged_differences((got, RaggedLines(ptr, lines.U, lines.total, lines.n_max)), want) == ["line_ptr"]
    assert ragged_differences((got, RaggedLines(lines.line_ptr, lines.U, lines.total, lines.n_max + 1)), want) == ["sizes"]


# ------------------------------------------------------------------------------------------------------------- the pool on the CPU
def _ragged(counts, device="cpu"):
    from recon_amd import RaggedLines
    return RaggedLines.from_counts(counts, device)


@pytest.mark.parametrize("name", sorted(CASES) + ["refused"])
def test_cpu_tensors_equal_the_padded_call_bit_for_bit(name):
    from recon_amd import entity_line_pool, entity_line_pool_ragged
    c = case(name)
    counts, k = c["counts"], c["k"]
    lines = _ragged(counts)
    Ln = max(max(counts), k)
    got = run(lambda s, w, b: entity_line_pool_ragged(s, lines, w, b), c)
    want = run(lambda s, w, b: entity_line_pool(lines.pad(s, Ln), w, b, lines.to_mask(Ln, k)), c)
    assert got[0].shape == (len(counts), c["E"]) and got[1].shape == c["states"].shape
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    short = torch.tensor([n < k for n in counts])
    assert (got[0][short] == -float('inf')).all() and torch.isfinite(got[0][~short]).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_near_ties_are_rare(name):
    c = case(name)
    share = c["ties"].float().mean().item()
    print("entity_line_pool_ragged %s: %d of %d cells near a tie" % (name, int(c["ties"].sum()), c["ties"].numel()))
    assert share <= MAX_TIE_SHARE, share


@pytest.mark.parametrize("name", sorted(CASES))
def test_fp32_restatement_passes_the_comparison_and_wrong_ones_are_reported(name):
    c = case(name)
    args = (c["counts"], c["states"], c["weight"], c["bias"], c["g_out"])
    good = restate(*args)
    assert not failures(good, good, c["ref"], "%s stand-in" % name)
    for wrong in WRONG:
        if applies(wrong, c):
            assert failures(restate(*args, wrong), good, c["ref"], "%s %s" % (name, wrong)), "%s is not reported at %s" % (wrong, name)


def test_every_wrong_restatement_applies_somewhere():
    for wrong in WRONG[:-1]:
        assert sum(applies(wrong, case(name)) for name in CASES) >= 3, wrong


def test_an_exact_tie_takes_the_lowest_position():
    c = tie_case()
    args = (c["counts"], c["states"], c["weight"], c["bias"], c["g_out"])
    good = restate(*args)
    assert not failures(good, good, c["ref"], "exact tie stand-in")
    for a, r in zip(good, c["ref"]):
        assert torch.equal(a.double(), r)
    bad = failures(restate(*args, "the highest position on a tie"), good, c["ref"], "exact tie, the highest position")
    assert [b[0] for b in bad] == ["d_states"], bad                      # (d_weight reads equal lines at either position)
    from recon_amd import entity_line_pool_ragged
    lines = _ragged(c["counts"])
    got = run(lambda s, w, b: entity_line_pool_ragged(s, lines, w, b), c)
    for a, r in zip(got, c["ref"]):
        assert torch.equal(a.double(), r)


def test_argument_errors():
    from recon_amd import entity_line_pool_ragged
    c = case("fixture_widths")
    s, w, b, lines = c["states"], c["weight"], c["bias"], _ragged(c["counts"])
    bad = [lambda: entity_line_pool_ragged(s[None], lines, w, b),         # not [L, C]
           lambda: entity_line_pool_ragged(s, lines, w[0], b),
           lambda: entity_line_pool_ragged(s, lines, w[:, :5], b),        # C of the states and of the filters differ
           lambda: entity_line_pool_ragged(s[:-1], lines, w, b),          # not the batch's L rows
           lambda: entity_line_pool_ragged(s, lines, w, b[:1]),
           lambda: entity_line_pool_ragged(s, lines, w.double(), b),
           lambda: entity_line_pool_ragged(s.long(), lines, w, b),
           lambda: entity_line_pool_ragged(s, lines.to_mask(32), w, b),   # a mask where the RaggedLines belongs
           lambda: entity_line_pool_ragged(s, None, w, b),
           lambda: entity_line_pool_ragged(s.numpy(), lines, w, b)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError, match="entity_line_pool_ragged"):
            f()
            pytest.fail("case %d raised nothing" % i)
    with pytest.raises(ValueError, match=r"L = 40 rows.*\(39, 6\)"):       # the shapes are in the text
        entity_line_pool_ragged(s[:-1], lines, w, b)


# ------------------------------------------------------------------------------------------------------------- the library's queries
def test_shape_queries():
    from recon_amd import _lib
    L = _lib.lib()
    ok, ws = L.recon_line_pool_ragged_supported, L.recon_line_pool_ragged_workspace_bytes
    for counts, C, E, k in CASES.values():
        assert ok(len(counts), sum(counts), max(counts), C, E, k)
    counts, C, E, k = REFUSED
    assert not ok(len(counts), sum(counts), max(counts), C, E, k)
    assert ok(450, 14400, 32, 100, 8, 1) and ok(450, 2000, 32, 100, 8, 1) and ok(0, 0, 0, 100, 8, 1) and ok(3, 0, 0, 4, 2, 1) and ok(3, 2, 1, 4, 2, 5)
    assert ok(1, 258, 258, 256, 64, 4) and not ok(1, 259, 259, 256, 64, 4)                 # 255 and 256 windows
    assert not ok(5, 40, 32, 1025, 8, 1) and not ok(5, 40, 32, 513, 8, 2) and not ok(5, 40, 32, 100, 65, 1) and not ok(5, 40, 32, 100, 0, 1)
    assert not ok(5, 40, 32, 0, 8, 1) and not ok(5, 40, 32, 100, 8, 0) and not ok(-1, 0, 0, 4, 2, 1) and not ok(5, -1, 0, 4, 2, 1)
    assert not ok(5, 40, 41, 4, 2, 1) and not ok(5, 40, 7, 4, 2, 1) and not ok(1, 2 ** 31, 2 ** 31 - 1, 4, 2, 1)      # n_max > L; L > U n_max; 2^31 rows
    for C, E, k in ((100, 8, 1), (4, 5, 2)):
        slab = E * (C * k + 1) * 4
        for U in (1, 2, 255, 256, 257, 450, 1029):
            G, per = groups_of(U)
            assert ws(U, 3 * U, 3, C, E, k) == -(-G * slab // 16) * 16 == L.recon_line_pool_workspace_bytes(U, 4, C, E, k), U
    assert ws(0, 0, 0, 100, 8, 1) == 0 and ws(1, 256, 256, 8, 4, 1) == 0


def test_status_codes_before_any_launch():
    from recon_amd import _lib
    L = _lib.lib()
    fake = 16                                                            # never dereferenced: every call returns before a launch
    fwd = lambda U, Lr, n_max, k, ld=6: L.recon_line_pool_ragged_fwd(fake, ld, fake, fake, fake, U, Lr, n_max, 6, 2, k, fake, fake, None)
    assert fwd(0, 0, 0, 2) == 0 and fwd(-1, 0, 0, 2) == -1 and fwd(3, -1, 0, 2) == -1 and fwd(3, 4, 2, 0) == -1
    assert fwd(1, 256, 256, 1) == -2 and fwd(3, 40, 7, 1) == -2 and fwd(3, 4, 2, 2, ld=5) == -1
    assert L.recon_line_pool_ragged_fwd(fake, 6, fake, fake, None, 3, 4, 2, 6, 2, 2, fake, fake, None) == -1       # no line_ptr
    assert L.recon_line_pool_ragged_fwd(None, 6, fake, fake, fake, 3, 4, 2, 6, 2, 2, fake, fake, None) == -1       # rows, but no states
    bwd = lambda U, Lr, n_max, k, nbytes: L.recon_line_pool_ragged_bwd(fake, 6, fake, fake, fake, fake, U, Lr, n_max, 6, 2, k, fake, fake, fake, fake,
                                                                       nbytes, None)
    assert bwd(3, 4, 2, 0, 1 << 20) == -1 and bwd(1, 256, 256, 1, 1 << 20) == -2 and bwd(3, 4, 2, 2, 16) == -4
    assert L.recon_line_pool_ragged_bwd(fake, 6, fake, fake, fake, fake, 3, 4, 2, 6, 2, 2, None, None, None, None, 0, None) == 0       # nothing wanted
    assert L.recon_line_pool_ragged_bwd(fake, 6, fake, fake, fake, None, 3, 4, 2, 6, 2, 2, fake, None, None, None, 0, None) == -1      # no line_ptr
    # recon_ctx_batch_fill_ragged: the sizes are checked in front of the tables
    fill = lambda U, Lr, P, T, ib: L.recon_ctx_batch_fill_ragged(None, None, fake, fake, U, Lr, P, T, ib, fake, fake, fake, fake, None)
    assert fill(0, 0, 4, 3, 8) == -1 and fill(3, 2, 4, 3, 8) == -1 and fill(3, 13, 4, 3, 8) == -1 and fill(3, 5, 4, 3, 2) == -1 and fill(3, 5, 4, 3, 8) == -1
    assert L.recon_ctx_batch_fill_ragged(None, None, fake, fake, 3, 5, 4, 3, 8, fake, fake, None, fake, None) == -1


def test_the_entries_are_declared_bound_and_cite_the_reference():
    entries_declared_and_bound(ENTRIES, CITES)
    entries_declared_and_bound(FILL_ENTRY, FILL_CITES)


# ------------------------------------------------------------------------------------------------------------- the encoder
@pytest.mark.parametrize("L", sorted(ENCODER_COUNTS))
@pytest.mark.parametrize("fused", (True, False), ids=("pool_op", "stock_pool"))
def test_entity_embedding_takes_a_ragged_batch(L, fused):
    """CPU tensors run the stock ops on either form: the ragged call's output and parameter gradients are the padded call's within the
    project's parity bound (a row's sums do not depend on the other rows, the batched products' blocking may)."""
    counts = ENCODER_COUNTS[L]
    lines = _ragged(counts)
    words, chars = encoder_inputs(counts)
    P = max(counts)
    grads = []
    for ragged in (True, False):
        m = encoder().eval()
        m.fused_line_pool = fused
        out = m(words, chars, lines) if ragged else m(lines.pad(words, P), lines.pad(chars, P), lines.to_mask(P))
        assert out.shape == (len(counts), 2)
        g = torch.Generator().manual_seed(3)
        gout = torch.randn(out.shape, generator=g)
        finite = torch.isfinite(out.detach())
        (out.masked_fill(~finite, 0.0) * gout).sum().backward()
        grads.append([out.detach().masked_fill(~finite, 0.0), finite] + [p.grad for p in m.parameters() if p.requires_grad])
    assert torch.equal(grads[0][1], grads[1][1]) and grads[0][1].sum() == 2 * sum(n > 0 for n in counts)
    for a, b in zip(grads[0], grads[1]):
        close(a.float(), b.float(), what="EntityEmbedding L = %d" % L)


def test_entity_embedding_other_branches_and_errors():
    """An embedding that is not a plain nn.Embedding and an entity convolution that is not plain run the stock ops on L rows and pad in
    front of the stock pool."""
    from torch import nn
    counts = ENCODER_COUNTS[15]
    lines, (words, chars) = _ragged(counts), encoder_inputs(counts)
    want = encoder(ecfs=2).eval()(lines.pad(words, 8), lines.pad(chars, 8), lines.to_mask(8, 2))

    class Table(nn.Embedding):
        pass

    class Conv(nn.Conv1d):
        pass
    m = encoder(ecfs=2).eval()
    m.word_embeddings.__class__ = Table
    got = m(words, chars, lines)
    assert torch.equal(torch.isinf(got), torch.isinf(want)) and torch.isinf(got[1]).all()
    close(got.masked_fill(torch.isinf(got), 0.0), want.masked_fill(torch.isinf(want), 0.0), what="a subclassed word table")
    m = encoder(ecfs=2).eval()
    m.conv1d_entity.__class__ = Conv
    got = m(words, chars, lines)
    assert torch.equal(torch.isinf(got), torch.isinf(want))
    close(got.masked_fill(torch.isinf(got), 0.0), want.masked_fill(torch.isinf(want), 0.0), what="a subclassed entity convolution")
    with pytest.raises(ValueError, match="RaggedLines"):
        m(lines.pad(words, 8), lines.pad(chars, 8), lines)
    with pytest.raises(ValueError, match="RaggedLines"):
        m(words[:-1], chars[:-1], lines)
