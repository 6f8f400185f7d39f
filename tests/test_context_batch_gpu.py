"""The stage-B entity-context batch through csrc/ctx_batch.hip (k_cb_index, k_cb_fill, k_cb_gat): the fixture recorded from the
reference's own functions, the smallest shapes at which each kernel can still go wrong, the kernels' id limit from both sides, the
reference's own [50, 72, 2], random batches against the torch-primitive path on the same device, guard rows around every buffer, two
runs bit for bit, the error flags, and a whole model fed with the batch.  Everything is compared exactly: nothing is computed."""
import numpy as np
import pytest
import torch

from context_batch_checks import (as_numpy, build, differences, expected, fixture, random_batch, random_dataset, restate, to_device)
from op_checks import calls_of, dev, state_dict_of
from conftest import load_golden

pytestmark = pytest.mark.gpu
MODES = (None, "all", "selected")
SENTINEL = {torch.int64: -7777, torch.int32: -7777, torch.float32: 12345.678, torch.bool: 0x5A}


def _paths(monkeypatch):
    from recon_amd.context_batch import ContextBatcher
    return calls_of(monkeypatch, ContextBatcher, "_batch_kernels"), calls_of(monkeypatch, ContextBatcher, "_batch_torch")


def _torch_path(batcher, *args, **kw):
    from recon_amd import context_batch
    prev, context_batch._KERNELS = context_batch._KERNELS, False
    try:
        return batcher.batch(*args, **kw)
    finally:
        context_batch._KERNELS = prev


@pytest.fixture(scope="module")
def fx():
    return fixture()


@pytest.fixture(scope="module")
def big():
    """One dataset at the reference's scale for the tests that need many entities: 600 entities with up to 31 lines, G = 100."""
    rng = np.random.default_rng(7)
    return random_dataset(rng, 600, 100), rng


@pytest.mark.parametrize("layout", ("wikidata", "nyt"))
def test_fixture_through_the_kernels(fx, layout, monkeypatch):
    from recon_amd import ContextBatcher
    ds, g = fx
    all_sf = np.concatenate([sf for _, sf in ds["batches"]], axis=0)
    for mode in MODES:
        tables, surface_ids = build(ds, layout, all_sf, mode)
        batcher = ContextBatcher(tables.to(dev()))
        kernels, stock = _paths(monkeypatch)
        for b, (ids, _) in enumerate(ds["batches"]):
            args = to_device(ids, surface_ids[3 * b:3 * b + 3], dev())
            if mode == "all" and bool(g["b%d.gat_all_keyerror" % b]):
                with pytest.raises(KeyError):
                    batcher.batch(*args)
                continue
            assert differences(as_numpy(batcher.batch(*args)), expected(g, layout, b, mode)) == [], (layout, mode, b)
            got32 = as_numpy(batcher.batch(*args, index_dtype=torch.int32))
            assert differences(got32, expected(g, layout, b, mode), index_dtype=np.int32) == [], (layout, mode, b)
        assert len(kernels) == 2 * len(ds["batches"]) - (mode == "all") and not stock


def _agree(batcher, args, want_kernels, monkeypatch, index_dtype=torch.int64):
    kernels, stock = _paths(monkeypatch)
    got = batcher.batch(*args, index_dtype=index_dtype)
    assert (len(kernels), len(stock)) == ((1, 0) if want_kernels else (0, 1))
    ref = _torch_path(batcher, *args, index_dtype=index_dtype)
    np_dtype = np.int32 if index_dtype == torch.int32 else np.int64
    assert got.context_words.dtype == index_dtype and got.context_chars.dtype == index_dtype
    assert differences(as_numpy(got), as_numpy(ref), index_dtype=np_dtype) == []
    return got


# (entities, lines at most, B, C, G, share of padding pairs, every id distinct, one-token surface forms)
SMALL = {"B1_C2": (9, 5, 1, 2, 3, 0.3, False, False), "U1": (9, 5, 2, 6, 3, 1.0, False, False), "distinct": (30, 5, 2, 6, 1, 0.0, True, False),
         "T1": (9, 0, 2, 3, 3, 0.3, False, True), "no_padding_G100": (30, 31, 3, 6, 100, 0.0, False, False), "G1_one_pair": (3, 31, 1, 1, 1, 0.0, False, False)}


@pytest.mark.parametrize("case", sorted(SMALL))
@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32))
def test_small_shapes(case, index_dtype, monkeypatch):
    from recon_amd import ContextBatcher
    n_ent, lines, B, Cn, G, pad, distinct, one_token = SMALL[case]
    rng = np.random.default_rng(sorted(SMALL).index(case))
    ds = random_dataset(rng, n_ent, G, max_lines=lines)
    ids, sf = random_batch(rng, ds, B, Cn, pad_share=pad, distinct=distinct, one_token=one_token)
    for mode in MODES:
        tables, surface_ids = build(ds, "wikidata", sf, mode)
        args = to_device(ids, surface_ids, dev())
        got = _agree(ContextBatcher(tables.to(dev())), args, True, monkeypatch, index_dtype)
        np_dtype = np.int32 if index_dtype == torch.int32 else np.int64
        assert differences(as_numpy(got), restate(ds, "wikidata", ids, sf, mode), index_dtype=np_dtype) == []
    if case == "U1":
        assert got.unique_entities.tolist() == [-1] and got.nonzero_entity_pos.numel() == 0
    if case == "T1":
        assert got.context_words.shape[2] == 1
    if case == "distinct":
        assert got.unique_entities.numel() == 2 * B * Cn + 1


def test_reference_batch_and_the_limit_from_both_sides(big, monkeypatch):
    from recon_amd import ContextBatcher
    from recon_amd.context_batch import MAX_IDS
    ds, rng = big
    shapes = [(50, 72, True), (MAX_IDS // 128, 64, True), (MAX_IDS // 128 + 1, 64, False)]          # 7200 ids; 8192: the limit; 8320: above it
    batches = [random_batch(rng, ds, B, Cn) for B, Cn, _ in shapes]
    for (B, Cn, in_kernels), (ids, sf) in zip(shapes, batches):
        tables, surface_ids = build(ds, "wikidata", sf, "selected")
        got = _agree(ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev()), in_kernels, monkeypatch)
        assert got.context_chars.shape[1:] == (32, 386) and got.unique_entities.numel() > 100
    assert ids.size == MAX_IDS + 128


def test_a_full_hash_table(monkeypatch):
    """MAX_IDS distinct ids: every slot of the LDS table is taken and U = MAX_IDS + 1."""
    from recon_amd import ContextBatcher
    from recon_amd.context_batch import MAX_IDS
    rng = np.random.default_rng(11)
    ds = random_dataset(rng, MAX_IDS + 8, 1, max_lines=1)
    ids, sf = random_batch(rng, ds, MAX_IDS // 128, 64, distinct=True, one_token=True)
    tables, surface_ids = build(ds, "wikidata", sf, "all")
    got = _agree(ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev()), True, monkeypatch, torch.int32)
    assert got.unique_entities.numel() == MAX_IDS + 1


def test_random_batches_kernels_against_the_torch_path(monkeypatch):
    from recon_amd import ContextBatcher
    rng = np.random.default_rng(99)
    for trial in range(20):
        B, Cn, G = int(rng.choice([1, 3, 7, 20])), int(rng.choice([2, 6, 12])), int(rng.choice([1, 3, 100]))
        mode = MODES[trial % 3]
        layout = ("wikidata", "nyt")[trial % 2]
        ds = random_dataset(rng, int(rng.choice([5, 40, 200])), G, max_lines=int(rng.choice([0, 7, 31])), layout=layout)
        ids, sf = random_batch(rng, ds, B, Cn, pad_share=float(rng.choice([0.0, 0.3])))
        tables, surface_ids = build(ds, layout, sf, mode)
        _agree(ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev()), True, monkeypatch, (torch.int64, torch.int32)[trial % 2])


@pytest.mark.parametrize("index_dtype", (torch.int64, torch.int32))
def test_every_cell_is_written_and_nothing_outside(big, index_dtype, monkeypatch):
    """Every buffer of a call lies inside sentinel-filled memory, behind a guard of 37 elements (so no base is 16-byte aligned) and in
    front of another: the guards stay, and the outputs equal the torch path's, so no cell kept its sentinel."""
    from recon_amd import ContextBatcher, context_batch
    ds, rng = big
    ids, sf = random_batch(rng, ds, 5, 6)
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    batcher, args = ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev())
    ref = as_numpy(_torch_path(batcher, *args, index_dtype=index_dtype))
    held, guard = [], 37

    def guarded(shape, dtype, device):
        n = int(np.prod(shape))
        raw = torch.uint8 if dtype == torch.bool else dtype
        flat = torch.full((n + 2 * guard,), SENTINEL[dtype], dtype=raw, device=device)
        held.append((flat, n, dtype))
        inner = flat[guard:guard + n]
        return (inner.view(torch.bool) if dtype == torch.bool else inner).view(shape)
    monkeypatch.setattr(context_batch, "_new", guarded)
    kernels, stock = _paths(monkeypatch)
    got = batcher.batch(*args, index_dtype=index_dtype)
    assert len(kernels) == 1 and not stock and len(held) >= 10
    for flat, n, dtype in held:
        sentinel = torch.full((guard,), SENTINEL[dtype], dtype=flat.dtype, device=flat.device)
        assert torch.equal(flat[:guard], sentinel) and torch.equal(flat[guard + n:], sentinel), (dtype, n)
    assert got.context_chars.data_ptr() % 16 != 0
    assert int(got.context_mask.view(torch.uint8).max()) <= 1
    assert differences(as_numpy(got), ref, index_dtype=np.int32 if index_dtype == torch.int32 else np.int64) == []


def test_two_runs_give_the_same_bits(big):
    from recon_amd import ContextBatcher
    ds, rng = big
    ids, sf = random_batch(rng, ds, 20, 12)
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    batcher, args = ContextBatcher(tables.to(dev())), to_device(ids, surface_ids, dev())
    assert differences(as_numpy(batcher.batch(*args)), as_numpy(batcher.batch(*args))) == []


def test_bad_input_raises_and_nothing_faults(fx):
    """The flags come from the header; a flagged value is never an address, and the device is fine afterwards."""
    from recon_amd import ContextBatcher
    ds, g = fx
    ids, sf = ds["batches"][0]
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    batcher = ContextBatcher(tables.to(dev()))
    ok = to_device(ids, surface_ids, dev())
    for value in (tables.dims["Ne"], -2, 2 ** 40, -2 ** 40, tables.dims["Ne"] - 2):              # (Ne - 2: the id init_random leaves to nobody)
        bad = ok[0].clone()
        bad[2, 1, 0] = value
        with pytest.raises(IndexError):
            batcher.batch(bad, ok[1])
    for value in (tables.dims["S"], -1, 2 ** 31 - 1):
        bad = ok[1].clone()
        bad[0, 3, 1] = value
        with pytest.raises(IndexError):
            batcher.batch(ok[0], bad)
    wide = ok[1].to(torch.int64)
    wide[1, 0, 0] = 2 ** 32 + 1                                         # would wrap into the table as an int32
    with pytest.raises(IndexError):
        batcher.batch(ok[0], wide)
    half = ok[0].clone()
    half[0, 0, 1] = -1
    with pytest.raises(ValueError):
        batcher.batch(half, ok[1])
    torch.cuda.synchronize()
    assert differences(as_numpy(batcher.batch(*ok)), expected(g, "wikidata", 0, "selected")) == []


def test_a_whole_model_fed_with_the_batch(monkeypatch):
    """RECON with the whole-model fixture's weights, fed once with batch.model_args() from the kernels and once with the arrays of the
    plain-loop restatement: the same logits, bit for bit, because the inputs are identical.  The shell is built with
    entity_conv_filter_size = 1, the reference's own setting (model_params.json), under which context_mask is [U, P_b] as
    get_mask writes it; the fixture's line conv is 2 wide, so that one weight keeps its seeded initial value."""
    from recon_amd import ContextBatcher
    from recon_amd.gpgnn import RECON
    from tests.test_host_cpu import KGGAT_P, recon_constructor_tables
    g = load_golden("recon1_untied")
    torch.manual_seed(0)
    m = RECON(dict(KGGAT_P, entity_conv_filter_size=1), g["emb"], 4, 3, list(range(int(g["n_chars"]))), *recon_constructor_tables(g))
    own = m.state_dict()
    m.load_state_dict({k: v for k, v in state_dict_of(g).items() if k in own and own[k].shape == v.shape}, strict=False)
    m.eval().to(dev())
    rng = np.random.default_rng(5)
    ds = random_dataset(rng, 9, 3, max_lines=5, n_words=g["emb"].shape[0], n_chars=int(g["n_chars"]), conv_filter_size=KGGAT_P["conv_filter_size"])
    ids, sf = random_batch(rng, ds, 4, 6, pad_share=0.3)
    tables, surface_ids = build(ds, "wikidata", sf, "selected", max_char_len=KGGAT_P["max_char_len"])
    kernels, stock = _paths(monkeypatch)
    batch = ContextBatcher(tables.to(dev())).batch(*to_device(ids, surface_ids, dev()))
    assert len(kernels) == 1 and not stock
    r = restate(ds, "wikidata", ids, sf, "selected", max_char_len=KGGAT_P["max_char_len"])
    t = lambda k: torch.from_numpy(r[k]).to(dev())
    sent, mark = torch.from_numpy(g["sent"]).to(dev()), torch.from_numpy(g["mark"]).to(dev())
    with torch.no_grad():
        fed = m(sent, mark, None, *batch.model_args())
        recorded = m(sent, mark, None, t("unique"), torch.from_numpy(ids).to(dev()), t("words"), t("chars"), t("mask"), t("pos"), r["max_pos"],
                     t("nz"), t("nz_pos"), t("gat"))
    assert fed.shape == (24, 3) and torch.isfinite(fed).all() and torch.equal(fed, recorded)
