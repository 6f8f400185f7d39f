"""The stage-B entity-context batch (recon_amd/context_batch.py) on the host: the public call on CPU tensors (the torch-primitive path) and
the plain-loop restatement against tests/golden/context_batch1.npz, recorded from the reference's own functions; the two against each
other on random batches; the guards that show the fixture can fail; the builder's errors; the C ABI's entries and status codes."""
import sys

import numpy as np
import pytest
import torch

from context_batch_checks import (WRONG, as_numpy, build, differences, expected, fixture, random_batch, random_dataset, restate, to_device)
from op_checks import entries_declared_and_bound

ENTRIES = ["recon_ctx_batch_supported", "recon_ctx_batch_index", "recon_ctx_batch_fill", "recon_ctx_batch_gat"]
MODES = (None, "all", "selected")
LAYOUTS = ("wikidata", "nyt")


@pytest.fixture(scope="module")
def fx():
    return fixture()


def _recorded(g, b, mode):
    return not (mode == "all" and bool(g["b%d.gat_all_keyerror" % b]))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_public_call_on_cpu_tensors_meets_the_fixture(fx, layout, mode):
    from recon_amd import ContextBatcher
    ds, g = fx
    all_sf = np.concatenate([sf for _, sf in ds["batches"]], axis=0)
    tables, surface_ids = build(ds, layout, all_sf, mode)
    assert surface_ids.shape == (15, 6, 2) and surface_ids.dtype == np.int32
    batcher = ContextBatcher(tables)
    for b, (ids, _) in enumerate(ds["batches"]):
        args = to_device(ids, surface_ids[3 * b:3 * b + 3], "cpu")
        if not _recorded(g, b, mode):
            with pytest.raises(KeyError):                              # the reference raises KeyError on this batch as well
                batcher.batch(*args)
            continue
        assert differences(as_numpy(batcher.batch(*args)), expected(g, layout, b, mode)) == [], (layout, mode, b)
        got32 = as_numpy(batcher.batch(*args, index_dtype=torch.int32))
        assert differences(got32, expected(g, layout, b, mode), index_dtype=np.int32) == []


def test_the_fixture_holds_the_cases_it_is_there_for(fx):
    ds, g = fx
    u = lambda b: g["wikidata.b%d.unique" % b]
    assert g["wikidata.b0.words"].shape[1:] == (32, 32) and g["wikidata.b2.words"].shape[2] < 32            # P_b = 32, T_b = 32; a short batch
    assert list(u(1)) == [-1] and g["b1.nz_pos"].size == 0 and g["b1.nz"].shape == (0, 6)                   # all padding
    assert int(g["wikidata.b3.max_pos"]) > 0 and len(u(4)) == 37                                             # not -1; every id distinct (+ -1)
    assert bool(g["b4.gat_all_keyerror"]) and not bool(g["b0.gat_all_keyerror"])
    assert list(u(0)) != sorted(u(0))
    assert g["wikidata.b0.chars"].dtype == np.int64 and g["wikidata.b0.mask"].dtype == bool and g["b0.gat_sel"].dtype == np.float32


@pytest.mark.parametrize("layout", LAYOUTS)
def test_restatement_meets_the_fixture(fx, layout):
    ds, g = fx
    for b, (ids, sf) in enumerate(ds["batches"]):
        for mode in MODES:
            if _recorded(g, b, mode):
                assert differences(restate(ds, layout, ids, sf, mode), expected(g, layout, b, mode)) == [], (b, mode)
    with pytest.raises(KeyError):
        restate(ds, layout, ds["batches"][4][0], ds["batches"][4][1], "all")


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_restatement_is_caught_by_the_fixture(fx, wrong):
    ds, g = fx
    caught = []
    for b, (ids, sf) in enumerate(ds["batches"]):
        caught += differences(restate(ds, "wikidata", ids, sf, "selected", wrong=wrong), expected(g, "wikidata", b, "selected"))
    assert caught, wrong


def test_random_batches_restatement_against_the_torch_path():
    from recon_amd import ContextBatcher
    rng = np.random.default_rng(20240527)
    seen_u1 = 0
    for trial in range(200):
        B, Cn, G = int(rng.choice([1, 2, 3, 5])), int(rng.choice([2, 3, 6])), int(rng.choice([1, 3, 4]))
        mode, layout = MODES[trial % 3], LAYOUTS[trial % 2]
        ds = random_dataset(rng, int(rng.choice([3, 9, 30])), G, max_lines=int(rng.choice([0, 5, 31])), layout=layout)
        ids, sf = random_batch(rng, ds, B, Cn, pad_share=float(rng.choice([0.0, 0.3, 1.0])))
        tables, surface_ids = build(ds, layout, sf, mode)
        dtype = (torch.int64, torch.int32)[trial % 2]
        got = as_numpy(ContextBatcher(tables).batch(*to_device(ids, surface_ids, "cpu"), index_dtype=dtype))
        want = restate(ds, layout, ids, sf, mode)
        assert differences(got, want, index_dtype=np.int32 if dtype == torch.int32 else np.int64) == [], trial
        seen_u1 += len(want["unique"]) == 1
    assert seen_u1 > 0


def test_public_call_rejects_bad_input(fx):
    from recon_amd import ContextBatcher
    ds, g = fx
    ids, sf = ds["batches"][0]
    tables, surface_ids = build(ds, "wikidata", sf, "selected")
    batcher = ContextBatcher(tables)
    ok = to_device(ids, surface_ids, "cpu")
    bad = ok[0].clone()
    bad[0, 0, 0] = tables.dims["Ne"]                                   # one past the last id
    with pytest.raises(IndexError):
        batcher.batch(bad, ok[1])
    gap = [i for i in range(tables.dims["Ne"]) if i not in ds["entity2idx"].values()]
    assert gap                                                         # context_utils.init_random leaves the id in front of _UNKNOWN to nobody
    bad[0, 0, 0] = gap[0]
    with pytest.raises(IndexError):
        batcher.batch(bad, ok[1])
    bad[0, 0, 0] = -2
    with pytest.raises(IndexError):
        batcher.batch(bad, ok[1])
    bad_sf = ok[1].clone()
    bad_sf[1, 1, 1] = tables.dims["S"]
    with pytest.raises(IndexError):
        batcher.batch(ok[0], bad_sf)
    half = ok[0].clone()
    half[0, 0, 1] = -1
    with pytest.raises(ValueError):
        batcher.batch(half, ok[1])
    assert ContextBatcher(build(ds, "wikidata", sf, None)[0]).batch(half, ok[1]).unique_entities[0] == -1      # no GAT table: a half pair is data
    with pytest.raises(TypeError):
        batcher.batch(*ok, index_dtype=torch.int16)
    with pytest.raises(ValueError):
        batcher.batch(ok[0][0], ok[1][0])


def test_builder_errors(fx, monkeypatch):
    from recon_amd import ContextTables
    ds, g = fx
    sf = ds["batches"][0][1]
    with pytest.raises(ValueError, match="Q04"):                       # 1 + 15 + 15 lines behind the surface form need max_num_contexts = 32
        build(ds, "wikidata", sf, None, max_num_contexts=31)
    build(ds, "wikidata", sf, None, max_num_contexts=32)
    monkeypatch.setitem(sys.modules, "nltk", None)                     # `import nltk` now raises ImportError, installed or not
    with pytest.raises(ImportError, match="word_tokenize"):
        ContextTables.build(ds["entity2idx"], ds["context_wikidata"], ds["word2idx"], ds["char2idx"], 3, sf)
    with pytest.raises(ValueError):
        ContextTables.build(ds["entity2idx"], ds["context_wikidata"], ds["word2idx"], ds["char2idx"], 3, sf, data="other", word_tokenize=str.split,
                            sent_tokenize=lambda s: [s])
    with pytest.raises(ValueError):
        build(ds, "wikidata", sf, "some")


def test_tables_stay_compact(fx):
    ds, g = fx
    tables, _ = build(ds, "wikidata", ds["batches"][0][1], "selected")
    dense = (len(ds["entity2idx"])) * 32 * 386 * 8
    assert sum(t.numel() * t.element_size() for t in tables.arrays.values()) < dense // 50
    assert all(t.dtype == (torch.float32 if k == "gat_emb" else torch.int32) for k, t in tables.arrays.items())


def test_entries_are_declared_and_bound():
    entries_declared_and_bound(ENTRIES, "train.py:250-258")


def test_status_codes_before_any_launch():
    import ctypes as C
    from recon_amd import _lib
    from recon_amd.context_batch import MAX_IDS
    L = _lib.lib()
    ok = L.recon_ctx_batch_supported
    assert ok(7200, 500, 900) and ok(2, 0, 1) and ok(MAX_IDS, 2 ** 31 - 2, 2 ** 31 - 1)
    assert not ok(MAX_IDS + 2, 500, 900) and not ok(0, 500, 900) and not ok(7, 500, 900) and not ok(8, 2 ** 31 - 1, 900) and not ok(8, 5, 0)
    fake = 16                                                          # never dereferenced: every call returns before a launch
    tabs = lambda gat=True, hole=None: (C.c_void_p * 11)(*[None if (i == hole or (not gat and i >= 9)) else fake for i in range(11)])
    dims = lambda **kw: (C.c_int64 * 12)(*[kw.get(k, v) for k, v in (("Ne", 500), ("S", 900), ("V", 50), ("L", 70), ("NF", 90), ("T", 32), ("P", 32),
                                                                     ("mcl", 10), ("cfs", 3), ("pad", 0), ("G", 100), ("Ng", 500))])
    index = lambda n, mode=2, t=None, d=None, ids=fake, hdr=fake: L.recon_ctx_batch_index(t or tabs(), d or dims(), ids, fake, n, mode, fake, fake, fake, fake,
                                                                                       fake, hdr, None)
    assert index(0) == -1 and index(-3) == -1 and index(MAX_IDS // 2 + 1) == -2 and index(5, mode=3) == -1
    assert index(5, ids=None) == -1 and index(5, hdr=None) == -1 and index(5, t=tabs(hole=6)) == -1 and index(5, t=tabs(gat=False)) == -1
    assert index(5, d=dims(T=0)) == -1 and index(5, d=dims(Ne=2 ** 31)) == -2 and L.recon_ctx_batch_index(None, dims(), fake, fake, 5, 0, fake, fake, fake,
                                                                                                        fake, fake, fake, None) == -1
    fill = lambda U=4, P=8, T=8, nbytes=8, words=fake, t=None: L.recon_ctx_batch_fill(t or tabs(gat=False), dims(), fake, fake, U, P, T, nbytes, words, fake,
                                                                                     fake, None)
    assert fill(U=0) == -1 and fill(P=0) == -1 and fill(P=33) == -1 and fill(T=33) == -1 and fill(nbytes=2) == -1 and fill(words=None) == -1
    assert fill(words=20, nbytes=8) == -1 and fill(U=MAX_IDS + 2) == -2 and fill(t=tabs(hole=0)) == -1
    wide = dims(T=4096, P=4096)                                         # 8000 x 4096 rows of 49 154 cells: beyond int32 flat indices
    assert L.recon_ctx_batch_fill(tabs(gat=False), wide, fake, fake, 8000, 4096, 4096, 4, fake, fake, fake, None) == -2
    assert 11 * 4096 * 49154 >= 2 ** 31 - 4096 > 10 * 4096 * 49154      # the first U past the limit at this width
    assert L.recon_ctx_batch_fill(tabs(gat=False), wide, fake, fake, 11, 4096, 4096, 4, fake, fake, fake, None) == -2
    gat = lambda n, t=None, out=fake, nz=None, slot=fake: L.recon_ctx_batch_gat(t or tabs(), dims(), fake, n, slot, out, nz, None)
    assert gat(0) == -1 and gat(MAX_IDS // 2 + 1) == -2 and gat(5, t=tabs(gat=False)) == -1 and gat(5, out=None) == -1
    assert gat(5, nz=fake, slot=None) == -1
