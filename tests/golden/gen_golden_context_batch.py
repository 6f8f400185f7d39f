#!/usr/bin/env python3
"""Writes tests/golden/context_batch1.npz and context_batch1.json by RUNNING THE REFERENCE's own batch assembly on a synthetic dataset:

  utils/context_utils.py:62-84    get_batch_unique_entities
  utils/context_utils.py:293-301  get_entity_location_unique_entities
  utils/context_utils.py:365-385  get_context_indices (over :120-152, :256-291, :303-319 and utils/embedding_utils.py:73-112)
  utils/context_utils.py:444-453  get_gat_entity_embeddings
  utils/context_utils.py:455-475  get_selected_gat_entity_embeddings

imported from where they lie, under the same `nltk` stub as tests/golden/gen_golden.py (word_tokenize = str.split, sent_tokenize =
one sentence), with the casts of train.py:261-273 applied to what they return.  Runs only where the reference tree is; the two files it
writes hold data only (the .json: the dataset's dictionaries and strings; the .npz: index arrays and the recorded results).

Usage:  python tests/golden/gen_golden_context_batch.py
"""
import json
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
G = 3
CFS = 3


def _shims():
    nltk = types.ModuleType("nltk")
    nltk.word_tokenize = lambda s: s.split()
    nltk.sent_tokenize = lambda s: [s]
    sys.modules["nltk"] = nltk
    if not hasattr(np, "long"):
        np.long = np.int64
    sys.path.insert(0, REF)


def dataset():
    ctx = {
        "Q01": {"desc": "capital and largest city of Germany", "instances": [{"label": "city"}, {"label": "capital"}], "aliases": ["Berlin, Germany"]},
        # Q02: no context entry at all
        "Q03": {"desc": "", "instances": [{"label": "river"}], "aliases": []},
        "Q04": {"desc": "a thing of many kinds", "instances": [{"label": "kind %d" % i} for i in range(20)], "aliases": ["name %d" % i for i in range(20)]},
        "Q05": {"desc": " ".join("w%d" % i for i in range(40)), "instances": [], "aliases": ["long one"]},
        "Q06": {"desc": "the Donaudampfschifffahrtsgesellschaft café by the river", "instances": [{"label": "company"}], "aliases": []},
        "Q07": {"desc": "Berlin river, (Lake 1999 zzyzx &ndash; 3,5.2 capital", "instances": [], "aliases": ["The City", "x"]},
        "Q08": {"desc": "x", "instances": [{"label": "lake"}], "aliases": []},
        "Q09": {"desc": "city by the lake", "instances": [], "aliases": []},
        "Q10": {"desc": "largest river of Germany", "instances": [{"label": "river"}], "aliases": ["the river"]},
        "Q11": {"desc": "company of the capital", "instances": [{"label": "company"}], "aliases": []},
        "Q12": {"desc": "known to the text, unknown to the graph", "instances": [], "aliases": []},
    }
    for i in range(13, 39):                                            # filler, so that a [3, 6, 2] batch can hold 36 distinct ids
        ctx["Q%02d" % i] = {"desc": "thing %d of the city" % i, "instances": [{"label": "kind %d" % (i % 3)}] * (i % 3), "aliases": ["t%d" % i] * (i % 2)}
    nyt = {k: {"desc": [v["desc"], "a second sentence"] if v["desc"] else [], "en_instances": [i["label"] for i in v["instances"]], "alias": list(v["aliases"])}
           for k, v in ctx.items()}
    names = sorted(ctx) + ["Q02"]
    words = ["capital", "and", "largest", "city", "of", "germany", "instance", "also", "known", "as", "berlin", "river", "lake", "0", "–", "the",
             "a", "thing", "kind", "name", "company", "by", "x", "long", "one", "w1", "w31", "w32", "ALL_ZERO", "to", "text"]
    word2idx = {"_UNKNOWN": 1}
    for w in words:
        word2idx[w] = len(word2idx) + 1
    chars = "abcdefghijklmnopqrstuvwxyzBDGLQCT0123459,(&;_"
    char2idx = {"<PAD>": 3, "<UNK>": 1}
    for c in chars:
        char2idx[c] = len(char2idx) + 3
    return ctx, nyt, sorted(names), word2idx, char2idx


def batches(e):
    """Five [3, 6, 2] batches of (entity name or None, surface form) pairs; a None half is padding: id -1, ['ALL_ZEROS']."""
    pad = (None, ["ALL_ZEROS"])
    P = (pad, pad)
    s = lambda n, *toks: (n, list(toks) if toks else [n.lower()])
    b0 = [[(s("Q01", "Berlin"), s("Q03", "Spree")), (s("Q03", "Spree"), s("Q01", "Berlin")), (s("Q01", "Berlin"), s("_UNKNOWN", "Nowhere", "Town")), P, P, P],
          [(s("Q05", "Long"), s("Q06", "DDSG")), (s("Q06", "DDSG"), s("Q05", "Long")), P, P, P, P],
          [(s("Q02", "Q-two"), s("Q04", "Many")), (s("Q04", "Many"), s("Q07", "Mix")), (s("Q07", "Mix"), s("Q02", "Q-two")), P, P, P]]
    b1 = [[P] * 6 for _ in range(3)]
    b2 = [[(s("Q01", "Berlin"), s("Q09", "Lakeside")), (s("Q09", "Lakeside"), s("Q10", "Rhine")), P, P, P, P],
          [(s("Q10", "Rhein"), s("Q01", "the", "German", "capital")), P, P, P, P, P],
          [(s("Q11", "Firm"), s("Q09", "Lakeside")), P, P, P, P, P]]
    # Q07 and Q08 five times each (Q07 first), -1 four times, everything else less: the first maximum is Q07's, not -1's
    b3 = [[(s("Q09"), s("Q07", "Mix")), (s("Q07", "Mix"), s("Q08", "Pond")), (s("Q08", "Pond"), s("Q07", "Mix")), (s("Q07", "Mix"), s("Q08", "Pond")),
           (s("Q08", "Pond"), s("Q07", "Mix")), (s("Q08", "Pond"), s("Q10"))],
          [(s("Q10"), s("Q11")), (s("Q11"), s("Q09")), (s("Q13"), s("Q14")), (s("Q14"), s("Q13")), P, P],
          [(s("Q15"), s("Q16")), (s("Q16"), s("Q15")), (s("Q17"), s("Q18")), (s("Q18"), s("Q17")), (s("Q19"), s("Q20")), (s("Q20"), s("Q19"))]]
    every = [n for n in e if n not in ("ALL_ZERO", "Q04", "Q05")]     # 37 names; Q12 (not in the GAT table) and _UNKNOWN among them
    every = [n for n in every if n != "Q38"][:36]
    assert len(every) == 36 and "Q12" in every and "_UNKNOWN" in every
    b4 = [[(s(every[12 * i + 2 * j], "sf%d" % (12 * i + 2 * j)), s(every[12 * i + 2 * j + 1])) for j in range(6)] for i in range(3)]
    out_ids, out_sf = [], []
    for b in (b0, b1, b2, b3, b4):
        ids = -np.ones((3, 6, 2), dtype="int32")
        sf = [[[None, None] for _ in range(6)] for _ in range(3)]
        for i in range(3):
            for j in range(6):
                for k in range(2):
                    name, toks = b[i][j][k]
                    ids[i, j, k] = -1 if name is None else e[name]
                    sf[i][j][k] = toks
        out_ids.append(ids)
        out_sf.append(sf)
    return out_ids, out_sf


def main():
    _shims()
    from utils import context_utils as cu
    ctx_w, ctx_n, names, word2idx, char2idx = dataset()
    _, entity2idx = cu.init_random(set(names), 1, add_all_zeroes=True, add_unknown=True)
    idx2entity = {v: k for k, v in entity2idx.items()}
    ctx_w["ALL_ZERO"] = {"desc": "", "label": "ALL_ZERO", "instances": [], "aliases": []}          # train.py:168-173
    # the GAT table numbers the entities its own way; Q12 is not in it; its row entity2idx['_UNKNOWN'] exists (context_utils.py:467)
    in_gat = [n for n in reversed(names) if n != "Q12"]
    gat_entity2idx = {n: i for i, n in enumerate(in_gat)}
    n_rows = max(len(in_gat), entity2idx["_UNKNOWN"] + 1)
    gat_embeddings = {str(i): [0.1 * i + 0.01 * j + 1.0 / 3.0 for j in range(G)] for i in range(n_rows)}
    ids, sfs = batches(entity2idx)
    arrays = {"n_batches": np.int64(len(ids))}
    for b, (ei, sf) in enumerate(zip(ids, sfs)):
        arrays["b%d.ids" % b] = ei.astype(np.int64)
        sf_arr = np.empty((3, 6, 2), dtype=object)
        for i in range(3):
            for j in range(6):
                for k in range(2):
                    sf_arr[i, j, k] = sf[i][j][k]
        for layout, ctx in (("wikidata", ctx_w), ("nyt", ctx_n)):
            uniq, usf, max_pos = cu.get_batch_unique_entities(ei, sf_arr)
            words, chars, mask = cu.get_context_indices(uniq, usf, ctx, idx2entity, word2idx, char2idx, CFS, max_sent_len=32, max_num_contexts=32,
                                                        max_char_len=10, data=layout)
            pos = cu.get_entity_location_unique_entities(uniq, ei)
            k = "%s.b%d." % (layout, b)
            arrays[k + "unique"] = uniq.astype(np.long)
            arrays[k + "max_pos"] = np.int64(max_pos)
            arrays[k + "words"] = words.astype(np.long)
            arrays[k + "chars"] = chars.astype(np.long)
            arrays[k + "mask"] = mask.astype(bool)
            arrays[k + "pos"] = pos.astype(int)
        try:
            arrays["b%d.gat_all" % b] = cu.get_gat_entity_embeddings(ei, entity2idx, idx2entity, gat_entity2idx, gat_embeddings).astype(np.float32)
            arrays["b%d.gat_all_keyerror" % b] = np.bool_(False)
        except KeyError:
            arrays["b%d.gat_all_keyerror" % b] = np.bool_(True)
        g, nz, nz_pos = cu.get_selected_gat_entity_embeddings(ei, entity2idx, idx2entity, gat_entity2idx, gat_embeddings)
        arrays["b%d.gat_sel" % b] = g.astype(np.float32)
        arrays["b%d.nz" % b] = nz.astype(np.float32).reshape(len(nz_pos), 2 * G)
        arrays["b%d.nz_pos" % b] = np.asarray(nz_pos, dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "context_batch1.npz"), **arrays)
    with open(os.path.join(OUT, "context_batch1.json"), "w") as f:
        json.dump({"entity2idx": entity2idx, "word2idx": word2idx, "char2idx": char2idx, "context_wikidata": ctx_w, "context_nyt": ctx_n,
                   "gat_entity2idx": gat_entity2idx, "gat_embeddings": gat_embeddings, "surface_forms": sfs, "conv_filter_size": CFS},
                  f, indent=0, sort_keys=True, ensure_ascii=True)
    print("wrote context_batch1.npz (%d arrays) and context_batch1.json" % len(arrays))


if __name__ == "__main__":
    main()
