"""Fixture of the per-pair datasets (tests/golden/pair_data1.npz), written where the reference tree is available.

Five synthetic graphs (tokens, `vertexSet`, `edgeSet` with `left` / `right`), ten edges, max_sent_len = 8, go through the reference's own
`to_indices`, `to_indices_with_relative_positions_and_entity_pair` and `to_indices_with_relative_positions_and_pcnn_mask_and_entity_pair`
(parsing/legacy_sp_models.py:67-97, :530-603) with the position vocabulary of train.py:197.  Among them: an entity at token 0 and one at
the last token, a sentence of 11 tokens (longer than max_sent_len: cut, with an entity beyond the cut), an edge whose right entity
precedes its left (its mask planes overlap), two-token entities, a word outside the vocabulary and a label outside the properties.
Recorded: `marks_*`, `positions_*` and `segments_*` = sentences, markers, labels (and `segments_mask`), `n_words` and `n_positions` (the
sizes of the two vocabularies).  The entity-pair lists are Python lists of strings and are not stored.  Arrays only; nothing of the
reference's text is stored.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
MAX_SENT_LEN = 8
WORDS = "the a of in was born city river capital near lake and by north".split()


def _graph(tokens, entities, edges):
    return {"tokens": tokens.split(),
            "vertexSet": [{"tokenpositions": list(pos), "kbID": "Q%d" % (i + 1), "lexicalInput": "e%d" % i} for i, pos in enumerate(entities)],
            "edgeSet": [{"left": list(entities[a]), "right": list(entities[b]), "kbID": kb} for a, b, kb in edges]}


GRAPHS = [
    _graph("Lima was the capital of Peru", [(0,), (5,)], [(0, 1, "P1"), (1, 0, "P2")]),                   # token 0 and the last token; right before left
    _graph("the river Rimac near the city of Lima and by the north lake", [(1, 2), (7,), (11,)],        # 13 tokens > 8; an entity beyond the cut
           [(0, 1, "P3"), (1, 0, "P0"), (0, 2, "P1")]),
    _graph("a lake", [(0,), (1,)], [(0, 1, "P0")]),                                                       # two tokens: a padded tail of six
    _graph("born in the north of the city Cusco", [(3,), (6, 7)], [(0, 1, "P2"), (1, 0, "P9")]),         # exactly 8; P9 is no known property
    _graph("Cusco and Lima", [(0,), (2,)], [(0, 1, "P0"), (1, 0, "P3")]),
]


def main():
    sys.path.insert(0, HERE)
    import gen_golden
    gen_golden._install_shims()
    cwd = os.getcwd()
    os.chdir(REF)
    sys.path.insert(0, REF)
    try:
        from parsing import legacy_sp_models as ref
        from utils import embedding_utils
    finally:
        os.chdir(cwd)
    assert ref.__file__.startswith(REF)
    word2idx = {embedding_utils.all_zeroes: 0}
    for w in WORDS + ["lima", "peru", "cusco"]:
        word2idx[w] = len(word2idx)
    word2idx[embedding_utils.unknown] = len(word2idx)                                         # "Rimac" maps here
    property2idx = {embedding_utils.all_zeroes: 0, "P0": 1, "P1": 2, "P2": 3, "P3": 4, embedding_utils.unknown: 5}
    _, position2idx = embedding_utils.init_random(np.arange(-MAX_SENT_LEN, MAX_SENT_LEN), 1, add_all_zeroes=True)      # train.py:197
    marks = ref.to_indices(GRAPHS, word2idx, property2idx, MAX_SENT_LEN)
    positions = ref.to_indices_with_relative_positions_and_entity_pair(GRAPHS, word2idx, property2idx, MAX_SENT_LEN, position2idx)
    segments = ref.to_indices_with_relative_positions_and_pcnn_mask_and_entity_pair(GRAPHS, word2idx, property2idx, MAX_SENT_LEN, position2idx)
    assert len(marks) == 3 and len(positions) == 4 and len(segments) == 5 and isinstance(positions[3], list) and isinstance(segments[4], list)
    n = sum(len(g["edgeSet"]) for g in GRAPHS)
    assert marks[1].shape == (n, MAX_SENT_LEN) and positions[1].shape == (n, 2, MAX_SENT_LEN) and segments[3].shape == (n, 3, MAX_SENT_LEN)
    assert segments[3].dtype == np.float32 and set(np.unique(segments[3])) == {0.0, 1.0}
    arrays = {"n_words": np.int64(len(word2idx)), "n_positions": np.int64(len(position2idx))}
    for form, a in (("marks", marks), ("positions", positions), ("segments", segments)):
        arrays.update({form + "_sentences": a[0], form + "_markers": a[1], form + "_labels": a[2]})
    arrays["segments_mask"] = segments[3]
    path = os.path.join(HERE, "pair_data1.npz")
    np.savez_compressed(path, **arrays)
    print("wrote %-28s %5.1f KB, %d rows" % ("pair_data1.npz", os.path.getsize(path) / 1024, n))
    bits = (segments[3][:, 0] + 2 * segments[3][:, 1] + 4 * segments[3][:, 2]).astype(int)
    print("mask patterns:", sorted(set(bits.reshape(-1).tolist())), "labels:", marks[2].tolist())


if __name__ == "__main__":
    main()
