"""Shared by tests/test_context_batch_cpu.py, tests/test_context_batch_gpu.py and tools/context_batch_bench.py: the fixture's loader, synthetic
datasets and batches, and `restate` — the stage-B batch assembly written once more as plain loops over the dataset's dictionaries, from
the definitions in recon_amd/context_batch.py's docstrings, sharing no code with the package.  `wrong=` makes it wrong
in one named way, so that the tests can show the fixture catches each.  Not a test module and not a conftest."""
import json
import os
import re

import numpy as np
import torch

from conftest import GOLDEN, load_golden

TOKENIZERS = dict(word_tokenize=str.split, sent_tokenize=lambda s: [s])
FIELDS = ("unique", "pos", "max_pos", "words", "chars", "mask", "gat", "nz", "nz_pos")
WRONG = ("sorted_order", "first_surface", "last_maximum", "full_width", "all_zeros_in_selected")


def fixture():
    with open(os.path.join(GOLDEN, "context_batch1.json")) as f:
        ds = json.load(f)
    g = load_golden("context_batch1")
    ds["batches"] = []
    for b in range(int(g["n_batches"])):
        sf = np.empty((3, 6, 2), dtype=object)
        for i in range(3):
            for j in range(6):
                for k in range(2):
                    sf[i, j, k] = ds["surface_forms"][b][i][j][k]
        ds["batches"].append((g["b%d.ids" % b], sf))
    return ds, g


def expected(g, layout, b, gat_mode):
    """The fixture's record of batch b as a dict over FIELDS (None where the mode has no such output)."""
    k = "%s.b%d." % (layout, b)
    out = {"unique": g[k + "unique"], "pos": g[k + "pos"], "max_pos": int(g[k + "max_pos"]), "words": g[k + "words"], "chars": g[k + "chars"],
           "mask": g[k + "mask"], "gat": None, "nz": None, "nz_pos": None}
    if gat_mode == "all":
        out["gat"] = g["b%d.gat_all" % b]
    elif gat_mode == "selected":
        out["gat"], out["nz"], out["nz_pos"] = g["b%d.gat_sel" % b], g["b%d.nz" % b], g["b%d.nz_pos" % b]
    return out


def as_numpy(batch):
    """A StageBBatch as a dict over FIELDS."""
    n = lambda t: None if t is None else t.detach().cpu().numpy()
    return {"unique": n(batch.unique_entities), "pos": n(batch.entities_position), "max_pos": batch.max_occurred_entity_in_batch_pos,
            "words": n(batch.context_words), "chars": n(batch.context_chars), "mask": n(batch.context_mask), "gat": n(batch.gat_entity_embeddings),
            "nz": n(batch.nonzero_gat_entity_embeddings), "nz_pos": n(batch.nonzero_entity_pos)}


def differences(got, want, index_dtype=np.int64):
    """The FIELDS in which two results differ in shape, dtype or any value (floats: any bit)."""
    bad = []
    for f in FIELDS:
        a, b = got[f], want[f]
        if (a is None) != (b is None):
            bad.append(f)
        elif a is None:
            continue
        elif f == "max_pos":
            if not (isinstance(a, int) and a == b):
                bad.append(f)
        else:
            a, b = np.asarray(a), np.asarray(b)
            if f in ("words", "chars") and index_dtype != np.int64:
                b = b.astype(index_dtype)
            if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
                bad.append(f)
    return bad


def build(ds, layout, surface_forms, gat_mode, **kw):
    from recon_amd import ContextTables
    gat = (ds["gat_entity2idx"], ds["gat_embeddings"], gat_mode) if gat_mode else None
    return ContextTables.build(ds["entity2idx"], ds["context_" + layout], ds["word2idx"], ds["char2idx"], ds["conv_filter_size"], surface_forms,
                               data=layout, gat=gat, **dict(TOKENIZERS, **kw))


# ------------------------------------------------------------------------------------------------------------- the restatement
def _word_id(word, vocab):
    word = word.strip()
    for candidate in (word, word.lower()):
        if candidate in vocab:
            return vocab[candidate]
    special = {"&ndash;": "–", "&mdash;": "—", "@card@": "0"}
    if word in special:
        return vocab[special[word]]
    core = re.sub(r"(^\W|\W$)", "", word)
    for candidate in (core, core.lower()):
        if candidate in vocab:
            return vocab[candidate]
    return vocab.get(re.sub(r"([0-9][0-9.,]*)", "0", word), vocab["_UNKNOWN"])


def _lines(name, context, layout):
    """The entity's text lines behind its surface form, tokenised."""
    split = str.split
    if layout == "wikidata":
        c = context.get(name, {"desc": "", "instances": [], "aliases": []})
        head = [c["desc"]] if c["desc"] != "" else []
        kinds, names = [i["label"] for i in c["instances"]], c["aliases"]
    else:
        c = context.get(name, {"desc": [], "en_instances": [], "alias": []})
        head = [c["desc"][0]] if len(c["desc"]) > 0 else []
        kinds, names = c["en_instances"], c["alias"]
    return [split(s) for s in head + ["instance of %s" % k for k in kinds[:15]] + ["also known as %s" % a for a in names[:15]]]


def restate(ds, layout, ids, surface_forms, gat_mode=None, wrong=None, max_sent_len=32, max_num_contexts=32, max_char_len=10, cached_lines=None):
    """One batch by plain loops -> a dict over FIELDS (numpy, the reference's dtypes after its casts).  cached_lines: a dict that keeps
    every entity's tokenised lines between calls (the bench's "without tokenising" variant)."""
    e2i, context, vocab, chars_of = ds["entity2idx"], ds["context_" + layout], ds["word2idx"], ds["char2idx"]
    name_of = {v: k for k, v in e2i.items()}
    cfs = ds["conv_filter_size"]
    order, surface, count, seen = [-1], {-1: ["ALL_ZERO"]}, {-1: 0}, set()
    B, Cn = ids.shape[0], ids.shape[1]
    for i in range(B):
        for j in range(Cn):
            for k in range(2):
                e = int(ids[i, j, k])
                if e not in count:
                    order.append(e)
                    count[e] = 0
                count[e] += 1
                if wrong != "first_surface" or e not in seen:
                    surface[e] = list(surface_forms[i, j, k])
                seen.add(e)
    if wrong == "sorted_order":
        order = sorted(order)
    where = {e: r for r, e in enumerate(order)}
    pos = np.zeros((B, Cn, 2), dtype=np.int64)
    for i in range(B):
        for j in range(Cn):
            for k in range(2):
                pos[i, j, k] = where[int(ids[i, j, k])]
    counts = [count[e] for e in order]
    best = max(counts)
    winners = [r for r, c in enumerate(counts) if c == best]
    max_pos = winners[-1] if wrong == "last_maximum" else winners[0]
    texts = []
    for e in order:
        if cached_lines is not None and e in cached_lines:
            body = cached_lines[e]
        else:
            body = _lines(name_of[e], context, layout)
            if cached_lines is not None:
                cached_lines[e] = body
        texts.append([surface[e]] + body)
    T = min(max_sent_len, max(len(line) for lines in texts for line in lines))
    if wrong == "full_width":
        T = max_sent_len
    P = min(max_num_contexts, max(len(lines) for lines in texts))
    step = max_char_len + cfs - 1
    words = np.zeros((len(order), P, T), dtype=np.int64)
    chars = np.full((len(order), P, cfs - 1 + T * step), chars_of["<PAD>"], dtype=np.int64)
    mask = np.ones((len(order), P), dtype=bool)
    for u, lines in enumerate(texts):
        for p, line in enumerate(lines):
            mask[u, p] = False
            for w, token in enumerate(line[:T]):
                words[u, p, w] = _word_id(token, vocab)
                for c, ch in enumerate(token[:max_char_len]):
                    known = chars_of.get(ch)
                    chars[u, p, cfs - 1 + w * step + c] = known if known is not None else chars_of["<UNK>"]
    out = {"unique": np.asarray(order, dtype=np.int64), "pos": pos, "max_pos": int(max_pos), "words": words, "chars": chars, "mask": mask,
           "gat": None, "nz": None, "nz_pos": None}
    if gat_mode:
        table, rows_of = ds["gat_embeddings"], ds["gat_entity2idx"]
        G = len(table["0"])
        gat = np.zeros((B, Cn, 2 * G), dtype=np.float32)
        nz, nz_pos = [], []
        zeros = [-1, e2i["_UNKNOWN"]] if (gat_mode == "all" or wrong == "all_zeros_in_selected") else [-1]
        for i in range(B):
            for j in range(Cn):
                present = False
                for k in range(2):
                    e = int(ids[i, j, k])
                    if e in zeros:
                        present = present or e != -1
                        continue
                    if gat_mode == "all":
                        row = rows_of[name_of[e]]                     # KeyError for an entity the GAT table lacks
                    else:
                        row = rows_of.get(name_of[e], e2i["_UNKNOWN"])
                    gat[i, j, k * G:(k + 1) * G] = np.asarray(table[str(row)], dtype=np.float64).astype(np.float32)
                    present = True
                if present:
                    nz.append(gat[i, j].copy())
                    nz_pos.append(i * Cn + j)
        out["gat"] = gat
        if gat_mode == "selected":
            out["nz"] = np.asarray(nz, dtype=np.float32).reshape(len(nz), 2 * G)
            out["nz_pos"] = np.asarray(nz_pos, dtype=np.int64)
    return out


# ------------------------------------------------------------------------------------------------------------- synthetic data
def random_dataset(rng, n_entities, G, max_lines=31, layout="wikidata", n_words=None, n_chars=None, conv_filter_size=3):
    """A dataset in the fixture's form: entities E0000.. with 0 .. max_lines context lines of 1-6 tokens (a few of 32+), a GAT table that
    lacks no entity, and a vocabulary that knows about two thirds of the words.  n_words / n_chars: fold the word and char ids into
    [1, n_words) and [0, n_chars), for a model with tables that small."""
    names = ["E%04d" % i for i in range(n_entities)]
    e2i = {"ALL_ZERO": -1}
    e2i.update({n: i for i, n in enumerate(names)})
    e2i["_UNKNOWN"] = len(names)
    pool = ["tok%d" % i for i in range(60)] + ["Tok7", "tok3,", "1234", "averyveryverylongtoken", "café"]
    vocab = {"_UNKNOWN": 1, "ALL_ZERO": 2, "instance": 3, "of": 4, "also": 5, "known": 6, "as": 7, "0": 8}
    for w in pool[:40]:
        vocab[w] = len(vocab) + 1
    chars = {"<PAD>": 0, "<UNK>": 1}
    for c in "abcdefghijklmnopqrstuvwxyT0123456789":
        chars[c] = len(chars)
    if n_words:
        vocab = {w: 1 + (i - 1) % (n_words - 1) for w, i in vocab.items()}
    if n_chars:
        chars = {c: i if i < 2 else 2 + (i - 2) % (n_chars - 2) for c, i in chars.items()}
    text = lambda n: " ".join(pool[int(i)] for i in rng.integers(0, len(pool), n))
    ctx = {}
    for n in names:
        if rng.random() < 0.1:
            continue
        lines = int(rng.integers(0, max_lines + 1))
        n_kind = min(15, lines // 2)
        n_alias = min(15, max(lines - 1 - n_kind, 0))
        desc = text(int(rng.integers(1, 7)) if rng.random() < 0.9 else 34) if lines > n_kind + n_alias else ""
        kinds, aliases = [text(int(rng.integers(1, 4))) for _ in range(n_kind)], [text(int(rng.integers(1, 4))) for _ in range(n_alias)]
        if layout == "wikidata":
            ctx[n] = {"desc": desc, "instances": [{"label": k} for k in kinds], "aliases": aliases}
        else:
            ctx[n] = {"desc": [desc] if desc else [], "en_instances": kinds, "alias": aliases}
    order = rng.permutation(len(names) + 1)
    gat_e2i = {n: int(order[i]) for i, n in enumerate(names)}
    emb = rng.standard_normal((len(names) + 1, G))
    ds = {"entity2idx": e2i, "context_" + layout: ctx, "word2idx": vocab, "char2idx": chars, "conv_filter_size": conv_filter_size, "gat_entity2idx": gat_e2i,
          "gat_embeddings": {str(i): [float(x) for x in emb[i]] for i in range(emb.shape[0])}, "pool": pool}
    return ds


def random_batch(rng, ds, B, Cn, zipf=1.3, pad_share=0.3, distinct=False, one_token=False):
    """ids int64 [B, Cn, 2] drawn Zipf-distributed over the entities (_UNKNOWN included), a share of the pairs padding (-1, -1), and an
    object array of surface forms: each entity has two spellings, so that the last occurrence matters."""
    Ne = len(ds["entity2idx"]) - 1
    ids = -np.ones((B, Cn, 2), dtype=np.int64)
    sf = np.empty((B, Cn, 2), dtype=object)
    perm = rng.permutation(Ne)
    fresh = iter(perm)
    for i in range(B):
        for j in range(Cn):
            pad = rng.random() < pad_share and not distinct
            for k in range(2):
                if pad:
                    sf[i, j, k] = ["ALL_ZEROS"]
                    continue
                e = int(next(fresh)) if distinct else int(perm[min(int(rng.zipf(zipf)) - 1, Ne - 1)])
                ids[i, j, k] = e
                sf[i, j, k] = ["sf%d" % e] if (one_token or rng.random() < 0.5) else ["the", ds["pool"][e % len(ds["pool"])], "x%d" % e]
    return ids, sf


def to_device(ids, surface_ids, device):
    return torch.from_numpy(np.ascontiguousarray(ids)).to(device), torch.from_numpy(np.ascontiguousarray(surface_ids)).to(device)
