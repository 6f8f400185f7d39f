"""The stage-B entity-context batch, assembled on the device — SURVEY.md 8(f), DESIGN.md §27.

For every batch the reference's loop (train.py:250-258, again :337-344, and test.py) calls, on the host,
`context_utils.get_batch_unique_entities` (utils/context_utils.py:62-84: a triple loop over the [B, C, 2] ids into two dicts),
`get_entity_location_unique_entities` (:293-301: the same loop with a `list.index` inside), `get_context_indices` (:365-385:
`word_tokenize` on every description, instance label and alias of every unique entity, `get_idx` per token, float64 blocks filled a
character at a time) and `get_gat_entity_embeddings` / `get_selected_gat_entity_embeddings` (:444-475), and then `astype`, `from_numpy`
and `.cuda()` on each result.  Here the text is tokenised ONCE per dataset into compact tables, and a batch is two or three launches:

    tables, surface_ids = ContextTables.build(entity2idx, context_data, word2idx, char2idx, conv_filter_size, surface_forms,
                                              word_tokenize=..., sent_tokenize=..., gat=(gat_entity2idx, gat_embeddings, 'selected'))
    batcher = ContextBatcher(tables.to(device))
    batch = batcher.batch(entity_indices[rows], surface_ids[rows])          # both on the device
    logits = model(sentence, markers, n, *batch.model_args())

Every result equals the reference's array exactly — integers to the value, floats to the bit: nothing is computed, only selected,
ordered and copied (pinned by tests/golden/context_batch1.npz, recorded from the reference's own functions).

Host reads: ONE per call — a header of eight int32 (U, T_b, P_b, Mnz, the most frequent entity's position, error flags, L): the
output shapes depend on it, as `sampler.py`'s do.  It is read behind the first launch and before the model's forward is queued, so a
caller's step waits once, on a kernel of a few microseconds, and the forward then runs without the host waiting again.

The tables (no dense [entities, 32, 386] block: at Wikidata's size that is tens of GB): a token table (word id by the rules of
`embedding_utils.get_idx`, the first `max_char_len` characters as char ids), a CSR entity -> lines -> tokens and a CSR surface
form -> tokens, all int32, plus with `gat=` an fp32 [Ng, G] matrix and a row map.

Two implementations of one result: csrc/ctx_batch.hip (k_cb_index, k_cb_fill, k_cb_gat) on the GPU for batches up to
`MAX_IDS` ids, and the same assembled from torch primitives (`unique`, `scatter_reduce`, a sort, ragged gathers), which is the CPU
path, the path beyond the kernels' limit and what the randomised GPU test compares with; `_KERNELS = False` forces it.

`batch(..., ragged_lines=True)` leaves the padding lines out: context_words [L, T_b] and context_chars [L, W] hold the
entities' present lines one after another, L = the sum of their line counts (the header's seventh word: still one host read), and
context_mask is a `RaggedLines` (line_ptr int32 [U + 1]) in the mask's place, which `EntityEmbedding.forward` takes as its third argument.
The default, False, is the reference's padded form.

`batch(..., word_forms=True)` hands the char block over as its distinct word windows: context_chars is a `WordForms` —
chars [S_d, cfs - 1 + word_span], one row per distinct window of the batch, and slot_form [rows T_b] with its occurrence lists — in the
padded form (rows = U P_b) and in the ragged one (rows = L).  The tables carry a form id per token (`tok_form`; two tokens that agree in
their first `max_char_len` characters share a form, form 0 is the all-pad row of an empty slot) and the forms' rows (`form_chars`); the
batch numbers the forms it holds by ascending table form id.  S_d travels in the header's eighth word: still one host read, and the
dense [rows, W] block is never written.  `EntityEmbedding.forward` takes the `WordForms` where it takes the block.  Under dropout every
occurrence of a form then shares one draw, which is why the default is False.  `ContextBatcher(tables, ragged_lines=, word_forms=)` sets
what `batch` falls back to.
"""
import ctypes as C
import re

import numpy as np
import torch

from . import _lib
from .ragged_lines import RaggedLines
from .word_forms import WordForms, occurrence_lists

ALL_ZERO, UNKNOWN = "ALL_ZERO", "_UNKNOWN"
# embedding_utils.get_idx (utils/embedding_utils.py:13-16, :87-88): three spellings mapped onto a vocabulary entry
_SPECIAL = {"&ndash;": "–", "&mdash;": "—", "@card@": "0"}
MAX_IDS = 8192                  # 2 B C of a batch the kernels take (recon_ctx_batch_supported); the reference's is 7200
MAX_CELLS = 2 ** 31 - 4096      # cells of context_chars the fill kernel takes (int32 flat indices)
_KERNELS = True                 # False: the torch path on every device
_ERR_ID, _ERR_SURFACE, _ERR_HALF, _ERR_MISSING = 1, 2, 4, 8
_TABLES = ("ent_line_ptr", "ent_max_len", "line_start", "line_len", "sf_start", "sf_len", "tok_flat", "tok_word", "tok_chars", "gat_row", "gat_emb")


def word_index(word, word2idx):
    """embedding_utils.get_idx (utils/embedding_utils.py:73-97): exact, lower-cased, a special spelling, one non-word character trimmed
    from either end (and that lower-cased), digit runs -> '0', else the unknown word."""
    word = word.strip()
    if word in word2idx:
        return word2idx[word]
    if word.lower() in word2idx:
        return word2idx[word.lower()]
    if word in _SPECIAL:
        return word2idx[_SPECIAL[word]]
    trimmed = re.sub(r"(^\W|\W$)", "", word)
    if trimmed in word2idx:
        return word2idx[trimmed]
    if trimmed.lower() in word2idx:
        return word2idx[trimmed.lower()]
    no_digits = re.sub(r"([0-9][0-9.,]*)", "0", word)
    if no_digits in word2idx:
        return word2idx[no_digits]
    return word2idx[UNKNOWN]


def _nltk_tokenizers(word_tokenize, sent_tokenize):
    if word_tokenize is not None and sent_tokenize is not None:
        return word_tokenize, sent_tokenize
    try:
        import nltk
    except ImportError:
        raise ImportError("recon_amd.ContextTables.build: nltk is not installed; pass word_tokenize= and sent_tokenize= "
                          "(the reference uses nltk.word_tokenize and nltk.sent_tokenize)") from None
    return word_tokenize or nltk.word_tokenize, sent_tokenize or nltk.sent_tokenize


def entity_lines(name, context_data, data, word_tokenize, sent_tokenize):
    """The lines of get_entity_context_data (utils/context_utils.py:120-152) behind the surface form: the description, 'instance of ...'
    x <= 15, 'also known as ...' x <= 15, each a token list."""
    if data == "wikidata":
        ctx = context_data.get(name, {"desc": "", "instances": [], "aliases": []})
        lines = [word_tokenize(ctx["desc"])] if ctx["desc"] != "" else []
        lines += [word_tokenize("instance of {}".format(i["label"])) for i in ctx["instances"][:15]]
        lines += [word_tokenize("also known as {}".format(i)) for i in ctx["aliases"][:15]]
    elif data == "nyt":
        ctx = context_data.get(name, {"desc": [], "en_instances": [], "alias": []})
        lines = [word_tokenize(s) for s in sent_tokenize(ctx["desc"][0])[:1]] if len(ctx["desc"]) > 0 else []
        lines += [word_tokenize("instance of {}".format(i)) for i in ctx["en_instances"][:15]]
        lines += [word_tokenize("also known as {}".format(i)) for i in ctx["alias"][:15]]
    else:
        raise ValueError("data must be one of ['wikidata', 'nyt'], got: %r" % (data,))
    return lines


class ContextTables:
    """What a dataset's batches are cut from; built by `ContextTables.build`, moved by `.to(device)`."""

    def __init__(self, arrays, dims, gat_mode):
        arrays = dict(arrays)                                          # (the caller's dict stays as it is)
        self.arrays, self.dims, self.gat_mode = arrays, dict(dims), gat_mode
        self.device = arrays["tok_flat"].device
        d = self.dims
        if "tok_form" not in arrays:                                   # arrays from before the forms: derived once, on the host, where the tables are made
            tok_form, form_chars = _forms_of(arrays["tok_chars"].cpu().numpy(), d["pad_char"])
            arrays["tok_form"], arrays["form_chars"] = torch.from_numpy(tok_form).to(self.device), torch.from_numpy(form_chars).to(self.device)
        d["NFm"] = int(arrays["form_chars"].shape[0])
        self._dims_c = (C.c_int64 * 12)(d["Ne"], d["S"], d["V"], d["L"], d["NF"], d["max_sent_len"], d["max_num_contexts"], d["max_char_len"],
                                        d["conv_filter_size"], d["pad_char"], d["G"], d["Ng"])
        self._ptrs_c = _lib.ptr_array([arrays.get(k) for k in _TABLES]) if self.device.type == "cuda" else None

    @classmethod
    def build(cls, entity2idx, context_data, word2idx, char2idx, conv_filter_size, surface_forms, *, word_tokenize=None, sent_tokenize=None,
              data="wikidata", max_sent_len=32, max_num_contexts=32, max_char_len=10, gat=None):
        """-> (tables on the CPU, surface_ids int32 [N, C, 2]).  Runs on the host, once per dataset.  `surface_forms` is the dataset's
        object array [N, C, 2] of token lists (parsing/legacy_sp_models.py:299-326); surface id 0 is ['ALL_ZERO'].
        gat = (gat_entity2idx, gat_embeddings, mode): gat_embeddings maps str(row) (or row) to a vector, or is a matrix.  mode 'all' is
        get_gat_entity_embeddings (:444-453: ALL_ZERO and _UNKNOWN give zeros, an entity missing from gat_entity2idx makes a batch that
        holds it raise KeyError); mode 'selected' is get_selected_gat_entity_embeddings (:455-475: only ALL_ZERO gives zeros, and a
        missing entity takes the GAT row numbered entity2idx['_UNKNOWN'] — the reference's `gat_entity2id.get(..., entity2id[unknown])`
        at :467 indexes the GAT table with an id of the OTHER table; kept as it is)."""
        word_tokenize, sent_tokenize = _nltk_tokenizers(word_tokenize, sent_tokenize)
        idx2entity = {v: k for k, v in entity2idx.items()}
        Ne = max(idx2entity) + 1
        if entity2idx.get(ALL_ZERO) != -1 or min(idx2entity) != -1 or len(idx2entity) != len(entity2idx):
            raise ValueError("entity2idx must map ALL_ZERO to -1 and every other entity to an id of its own, 0 or above")
        # (context_utils.init_random numbers _UNKNOWN len(entities) + 1: the id in front of it has no entity, and the reference's
        # idx2entity raises KeyError on it; here such an id is marked and a batch that holds it raises IndexError)
        tok_id, tok_word, tok_chars = {}, [], []
        pad, unk = char2idx["<PAD>"], char2idx["<UNK>"]

        def intern(tokens):
            out = []
            for w in tokens[:max_sent_len]:
                i = tok_id.get(w)
                if i is None:
                    i = tok_id[w] = len(tok_word)
                    tok_word.append(word_index(w, word2idx))
                    ids = [char2idx[c] if char2idx.get(c, None) is not None else unk for c in w[:max_char_len]]
                    tok_chars.append(ids + [pad] * (max_char_len - len(ids)))
                out.append(i)
            return out

        flat, line_start, line_len, ent_line_ptr, ent_max_len = [], [], [], [0], []
        for e in range(-1, Ne):
            if e not in idx2entity:
                ent_line_ptr.append(len(line_start))
                ent_max_len.append(-1)
                continue
            lines = entity_lines(idx2entity[e], context_data, data, word_tokenize, sent_tokenize)
            if len(lines) > max_num_contexts - 1:
                raise ValueError("entity %r has %d context lines behind its surface form, more than max_num_contexts - 1 = %d (the reference "
                                 "raises IndexError in get_word_indices)" % (idx2entity[e], len(lines), max_num_contexts - 1))
            longest = 0
            for ln in lines:
                ids = intern(ln)
                line_start.append(len(flat))
                line_len.append(len(ids))
                flat.extend(ids)
                longest = max(longest, len(ids))
            ent_line_ptr.append(len(line_start))
            ent_max_len.append(longest)
        L = len(line_start)
        # ---- surface forms, interned by their token tuple; id 0 = ['ALL_ZERO'] (context_utils.py:63)
        sf_id, sf_start, sf_len = {}, [], []

        def surface(tokens):
            key = tuple(tokens)
            i = sf_id.get(key)
            if i is None:
                i = sf_id[key] = len(sf_start)
                ids = intern(list(key))
                sf_start.append(len(flat))
                sf_len.append(len(ids))
                flat.extend(ids)
            return i
        surface([ALL_ZERO])
        sf = np.asarray(surface_forms, dtype=object) if not isinstance(surface_forms, np.ndarray) else surface_forms
        if sf.ndim < 3 or sf.shape[2] != 2:
            raise ValueError("surface_forms must be an object array [N, C, 2] of token lists")
        surface_ids = np.empty(sf.shape[:3], dtype=np.int32)
        for i in range(sf.shape[0]):
            for j in range(sf.shape[1]):
                for k in range(2):
                    surface_ids[i, j, k] = surface(list(sf[i, j, k]))
        i32 = lambda a, shape=None: torch.from_numpy(np.asarray(a if len(a) else [0], dtype=np.int32).reshape(shape or -1))
        tok_form, form_chars = _forms_of(np.asarray(tok_chars, dtype=np.int32).reshape(-1, max_char_len), pad)
        arrays = {"tok_form": torch.from_numpy(tok_form), "form_chars": torch.from_numpy(form_chars), "ent_line_ptr": i32(ent_line_ptr), "ent_max_len": i32(ent_max_len), "line_start": i32(line_start), "line_len": i32(line_len),
                  "sf_start": i32(sf_start), "sf_len": i32(sf_len), "tok_flat": i32(flat), "tok_word": i32(tok_word),
                  "tok_chars": i32(tok_chars, (-1, max_char_len))}
        dims = {"Ne": Ne, "S": len(sf_start), "V": len(tok_word), "L": L, "NF": len(flat), "max_sent_len": max_sent_len,
                "max_num_contexts": max_num_contexts, "max_char_len": max_char_len, "conv_filter_size": conv_filter_size, "pad_char": pad,
                "G": 0, "Ng": 0}
        gat_mode = None
        if gat is not None:
            gat_entity2idx, gat_embeddings, gat_mode = gat
            if gat_mode not in ("all", "selected"):
                raise ValueError("gat mode must be 'all' or 'selected', got %r" % (gat_mode,))
            if isinstance(gat_embeddings, dict):
                keys = sorted(gat_embeddings, key=int)
                row_of = {int(k): r for r, k in enumerate(keys)}
                # the reference writes the JSON lists into a float64 block and casts it: one rounding, double -> float
                emb = np.asarray([gat_embeddings[k] for k in keys], dtype=np.float64).astype(np.float32)
            else:
                emb = np.asarray(gat_embeddings, dtype=np.float64).astype(np.float32)
                row_of = {r: r for r in range(emb.shape[0])}
            G = emb.shape[1]
            unknown_id = entity2idx[UNKNOWN]
            gat_row = np.full(Ne + 1, -1, dtype=np.int32)            # -1: zeros, -2: missing (KeyError in a batch that holds it)
            for e in range(0, Ne):
                if e not in idx2entity:
                    continue
                if gat_mode == "all":
                    if e == unknown_id:
                        continue
                    g = gat_entity2idx.get(idx2entity[e])
                else:
                    g = gat_entity2idx.get(idx2entity[e], unknown_id)
                gat_row[e + 1] = row_of.get(int(g), -2) if g is not None else -2
            arrays["gat_row"] = torch.from_numpy(gat_row)
            arrays["gat_emb"] = torch.from_numpy(emb if emb.shape[0] else np.zeros((1, G), np.float32)).contiguous()
            dims["G"], dims["Ng"] = G, emb.shape[0]
        return cls(arrays, dims, gat_mode), surface_ids

    def to(self, device):
        device = torch.device(device)
        return ContextTables({k: v.to(device) for k, v in self.arrays.items()}, self.dims, self.gat_mode)


def _forms_of(tok_chars, pad):
    """(tok_form int32 [V], form_chars int32 [NFm, mcl]) of tok_chars [V, mcl]: the distinct rows numbered from 1 in first-occurrence
    order behind form 0, the all-pad row of an empty word slot (a token whose row is all pad takes form 0: no two forms are equal)."""
    mcl = tok_chars.shape[1]
    ids = {(pad,) * mcl: 0}
    tok_form = np.empty(tok_chars.shape[0], dtype=np.int32)
    for i, row in enumerate(tok_chars.tolist()):
        tok_form[i] = ids.setdefault(tuple(row), len(ids))
    return (tok_form if len(tok_form) else np.zeros(1, np.int32)), np.asarray(list(ids), dtype=np.int32).reshape(len(ids), mcl)


class StageBBatch:
    """The inputs of one stage-B forward; the fields carry the names of the arguments of RECON.forward.  With `ragged_lines=True`
    context_words and context_chars are [L, .] and context_mask is a `RaggedLines`, in the same three positions; with `word_forms=True`
    context_chars is a `WordForms`."""
    __slots__ = ("unique_entities", "entity_indices", "context_words", "context_chars", "context_mask", "entities_position",
                 "max_occurred_entity_in_batch_pos", "gat_entity_embeddings", "nonzero_gat_entity_embeddings", "nonzero_entity_pos", "gat_mode")

    def model_args(self):
        """What follows (sentence_input, entity_markers, num_entities) in the forward of RECON_EAC (no GAT table), RECON_EAC_KGGAT
        (mode 'all') or RECON (mode 'selected')."""
        a = (self.unique_entities, self.entity_indices, self.context_words, self.context_chars, self.context_mask, self.entities_position,
             self.max_occurred_entity_in_batch_pos)
        if self.gat_mode == "all":
            return a + (self.gat_entity_embeddings,)
        if self.gat_mode == "selected":
            return a + (self.nonzero_gat_entity_embeddings, self.nonzero_entity_pos, self.gat_entity_embeddings)
        return a


def _new(shape, dtype, device):
    """Every output and scratch buffer of a batch comes from here (the tests put guard rows around them)."""
    return torch.empty(shape, dtype=dtype, device=device)


def _raise_flags(err, tables):
    if err & _ERR_ID:
        raise IndexError("recon_amd: entity id outside [-1, %d)" % tables.dims["Ne"])
    if err & _ERR_SURFACE:
        raise IndexError("recon_amd: surface id outside [0, %d)" % tables.dims["S"])
    if err & _ERR_MISSING:
        raise KeyError("recon_amd: the batch holds an entity that gat_entity2idx (or gat_embeddings) does not have")
    if err & _ERR_HALF:
        raise ValueError("recon_amd: a pair with exactly one ALL_ZERO half (the reference builds a ragged nonzero_gat_entity_embeddings)")


class ContextBatcher:
    def __init__(self, tables, ragged_lines=False, word_forms=False):
        """ragged_lines, word_forms: what `batch` does where its arguments of these names are left at None."""
        self.tables, self.ragged_lines, self.word_forms = tables, bool(ragged_lines), bool(word_forms)

    def batch(self, entity_indices, surface_ids, index_dtype=torch.int64, ragged_lines=None, word_forms=None):
        """entity_indices int64 [B, C, 2] (values -1 .. Ne - 1) and surface_ids [B, C, 2] (of `ContextTables.build`), both on the tables'
        device -> StageBBatch.  One host read per call (the header: sizes, the most frequent entity's position, error flags), made
        before the model's forward is queued.  index_dtype: of context_words and context_chars (torch.int64, the reference's, or
        torch.int32: the char-CNN and line-LSTM ops take both, and the char block is half the bytes).
        ragged_lines: context_words [L, T_b] and context_chars [L, W] without the padding lines and a `RaggedLines` as context_mask.
        word_forms: context_chars as a `WordForms` over the rows of either form (S_d in the header: still one read).  None for either:
        the constructor's value.
        IndexError for an id or a surface id outside its table, KeyError for an entity the GAT table lacks, ValueError for a pair with
        exactly one ALL_ZERO half in 'selected' mode — raised from the header's flags; such a value is never used as an address."""
        t = self.tables
        ragged_lines = self.ragged_lines if ragged_lines is None else bool(ragged_lines)
        word_forms = self.word_forms if word_forms is None else bool(word_forms)
        if index_dtype not in (torch.int64, torch.int32):
            raise TypeError("index_dtype must be torch.int64 or torch.int32")
        if entity_indices.dim() != 3 or entity_indices.shape[2] != 2 or surface_ids.shape != entity_indices.shape:
            raise ValueError("entity_indices and surface_ids must both be [B, C, 2]")
        if entity_indices.device != t.device or surface_ids.device != t.device:
            raise RuntimeError("recon_amd: entity_indices, surface_ids and the tables must live on one device")
        ids = entity_indices.to(torch.int64).contiguous()
        n = ids.numel()
        if (_KERNELS and ids.is_cuda and n <= MAX_IDS
                and _lib.lib().recon_ctx_batch_supported(n, t.dims["Ne"], t.dims["S"])):
            if surface_ids.dtype != torch.int32:                       # (a value beyond int32 stays outside the table instead of wrapping into it)
                surface_ids = surface_ids.clamp(-1, 2 ** 31 - 1).to(torch.int32)
            return self._batch_kernels(ids, surface_ids.contiguous(), index_dtype, ragged_lines, word_forms)
        return self._batch_torch(ids, surface_ids.to(torch.int64).contiguous(), index_dtype, ragged_lines, word_forms)

    # ------------------------------------------------------------------------------------------------------------- the kernels
    def _batch_kernels(self, ids, surf, index_dtype, ragged_lines=False, word_forms=False):
        t, L, dev = self.tables, _lib.lib(), ids.device
        B, Cn = ids.shape[0], ids.shape[1]
        npairs, d = B * Cn, t.dims
        mode = {None: 0, "all": 1, "selected": 2}[t.gat_mode]
        hdr = _new((8,), torch.int32, dev)
        uniq = _new((2 * npairs + 1,), torch.int64, dev)
        uinfo = _new((2 * npairs + 1, 2), torch.int32, dev)
        pos = _new((B, Cn, 2), torch.int64, dev)
        nzpos = _new((npairs,), torch.int64, dev)
        slot = _new((npairs,), torch.int32, dev)
        out = StageBBatch()
        with _lib.on_device(dev):
            st = _lib.current_stream()
            _lib.check(L.recon_ctx_batch_index(t._ptrs_c, t._dims_c, ids.data_ptr(), surf.data_ptr(), npairs, mode, uniq.data_ptr(), uinfo.data_ptr(),
                                               pos.data_ptr(), nzpos.data_ptr(), slot.data_ptr(), hdr.data_ptr(), st), "recon_ctx_batch_index")
            if word_forms:                                             # marked and counted in front of the read: S_d is the header's eighth word
                NFm, tok_form, form_chars = d["NFm"], t.arrays["tok_form"], t.arrays["form_chars"]
                nbytes = L.recon_ctx_batch_forms_scratch_bytes(NFm)
                if nbytes == 0:                                        # more table forms than the scan takes
                    return self._batch_torch(ids, surf.to(torch.int64), index_dtype, ragged_lines, word_forms)
                scratch = _new((nbytes // 4,), torch.int32, dev)       # flags, ranks and the list of present forms
                _lib.check(L.recon_ctx_batch_forms_count(t._ptrs_c, t._dims_c, tok_form.data_ptr(), form_chars.data_ptr(), NFm, uniq.data_ptr(),
                                                         uinfo.data_ptr(), npairs, int(ragged_lines), scratch.data_ptr(), hdr.data_ptr(), st),
                           "recon_ctx_batch_forms_count")
            U, T, P, Mnz, max_pos, err, Lr, S_d = hdr.tolist()             # the one host read
            _raise_flags(err, t)
            W = d["conv_filter_size"] - 1 + T * (d["max_char_len"] + d["conv_filter_size"] - 1)
            if U * P * W >= MAX_CELLS:                                 # (beyond the defaults' reach: 8193 entities of 32 x 386 are 1e8 cells)
                return self._batch_torch(ids, surf.to(torch.int64), index_dtype, ragged_lines, word_forms)
            ib = 8 if index_dtype == torch.int64 else 4
            if word_forms:                                             # the words (and the mask or the line map) as below; no char block
                n_rows = Lr if ragged_lines else U * P
                span = d["max_char_len"] + d["conv_filter_size"] - 1
                words = _new((n_rows, T) if ragged_lines else (U, P, T), index_dtype, dev)
                form_rows = _new((S_d, d["conv_filter_size"] - 1 + span), index_dtype, dev)
                slot_form = _new((n_rows * T,), torch.int32, dev)
                line_ptr = row_ent = mask = None
                if ragged_lines:
                    line_ptr, row_ent = _new((U + 1,), torch.int32, dev), _new((Lr,), torch.int32, dev)
                else:
                    mask = _new((U, P), torch.bool, dev)
                _lib.check(L.recon_ctx_batch_fill_forms(t._ptrs_c, t._dims_c, tok_form.data_ptr(), form_chars.data_ptr(), NFm, scratch.data_ptr(),
                                                        uniq.data_ptr(), uinfo.data_ptr(), U, n_rows, P, T, S_d, int(ragged_lines), ib,
                                                        words.data_ptr() if T else None, _lib.ptr(mask), _lib.ptr(line_ptr), _lib.ptr(row_ent),
                                                        form_rows.data_ptr() if S_d else None, slot_form.data_ptr() if n_rows * T else None, st),
                           "recon_ctx_batch_fill_forms")
                if ragged_lines:
                    mask = RaggedLines(line_ptr, U, Lr, P)
                form_ptr, form_slots = occurrence_lists(slot_form, S_d)
                chars = WordForms(form_rows, slot_form, form_ptr, form_slots, n_rows, T, S_d, span, d["conv_filter_size"])
            elif ragged_lines:                                           # the present lines alone: Lr rows, a RaggedLines in the mask's place
                words = _new((Lr, T), index_dtype, dev)
                chars = _new((Lr, W), index_dtype, dev)
                line_ptr = _new((U + 1,), torch.int32, dev)
                row_ent = _new((Lr,), torch.int32, dev)
                _lib.check(L.recon_ctx_batch_fill_ragged(t._ptrs_c, t._dims_c, uniq.data_ptr(), uinfo.data_ptr(), U, Lr, P, T, ib,
                                                         words.data_ptr() if T else None, chars.data_ptr(), line_ptr.data_ptr(), row_ent.data_ptr(),
                                                         st), "recon_ctx_batch_fill_ragged")
                mask = RaggedLines(line_ptr, U, Lr, P)
            else:
                words = _new((U, P, T), index_dtype, dev)
                chars = _new((U, P, W), index_dtype, dev)
                mask = _new((U, P), torch.bool, dev)
                _lib.check(L.recon_ctx_batch_fill(t._ptrs_c, t._dims_c, uniq.data_ptr(), uinfo.data_ptr(), U, P, T, ib,
                                                  words.data_ptr() if T else None, chars.data_ptr(), mask.data_ptr(), st), "recon_ctx_batch_fill")
            gat = nz = None
            if mode:
                gat = _new((B, Cn, 2 * d["G"]), torch.float32, dev)
                if mode == 2:
                    nz = _new((Mnz, 2 * d["G"]), torch.float32, dev)
                _lib.check(L.recon_ctx_batch_gat(t._ptrs_c, t._dims_c, ids.data_ptr(), npairs, slot.data_ptr(), gat.data_ptr(),
                                                 nz.data_ptr() if (nz is not None and Mnz) else None, st), "recon_ctx_batch_gat")
        out.unique_entities, out.entity_indices, out.entities_position = uniq[:U], ids, pos
        out.context_words, out.context_chars, out.context_mask = words, chars, mask
        out.max_occurred_entity_in_batch_pos = int(max_pos)
        out.gat_entity_embeddings, out.nonzero_gat_entity_embeddings = gat, nz
        out.nonzero_entity_pos = nzpos[:Mnz] if mode == 2 else None
        out.gat_mode = t.gat_mode
        return out

    # ------------------------------------------------------------------------------------------------------------- torch primitives
    def _batch_torch(self, ids, surf, index_dtype, ragged_lines=False, word_forms=False):
        t, dev, d, a = self.tables, ids.device, self.tables.dims, self.tables.arrays
        B, Cn = ids.shape[0], ids.shape[1]
        n, Ne, S, G = ids.numel(), d["Ne"], d["S"], d["G"]
        flat_ids, flat_surf = ids.reshape(-1), surf.reshape(-1)
        mode = t.gat_mode
        i64 = dict(dtype=torch.int64, device=dev)
        err = 0
        if n:                                                          # (the flags' host read; the sizes' follows)
            bad_id = (flat_ids < -1) | (flat_ids >= Ne)
            bad_id |= a["ent_max_len"][(flat_ids + 1).clamp(0, Ne)] < 0                # an id that no entity has
            bad_sf = (flat_surf < 0) | (flat_surf >= S)
            checks = [bad_id.any(), bad_sf.any()]
            if mode:
                rows_all = a["gat_row"].to(torch.int64)[(flat_ids + 1).clamp(0, Ne)]
                checks.append(((rows_all == -2) & ~bad_id).any())
                present = (flat_ids != -1).view(-1, 2)
                checks.append((present[:, 0] != present[:, 1]).any() if mode == "selected" else torch.zeros((), dtype=torch.bool, device=dev))
            flags = torch.stack(checks).tolist()
            err = sum(bit for bit, f in zip((_ERR_ID, _ERR_SURFACE, _ERR_MISSING, _ERR_HALF), flags) if f)
        _raise_flags(err, t)
        # ---- unique ids in dict insertion order: a virtual occurrence of -1 at position -1 seeds the dict (context_utils.py:63-64)
        keys = torch.cat((torch.zeros(1, **i64), flat_ids + 1))
        where = torch.arange(-1, n, **i64)
        sorted_keys, inv = torch.unique(keys, return_inverse=True)
        K = sorted_keys.numel()
        first = torch.full((K,), n, **i64).scatter_reduce(0, inv, where, "amin")
        last = torch.full((K,), -1, **i64).scatter_reduce(0, inv, where, "amax")
        count = torch.bincount(inv, minlength=K)
        count[0] -= 1                                                  # key 0 (-1) is the smallest: the virtual occurrence does not count
        order = torch.argsort(first)                                   # first positions are distinct
        rank = torch.empty(K, **i64)
        rank[order] = torch.arange(K, **i64)
        unique_entities = sorted_keys[order] - 1
        count, last = count[order], last[order]
        entities_position = rank[inv[1:]].view(B, Cn, 2)
        top = count.max()
        max_pos = torch.where(count == top, torch.arange(K, **i64), K).min()           # np.argmax: the FIRST maximum
        last_sid = torch.where(last >= 0, flat_surf[last.clamp(min=0)] if n else last, torch.zeros((), **i64))
        # ---- lines
        lp = a["ent_line_ptr"].to(torch.int64)
        key = unique_entities + 1
        nlines = 1 + lp[key + 1] - lp[key]
        longest = torch.maximum(a["ent_max_len"].to(torch.int64)[key], a["sf_len"].to(torch.int64)[last_sid])
        T, P, max_pos = torch.stack((longest.max().clamp(max=d["max_sent_len"]), nlines.max().clamp(max=d["max_num_contexts"]), max_pos)).tolist()
        p = torch.arange(P, **i64)[None, :]
        table_line = (lp[key][:, None] + p - 1).clamp(0, max(d["L"] - 1, 0))
        is_sf, live = p == 0, p < nlines[:, None]
        start = torch.where(is_sf, a["sf_start"].to(torch.int64)[last_sid][:, None], a["line_start"].to(torch.int64)[table_line])
        length = torch.where(is_sf, a["sf_len"].to(torch.int64)[last_sid][:, None], a["line_len"].to(torch.int64)[table_line])
        length = torch.where(live, length, torch.zeros((), **i64)).clamp(max=T)
        tpos = torch.arange(T, **i64)
        has = tpos[None, None, :] < length[:, :, None]
        tok = a["tok_flat"].to(torch.int64)[(start[:, :, None] + tpos).clamp(0, d["NF"] - 1)]
        words = torch.where(has, a["tok_word"].to(torch.int64)[tok], torch.zeros((), **i64)).to(index_dtype)
        mcl, cfs, pad = d["max_char_len"], d["conv_filter_size"], d["pad_char"]
        U = key.numel()
        cells = torch.full((U, P, T, mcl + cfs - 1), pad, **i64)
        cells[..., :mcl] = torch.where(has[..., None], a["tok_chars"].to(torch.int64)[tok], torch.full((), pad, **i64))
        chars = torch.cat((torch.full((U, P, cfs - 1), pad, **i64), cells.view(U, P, T * (mcl + cfs - 1))), dim=2).to(index_dtype)
        table_form = torch.where(has, a["tok_form"].to(torch.int64)[tok], torch.zeros((), **i64)) if word_forms else None       # [U, P, T]; 0: an empty slot
        out = StageBBatch()
        out.unique_entities, out.entity_indices, out.entities_position = unique_entities, ids, entities_position
        out.context_words, out.context_chars, out.context_mask = words, chars, ~live
        if ragged_lines:                                               # the rows under ~mask, entity by entity (boolean indexing: a host read on a GPU)
            out.context_words, out.context_chars = words[live], chars[live]
            out.context_mask = RaggedLines.from_counts(live.sum(1), dev)
            table_form = table_form[live] if word_forms else None
        if word_forms:                                                 # the kernels' numbering: the present table forms, ascending
            present = torch.zeros(d["NFm"], **i64).index_fill_(0, table_form.reshape(-1), 1)
            rank = present.cumsum(0) - 1
            form_of = torch.nonzero(present).squeeze(1)                # (a host read on a GPU)
            lead = torch.full((form_of.numel(), cfs - 1), pad, **i64)
            form_rows = torch.cat((lead, a["form_chars"].to(torch.int64)[form_of], lead), dim=1).to(index_dtype).contiguous()
            slot_form = rank[table_form.reshape(-1)].to(torch.int32).contiguous()
            form_ptr, form_slots = occurrence_lists(slot_form, form_of.numel())
            out.context_chars = WordForms(form_rows, slot_form, form_ptr, form_slots, table_form.shape[0] * (1 if ragged_lines else P), T, form_of.numel(),
                                          mcl + cfs - 1, cfs)
        out.max_occurred_entity_in_batch_pos = int(max_pos)
        out.gat_entity_embeddings = out.nonzero_gat_entity_embeddings = out.nonzero_entity_pos = None
        out.gat_mode = mode
        if mode:
            rows = rows_all if n else torch.zeros(0, **i64)
            halves = torch.where((rows >= 0)[:, None], a["gat_emb"][rows.clamp(min=0)], torch.zeros((), dtype=torch.float32, device=dev))
            out.gat_entity_embeddings = halves.view(B, Cn, 2 * G)
            if mode == "selected":
                pair_present = (flat_ids != -1).view(-1, 2).any(dim=1)
                out.nonzero_entity_pos = torch.nonzero(pair_present).squeeze(1)
                out.nonzero_gat_entity_embeddings = halves.view(-1, 2 * G)[out.nonzero_entity_pos]
        return out
