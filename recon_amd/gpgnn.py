"""Stage-B caller of the propagation path, shaped like the reference's `GPGNN` (models/models.py:85-277):
same constructor, forward signature and state_dict keys (word_embedding.weight, pos_embedding.weight, rnn1.*,
representation_to_adj[.i].weight/bias, identity_transformation, start_embedding, head_indices, tail_indices,
linear3.*), so a checkpoint written by the reference's train.py:415-416 loads unchanged.  The sentence encoder's
embeddings and LSTM run as `pair_sentence_states` (csrc/sent_lstm.hip; the stock PyTorch-ROCm ops where it does not apply), its
per-hop projections as `pair_transitions` (csrc/pair_trans.hip; `F.linear` and the activation where it does not apply); the
block-adjacency construction and the L-hop propagation with its fused head*tail gather run on the HIP kernels of csrc/prop.hip.  The
classifier behind them is `classify`: `linear3` alone where the propagation features are its only input (GPGNN, RECON_EAC), and
`relation_logits` (csrc/rel_head.hip) over the feature blocks where they lie — no `cat`, no `zeros`, no `index_put` — in RECON_EAC_KGGAT
and RECON when `fused_classifier` is on (the stock ops otherwise).  SURVEY.md 8f row N3."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .propagation import (build_block_adjacency, propagate, propagate_blocks, make_start_embedding, make_start_entity_embeddings, get_head_indices,
                          get_tail_indices)
from .char_features import char_word_features, draw_packed_keep
from .context_lstm import context_line_states
from .sentence_lstm import pair_sentence_states
from .transitions import pair_transitions
from .relation_head import relation_logits
from .line_pool import entity_line_pool, entity_line_pool_ragged
from .ragged_lines import RaggedLines
from .word_forms import WordForms, word_form_features
from .pair_groups import PairGroups


def _fused_encode_applies(m, sentence_input, entity_markers, active):
    we, pe = m.word_embedding, m.pos_embedding
    plain = all(type(e) is nn.Embedding and e.max_norm is None and not e.sparse and not e.scale_grad_by_freq for e in (we, pe))
    return (m.fused_sentence_encoder and plain and not we.weight.requires_grad and (not active or (m.packed_word_dropout and m.dropout1.p < 1))
            and sentence_input.dim() == 2 and entity_markers.dim() == 3 and sentence_input.size(1) == m.max_sent_len
            and tuple(entity_markers.shape) == (sentence_input.size(0), m.MAX_EDGES_PER_GRAPH, m.max_sent_len))


def pair_states(m, sentence_input, entity_markers):
    """models/models.py:160-183 (and models/baselines.py:62-84, the same lines): one LSTM pass per (sentence, ordered entity pair) of a model
    with word_embedding, pos_embedding, dropout1 and rnn1; returns [B, C, 2*units1], what `GPGNN.encode` hands to its dropout2 and
    `ContextAware` to its attention.  `pair_sentence_states` where `fused_sentence_encoder` / `packed_word_dropout` allow, the stock ops
    otherwise; there, with `distinct_pair_sequences`, over the `PairGroups` of the batch's markers."""
    B, C = sentence_input.size(0), m.MAX_EDGES_PER_GRAPH
    active = m.training and m.dropout1.p > 0
    if _fused_encode_applies(m, sentence_input, entity_markers, active):
        we = m.word_embedding
        # distinct_pair_sequences: the distinct (sentence, marker row) sequences alone run, one dropout draw each
        groups = PairGroups.from_markers(sentence_input, entity_markers) if getattr(m, "distinct_pair_sequences", False) and B * C else None
        rows = B * C if groups is None else groups.total
        keep = draw_packed_keep(rows, m.max_sent_len, we.embedding_dim, m.dropout1.p, sentence_input.device) if active else None
        return pair_sentence_states(m.rnn1, sentence_input, entity_markers, we.weight, m.pos_embedding.weight, keep,
                                    pos_padding_idx=m.pos_embedding.padding_idx, groups=groups)
    expanded = torch.transpose(sentence_input.expand(C, B, m.max_sent_len), 0, 1)
    word = m.word_embedding(expanded.contiguous().view(-1, m.max_sent_len)).view(B, C, m.max_sent_len, -1)
    word = m.dropout1(word)
    pos = m.pos_embedding(entity_markers.contiguous().view(-1, m.max_sent_len)).view(B, C, m.max_sent_len, -1)
    merged = torch.cat([word, pos], dim=3)
    merged = merged.view(-1, m.max_sent_len, merged.size(-1))
    rnn_output, _ = m.rnn1(merged)
    u = m.p['units1']
    return torch.cat([rnn_output[:, -1, :u], rnn_output[:, 0, u:]], dim=1).view(B, C, -1)


class GPGNN(nn.Module):
    def __init__(self, p, embeddings, max_sent_len, n_out, MAX_EDGES_PER_GRAPH=72):
        super().__init__()
        self.p = p
        n, d, L = p['max_num_nodes'], p['embedding_dim'], p['layer_number']
        self.MAX_EDGES_PER_GRAPH = n * (n - 1) if p.get('max_num_nodes') else MAX_EDGES_PER_GRAPH      # :93-96
        self.max_sent_len = max_sent_len
        self.word_embedding = nn.Embedding(embeddings.shape[0], embeddings.shape[1], padding_idx=0)   # :102-105
        self.word_embedding.weight.data.copy_(torch.from_numpy(embeddings))
        self.word_embedding.weight.requires_grad = False
        self.dropout1 = nn.Dropout(p=p['dropout1'])
        self.pos_embedding = nn.Embedding(4, p['position_emb'], padding_idx=0)                        # :109-110
        nn.init.orthogonal_(self.pos_embedding.weight)
        self.rnn1 = nn.LSTM(batch_first=True, input_size=embeddings.shape[1] + int(p['position_emb']),
                            hidden_size=int(p['units1']), num_layers=int(p['rnn1_layers']),
                            bidirectional=bool(p['bidirectional']))                                   # :113-119
        for parameter in self.rnn1.parameters():
            if len(parameter.size()) >= 2:
                nn.init.orthogonal_(parameter)
        self.dropout2 = nn.Dropout(p=p['dropout1'])
        self.tied = L == 1 or p['projection_style'] == 'tie'                                          # :123-132
        if self.tied:
            self.representation_to_adj = nn.Linear(p['units1'] * 2, (d * 2) ** 2)
            nn.init.xavier_uniform_(self.representation_to_adj.weight)
        else:
            self.representation_to_adj = nn.ModuleList([nn.Linear(p['units1'] * 2, (d * 2) ** 2) for _ in range(L)])
            for lin in self.representation_to_adj:
                nn.init.xavier_uniform_(lin.weight)
        self.identity_transformation = nn.Parameter(torch.eye(d * 2), requires_grad=True)             # :134-135
        self.start_embedding = nn.Parameter(torch.from_numpy(make_start_embedding(n, d)).float(), requires_grad=False)
        self.head_indices = nn.Parameter(torch.LongTensor(get_head_indices(n, d)), requires_grad=False)   # [50,C,2d] as stored
        self.tail_indices = nn.Parameter(torch.LongTensor(get_tail_indices(n, d)), requires_grad=False)
        self.linear3 = nn.Linear(d * 2 * L, n_out)                                                    # :143-146
        nn.init.xavier_uniform_(self.linear3.weight)

    # fused_sentence_encoder: run `encode` as `pair_sentence_states` (csrc/sent_lstm.hip) whenever the embeddings are plain, the word table
    # is frozen and dropout1 is inactive or drawn as packed bits; DESIGN.md section 21 says why this is the default it is.
    # packed_word_dropout (default False): draw dropout1 as packed bits (`draw_packed_keep`), so that training batches run the kernels too.
    # Same distribution, another random stream than the reference's nn.Dropout call: an opt-in, like EntityEmbedding.packed_char_dropout.
    # distinct_pair_sequences (default False): wherever the fused encoder applies, encode each distinct (sentence, marker row) sequence of
    # the batch once (`PairGroups.from_markers`, csrc/pair_groups.hip) and copy its state to the pair slots that share it.  In eval mode
    # and at p = 0 the values are the dense call's.  Under `packed_word_dropout` the slots that share a sequence share ONE draw: each
    # pair's factors still have dropout's distribution, but the joint distribution over a sentence's copies is another one (the dense
    # call draws every copy independently).  That is why it is an opt-in.  DESIGN.md section 35.
    fused_sentence_encoder = True
    packed_word_dropout = False
    distinct_pair_sequences = False

    def encode(self, sentence_input, entity_markers):
        """models/models.py:160-184: one LSTM pass per (sentence, ordered entity pair); returns [B, C, 2*units1]."""
        return self.dropout2(pair_states(self, sentence_input, entity_markers))

    # fused_transitions: run the L per-hop projections of the pair states as `pair_transitions` (csrc/pair_trans.hip) whenever every
    # projection is a plain nn.Linear; DESIGN.md section 22 says why this is the default it is.
    fused_transitions = True

    def transitions(self, rnn_result):
        """[B, C, 2*units1] -> the list of L transition tensors [B, C, (2d)^2] `propagate_blocks` takes.  Tied (models/models.py:186-192): ONE
        tensor under `non-linear`, repeated L times; untied (:240-249): one per hop under `non-linear1`."""
        p, L = self.p, self.p['layer_number']
        name = p['non-linear'] if self.tied else p['non-linear1']
        lins = [self.representation_to_adj] if self.tied else [self.representation_to_adj[i] for i in range(L)]
        if self.fused_transitions and all(type(lin) is nn.Linear for lin in lins):
            Ts = list(pair_transitions(rnn_result, [lin.weight for lin in lins], [lin.bias for lin in lins], name))
        else:
            Ts = []
            for lin in lins:
                T = lin(rnn_result)
                if name != "linear":
                    T = getattr(F, name)(T)
                Ts.append(T)
        return Ts * L if self.tied else Ts

    # fused_classifier: run the classifier as `relation_logits` (csrc/rel_head.hip) whenever linear3 is a plain nn.Linear and there is
    # something to fuse, a second feature block or the scattered one; DESIGN.md section 23 says why this is the default it is.
    fused_classifier = True

    def classify(self, relation, gat=None, scores=None, positions=None):
        """The logits of the feature blocks, in relation's leading shape: `relation` [..., 2d L] alone (models/models.py:213, :234, :275), with the
        KB-GAT columns `gat` behind it (:693-697), and with the scattered block of `scores` [Mnz, n_out] at the rows `positions` behind both
        (:954-966; relation and gat are then [M, .] as `RECON.forward` reshapes them: the positions count rows).  `scores` may be a function without arguments that returns the tensor: the stock lines call it where they call
        `translation_scores` today, after the `zeros` and only when there is a position.  One block is one GEMM and has nothing to fuse
        (DESIGN.md section 22 found the same for the tied projection): it always runs `linear3`."""
        lin = self.linear3
        if self.fused_classifier and type(lin) is nn.Linear and (gat is not None or positions is not None):
            if positions is not None:
                positions = positions.to(relation.device)
                if positions.shape[0] == 0:
                    scores = relation.new_zeros((0, self.W_ent2rel.shape[0]))
                elif callable(scores):
                    scores = scores()
            return relation_logits([relation] if gat is None else [relation, gat], lin.weight, lin.bias, scores, positions)
        if positions is None:
            return lin(relation if gat is None else torch.cat([relation, gat], dim=-1))                                       # :693-694
        block = torch.zeros(relation.shape[:-1] + (self.W_ent2rel.shape[0],), device=relation.device, dtype=relation.dtype)   # :954-958
        if positions.shape[0] > 0:
            block = block.index_put((positions.to(relation.device),), scores() if callable(scores) else scores)
        return lin(torch.cat([relation, gat, block], dim=-1))                                                                # :960-961

    def forward(self, sentence_input, entity_markers, num_entities=None):
        """(B, max_sent_len), (B, C, max_sent_len) -> (B*C, n_out).  Unlike the reference, any batch size works
        (its head/tail index tensors bake in 50, models/models.py:138-142; the kernels take the [C,2d] pattern)."""
        p = self.p
        n, L = p['max_num_nodes'], p['layer_number']
        rnn_result = self.encode(sentence_input, entity_markers)
        B = rnn_result.size(0)
        Ts = self.transitions(rnn_result)
        # :240-274 — block adjacency + propagation; fused (A_l never materialised) where the kernels allow, else build_block_adjacency + propagate
        relation = propagate_blocks(Ts, self.identity_transformation, n, self.start_embedding, p['non-linear1'], self.head_indices[0], self.tail_indices[0])
        return self.classify(relation).view(B * self.MAX_EDGES_PER_GRAPH, -1)


class CharEmbeddings(nn.Module):
    """models/models.py:15-24 (state_dict key `embeddings.weight`)."""

    def __init__(self, vocab_size, embed_dim, drop_out_rate):
        super().__init__()
        self.embeddings = nn.Embedding(vocab_size, embed_dim, padding_idx=0)
        self.dropout = nn.Dropout(drop_out_rate)

    def forward(self, chars):
        return self.dropout(self.embeddings(chars))

    def draw_keep(self, S, Lc, C, device):
        """Dropout factors for the [S, Lc, C] gathered embedding, drawn as `forward` draws them (one nn.Dropout call on a tensor of that
        shape); None in eval mode or at p = 0.  `char_word_features` multiplies them in, so recorded factors can be replayed."""
        if self.training and self.dropout.p > 0:
            return self.dropout(torch.ones(S, Lc, C, dtype=self.embeddings.weight.dtype, device=device))
        return None

    def draw_packed_keep(self, S, Lc, C, device):
        """The same factors one bit each (`char_features.draw_packed_keep`: Bernoulli(1 - p) from a counter-based draw governed by
        torch.manual_seed, NOT the stream nn.Dropout consumes), which `char_word_features` takes into its masked kernels; None in eval
        mode or at p = 0."""
        if self.training and self.dropout.p > 0:
            return draw_packed_keep(S, Lc, C, self.dropout.p, device)
        return None


class EntityEmbedding(nn.Module):
    """Entity attribute context encoder, models/models.py:26-83: every context line of an entity is a word sequence (word
    vectors + char-CNN features) run through an LSTM; the final states of all lines of one entity are convolved and max-pooled
    over the unmasked lines into one vector per entity.  The char-CNN is `char_word_features` (csrc/char_cnn.hip), the word gather and
    the LSTM are `context_line_states` (csrc/ctx_lstm.hip; the stock ops when word_embeddings is not a plain nn.Embedding); the entity-level
    convolution, the line mask and the max over the lines are `entity_line_pool` (csrc/line_pool.hip) when `fused_line_pool` is on and
    conv1d_entity is a plain nn.Conv1d (stride 1, no padding, dilation 1, groups 1, with a bias), the stock ops otherwise.
    Keys: word_embeddings.weight (the caller's table, shared), char_embeddings.embeddings.weight, lstm.*, conv1d.*, conv1d_entity.*.
    packed_char_dropout (default False): draw the char embedding's dropout as packed bits (`CharEmbeddings.draw_packed_keep`), so that
    training batches run the masked char-CNN kernels instead of the op chain.  Same distribution, another random stream than the
    reference's nn.Dropout call: an opt-in, like `iid_keep_draws` of models.SpKBGATModified."""

    packed_char_dropout = False
    # fused_line_pool: run the last three lines of `forward` as `entity_line_pool` (DESIGN.md section 24 has the measurement behind the default)
    fused_line_pool = True

    def __init__(self, input_dim, hidden_dim, layers, is_bidirectional, drop_out_rate, entity_embed_dim, conv_filter_size,
                 entity_conv_filter_size, word_embeddings, char_embed_dim, max_word_len_entity, char_vocab, char_feature_size):
        super().__init__()
        self.input_dim, self.hidden_dim, self.layers = input_dim, hidden_dim, layers
        self.is_bidirectional, self.drop_rate = is_bidirectional, drop_out_rate
        self.word_embeddings = word_embeddings
        self.char_embeddings = CharEmbeddings(len(char_vocab), char_embed_dim, drop_out_rate)
        self.lstm = nn.LSTM(input_dim, hidden_dim, layers, batch_first=True, bidirectional=bool(is_bidirectional))
        self.conv1d = nn.Conv1d(char_embed_dim, char_feature_size, conv_filter_size)
        self.word_span = max_word_len_entity + conv_filter_size - 1      # chars one word occupies in the padded char sequence
        self.conv1d_entity = nn.Conv1d(2 * hidden_dim, entity_embed_dim, entity_conv_filter_size)

    def forward(self, words, chars, conv_mask):
        """words [U, lines, len], chars [U, lines, cfs-1 + len*(max_char+cfs-1)], conv_mask bool [U, lines-ecfs+1] (True = padding
        line) -> [U, entity_embed_dim].  With a `RaggedLines` as the third argument: words [L, len], chars [L, .], the entities'
        present lines alone (`forward_ragged`).  chars may be a `WordForms` over the U lines (or L) rows in either form (`_char_features`)."""
        if isinstance(conv_mask, RaggedLines):
            return self.forward_ragged(words, chars, conv_mask)
        U, lines = words.shape[0], words.shape[1]
        words = words.reshape(U * lines, words.shape[2])
        we = self.word_embeddings
        plain = type(we) is nn.Embedding and we.max_norm is None and not we.sparse and not we.scale_grad_by_freq
        word_vec = None if plain else we(words)
        char_feat = self._char_features(chars if isinstance(chars, WordForms) else chars.reshape(U * lines, chars.shape[2]), words)   # :57-61
        if plain:        # gather, cat, LSTM and the h_n reshape as one op (csrc/ctx_lstm.hip; the stock ops where its kernels do not apply)   # :62-70
            h_n = context_line_states(self.lstm, char_feat, words, we.weight, padding_idx=we.padding_idx).reshape(U, lines, 2 * self.hidden_dim)
        else:
            _, (h_n, _) = self.lstm(torch.cat((word_vec, char_feat), -1))
            # last layer, both directions side by side (the reference reshapes to (layers, 2, batch, hidden): bidirectional only)
            h_n = h_n.view(self.layers, 2, U * lines, self.hidden_dim)[-1].permute(1, 0, 2).reshape(U, lines, 2 * self.hidden_dim)
        ce = self.conv1d_entity
        if (self.fused_line_pool and type(ce) is nn.Conv1d and ce.bias is not None and ce.stride == (1,) and ce.padding == (0,)
                and ce.dilation == (1,) and ce.groups == 1):                                                                # :73-81
            return entity_line_pool(h_n, ce.weight, ce.bias, conv_mask)
        conv = self.conv1d_entity(h_n.permute(0, 2, 1))
        conv = conv.masked_fill(conv_mask.unsqueeze(1), -float('inf'))
        return conv.max(dim=2).values

    def _char_features(self, chars, words):
        """[rows, len, char_feature_size] of chars [rows, .] or of a `WordForms` over the rows of words [rows, len] (models/models.py:57-61).
        With a `WordForms` the char-CNN runs over the S_d distinct windows and the dropout factors are drawn for them: every occurrence
        of a form in the batch shares one draw, where the dense block draws per slot — another distribution, hence an opt-in of the
        batcher (`word_forms=True`).  In eval mode or at p = 0 the result is the dense call's."""
        emb = self.char_embeddings
        draw = emb.draw_packed_keep if self.packed_char_dropout else emb.draw_keep
        weights = (emb.embeddings.weight, self.conv1d.weight, self.conv1d.bias)
        if isinstance(chars, WordForms):
            if (chars.rows, chars.T) != tuple(words.shape) or chars.word_span != self.word_span or chars.cfs != self.conv1d.kernel_size[0]:
                raise ValueError("EntityEmbedding: %r does not fit words %s with word_span = %d, cfs = %d"
                                 % (chars, tuple(words.shape), self.word_span, self.conv1d.kernel_size[0]))
            keep = draw(chars.total, chars.chars.shape[1], emb.embeddings.embedding_dim, chars.device)
            return word_form_features(chars, *weights, keep=keep, padding_idx=emb.embeddings.padding_idx)
        keep = draw(chars.shape[0], chars.shape[1], emb.embeddings.embedding_dim, chars.device)
        return char_word_features(chars, *weights, self.word_span, keep=keep, padding_idx=emb.embeddings.padding_idx)

    def forward_ragged(self, words, chars, lines):
        """words [L, len], chars [L, cfs-1 + len*(max_char+cfs-1)], lines a RaggedLines over the L rows -> [U, entity_embed_dim]: `forward`
        without the padding lines.  The char-CNN and the line LSTM run over the L present lines, and
        `entity_line_pool_ragged` finds an entity's states by offset; where conv1d_entity is not plain (or `fused_line_pool` is off) the
        states are padded for the stock pool.  A padding line never reaches `forward`'s output (its position is masked to -inf in front
        of the max) and gets a zero gradient, so the results are those of the padded call.  Dropout: the char embedding's factors are
        drawn for L rows — the same distribution on another random stream than a padded batch draws from, the standing of
        `packed_char_dropout`."""
        forms = isinstance(chars, WordForms)
        shapes_fit = words.dim() == 2 and (forms or chars.dim() == 2)
        rows_fit = shapes_fit and words.shape[0] == lines.total and (chars.rows if forms else chars.shape[0]) == lines.total
        if not rows_fit:
            raise ValueError("EntityEmbedding: with a RaggedLines, words and chars must be [L, .] with L = %d rows, got %s and %s"
                             % (lines.total, tuple(words.shape), chars if forms else tuple(chars.shape)))
        we = self.word_embeddings
        plain = type(we) is nn.Embedding and we.max_norm is None and not we.sparse and not we.scale_grad_by_freq
        char_feat = self._char_features(chars, words)
        if plain:
            h_n = context_line_states(self.lstm, char_feat, words, we.weight, padding_idx=we.padding_idx)
        else:
            _, (h_n, _) = self.lstm(torch.cat((we(words), char_feat), -1))
            h_n = h_n.view(self.layers, 2, lines.total, self.hidden_dim)[-1].permute(1, 0, 2)
        h_n = h_n.reshape(lines.total, 2 * self.hidden_dim)
        ce = self.conv1d_entity
        if (self.fused_line_pool and type(ce) is nn.Conv1d and ce.bias is not None and ce.stride == (1,) and ce.padding == (0,)
                and ce.dilation == (1,) and ce.groups == 1):
            return entity_line_pool_ragged(h_n, lines, ce.weight, ce.bias)
        Ln = max(lines.n_max, ce.kernel_size[0] if isinstance(ce, nn.Conv1d) else 1)
        conv = ce(lines.pad(h_n, Ln).permute(0, 2, 1))
        conv = conv.masked_fill(lines.to_mask(Ln, Ln - conv.shape[2] + 1).unsqueeze(1), -float('inf'))
        return conv.max(dim=2).values


class RECON_EAC(GPGNN):
    """The reference's `RECON_EAC` (models/models.py:279-487): GPGNN whose start embedding is built PER BATCH from the entity
    attribute context (`EntityEmbedding` -> `make_start_entity_embeddings`, utils/context_utils.py:387-426) instead of the
    fixed one-hot template.  Same constructor, forward signature and state_dict keys (GPGNN's plus entity_embedding_module.*).
    The per-batch start vectors, the block adjacency and the L-hop propagation run on the HIP kernels of csrc/prop.hip; the classifier
    is `linear3` alone (`classify` with one block: one GEMM has nothing to fuse).

    Two places where the reference's code cannot be followed literally: its tied-projection branch (:401-445) hard-codes
    9 nodes AND ignores the context embeddings (it propagates the fixed template) — kept as is, through GPGNN.forward; and its
    head / tail index tensors bake in `batch_size` — the kernels take the [C,2d] pattern, so any batch size runs."""

    def __init__(self, p, embeddings, max_sent_len, n_out, char_vocab, MAX_EDGES_PER_GRAPH=72):
        super().__init__(p, embeddings, max_sent_len, n_out, MAX_EDGES_PER_GRAPH)
        n, d = p['max_num_nodes'], p['embedding_dim']
        self.head_indices = nn.Parameter(torch.LongTensor(get_head_indices(n, d, bs=p['batch_size'])), requires_grad=False)   # :338-342
        self.tail_indices = nn.Parameter(torch.LongTensor(get_tail_indices(n, d, bs=p['batch_size'])), requires_grad=False)
        self.entity_embedding_module = EntityEmbedding(
            p['char_embed_dim'] + embeddings.shape[1], p['hidden_dim_ent'], p['num_entEmb_layers'], p['is_bidirectional_ent'],
            p['drop_out_rate_ent'], p['entity_embed_dim'], p['conv_filter_size'], p['entity_conv_filter_size'], self.word_embedding,
            p['char_embed_dim'], p['max_char_len'], char_vocab, p['char_feature_size'])

    def relation_features(self, sentence_input, entity_markers, context_words, context_chars, context_mask, entities_position,
                          max_occurred_entity_in_batch_pos):
        """Untied branch up to the classifier (:365-484): [B, C, 2d L] head*tail features of every hop."""
        p = self.p
        n, L = p['max_num_nodes'], p['layer_number']
        entity_embeddings = self.entity_embedding_module(context_words, context_chars, context_mask)
        h0 = make_start_entity_embeddings(entity_embeddings, entities_position, None, p['embedding_dim'],
                                          max_occurred_entity_in_batch_pos, self.start_embedding, max_num_nodes=n)     # :365
        rnn_result = self.encode(sentence_input, entity_markers)
        Ts = self.transitions(rnn_result)                                # :447-466
        return propagate_blocks(Ts, self.identity_transformation, n, h0, p['non-linear1'], self.head_indices[0], self.tail_indices[0])     # :447-484

    def forward(self, sentence_input, entity_markers, num_entities, unique_entites, entity_indices, context_words, context_chars,
                context_mask, entities_position, max_occurred_entity_in_batch_pos):
        if self.tied:
            return GPGNN.forward(self, sentence_input, entity_markers, num_entities)
        relation = self.relation_features(sentence_input, entity_markers, context_words, context_chars, context_mask, entities_position,
                                          max_occurred_entity_in_batch_pos)
        return self.classify(relation).view(relation.size(0) * self.MAX_EDGES_PER_GRAPH, -1)


class RECON_EAC_KGGAT(RECON_EAC):
    """The reference's `RECON_EAC_KGGAT` (models/models.py:489-701): RECON_EAC whose classifier also sees the stage-A KB-GAT
    embeddings of each pair's head and tail entity (`gat_entity_embeddings` [B, C, 2 * gat_entity_embedding_dim], concatenated
    behind the propagation features, :693-697).  With `fused_classifier` on, `classify` runs `linear3` over the two blocks where they
    lie (`relation_logits`, csrc/rel_head.hip: no `cat`, no gradient for the KB-GAT columns); otherwise `cat` and `linear3` as there.
    Same constructor, forward signature and state_dict keys as the reference.

    The reference's tied-projection branch (:597-649) feeds the propagation features alone to a classifier sized for the
    concatenation and fails in `linear3`; here it fails with the same exception type before any work is done."""

    def __init__(self, p, embeddings, max_sent_len, n_out, char_vocab, MAX_EDGES_PER_GRAPH=72):
        super().__init__(p, embeddings, max_sent_len, n_out, char_vocab, MAX_EDGES_PER_GRAPH)
        self.linear3 = nn.Linear(p['embedding_dim'] * 2 * p['layer_number'] + 2 * p['gat_entity_embedding_dim'], n_out)      # :547-549
        nn.init.xavier_uniform_(self.linear3.weight)

    def forward(self, sentence_input, entity_markers, num_entities, unique_entites, entity_indices, context_words, context_chars,
                context_mask, entities_position, max_occurred_entity_in_batch_pos, gat_entity_embeddings):
        if self.tied:
            raise RuntimeError("RECON_EAC_KGGAT: the tied projection feeds %d features to a classifier built for %d (models/models.py:622, :647)"
                               % (self.p['embedding_dim'] * 2 * self.p['layer_number'], self.linear3.in_features))
        relation = self.relation_features(sentence_input, entity_markers, context_words, context_chars, context_mask, entities_position,
                                          max_occurred_entity_in_batch_pos)
        logits = self.classify(relation, gat_entity_embeddings.to(relation.dtype))                                         # :693-697
        return logits.view(relation.size(0) * self.MAX_EDGES_PER_GRAPH, -1)


class RECON(RECON_EAC):
    """The reference's full model `RECON` (models/models.py:703-968): RECON_EAC + the KB-GAT entity embeddings of every pair +
    a per-relation triple score in the relation space of GAT_sep_space: for each pair with known embeddings,
    `|| tanh(head W_r) + g_r - tanh(tail W_r) ||_1` for every output relation r (:940-958), scattered into a [B*C, n_out]
    block behind the other features.  With `fused_classifier` on, `classify` hands the scores and their positions to `relation_logits`
    (csrc/rel_head.hip), which runs `linear3` over the three blocks without the `zeros`, the `index_put` or the `cat`; otherwise the
    stock lines.  Constructor arguments, forward signature and state_dict keys follow the reference
    (`gat_relation_embeddings` trainable, `W_ent2rel` frozen; head / tail index tensors are plain attributes there, :759-768,
    and non-persistent buffers here so that `.to(device)` moves them and checkpoints stay key-compatible).

    `gat_relation_embeddings` is the dict the reference loads from JSON (string index -> vector), `W_ent2rel_all_rels` the
    [n_gat_rel, ent_dim, rel_dim] array, `idx2property` output index -> property, `gat_relation2idx` property -> string index."""

    def __init__(self, p, embeddings, max_sent_len, n_out, char_vocab, gat_relation_embeddings, W_ent2rel_all_rels, idx2property,
                 gat_relation2idx, MAX_EDGES_PER_GRAPH=72):
        super().__init__(p, embeddings, max_sent_len, n_out, char_vocab, MAX_EDGES_PER_GRAPH)
        n, d, L = p['max_num_nodes'], p['embedding_dim'], p['layer_number']
        head, tail = self.head_indices.data, self.tail_indices.data
        del self.head_indices, self.tail_indices
        self.register_buffer("head_indices", head, persistent=False)
        self.register_buffer("tail_indices", tail, persistent=False)
        self.linear3 = nn.Linear(d * 2 * L + 2 * p['gat_entity_embedding_dim'] + n_out, n_out)                               # :772-773
        nn.init.xavier_uniform_(self.linear3.weight)
        W_all = torch.as_tensor(W_ent2rel_all_rels, dtype=torch.float32)
        rel0 = torch.zeros(n_out, len(gat_relation_embeddings["0"]))                                                        # :779-785
        W0 = torch.zeros(n_out, W_all.shape[1], W_all.shape[2])                                                             # :787-793
        for i in range(n_out):
            gat_idx = gat_relation2idx.get(idx2property[i], None)
            if gat_idx is not None:
                rel0[i] = torch.as_tensor(gat_relation_embeddings[gat_idx], dtype=torch.float32)
                W0[i] = W_all[int(gat_idx)]
        self.gat_relation_embeddings = nn.Parameter(rel0, requires_grad=True)
        self.W_ent2rel = nn.Parameter(W0, requires_grad=False)

    def translation_scores(self, nonzero_gat_entity_embeddings):
        """[M, 2 ent_dim] (head | tail) -> [M, n_out] L1 translation residuals in each output relation's space (:934-953):
        `translation_residuals` on the two halves, read in place (one fused launch; W_ent2rel is frozen, the gradient is
        gat_relation_embeddings')."""
        from .translation import translation_residuals
        W = self.W_ent2rel
        half = nonzero_gat_entity_embeddings.shape[-1] // 2
        emb = nonzero_gat_entity_embeddings.to(device=W.device, dtype=W.dtype)
        return translation_residuals(emb[:, :half], emb[:, half:], W, self.gat_relation_embeddings)

    def forward(self, sentence_input, entity_markers, num_entities, unique_entites, entity_indices, context_words, context_chars,
                context_mask, entities_position, max_occurred_entity_in_batch_pos, nonzero_gat_entity_embeddings, nonzero_entity_pos,
                gat_entity_embeddings):
        if self.tied:
            raise RuntimeError("RECON: the tied projection feeds %d features to a classifier built for %d (models/models.py:836, :861)"
                               % (self.p['embedding_dim'] * 2 * self.p['layer_number'], self.linear3.in_features))
        relation = self.relation_features(sentence_input, entity_markers, context_words, context_chars, context_mask, entities_position,
                                          max_occurred_entity_in_batch_pos)
        rows = relation.size(0) * self.MAX_EDGES_PER_GRAPH
        relation = relation.reshape(rows, -1)                                                                               # :926
        gat = gat_entity_embeddings.to(relation.dtype).reshape(rows, -1)                                                    # :927
        # (no pair with known embeddings: an all-zero score block, whatever the positions hold)
        positions = nonzero_entity_pos if nonzero_gat_entity_embeddings.shape[0] > 0 else nonzero_entity_pos[:0]
        return self.classify(relation, gat, lambda: self.translation_scores(nonzero_gat_entity_embeddings), positions)     # :954-966
