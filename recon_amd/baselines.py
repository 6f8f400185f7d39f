"""The baselines of the stage-B result tables, shaped like the reference's classes of models/baselines.py: same constructors and the same
state_dict keys, so a checkpoint of the reference loads with strict=True.

`ContextAware` (:10-119, the model of "Context-Aware Representations for Knowledge Base Relation Extraction", thirteen keys) takes what
GPGNN takes, (sentence_input [B, T], entity_markers [B, C, T]), so `run_epoch` trains and scores it as it does GPGNN.  Its encoder is
`gpgnn.pair_states` (csrc/sent_lstm.hip), the attention over ghosts `pair_context_attention` (csrc/pair_attn.hip) and the head a plain
nn.Linear.  DESIGN.md section 30.

`LSTM` (:122-188, thirteen keys), `CNN` (:190-252, ten keys) and `PCNN` (:254-314, six keys) read one pair per row from the per-pair
preprocessing (train.py:301-307).  `LSTM`'s encoder is `gpgnn.pair_states` with one pair per row; `CNN` and `PCNN` run their gathers,
convolutions, pool, pooled dropout and activation as `sentence_conv_pool` (csrc/sent_conv.hip) and keep `linear1` a stock nn.Linear.
DESIGN.md section 31."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .gpgnn import pair_states
from .char_features import draw_packed_keep
from .pair_attention import pair_context_attention
from .sentence_conv import sentence_conv_pool


class ContextAware(nn.Module):
    def __init__(self, p, embeddings, max_sent_len, n_out, MAX_EDGES_PER_GRAPH=72):
        super().__init__()
        self.p = p
        n = p.get('max_num_nodes')
        self.MAX_EDGES_PER_GRAPH = n * (n - 1) if n else MAX_EDGES_PER_GRAPH                          # :20-23
        self.max_sent_len = max_sent_len
        self.word_embedding = nn.Embedding(embeddings.shape[0], embeddings.shape[1], padding_idx=0)   # :29-32
        self.word_embedding.weight.data.copy_(torch.from_numpy(embeddings))
        self.word_embedding.weight.requires_grad = False
        self.dropout1 = nn.Dropout(p=p['dropout1'])
        self.pos_embedding = nn.Embedding(4, p['position_emb'], padding_idx=0)                        # :36-37
        nn.init.orthogonal_(self.pos_embedding.weight)
        self.rnn1 = nn.LSTM(embeddings.shape[1] + int(p['position_emb']), int(p['units1']), num_layers=int(p['rnn1_layers']),
                            batch_first=True, bidirectional=bool(p['bidirectional']))                 # :40-41
        self.linear1 = nn.Linear(in_features=p['units1'] * 2, out_features=p['units1'] * 2, bias=False)   # :43-46
        nn.init.xavier_uniform_(self.linear1.weight)
        self.dropout2 = nn.Dropout(p=p['dropout1'])
        self.linear2 = nn.Linear(in_features=p['units1'] * 4, out_features=n_out)                     # :49-51
        nn.init.xavier_uniform_(self.linear2.weight)

    # fused_sentence_encoder, packed_word_dropout, distinct_pair_sequences: GPGNN's switches of the same names (`gpgnn.pair_states` reads
    # them).  distinct_pair_sequences is an opt-in for GPGNN's reason: under packed dropout the pair slots that share a sequence share one draw.
    fused_sentence_encoder = True
    packed_word_dropout = False
    distinct_pair_sequences = False
    # fused_ghost_attention: run the attention over ghosts as `pair_context_attention` (csrc/pair_attn.hip) whenever linear1 is a plain
    # bias-free nn.Linear; DESIGN.md section 30 has the measurement behind the default.
    fused_ghost_attention = True

    def ghost_attention(self, rnn_result):
        """[B, C, 2*units1] -> [B, C, 4*units1]: every pair's state beside the attention-weighted sum of the other pairs' (:86-112)."""
        lin = self.linear1
        if self.fused_ghost_attention and type(lin) is nn.Linear and lin.bias is None:
            return pair_context_attention(rnn_result, lin.weight)
        C = rnn_result.size(1)
        layers_to_concat = []
        for i in range(C):
            sentence_vector = rnn_result[:, i, :]
            target_sentence_memory = lin(sentence_vector)
            context_vectors = torch.cat([rnn_result[:, :i, :], rnn_result[:, i + 1:, :]], dim=1)
            sentence_scores = torch.matmul(target_sentence_memory.unsqueeze(1).unsqueeze(1), context_vectors.unsqueeze(3)).squeeze(-1).squeeze(-1)
            sentence_scores = F.softmax(sentence_scores, dim=1)
            # (the reference's bare .squeeze() at :107 also drops a batch axis of one; squeeze(1) keeps it)
            context_vector = torch.matmul(sentence_scores.unsqueeze(1), context_vectors).squeeze(1)
            layers_to_concat.append(torch.cat([sentence_vector, context_vector], dim=1).unsqueeze(1))
        return torch.cat(layers_to_concat, dim=1)

    def forward(self, sentence_input, entity_markers, num_entities=None):
        """(B, max_sent_len), (B, C, max_sent_len) -> (B*C, n_out).  num_entities is ignored (`run_epoch` passes it to every model).  Unlike
        the reference, a batch of one works."""
        rnn_result = pair_states(self, sentence_input, entity_markers)                                # :62-84
        edge_vectors = self.ghost_attention(rnn_result)
        edge_vectors = edge_vectors.reshape(sentence_input.size(0) * self.MAX_EDGES_PER_GRAPH, -1)
        return self.linear2(self.dropout2(edge_vectors))                                              # :115-119


class LSTM(nn.Module):
    def __init__(self, p, embeddings, max_sent_len, n_out):
        super().__init__()
        self.p = p
        self.MAX_EDGES_PER_GRAPH = 1                                                                  # one pair per row
        self.max_sent_len = max_sent_len
        self.word_embedding = nn.Embedding(embeddings.shape[0], embeddings.shape[1], padding_idx=0)   # :137-140
        self.word_embedding.weight.data.copy_(torch.from_numpy(embeddings))
        self.word_embedding.weight.requires_grad = False
        self.dropout1 = nn.Dropout(p=p['dropout1'])
        self.pos_embedding = nn.Embedding(4, p['position_emb'], padding_idx=0)                        # :144
        self.rnn1 = getattr(nn, p.get('rnn1', 'LSTM'))(batch_first=True, input_size=embeddings.shape[1] + int(p['position_emb']),
                                                       hidden_size=int(p['units1']), num_layers=int(p['rnn1_layers']),
                                                       bidirectional=bool(p['bidirectional']))        # :147-154
        for parameter in self.rnn1.parameters():
            if len(parameter.size()) >= 2:
                nn.init.orthogonal_(parameter)
        self.linear1 = nn.Linear(in_features=p['units1'], out_features=p['units1'], bias=False)      # :156-158 (unused, as there)
        nn.init.xavier_uniform_(self.linear1.weight)
        self.dropout2 = nn.Dropout(p=p['dropout1'])
        self.linear2 = nn.Linear(in_features=p['units1'] * 2, out_features=n_out)                     # :161-163
        nn.init.xavier_uniform_(self.linear2.weight)

    # GPGNN's switches of the same names (`gpgnn.pair_states` reads them)
    fused_sentence_encoder = True
    packed_word_dropout = False

    def forward(self, sentence_input, entity_markers):
        """(B, max_sent_len), (B, max_sent_len) -> (B, n_out) (:175-188)."""
        rnn_result = pair_states(self, sentence_input, entity_markers.unsqueeze(1)).reshape(sentence_input.size(0), -1)
        return self.linear2(self.dropout2(rnn_result))


class _SentenceConv(nn.Module):
    """What CNN and PCNN share: the three embeddings, dropout1 on the word rows and again on the pooled values, and `linear1`."""

    # fused_sentence_conv: run the stretch in front of linear1 as `sentence_conv_pool` (csrc/sent_conv.hip); DESIGN.md section 31 has the
    # measurement behind the default.  packed_word_dropout: GPGNN's switch; on, the word factors are a `draw_packed_keep` (another random
    # stream); off, they are torch's own draw handed to the op as fp32 factors (the reference's stream).
    fused_sentence_conv = True
    packed_word_dropout = False

    def _embeddings(self, p, embeddings, max_sent_len):
        self.p = p
        self.max_sent_len = max_sent_len
        self.word_embedding = nn.Embedding(embeddings.shape[0], embeddings.shape[1], padding_idx=0)
        self.word_embedding.weight.data.copy_(torch.from_numpy(embeddings))
        self.word_embedding.weight.requires_grad = False
        self.dropout1 = nn.Dropout(p=p['dropout1'])
        self.pos_embedding_0 = nn.Embedding(2 * max_sent_len + 1, p['position_emb'], padding_idx=0)
        self.pos_embedding_1 = nn.Embedding(2 * max_sent_len + 1, p['position_emb'], padding_idx=0)
        return embeddings.shape[1] + p['position_emb'] * 2

    def _pooled(self, convs, activation, sentence_input, entity_markers, segments=None):
        we, p0, p1 = self.word_embedding, self.pos_embedding_0, self.pos_embedding_1
        B, T = sentence_input.shape
        active = self.training and self.dropout1.p > 0
        n_out = (3 if segments is not None else len(convs)) * convs[0].out_channels
        plain = all(type(e) is nn.Embedding and e.max_norm is None and not e.sparse and not e.scale_grad_by_freq for e in (we, p0, p1)) \
            and all(type(c) is nn.Conv1d and c.bias is not None and c.stride == (1,) and c.dilation == (1,) and c.groups == 1
                    and c.padding_mode == 'zeros' for c in convs) and p0.padding_idx == p1.padding_idx
        if self.fused_sentence_conv and plain and self.dropout1.p < 1:
            keep = pool_keep = None
            if active:
                if self.packed_word_dropout:
                    keep = draw_packed_keep(B, T, we.embedding_dim, self.dropout1.p, sentence_input.device)
                else:
                    keep = self.dropout1(torch.ones(B, T, we.embedding_dim, dtype=we.weight.dtype, device=sentence_input.device))
                # (the reference draws the pooled factors once per window in CNN, once over the three segments in PCNN: the same draws here)
                ones = torch.ones(B, n_out if segments is not None else convs[0].out_channels, dtype=we.weight.dtype, device=sentence_input.device)
                pool_keep = self.dropout1(ones) if segments is not None else torch.cat([self.dropout1(ones) for _ in convs], dim=1)
            return sentence_conv_pool(sentence_input, entity_markers, we.weight, p0.weight, p1.weight, [c.weight for c in convs],
                                      [c.bias for c in convs], segments=None if segments is None else segments.to(we.weight.dtype),
                                      keep=keep, pool_keep=pool_keep, activation=activation, pos_padding_idx=p0.padding_idx)
        word_embeddings = self.dropout1(we(sentence_input.long()))
        merged = torch.cat([word_embeddings, p0(entity_markers[:, 0, :].long()), p1(entity_markers[:, 1, :].long())], dim=2).transpose(1, 2)
        act = torch.tanh if activation == "tanh" else torch.relu
        if segments is None:
            return torch.cat([act(self.dropout1(torch.max(c(merged), dim=2)[0])) for c in convs], dim=1)
        conv = convs[0](merged)
        return act(self.dropout1(torch.cat([torch.max(conv * segments[:, s].unsqueeze(1), dim=2)[0] for s in range(3)], dim=1)))


class CNN(_SentenceConv):
    def __init__(self, p, embeddings, max_sent_len, n_out):
        super().__init__()
        cin = self._embeddings(p, embeddings, max_sent_len)                                           # :205-213
        self.cnn_3 = nn.Conv1d(cin, p['units1'], p['window_size'], bias=True)                         # :216-221
        self.cnn_5 = nn.Conv1d(cin, p['units1'], 5, bias=True)
        self.cnn_7 = nn.Conv1d(cin, p['units1'], 7, bias=True)
        for c in (self.cnn_3, self.cnn_5, self.cnn_7):
            nn.init.xavier_uniform_(c.weight)
        self.linear1 = nn.Linear(in_features=p['units1'] * 3, out_features=n_out, bias=False)         # :223-225
        nn.init.xavier_uniform_(self.linear1.weight)

    def forward(self, sentence_input, entity_markers):
        """(B, max_sent_len), (B, 2, max_sent_len) -> (B, n_out) (:237-252)."""
        return self.linear1(self._pooled([self.cnn_3, self.cnn_5, self.cnn_7], "tanh", sentence_input, entity_markers))


class PCNN(_SentenceConv):
    def __init__(self, p, embeddings, max_sent_len, n_out):
        super().__init__()
        cin = self._embeddings(p, embeddings, max_sent_len)                                           # :269-277
        self.cnn = nn.Conv1d(cin, p['units1'], p['window_size'], bias=True, padding=int(p['window_size'] / 2))    # :280-281
        nn.init.xavier_uniform_(self.cnn.weight)
        self.linear1 = nn.Linear(in_features=p['units1'] * 3, out_features=n_out, bias=False)         # :283-285
        nn.init.xavier_uniform_(self.linear1.weight)

    def forward(self, sentence_input, entity_markers, pcnn_mask):
        """(B, max_sent_len), (B, 2, max_sent_len), (B, 3, max_sent_len) -> (B, n_out) (:297-314)."""
        return self.linear1(self._pooled([self.cnn], "relu", sentence_input, entity_markers, pcnn_mask))
