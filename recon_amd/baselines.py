"""The baseline of the stage-B result tables, shaped like the reference's `ContextAware` (models/baselines.py:10-119, the model of
"Context-Aware Representations for Knowledge Base Relation Extraction"): same constructor and the same thirteen state_dict keys
(word_embedding.weight, pos_embedding.weight, rnn1.*, linear1.weight, linear2.weight, linear2.bias), so a checkpoint of the reference
loads with strict=True.  It takes what GPGNN takes, (sentence_input [B, T], entity_markers [B, C, T]), so `run_epoch` trains and scores
it as it does GPGNN.  The encoder is `gpgnn.pair_states` (csrc/sent_lstm.hip), the attention over ghosts `pair_context_attention`
(csrc/pair_attn.hip) and the head a plain nn.Linear.  The other baselines (LSTM, CNN, PCNN) read one pair per row from another
preprocessing and are not here.  DESIGN.md section 30."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .gpgnn import pair_states
from .pair_attention import pair_context_attention


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

    # fused_sentence_encoder, packed_word_dropout: GPGNN's switches of the same names (`gpgnn.pair_states` reads them).
    fused_sentence_encoder = True
    packed_word_dropout = False
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
