"""Fixture of the entity-context line LSTM (tests/golden/ctx_lstm1.npz), written where the reference tree is available.

The reference's own `models.models.EntityEmbedding` (models/models.py:26-83) is built at U = 3 entities, 4 context lines of 3 words, word
vectors of 4 (a TRAINABLE table of 7 rows), char features of 6, hidden 3, in eval mode and in fp64, and run on random ids.  Recorded: the
inputs, the module's output, the upstream gradient G of (out * G).sum(), the state_dict and the gradient of EVERY parameter, lstm.* and
word_embeddings.weight included (char_features1_eval.npz holds the char-CNN's three only).  Arrays only; nothing of the reference's text
is stored.
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
U, LINES, WORDS, MAX_CHAR, CFS, C, FO, V, HIDDEN, WORD_DIM, N_WORDS, ENT_DIM, ECFS = 3, 4, 3, 4, 3, 5, 6, 9, 3, 4, 7, 5, 2


def _case(ref_models, name, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    word_emb = nn.Embedding(N_WORDS, WORD_DIM, padding_idx=0)
    m = ref_models.EntityEmbedding(WORD_DIM + FO, HIDDEN, 1, 1, 0.0, ENT_DIM, CFS, ECFS, word_emb, C, MAX_CHAR, list(range(V)), FO)
    m.double().eval()
    span = MAX_CHAR + CFS - 1
    chars = torch.zeros(U * LINES, CFS - 1 + WORDS * span, dtype=torch.int64)
    for s in range(U * LINES):
        for w in range(int(torch.randint(0, WORDS + 1, (1,), generator=g))):
            n = int(torch.randint(1, MAX_CHAR + 1, (1,), generator=g))
            chars[s, CFS - 1 + w * span:CFS - 1 + w * span + n] = torch.randint(1, V, (n,), generator=g)
    chars = chars.view(U, LINES, -1)
    words = torch.randint(0, N_WORDS, (U, LINES, WORDS), generator=g)         # id 0, the padding row, occurs: its gradient stays zero
    words[0, 0, 0] = 0
    mask = torch.zeros(U, LINES - ECFS + 1, dtype=torch.bool)
    mask[2, 0] = True
    out = m(words, chars, mask)
    G = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * G).sum().backward()
    arrays = {"words": words.numpy(), "chars": chars.numpy(), "mask": mask.numpy(), "word_span": np.int64(span), "p": np.float64(0.0),
              "out": out.detach().numpy(), "G": G.numpy()}
    for k, v in m.state_dict().items():
        arrays["sd." + k] = v.detach().numpy()
    for k, v in m.named_parameters():
        assert v.grad is not None, k
        arrays["g." + k] = v.grad.numpy()
    assert any(k.startswith("g.lstm.") for k in arrays) and "g.word_embeddings.weight" in arrays
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote %-28s %5.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))


def main():
    sys.path.insert(0, HERE)
    import gen_golden
    gen_golden._install_shims()
    cwd = os.getcwd()
    os.chdir(REF)
    sys.path.insert(0, REF)
    try:
        from models import models as ref_models
    finally:
        os.chdir(cwd)
    assert ref_models.__file__.startswith(REF)
    _case(ref_models, "ctx_lstm1", 41)


if __name__ == "__main__":
    main()
