"""Fixtures of the entity-context char-CNN (tests/golden/char_features*.npz), written where the reference tree is available.

The reference's own `models.models.EntityEmbedding` (models/models.py:26-83) is built at U = 3 entities, 4 context lines of 3 words,
max_char_len 4, conv_filter_size 3, char_embed_dim 5, char_feature_size 6, 9 characters, hidden 3, and run on random ids with padding
inside and at the end of words.  Recorded: the inputs, the module's parameters, the output of its `max_pool` (a forward hook), its
output and, after a backward on a stored upstream gradient, the gradients of char_embeddings.embeddings.weight, conv1d.weight and
conv1d.bias, all with the module in fp64.  char_features1_eval: eval mode.  char_features2_train: training mode at p = 0.5, the char dropout replaced at generation
time by an nn.Dropout that records its factors (output / input where the input is non-zero would lose the factors of padding rows: the
recorder draws them itself, on a ones tensor, and multiplies).  Arrays only; nothing of the reference's text is stored.
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
U, LINES, WORDS, MAX_CHAR, CFS, C, FO, V, HIDDEN, WORD_DIM, N_WORDS, ENT_DIM, ECFS = 3, 4, 3, 4, 3, 5, 6, 9, 3, 4, 7, 5, 2


class RecordingDropout(nn.Dropout):
    """nn.Dropout whose factors (0 or 1 / (1 - p)) are kept: drawn by the stock dropout on a ones tensor, then multiplied in."""

    def forward(self, x):
        self.keep = super().forward(torch.ones_like(x))
        return x * self.keep


def _ids(g):
    span = MAX_CHAR + CFS - 1
    chars = torch.zeros(U * LINES, CFS - 1 + WORDS * span, dtype=torch.int64)
    for s in range(U * LINES):
        for w in range(int(torch.randint(0, WORDS + 1, (1,), generator=g))):
            n = int(torch.randint(1, MAX_CHAR + 1, (1,), generator=g))
            chars[s, CFS - 1 + w * span:CFS - 1 + w * span + n] = torch.randint(1, V, (n,), generator=g)
    chars[0, CFS - 1 + 1] = 0                                             # padding inside a word
    chars[0, CFS - 1] = chars[0, CFS - 1].clamp_min(1)
    chars[0, CFS - 1 + 2] = 3
    return chars.view(U, LINES, -1)


def _case(ref_models, name, p, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    word_emb = nn.Embedding(N_WORDS, WORD_DIM, padding_idx=0)
    m = ref_models.EntityEmbedding(WORD_DIM + FO, HIDDEN, 1, 1, p, ENT_DIM, CFS, ECFS, word_emb, C, MAX_CHAR, list(range(V)), FO)
    with torch.no_grad():
        m.char_embeddings.embeddings.weight.copy_(torch.randn(V, C, generator=g))
        m.char_embeddings.embeddings.weight[0].zero_()
    m.double()                                                            # the fixture is the reference in fp64: tests hold fp32 code to it
    if p > 0:
        m.char_embeddings.dropout = RecordingDropout(p)
        m.train()
    else:
        m.eval()
    chars = _ids(g)
    words = torch.randint(1, N_WORDS, (U, LINES, WORDS), generator=g)
    mask = torch.zeros(U, LINES - ECFS + 1, dtype=torch.bool)
    mask[1, -1] = True
    pooled = {}
    hook = m.max_pool.register_forward_hook(lambda mod, inp, out: pooled.__setitem__("v", out.detach().clone()))
    out = m(words, chars, mask)
    hook.remove()
    G = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * G).sum().backward()
    arrays = {"words": words.numpy(), "chars": chars.numpy(), "mask": mask.numpy(), "p": np.float64(p), "word_span": np.int64(MAX_CHAR + CFS - 1),
              "pool": pooled["v"].numpy(), "out": out.detach().numpy(), "G": G.numpy(),
              "g.char_embeddings.embeddings.weight": m.char_embeddings.embeddings.weight.grad.numpy(),
              "g.conv1d.weight": m.conv1d.weight.grad.numpy(), "g.conv1d.bias": m.conv1d.bias.grad.numpy()}
    for k, v in m.state_dict().items():
        arrays["sd." + k] = v.detach().numpy()
    if p > 0:
        arrays["keep"] = m.char_embeddings.dropout.keep.numpy()
        assert set(np.unique(arrays["keep"])) == {0.0, 1.0 / (1.0 - p)}
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
    _case(ref_models, "char_features1_eval", 0.0, 31)
    _case(ref_models, "char_features2_train", 0.5, 32)


if __name__ == "__main__":
    main()
