"""Fixtures of the ContextAware baseline (tests/golden/context_aware1.npz, context_aware2.npz), written where the reference tree is
available.

The reference's own `models.baselines.ContextAware` (models/baselines.py:10-119) is built at B = 2 sentences of T = 6 tokens, 11 words of
5, position_emb 3, units1 4, n_out 7, in eval mode and in fp64, at n = 3 entities (C = 6 pairs) and at n = 2 (C = 2: one ghost, P = 1),
and run on random ids.  Recorded: the word table `emb`, the inputs `sent` and `mark`, the logits `out`, the upstream gradient G of
(out * G).sum(), the state_dict (`sd.*`) and the gradient of every parameter that gets one (`g.*`; word_embedding.weight is frozen).
Arrays only; nothing of the reference's text is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
B, T, N_WORDS, WORD_DIM, POS_DIM, UNITS, N_OUT = 2, 6, 11, 5, 3, 4, 7


def _case(ref_baselines, name, n, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    C = n * (n - 1)
    p = {"max_num_nodes": n, "dropout1": 0.0, "position_emb": POS_DIM, "units1": UNITS, "rnn1_layers": 1, "bidirectional": 1}
    emb = torch.randn(N_WORDS, WORD_DIM, generator=g).numpy().astype(np.float32)
    m = ref_baselines.ContextAware(p, emb, T, N_OUT)
    m.double().eval()
    sent = torch.randint(1, N_WORDS, (B, T), generator=g)
    sent[1, T - 2:] = 0                                                   # a padded tail
    mark = torch.randint(0, 4, (B, C, T), generator=g)
    mark[1, C - 1] = 0                                                    # a padding pair: all-zero markers, attended over like the rest
    out = m(sent, mark)
    assert tuple(out.shape) == (B * C, N_OUT)
    G = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * G).sum().backward()
    arrays = {"emb": emb, "sent": sent.numpy(), "mark": mark.numpy(), "n": np.int64(n), "out": out.detach().numpy(), "G": G.numpy()}
    for k, v in m.state_dict().items():
        arrays["sd." + k] = v.detach().numpy()
    for k, v in m.named_parameters():
        if v.requires_grad:
            assert v.grad is not None, k
            arrays["g." + k] = v.grad.numpy()
    assert len([k for k in arrays if k.startswith("sd.")]) == 13 and "g.word_embedding.weight" not in arrays
    assert "g.linear1.weight" in arrays and any(k.startswith("g.rnn1.") for k in arrays)
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
        from models import baselines as ref_baselines
    finally:
        os.chdir(cwd)
    assert ref_baselines.__file__.startswith(REF)
    _case(ref_baselines, "context_aware1", 3, 51)
    _case(ref_baselines, "context_aware2", 2, 52)


if __name__ == "__main__":
    main()
