"""Fixtures of the per-pair baselines (tests/golden/cnn1.npz, pcnn1.npz, lstm_baseline1.npz), written where the reference tree is available.

The reference's own `models.baselines.CNN`, `PCNN` and `LSTM` (models/baselines.py:122-314) are built at B = 3 rows of T = 9 tokens, 11
words of 5, position_emb 3, units1 4, n_out 7, window_size 3, in eval mode and in fp64, and run on random ids.  The last row has a padded
tail: zero word and position ids, and a zero mask there.  Recorded: the word table `emb`, the inputs `sent`, `mark` (CNN, PCNN: the two
relative positions [B, 2, T]; LSTM: the markers [B, T]) and, for PCNN, `mask` [B, 3, T]; the logits `out`, the upstream gradient G of
(out * G).sum(), the state_dict (`sd.*`) and the gradient of every parameter that gets one (`g.*`; word_embedding.weight is frozen and
LSTM's linear1 is unused).  Arrays only; nothing of the reference's text is stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
B, T, N_WORDS, WORD_DIM, POS_DIM, UNITS, N_OUT, WINDOW, TAIL = 3, 9, 11, 5, 3, 4, 7, 3, 3
P = {"dropout1": 0.0, "position_emb": POS_DIM, "units1": UNITS, "rnn1": "LSTM", "rnn1_layers": 1, "bidirectional": True, "window_size": WINDOW}


def _case(cls, name, kind, seed, n_keys):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    emb = torch.randn(N_WORDS, WORD_DIM, generator=g).numpy().astype(np.float32)
    m = cls(dict(P), emb, T, N_OUT)
    m.double().eval()
    sent = torch.randint(1, N_WORDS, (B, T), generator=g)
    sent[B - 1, T - TAIL:] = 0
    arrays = {"emb": emb, "sent": sent.numpy()}
    if kind == "lstm":
        mark = torch.randint(1, 4, (B, T), generator=g)
        mark[B - 1, T - TAIL:] = 0
        args = (sent, mark)
    else:
        mark = torch.randint(1, 2 * T + 1, (B, 2, T), generator=g)
        mark[B - 1, :, T - TAIL:] = 0
        args = (sent, mark)
        if kind == "pcnn":
            mask = torch.zeros(B, 3, T, dtype=torch.float64)
            for b in range(B):
                n = T - TAIL if b == B - 1 else T
                lo, hi = sorted(torch.randint(1, n, (2,), generator=g).tolist())
                mask[b, 0, :lo] = 1
                mask[b, 1, lo:hi + 1] = 1
                mask[b, 2, hi + 1:n] = 1
            arrays["mask"] = mask.numpy()
            args = (sent, mark, mask)
    arrays["mark"] = mark.numpy()
    out = m(*args)
    assert tuple(out.shape) == (B, N_OUT)
    G = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * G).sum().backward()
    arrays.update(out=out.detach().numpy(), G=G.numpy())
    for k, v in m.state_dict().items():
        arrays["sd." + k] = v.detach().numpy()
    for k, v in m.named_parameters():
        if v.requires_grad and v.grad is not None:
            arrays["g." + k] = v.grad.numpy()
    assert len([k for k in arrays if k.startswith("sd.")]) == n_keys and "g.word_embedding.weight" not in arrays
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
    _case(ref_baselines.CNN, "cnn1", "cnn", 61, 10)
    _case(ref_baselines.PCNN, "pcnn1", "pcnn", 62, 6)
    _case(ref_baselines.LSTM, "lstm_baseline1", "lstm", 63, 13)


if __name__ == "__main__":
    main()
