"""Training of the ConvKB scorer (recon_amd.kg_train, csrc/kg_train.hip): the parts that need no GPU — the reference
fixture's loss against the weighted-BCE formula, the corruption layout rule against the reference's batches, and argument checks."""
import numpy as np
import pytest
import torch

from conftest import load_golden


def _bce(preds, values, ratio):
    y = (values.astype(np.float64) + 1) / 2
    w = y + (1 - y) / (2 * ratio)
    s = preds.astype(np.float64)
    m = np.maximum(-s, 0)
    return float(np.mean(w * ((1 - y) * s + m + np.log(np.exp(-m) + np.exp(-s - m)))))


def test_fixture_loss_is_the_weighted_bce_formula():
    g = load_golden("convkb_train1")
    loss = _bce(g["preds"], g["step_values"], int(g["step_ratio"]))
    assert abs(loss - float(g["loss"])) <= 1e-6 * max(1.0, abs(loss))


def layout(B, ratio):
    """The documented row layout of recon_kg_corrupt: base positive and replaced column (-1: an untouched copy) of every row."""
    base, col = list(range(B)), [-1] * B
    half = B * (ratio // 2)
    for c in range(2 * B * ratio):
        base.append(c % B)
        col.append(0 if c < half else 2 if c < 2 * half else 1 if c >= B * ratio else -1)
    return np.array(base), np.array(col)


@pytest.mark.parametrize("case", ["r4", "r3", "short"])
def test_reference_batches_follow_the_layout_rule(case):
    g = load_golden("convkb_train1")
    pos = g[case + "_positives"]
    base, col = layout(len(pos), int(g[case + "_ratio"]))
    assert (g[case + "_base"] == base).all()
    known = set(map(tuple, np.concatenate([g["train"], g["valid"], g["test"]]).tolist()))
    rel_full = {(h, t) for h, r, t in known if sum((h, q, t) in known for q in range(int(g["n_rel"]))) == int(g["n_rel"])}
    want = col.copy()
    for o in range(len(pos), len(col)):                                      # the give-up rule: saturated (h, t) pairs keep the relation
        h, _, t = pos[base[o]]
        if col[o] == 1 and (h, t) in rel_full:
            want[o] = -1
    assert (g[case + "_col"] == want).all()
    v = g[case + "_values"]
    assert (v[want >= 0] == -1).all() and (v[want < 0] == 1).all()
    for row, b, c in zip(g[case + "_indices"], g[case + "_base"], g[case + "_col"]):
        if c >= 0:
            assert tuple(row) not in known


def test_kg_train_rejects_cpu_and_bad_arguments():
    from recon_amd import kg_train
    from recon_amd.models import SpKBGATConvOnly
    with pytest.raises(RuntimeError):
        kg_train.TripleFilter(torch.zeros(4, 3, dtype=torch.int64), 10, 3)
    m = SpKBGATConvOnly(torch.randn(10, 8), torch.randn(3, 8), [4, 8], [4, 8], 0.0, 0.0, 0.2, 0.2, [2, 2], 50)
    tri = torch.zeros(6, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="741-742"):                       # the tables are trainable: refused, not silently frozen
        kg_train.convkb_scores(m, tri)
    m.final_entity_embeddings.requires_grad_(False)
    m.final_relation_embeddings.requires_grad_(False)
    with pytest.raises(RuntimeError):                                        # no CPU path
        kg_train.convkb_scores(m, tri)
    with pytest.raises(ValueError):
        kg_train.convkb_bce_loss(m, tri, torch.ones(6), 0)


def test_kg_train_abi_rejects_before_launching():
    from recon_amd import _lib
    L = _lib.lib()
    fake = 16                                                                # never dereferenced: every call below returns before a launch
    args = lambda D, values, ratio: (fake, 8, 64, fake, fake, 10, 3, D, fake, fake, fake, fake, 0.01, fake, fake, values, ratio, None, fake, fake,
                                     fake, 1 << 20, None)
    assert L.recon_convkb_train_fwd(*args(513, None, 0)) == -2                # D above the limit
    assert L.recon_convkb_train_fwd(*args(8, fake, 0)) == -1                  # a loss with ratio 0 divides by zero
    assert L.recon_convkb_train_fwd(*args(8, None, 0)[:1], 3, *args(8, None, 0)[2:]) == -1        # index width
    assert L.recon_convkb_train_bwd(fake, 8, 64, fake, fake, 10, 3, 600, fake, 0.01, fake, fake, None, fake, fake, fake, fake, fake, 1 << 30,
                                    None) == -2
    assert L.recon_kg_corrupt(fake, 8, fake, 4, -1, fake, 1, 10, 3, 1, fake, fake, fake, None) == -1
