"""The GAT_sep_space ConvKB scorer (recon_amd.sep_space.SpKBGATConvOnly, recon_amd.kg_sep): the parts that need no GPU — the shell's state_dict
surface against the reference's, the relation-chunk planner, and argument checks that refuse bad input before any device work."""
import types

import pytest
import torch

from conftest import load_golden


def _shell(n_ent, n_rel, D):
    from recon_amd.sep_space import SpKBGATConvOnly
    return SpKBGATConvOnly(torch.randn(n_ent, 8), torch.randn(n_rel, 8), [D // 2, D], [D // 2, D], 0.0, 0.0, 0.2, 0.2, [2, 2], 50)


def test_sep_convonly_state_dict_keys_match_reference():
    g = load_golden("kgsep1")
    D = g["sd__final_entity_embeddings"].shape[1]
    m = _shell(int(g["n_ent"]), int(g["n_rel"]), D)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    for k, v in sd.items():
        assert tuple(v.shape) == g["sd__" + k].shape, k
    m.load_state_dict({k: torch.from_numpy(g["sd__" + k]) for k in sd}, strict=True)
    assert g["gat__W_ent2rel"].shape == (int(g["n_rel"]), D, D)


@pytest.mark.parametrize("n_rel,n_rows,D,budget", [(237, 14541, 200, 1 << 30), (237, 14541, 200, 3 * 2 * 4 * 14541 * 200 + 7), (11, 203, 37, 1),
                                                    (5, 10, 512, 2 * 4 * 10 * 512), (1, 1, 1, 1 << 30), (0, 50, 8, 1 << 20)])
def test_plan_chunks_under_budget_and_covering(n_rel, n_rows, D, budget):
    from recon_amd.kg_sep import plan_chunks
    per = 2 * 4 * n_rows * D
    rels = [r * 3 + 1 for r in range(n_rel)]                                    # any ids, in order
    if per > budget:
        with pytest.raises(ValueError):
            plan_chunks(rels, n_rows, D, budget)
        return
    chunks = plan_chunks(rels, n_rows, D, budget)
    assert [r for c in chunks for r in c] == rels                               # every relation exactly once, in order
    assert all(0 < len(c) and len(c) * per <= budget for c in chunks)
    if n_rel:
        assert len(chunks) == -(-n_rel // min(n_rel, budget // per))            # as few chunks as the budget allows
    if (n_rel, n_rows, D, budget) == (237, 14541, 200, 1 << 30):
        assert len(chunks[0]) == 46


def test_sep_evaluate_rejects_bad_arguments_before_device_work():
    from recon_amd import kg_sep
    n_ent, n_rel, D = 40, 3, 16
    m = _shell(n_ent, n_rel, D)
    tri = torch.tensor([[1, 2, 3]])
    ok = types.SimpleNamespace(W_ent2rel=torch.randn(n_rel, D, D), nonlinearity_ent2rel=torch.tanh)
    bad_shapes = [torch.randn(n_rel + 1, D, D), torch.randn(n_rel, D, D + 1), torch.randn(n_rel, D * D), None]
    for W in bad_shapes:
        gat = types.SimpleNamespace(W_ent2rel=W, nonlinearity_ent2rel=torch.tanh)
        with pytest.raises(ValueError, match="W_ent2rel"):
            m.evaluate(gat, tri, tri)
        with pytest.raises(ValueError, match="W_ent2rel"):
            m.relation_scores(gat, tri)
    for nl in (torch.sigmoid, torch.relu, lambda x: torch.tanh(x), None):
        gat = types.SimpleNamespace(W_ent2rel=ok.W_ent2rel, nonlinearity_ent2rel=nl)
        with pytest.raises(ValueError, match="tanh"):
            m.evaluate(gat, tri, tri)
    for nl in (torch.tanh, torch.nn.functional.tanh, torch.nn.Tanh()):          # every spelling of tanh passes the check (then: no GPU)
        gat = types.SimpleNamespace(W_ent2rel=ok.W_ent2rel, nonlinearity_ent2rel=nl)
        with pytest.raises(RuntimeError, match="GPU"):
            m.evaluate(gat, tri, tri)
    big = _shell(n_ent, n_rel, 514)
    gat = types.SimpleNamespace(W_ent2rel=torch.zeros(n_rel, 514, 514), nonlinearity_ent2rel=torch.tanh)
    with pytest.raises(ValueError, match="512"):
        big.evaluate(gat, tri, tri)
    with pytest.raises(ValueError):
        kg_sep.sep_scorer(m.final_entity_embeddings, m.final_relation_embeddings[:, :8], m.convKB, ok)
