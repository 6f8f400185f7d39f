"""The float32 ragged GraphConvolution's checks on the CPU (tests/gcn_ragged_checks.py): the float32 restatement in the kernels' order
passes them for every shape, each of eight wrong restatements is reported, the mask check's margin stays under its cap, and the four
entries are declared, bound and struct-free."""
import pytest
import torch

import gcn_ragged_checks as R
import op_checks

ENTRIES = ("recon_gcn_ragged_supported", "recon_gcn_ragged_bwd_partial_floats", "recon_gcn_ragged_fwd", "recon_gcn_ragged_bwd")
BIG = ((5, 32, 17, 65, 100, 1, 33), 40, 136)


@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_restatement_passes_the_band(shape, bias):
    c = R.case(*shape, bias)
    bad = R.failures(c, R.restate(c), "cpu", "restatement " + R.shape_id(shape))
    assert not bad, bad


@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_margin_cap_per_shape(shape, bias):
    """With the float64 restatement alone, at the widest bound the band allows (2e-5): at most 0.1 % of a case's cells lie so close to
    zero that the mask check does not ask about them."""
    skipped, cells = R.margin_cells(R.case(*shape, bias))
    assert skipped <= R.MARGIN_CAP * cells, (skipped, cells)


def test_zero_row_gives_relu_bias():
    sizes, g, row = R.ZERO_ROW
    c = R.case(*BIG, True)
    assert c.sizes == sizes
    out64 = R.reference(c)[1]
    assert torch.equal(out64[int(c.node_ptr[g]) + row], torch.relu(c.b.double()))
    assert torch.equal(R.restate(c)[0][int(c.node_ptr[g]) + row], torch.relu(c.b))


@pytest.mark.parametrize("wrong", R.WRONG)
def test_wrong_restatement_is_reported(wrong):
    """Each wrong form misses on both multi-graph shapes it is tried on, in the output it spoils."""
    spoils = {"adj_transposed_fwd": "out", "adj_not_transposed_bwd": "g_x", "row_base_off_by_one_graph": "out", "adj_ptr_from_n": "out",
              "bias_left_out": "out", "mask_from_grad_out": "g_x", "g_adj_operands_swapped": "g_adj", "g_bias_one_graph": "g_bias"}
    for shape in (((31, 32, 33), 24, 16), BIG):
        c = R.case(*shape, True)
        bad = R.failures(c, R.restate(c, wrong), "cpu", "%s %s" % (wrong, R.shape_id(shape)))
        assert spoils[wrong] in [b[0] for b in bad], (wrong, shape, bad)


def test_entries_declared_and_bound():
    op_checks.entries_declared_and_bound(ENTRIES, "models/layers.py:57-63")


def test_header_gained_no_struct():
    from test_abi_layout_cpu import STRUCTS
    assert R.header_struct_typedefs() == set(STRUCTS.values())
    from recon_amd import _lib
    import ctypes
    for name, _, args in _lib.SYMBOLS:
        if name in ENTRIES:
            assert not any(isinstance(a, type) and issubclass(a, (ctypes.Structure, ctypes._Pointer)) for a in args), name
