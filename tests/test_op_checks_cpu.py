"""tests/op_checks.py on the CPU: the shared band, bitwise equality and call counter still bite."""
import pytest
import torch

from op_checks import band_failures, bound, calls_of, same


def test_bound_at_its_floor_its_slope_and_its_cap():
    assert bound(0.0) == 2.0 ** -20 and bound(1e-6) == 4e-6 and bound(1e-3) == 2e-5


def test_band_passes_an_error_on_the_bound_and_reports_one_just_above():
    ref = torch.tensor([1.0, 0.5], dtype=torch.float64)                 # max |ref| = 1: an absolute error is the relative one
    chain = ref + torch.tensor([0.0, 2.0 ** -19], dtype=torch.float64)  # e_chain = 2^-19 exactly: 2^-20 < 4 e_chain = 2^-17 < 2e-5
    assert bound(2.0 ** -19) == 2.0 ** -17
    on = ref + torch.tensor([0.0, 2.0 ** -17], dtype=torch.float64)
    above = ref + torch.tensor([0.0, 2.0 ** -17 + 2.0 ** -40], dtype=torch.float64)
    assert band_failures(["a", "b"], [on, on], [chain, chain], [ref, ref], "on the bound") == []
    bad = band_failures(["a", "b"], [on, above], [chain, chain], [ref, ref], "above")
    assert [b[0] for b in bad] == ["b"] and bad[0][1] > 2.0 ** -17 and bad[0][2] == 2.0 ** -19


def test_band_raises_on_a_shape_mismatch_and_on_none_against_a_tensor():
    ref = torch.ones(2, 3, dtype=torch.float64)
    with pytest.raises(AssertionError):
        band_failures(["a"], [torch.ones(3, 2)], [torch.ones(2, 3)], [ref], "shape")
    with pytest.raises(AssertionError):
        band_failures(["a"], [torch.ones(2, 3)], [None], [None], "tensor against None")
    with pytest.raises(AssertionError):
        band_failures(["a"], [None], [torch.ones(2, 3)], [ref], "None against tensor")
    assert band_failures(["a", "b"], [None, torch.ones(2, 3)], [None, torch.ones(2, 3)], [None, ref], "None against None") == []


def test_same_fails_on_one_bit_a_length_and_a_none():
    a = [torch.tensor([1.0, 2.0]), None]
    same(a, [torch.tensor([1.0, 2.0]), None])
    flipped = (torch.tensor([1.0, 2.0]).view(torch.int32) ^ torch.tensor([0, 1], dtype=torch.int32)).view(torch.float32)
    for other in ([flipped, None], a[:1], [a[0], a[0]], [None, None]):
        with pytest.raises(AssertionError):
            same(a, other)


def test_calls_of_counts_passes_through_and_is_undone():
    class Owner:
        @staticmethod
        def twice(x, plus=0):
            return 2 * x + plus

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x + 1
    real, real_apply = Owner.twice, Fn.apply
    with pytest.MonkeyPatch.context() as mp:
        calls, applies = calls_of(mp, Owner, "twice"), calls_of(mp, Fn, "apply")
        assert Owner.twice(3) == 6 and Owner.twice(3, plus=1) == 7 and len(calls) == 2
        assert Fn.apply(torch.tensor(1.0)).item() == 2.0 and len(applies) == 1 and isinstance(Fn.__dict__["apply"], staticmethod)
    assert Owner.twice is real and Fn.apply == real_apply and Owner.twice(3) == 6 and len(calls) == 2
