"""tests/grad_scales.py: the per-group and per-element yardsticks must themselves refuse what they are there to refuse."""
import pytest
import torch

from grad_scales import assert_close_by_element, assert_close_by_group, head_groups

GROUPS = [("small", 0, 2), ("large", 2, 5), ("none", 5, 6)]


def _ref():
    ref = torch.zeros(3, 6, dtype=torch.float64)
    ref[:, 0:2] = torch.tensor([1e-4, -2e-4])
    ref[:, 2:5] = torch.tensor([1.0, -3.0, 2.0])
    return ref


def test_each_group_is_judged_on_its_own_maximum():
    ref = _ref()
    got = ref.clone()
    got[1, 0] *= 1.1                                           # 10 % of a head that is 7e-5 of the largest
    assert (got - ref).abs().max() <= 2e-5 * ref.abs().max()   # invisible on one scale
    with pytest.raises(AssertionError, match="small.*worst at \\(1, 0\\) \\(channel 0\\)"):
        assert_close_by_group(got, ref, GROUPS, 2e-5, "x")
    got = ref.clone()
    got[2, 3] += 3.0 * 1e-5
    assert abs(assert_close_by_group(got, ref, GROUPS, 2e-5, "x") - 1e-5) < 1e-9
    got[2, 3] += 3.0 * 2e-5
    with pytest.raises(AssertionError, match="large"):
        assert_close_by_group(got, ref, GROUPS, 2e-5, "x")


def test_a_group_without_a_reference_gradient_must_be_exactly_zero_and_nan_is_an_error():
    ref = _ref()
    got = ref.clone()
    got[0, 5] = 1e-30
    with pytest.raises(AssertionError, match="none.*identically zero"):
        assert_close_by_group(got, ref, GROUPS, 2e-5, "x")
    got = ref.clone()
    got[0, 1] = float("nan")
    with pytest.raises(AssertionError, match="small"):
        assert_close_by_group(got, ref, GROUPS, 2e-5, "x")
    with pytest.raises(AssertionError, match="tile"):
        assert_close_by_group(ref, ref, GROUPS[:2], 2e-5, "x")


def test_element_wise_bound():
    ref = torch.tensor([1.0, 1e-6, 0.0, -2.0], dtype=torch.float64)
    bound = torch.tensor([0.0, 1e-9, 0.0, 1e-3], dtype=torch.float64)
    got = ref + torch.tensor([5e-7, 1e-9, 0.0, -1e-3])
    assert abs(assert_close_by_element(got, ref, 1e-6, bound, "x") - 1e-9 / (1e-12 + 1e-9)) < 1e-6
    for i, d in ((0, 2e-6), (1, 2e-9), (2, 1e-40), (3, 2e-3)):
        bad = ref.clone()
        bad[i] += d
        with pytest.raises(AssertionError, match="\\(%d,\\)" % i):
            assert_close_by_element(bad, ref, 1e-6, bound, "x")
    bad = ref.clone()
    bad[0] = float("nan")
    with pytest.raises(AssertionError):
        assert_close_by_element(bad, ref, 1e-6, bound, "x")


def test_head_groups_are_the_eleven_regression_heads():
    from dcd_amd.model.head.detector_loss import Loss_Computation
    from test_host_golden import small_cfg
    groups = head_groups(Loss_Computation(small_cfg("cpu")))
    assert [b - a for _, a, b in groups] == [4, 2, 20, 3, 3, 8, 8, 1, 1, 146, 219] and groups[-1][2] == 415
    assert [n for n, _, _ in groups][:2] == ["2d_dim", "3d_offset"] and all(a1 == b0 for (_, _, b0), (_, a1, _) in zip(groups, groups[1:]))
