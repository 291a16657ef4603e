"""CPU checks of the linear models' posterior-predictive reference (tests/_linear_predictive_ref.py): the gap
preconditions the GPU tests' exact comparisons rest on, asserted on the oracle alone (this file is the
authority for the cases' seeds), the reference's internal identities, and the Python twins of the fused
kernel's eligibility rule and of the path-0 selection rule at their bounds."""
import numpy as np
import pytest

import _linear_predictive_ref as lr
from oracle import models as om

ALL = lr.CASES + [lr.LDS_EDGE]


@pytest.mark.parametrize("c", ALL, ids=lr.case_id)
@pytest.mark.parametrize("dropout", [True, False], ids=["fixed", "off"])
def test_reference_gaps(c, dropout):
    """No decision of the reference hangs on rounding: every argmax of `mean` and of a draw's logits (logistic:
    every mean and every draw's probability against 0.5) is decided by more than GAP64 in float64 and by more
    than GAP32 at float32-rounded inputs."""
    r64, r32 = lr.case_ref(c, dropout), lr.case_ref(c, dropout, True)
    assert r64.mean_gap > lr.GAP64 and r64.draw_gap > lr.GAP64, (r64.mean_gap, r64.draw_gap)
    assert r32.mean_gap > lr.GAP32 and r32.draw_gap > lr.GAP32, (r32.mean_gap, r32.draw_gap)
    np.testing.assert_array_equal(r64.pred, r32.pred)
    np.testing.assert_array_equal(r64.draw_correct, r32.draw_correct)


@pytest.mark.parametrize("c", ALL, ids=lr.case_id)
def test_reference_identities(c):
    N, D, K, S, T = c.shape
    r = lr.case_ref(c)
    classes = 2 if c.model == 'logistic' else K
    assert r.mean.shape == (N, K) and r.pred.shape == (N,)
    assert r.draw_nll.shape == (S * T,) and r.draw_correct.shape == (S * T,)
    if c.model == 'softmax':
        np.testing.assert_allclose(r.mean.sum(axis=1), 1.0, rtol=1e-12)
    else:
        assert np.all((r.mean > 0) & (r.mean < 1))
    assert r.mutual_information.min() >= -1e-12
    assert r.entropy.max() <= np.log(classes) + 1e-12 and r.expected_entropy.min() >= 0
    assert np.all(r.lppd <= 0) and np.all(r.draw_nll >= 0)
    assert np.all((0 <= r.draw_correct) & (r.draw_correct <= N))


@pytest.mark.parametrize("c", [c for c in lr.CASES if c.shape[0] >= 2], ids=lr.case_id)
def test_single_draw_is_predict(c):
    """S = T = 1 without masks is the oracle's predict(prob=True) (logistic: its net, every row)."""
    pb = lr.problem(c)
    N = c.shape[0]
    r = lr.predictive_ref(c.model, pb.W[:1], pb.b[:1], pb.X, pb.y)
    par = {'weights': pb.W[0], 'bias': pb.b[0]}
    if c.model == 'logistic':
        want = om.logistic({"alpha": 1.0}).predict(par, pb.X, prob=True, batchsize=N)
        np.testing.assert_array_equal(r.mean.reshape(-1), want)
        np.testing.assert_array_equal(r.pred, om.logistic({"alpha": 1.0}).predict(par, pb.X, batchsize=N))
    else:
        np.testing.assert_array_equal(r.mean, om.softmax({"alpha": 1.0}).predict(par, pb.X, prob=True))
        np.testing.assert_array_equal(r.pred, om.softmax({"alpha": 1.0}).predict(par, pb.X))
    assert np.abs(r.mutual_information).max() <= 1e-12         # one draw: the mean is the draw


def test_fused_eligibility_bounds():
    # K: one MFMA tile
    assert lr.fused_eligible(24, 16, 8) and not lr.fused_eligible(24, 17, 8)
    assert lr.fused_eligible(1, 1, 4) and not lr.fused_eligible(24, 0, 4)
    # LDS: 16 rows of X (D rounded up to 16, one 16-byte pad per row) + 4 logit tiles + row partials <= 160 KiB
    for elt, last in ((8, 944), (4, 2144)):
        assert lr.fused_eligible(last, 10, elt) and not lr.fused_eligible(last + 1, 10, elt)
        assert lr.first_ineligible_D(3, elt) == last + 1
    assert lr.LDS_EDGE.shape == (5, 945, 3, 2, 1)
    assert lr.fused_eligible(784, 10, 8) and lr.fused_eligible(2048, 16, 4) and not lr.fused_eligible(2048, 16, 8)
    flags = [lr.eligible(c) for c in lr.CASES]
    assert flags == [True, True, True, True, True, False, True, True, True]


def test_path0_rule_twin():
    # the headline shapes: N = 10 000, D = 784, K = 10 (6 sets per unit)
    assert lr.path0_is_fused(10000, 784, 10, 4, 64, 1, False) and lr.path0_is_fused(10000, 784, 10, 8, 1000, 1, False)
    assert not lr.path0_is_fused(10000, 784, 10, 4, 8, 1, False)          # 2 units
    assert not lr.path0_is_fused(1000, 784, 10, 4, 64, 1, False)          # 63 x 11 pairs
    assert lr.path0_is_fused(2500, 784, 10, 4, 64, 1, False) and lr.path0_is_fused(1000, 784, 10, 4, 1000, 1, False)
    # the bounds: 4 units and 1536 pairs; K = 16 has 4 sets per unit
    assert lr.path0_is_fused(6144, 8, 16, 4, 16, 1, False)
    assert not lr.path0_is_fused(6128, 8, 16, 4, 16, 1, False) and not lr.path0_is_fused(8192, 8, 16, 4, 12, 1, False)
    # ... or 200 parameter sets (still 4 units: K = 1 packs 64 sets per unit)
    assert lr.path0_is_fused(32, 8, 16, 4, 200, 1, False) and not lr.path0_is_fused(32, 8, 16, 4, 199, 1, False)
    assert lr.path0_is_fused(256, 32, 1, 8, 1000, 1, False) and not lr.path0_is_fused(256, 32, 1, 8, 192, 1, False)
    # input dropout: 32 draws
    assert lr.path0_is_fused(16, 784, 10, 4, 2, 16, True) and not lr.path0_is_fused(16, 784, 10, 4, 1, 31, True)
    # never on an ineligible shape
    assert not lr.path0_is_fused(10000, 24, 38, 8, 1000, 1, False) and not lr.path0_is_fused(10000, 945, 3, 8, 1000, 1, False)
    assert not lr.path0_is_fused(10000, 24, 38, 8, 64, 16, True)
