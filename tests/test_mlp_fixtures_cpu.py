"""The MLP SGHMC fixtures of tests/_mlp_fixtures.py, checked on the oracle alone (no GPU): every
fixture's trajectory takes the accept / reject decisions the GPU parity tests
(test_gpu_mlp_accept.py) mean to exercise, and none of them hangs on rounding.

A step is "real" when its path length L >= 2 (at least one leapfrog iteration: the proposal differs
from the current state).  One libhmcx call is one epoch of six steps, so "inside a call" means two
consecutive steps of the same epoch; the last step of a call commits through k_mlp_commit, the others
inside the next step's start launch."""
import numpy as np
import pytest

import _mlp_fixtures as fx

MARGIN = 0.25       # min |dE - ln u|: no accept flag of the reference depends on rounding


def _pairs_in_call(tr):
    n = fx.STEPS_PER_CALL
    return [(tr[i], tr[i + 1]) for i in range(len(tr) - 1) if i // n == (i + 1) // n]


def _real(t):
    return t["L"] >= 2


@pytest.mark.parametrize("f", fx.FIXTURES, ids=lambda f: f.name)
def test_fixture_takes_real_accept_and_reject_decisions(f):
    tr = fx.fixture_oracle(f).trace
    n = fx.STEPS_PER_CALL
    assert len(tr) == n * fx.EPOCHS
    for t in tr:                                                    # the recorded quantities are consistent
        dE = t["E"][0] - t["E"][1]
        assert t["accepted"] == bool(np.log(t["u"]) < dE)
        assert t["A"] == min(1, np.exp(dE))
    assert sum(_real(t) and t["accepted"] for t in tr) >= 3
    assert sum(_real(t) and not t["accepted"] for t in tr) >= 3
    last = [tr[c * n + n - 1] for c in range(fx.EPOCHS)]
    assert any(_real(t) and not t["accepted"] for t in last)      # a call ends with a real reject ...
    assert any(_real(t) and t["accepted"] for t in last)          # ... and one with a real accept
    pairs = _pairs_in_call(tr)
    assert any(_real(a) and a["accepted"] and _real(b) and not b["accepted"] for a, b in pairs)
    assert any(_real(a) and not a["accepted"] and _real(b) and b["accepted"] for a, b in pairs)
    # the commit folded into a start launch that does not drift
    assert any(_real(a) and a["accepted"] and b["L"] == 1 for a, b in pairs)
    assert min(fx.margins(tr)) >= MARGIN


def test_fixture_table_covers_aliasing_path_lengths():
    """L = 2 and L = 5 (n - 1 = 0 and 3 iterations past the first: the proposal lies in the buffer the
    next start launch drifts into) occur over the table as a whole; shapes are on the intended side of
    the k_fwdr conditions."""
    Ls = {t["L"] for f in fx.FIXTURES for t in fx.fixture_oracle(f).trace}
    assert {2.0, 5.0} <= Ls
    for f in fx.FIXTURES:
        ok = (f.n_mid % 32 == 0 and f.n_mid <= 256 and f.n_out <= 16 and f.n_in % 8 == 0 and f.B % 4 == 0
              and (f.B // 4 * f.n_mid) % 32 == 0)
        assert ok == f.fwdr, f.name


def test_permuted_order_fixtures_also_mix():
    """The permuted variable order (another noise layout, so another trajectory) is run by the float64
    parity test on every fixture: it must take both decisions on real steps, with the same margin."""
    for f in fx.FIXTURES:
        tr = fx.fixture_oracle(f, fx.PERMUTED).trace
        assert any(_real(t) and t["accepted"] for t in tr), f.name
        assert any(_real(t) and not t["accepted"] for t in tr), f.name
        assert min(fx.margins(tr)) >= MARGIN, f.name


def test_wide_class_shapes_take_three_accepted_trajectories():
    """The fused-launch shapes with 17 to 32 classes (test_gpu_mlp_accept.py): path lengths [3, 2, 2], every
    step accepted, no decision within 11 of flipping; every shape has more logit items per row block than the
    fused workgroup has threads, and rows of a block that lie past the first 512 items."""
    for shape in fx.WIDE_CLASS:
        n_in, n_mid, n_out, B = shape
        tr = fx.wide_class_oracle(shape).trace
        assert [t["L"] for t in tr] == [3, 2, 2], shape
        assert all(t["accepted"] for t in tr), shape
        assert min(fx.margins(tr)) > 11, shape
        assert 16 < n_out <= 32 and 32 * n_out > 512 and min(B, 32) > 512 // n_out, shape
    assert {-(-s[1] // 32) for s in fx.WIDE_CLASS} == {1, 2, 3}                 # column slices
    assert {512 // s[2] for s in fx.WIDE_CLASS} == {30, 21, 16}                 # rows inside the first 512 items
    assert any(s[3] % 32 == 0 for s in fx.WIDE_CLASS) and any(s[3] % 32 for s in fx.WIDE_CLASS)


def test_near_miss_shapes_have_real_robust_steps():
    """The four shapes just outside fwdr_ok (test_gpu_mlp_accept.py) run three real trajectories whose
    flags do not hang on rounding either."""
    for shape in fx.NEAR_MISS:
        tr = fx.oracle_run(*shape, fx.NEAR_MISS_ALPHA, fx.NEAR_MISS_SEED, n_batches=3, epochs=1).trace
        assert len(tr) == 3 and min(t["L"] for t in tr) >= 2, shape
        assert min(fx.margins(tr)) >= MARGIN, shape
