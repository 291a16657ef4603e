"""CPU preconditions of the linear-model kernel tests (tests/_linear_cases.py), on the references alone:
the case tables reach the kernel instantiations they claim, every defect a kernel could plausibly have
(a dropped row, a dropped feature, a dropped class column) moves every compared output far past its
float32 tolerance, and the saturated logistic cases really do defeat the pre-fix float32 formula.  A case
that fails gets another seed or weight scale in the table; the checks stay as they are."""
import numpy as np
import pytest

import _linear_cases as lc

OUTPUTS = ("gW", "gb", "ll", "prob")
MOVE = 8            # a mutation must move some element by at least this many tolerances


def test_tiling_mirror_covers_every_instantiation():
    fwd, grad = set(), set()
    for c in lc.SOFTMAX_CASES:
        shape = (c["B"], c["D"], c["K"], c["C"])
        assert lc.fwd_instance(*shape) == c["fwd"], shape
        assert lc.grad_instance(*shape) == c["grad"], shape
        fwd.add(c["fwd"])
        grad.add(c["grad"])
    assert fwd == lc.ALL_FWD and len(lc.ALL_FWD) == 12
    assert grad == lc.ALL_GRAD and len(lc.ALL_GRAD) == 6
    for c in lc.LOGISTIC_CASES:
        assert lc.make_tiling(c["B"], c["D"], 1, c["C"])["NBLK"] == c["nblk"]
    assert {c["nblk"] for c in lc.LOGISTIC_CASES} >= {2, 3, 4}
    # the edges the table names
    t = lc.make_tiling(20, 784, 10, 61)
    assert (t["CB"], t["nCT"], 61 - 10 * t["CB"]) == (6, 11, 1)
    t = lc.make_tiling(19, 70, 10, 13)
    assert (t["CB"], t["nCT"], 13 - 2 * t["CB"]) == (6, 3, 1)
    t = lc.make_tiling(20, 160, 38, 52)
    assert t["nDB"] * t["nCT"] == 520
    t = lc.make_tiling(50, 8, 1, 70)
    assert (t["CB"], t["nCT"]) == (64, 2)


_CASES = [("softmax", i) for i in range(len(lc.SOFTMAX_CASES))] + \
         [("logistic", i) for i in range(len(lc.LOGISTIC_CASES))]


def _id(p):
    model, i = p
    return model + "-" + lc.case_id((lc.SOFTMAX_CASES if model == "softmax" else lc.LOGISTIC_CASES)[i])


@pytest.mark.parametrize("case", _CASES, ids=_id)
def test_mutations_move_every_output(case):
    model, i = case
    ref, tol = lc.reference(model, i, "float32"), lc.f32_tolerances(model, i)
    for mutation in lc.MUTATIONS:
        mut = lc.mutated(model, i, mutation)
        for o in OUTPUTS:
            with np.errstate(invalid="ignore"):
                moved = float(np.max(np.abs(mut[o] - ref[o]) / tol[o]))
            print("%s %s %s: moved by %.3g tolerances" % (_id(case), mutation, o, moved))
            assert moved >= MOVE, (mutation, o, moved)


@pytest.mark.parametrize("shape", lc.SGLD_SHAPES, ids=lambda s: "K%d-D%d-B%d" % s)
def test_sgld_mutations_move_states_and_logp(shape):
    """logp = −(ll + log_prior) / B is compared twice: as it is, and through the log-likelihood inside it
    (lc.sgld_loglik).  The bound on logp itself, 1e-5 of a value that is mostly the prior's constant, cannot
    see the mutations at the small shapes (a dropped row moves it by 0.9 tolerances at (64, 300, 40), 1.6 at
    (2, 1, 1)), whatever the seeds; the bound on ll sees them everywhere, so that is the one held to MOVE."""
    tol, d = lc.sgld_tolerances(*shape)
    s64, l64 = lc.sgld_reference(*shape)
    ll64 = lc.sgld_loglik(*shape, l64)
    print("K %d D %d B %d: d/scale states %.2e, logp %.2e, ll %.2e" % (
        shape + (d["states"] / np.max(np.abs(s64)), d["logp"] / np.max(np.abs(l64)),
                 d["ll"] / max(1.0, np.max(np.abs(ll64))))))
    for mutation in ("row", "feature"):
        sm, lm = lc.sgld_reference(*shape, mutation=mutation)
        ms = float(np.max(np.abs(sm - s64))) / tol["states"]
        mp = float(np.max(np.abs(lm - l64))) / tol["logp"]
        ml = float(np.max(np.abs(lc.sgld_loglik(*shape, lm) - ll64))) / tol["ll"]
        print("K %d D %d B %d %s: moved by (tolerances) states %.3g, ll %.3g, logp %.3g" % (
            shape + (mutation, ms, ml, mp)))
        assert ms >= MOVE and ml >= MOVE, (mutation, ms, ml)


@pytest.mark.parametrize("i", [i for i, c in enumerate(lc.LOGISTIC_CASES) if c["saturated"]])
def test_saturated_logistic_cases_defeat_the_old_float32_formula(i):
    X, y, Ws, bs = lc.logistic_problem(i, "float32")
    z = (X @ Ws[0] + bs[0])[:, 0]
    assert np.any((y == 1) & (z > 17)) and np.any((y == 0) & (z > 17))
    assert not np.isfinite(lc.old_logistic_loglik_f32(X, y, Ws[0], bs[0]))
    assert np.isfinite(lc.reference("logistic", i, "float32")["ll"][0])


def test_saturated_cases_are_in_the_table():
    assert sum(c["saturated"] for c in lc.LOGISTIC_CASES) == 2
