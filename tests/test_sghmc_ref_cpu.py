"""The scripted-schedule SGHMC reference (tests/_sghmc_ref.py) against the golden-pinned oracle
(oracle/samplers.py::sghmc, tests/test_oracle_golden.py): fed the draws the oracle's step makes from
its seeded streams, the helper reproduces that step bit for bit.  CPU only."""
import numpy as np
import pytest

from oracle import inputs as gi
from oracle import models as om
from oracle import samplers as osm

from _sghmc_ref import flip_features, sghmc_step


@pytest.mark.parametrize("name", ["sghmc_small", "sghmc_hot"])
def test_helper_reproduces_the_oracle_step_bit_for_bit(name):
    c = gi.TRAJ_CONFIGS[name]
    X, Y = gi.dataset(c["data_seed"], c["N"], c["D"], c["K"])
    D, K, B, eps = c["D"], c["K"], c["B"], c["step_size"]
    P = D * K + K
    start = {"weights": np.zeros((D, K)), "bias": np.zeros(K)}
    o = osm.sghmc(om.softmax({"alpha": c["alpha"]}), start, path_length=c["path_length"], step_size=eps)
    o.trace = []
    rows = list(range(0, c["N"] - B + 1, B)) * 3
    # the oracle's run: global np.random for path length and accept uniform, rng for the normals
    np.random.seed(c["np_seed"])
    rng = np.random.RandomState(c["rng_seed"])
    q = start
    states = []
    for r in rows:
        q, _, _ = o.step(q, None, rng, X_train=X[r:r + B], y_train=Y[r:r + B])
        states.append({v: np.array(q[v]) for v in q})
    # the same draws, made explicitly in the oracle's order (the order of inference/gpu/sghmc.py::_schedule)
    np.random.seed(c["np_seed"])
    rng = np.random.RandomState(c["rng_seed"])
    q = start
    n_acc = n_moved = 0
    for r, t, want in zip(rows, o.trace, states):
        L = np.ceil(2 * np.random.rand() * c["path_length"] / eps)
        n_iter = max(0, int(np.ceil(L - 1)))
        z = rng.standard_normal(P * (1 + n_iter))
        u = np.random.rand()
        q, A, E, accepted, ll = sghmc_step(q, X[r:r + B], Y[r:r + B], eps, c["alpha"], n_iter, z, u)
        assert L == t["L"] and accepted == t["accepted"]
        assert A == t["A"] and E == t["E"]
        for v in ("weights", "bias"):
            np.testing.assert_array_equal(q[v], want[v])
        assert ll == float(o.model.log_likelihood(q, X_train=X[r:r + B], y_train=Y[r:r + B]))
        n_acc += accepted
        n_moved += n_iter > 0
    assert n_moved >= len(rows) // 2 and n_acc > 0
    if name == "sghmc_hot":
        assert n_acc < len(rows)            # the hot configuration rejects: both branches compared


def test_zero_iterations_keep_the_state_and_report_accept():
    X, Y = gi.dataset(3, 20, 6, 10)
    rs = np.random.RandomState(0)
    q = {"weights": rs.normal(0, 0.1, (6, 10)), "bias": rs.normal(0, 0.1, 10)}
    z = rs.standard_normal(70)
    out, A, (E0, E1), accepted, ll = sghmc_step(q, X, Y, 0.05, 0.01, 0, z, 0.999)
    assert A == 1.0 and E0 == E1 and accepted
    np.testing.assert_array_equal(out["weights"], q["weights"])
    np.testing.assert_array_equal(out["bias"], q["bias"])
    assert ll == float(om.softmax({"alpha": 0.01}).log_likelihood(q, X_train=X, y_train=Y))


def test_flipped_features_state_the_same_problem():
    """flip_features reverses X, W and the weight draws together: the step's scalars agree with the
    unflipped ones to summation-order rounding and the kept state is the reversed one."""
    X, Y = gi.dataset(5, 30, 18, 10)
    rs = np.random.RandomState(1)
    q = {"weights": rs.normal(0, 0.1, (18, 10)), "bias": rs.normal(0, 0.1, 10)}
    z = rs.standard_normal(190 * 4)
    a = sghmc_step(q, X, Y, 0.01, 0.01, 3, z, 0.5)
    qf, Xf, zf = flip_features(q, X, z)
    b = sghmc_step(qf, Xf, Y, 0.01, 0.01, 3, zf, 0.5)
    assert a[3] == b[3]
    np.testing.assert_allclose(b[0]["weights"][::-1], a[0]["weights"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(b[0]["bias"], a[0]["bias"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose([b[1], *b[2], b[4]], [a[1], *a[2], a[4]], rtol=1e-12)
