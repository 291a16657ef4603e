"""CPU checks of the run_on_poll variant of the look-ahead lane model (tools/p2_lane_model.py, DESIGN §5.1
round 11) and of the argument checks of hmcx_sghmc_run_on_stats.

The variant prices parking a step whose verdict is pending and resolving it by the per-iteration poll of the
lane's next run, against round 10's protocol (`stop`, one boundary late) at the same round-9 coefficients.
Every figure is a model; the bounds below are what the change was decided on: at least 3 % at the
benchmark's accept rate, shrinking with the accept rate (a parked step behind a moved one is run twice
more) and still positive at 0.45, above the auto rule's 0.4."""
import ctypes
import importlib.util
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("p2_lane_model", os.path.join(REPO, "tools", "p2_lane_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _gain(m, rate, steps=50000, seed=1):
    n, moved = m.schedule(steps, rate, m.R9["nmax"], seed=seed)
    co = dict(m.R9, rate=rate)
    stop, _ = m.lanes(n, moved, variant="stop", late=1, **co)
    run_on, parked, voided = m.lanes_run_on_poll(n, moved, pending=1, late=1, **co)
    print("rate %.3f: stop %.2f, run_on_poll %.2f us per step, parked %.3f, voided %.3f" % (rate, stop, run_on, parked,
                                                                                             voided))
    return 1.0 - run_on / stop, parked, voided


def test_run_on_poll_gains_at_the_benchmark_rate():
    m = _model()
    gain, parked, voided = _gain(m, m.R9["rate"], steps=200000)
    assert gain >= 0.03
    assert 0.2 <= parked <= 0.45 and 0.0 < voided <= 0.06 and voided < parked


def test_gain_shrinks_with_the_accept_rate_and_stays_positive():
    m = _model()
    gains = [_gain(m, rate)[0] for rate in (0.092, 0.2, 0.3, 0.45)]
    assert gains == sorted(gains, reverse=True) and len(set(gains)) == 4
    assert gains[-1] > 0.0


def test_only_one_pending_step_is_modelled():
    m = _model()
    n, moved = m.schedule(100, 0.1, 19, seed=1)
    with pytest.raises(ValueError):
        m.lanes_run_on_poll(n, moved, pending=2, **m.R9)


def test_existing_rows_are_unchanged():
    """The variants round 10 was decided on give what they gave (200,000 steps, seed 1)."""
    m = _model()
    n, moved = m.schedule(200000, m.R9["rate"], m.R9["nmax"], seed=1)
    stop, _ = m.lanes(n, moved, variant="stop", late=1, **m.R9)
    assert stop == pytest.approx(51.2, abs=0.05)


def test_run_on_stats_refuses_a_null_context():
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    lib = nat.load_library()
    out = (ctypes.c_longlong * 2)(7, 7)
    assert lib.hmcx_sghmc_run_on_stats(None, out) != 0
    assert list(out) == [7, 7]
