"""CPU checks of the look-ahead lane model (tools/p2_lane_model.py) and of the argument checks of
hmcx_sghmc_ahead_stats.

The model's parent variant, at the round-9 coefficients (a lane runs a step in 10.4 µs + 7.6 per
leapfrog, a verdict costs 1.5, accept rate 0.092, leapfrogs uniform on 0 … 19), has to reproduce the one
figure of that curve that is a measurement: ×1.405 over the helper launch's 7.42·steps + 7.29·leapfrogs
(profiles/r09_ab.txt, 600 steps), within 3 %.  A model that misses it prices nothing."""
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


def test_parent_variant_matches_the_measured_ratio():
    m = _model()
    n, moved = m.schedule(100000, m.R9["rate"], m.R9["nmax"], seed=1)
    ser = m.serial(n, **m.SERIAL)
    assert ser == pytest.approx(7.42 + 7.29 * 9.5, rel=0.01)
    base, wait = m.lanes(n, moved, **m.R9)
    print("parent %.2f us per step, serial %.2f, ratio %.4f, verdict wait %.3f" % (base, ser, ser / base, wait))
    assert 1.405 * 0.97 <= ser / base <= 1.405 * 1.03
    # the measured verdict wait of the two lanes, 12.6 % and 16.5 % of a lane's ticks, brackets the model's
    assert 0.126 <= wait <= 0.165


def test_run_on_resolved_at_run_end_is_not_faster_and_stopping_is():
    m = _model()
    n, moved = m.schedule(100000, m.R9["rate"], m.R9["nmax"], seed=1)
    base, _ = m.lanes(n, moved, **m.R9)
    run_on, _ = m.lanes(n, moved, variant="run_on", **m.R9)
    print("parent %.2f, run on %.2f us per step" % (base, run_on))
    assert run_on >= base
    nxt, _ = m.lanes(n, moved, variant="stop", late=0, **m.R9)
    late, _ = m.lanes(n, moved, variant="stop", late=1, **m.R9)
    dear, _ = m.lanes(n, moved, variant="stop", late=1, overhead=0.1, **m.R9)
    print("stop: next boundary %.2f, one late %.2f, 0.1 us dearer %.2f" % (nxt, late, dear))
    assert nxt <= late <= dear < base


def test_stopping_gains_more_at_higher_accept_rates():
    m = _model()
    gains = []
    for rate in (0.092, 0.2, 0.3, 0.45):
        n, moved = m.schedule(50000, rate, m.R9["nmax"], seed=2)
        co = dict(m.R9, rate=rate)
        base, _ = m.lanes(n, moved, **co)
        late, _ = m.lanes(n, moved, variant="stop", late=1, **co)
        gains.append(1.0 - late / base)
    assert gains == sorted(gains) and gains[0] > 0.03


def test_ahead_stats_refuses_a_null_context():
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    lib = nat.load_library()
    out = (ctypes.c_longlong * 3)(7, 7, 7)
    assert lib.hmcx_sghmc_ahead_stats(None, out) != 0
    assert list(out) == [7, 7, 7]
