"""Stopping a voided look-ahead run in flight (csrc/hmcx_persist2.hip).

A speculative run of step s + 1 whose assumption failed (step s moved the state) is left at a leapfrog
boundary as soon as the other lane's verdict has arrived and the lane has agreed on it, instead of being
finished first.  Whether a given run is stopped depends on timing, results never do: every output must be
bit-equal to the plain launch (HMCX_P2_AHEAD=0 HMCX_P2_HELP=0), no launch may be re-run, and the counters of
hmcx_sghmc_ahead_stats show that the path ran.  float64, Philox noise, path 2 (persistent only).

Step sizes and seeds were picked by running the PLAIN launch alone over a grid (step sizes 0.02 … 0.5, seeds
1 … 60) and keeping pairs whose own flags hold the patterns asserted below; each test asserts its pattern on
the reference and fails, never skips, when it is lost.  With a path length of 5 step sizes L = ceil(10 u) runs
over 1 … 10, and a step runs L − 1 leapfrogs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_p2_ahead import AHEAD, KEYS, PLAIN, _dataset, _sampler  # noqa: E402


def _traj(monkeypatch, env, B, D, K, calls, step_size, seed, path_steps=5.0, alpha=0.01):
    """Every output of consecutive sampler calls of `calls` steps under `env`, and the look-ahead counters
    added over the calls; asserts that no call was re-run."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    for k in ("HMCX_P2_AHEAD", "HMCX_P2_HELP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    X, Y = _dataset(B, D, K)
    s = _sampler(B, D, K, path_steps * step_size, step_size, seed=seed, alpha=alpha)
    data = s._upload_data(X, Y)
    st = s._init_state()
    before = dict(nat.recoveries_all())
    out = {k: [] for k in ("A", "accepted", "ll", "E", "L", "mom")}
    stats = {"redone": 0, "stopped": 0, "skipped": 0}
    step = 0
    s._want_mom = True
    for n in calls:
        rows = [((step + i) % 3) * B for i in range(n)]
        step += n
        res = s._run(st, data, rows, [step_size] * n, None, B)
        for k in ("A", "accepted", "ll", "E", "L"):
            out[k].append(np.array(getattr(res, k)))
        out["mom"].append(res.mom.cpu().numpy())
        for k, v in s.model.ctx.sghmc_ahead_stats().items():
            stats[k] += v
    torch.cuda.synchronize()
    assert dict(nat.recoveries_all()) == before
    got = {k: np.concatenate([np.atleast_1d(v) for v in vs]) for k, vs in out.items()}
    host = s._state_to_host(st)
    got["W"], got["b"] = np.array(host["weights"]), np.array(host["bias"])
    got["stats"] = stats
    return got


_REF = {}


def _ref(monkeypatch, key, *args, **kw):
    if key not in _REF:
        _REF[key] = _traj(monkeypatch, PLAIN, *args, **kw)
        assert _REF[key]["stats"] == {"redone": 0, "stopped": 0, "skipped": 0}
    return _REF[key]


def _assert_equal(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


def _pattern(ref, calls):
    """moved, L, and the mask of the steps that have a successor in their own call."""
    acc, L = ref["accepted"].astype(bool), ref["L"].astype(int)
    moved = acc & (L > 1)
    succ = np.ones(len(L), bool)
    succ[np.cumsum(calls) - 1] = False
    return moved, L, succ


def _stop_pairs(ref, calls):
    """Steps s that moved the state after at most two leapfrogs while step s + 1, in the same call, runs at
    least five more: V(s) lands at least five iterations before the twin lane's voided run ends."""
    moved, L, succ = _pattern(ref, calls)
    idx = np.flatnonzero(succ)
    return [int(s) for s in idx if moved[s] and L[s] <= 3 and L[s + 1] >= L[s] + 5]


def _late_pairs(ref, calls):
    """Moved steps whose successor's run is at least three leapfrogs shorter: the voided run ends first."""
    moved, L, succ = _pattern(ref, calls)
    return [int(s) for s in np.flatnonzero(succ) if moved[s] and L[s] >= L[s + 1] + 3]


def _redone_expected(ref, calls):
    moved, _, succ = _pattern(ref, calls)
    return int((moved & succ).sum())


# B = 40, D = 32, K = 10: the 2x2 plan, both team dimensions above 1, so the flag needs both hops (the A-AG
# header across the row team, the B round's header across the feature team).
STOP_CALLS = [8, 5, 7]
# At 0.02 and seed 4 the plain launch gives flags 11111111 10110 1111111 with L = a5436526 2846a 522a117 (hex):
# stop pairs at step 8 (L = 2 then 8, step 0 of the second call) and step 15 (2 then 10), a late pair at step 0
# (10 then 5).
STOP = dict(step_size=0.02, seed=4)


def test_stop_observed_generic_kernel(monkeypatch):
    """At least two short moved steps followed by a run five iterations longer, one of them at step 0 of a
    call: those runs are stopped in flight.  Every voided run is redone, stopped or not."""
    args = (40, 32, 10, STOP_CALLS)
    ref = _ref(monkeypatch, "stop", *args, **STOP)
    pairs = _stop_pairs(ref, STOP_CALLS)
    starts = set(np.cumsum([0] + STOP_CALLS[:-1]).tolist())
    assert len(pairs) >= 2 and starts & set(pairs), (pairs, ref["accepted"], ref["L"])
    got = _traj(monkeypatch, AHEAD, *args, **STOP)
    print("stats", got["stats"], "pairs", pairs)
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, STOP_CALLS)
    assert got["stats"]["stopped"] >= 2 and got["stats"]["skipped"] >= 2
    assert got["stats"]["stopped"] <= got["stats"]["redone"]


def test_late_verdict_takes_the_old_path(monkeypatch):
    """A moved step at least three leapfrogs longer than its successor: the voided run reaches its accept
    round first when the lanes start together, waits for the verdict and is redone as before."""
    args = (40, 32, 10, STOP_CALLS)
    ref = _ref(monkeypatch, "stop", *args, **STOP)
    assert _late_pairs(ref, STOP_CALLS), (ref["accepted"], ref["L"])
    got = _traj(monkeypatch, AHEAD, *args, **STOP)
    _assert_equal(ref, got)
    # (when its lane started late the shorter run may still be caught in flight, so `stopped` has no bound here)
    assert got["stats"]["redone"] == _redone_expected(ref, STOP_CALLS)


ROW_CALLS = [6, 6]
# 0.02 and seed 15: flags 111111 011111 with L = 9a1126 a4142a: moved steps in a row throughout, and the stop pair
# of step 10 (L = 2 then 10) ends on the second call's last step.
ROW = dict(step_size=0.02, seed=15)


def test_two_moved_in_a_row_and_stop_on_a_calls_last_step(monkeypatch):
    """Two consecutive moved steps (the redo of the second starts from a state that was itself redone), and a
    stop pair whose long run is the last step of a call (the stopped lane's redo ends the call: lane 0 commits
    its own state, or reads lane 1's last verdict and state)."""
    args = (40, 32, 10, ROW_CALLS)
    ref = _ref(monkeypatch, "row", *args, **ROW)
    moved, L, succ = _pattern(ref, ROW_CALLS)
    assert np.any(moved[:-1] & moved[1:] & succ[:-1]), (ref["accepted"], L)
    ends = set((np.cumsum(ROW_CALLS) - 1).tolist())
    assert any(s + 1 in ends for s in _stop_pairs(ref, ROW_CALLS)), (ref["accepted"], L)
    got = _traj(monkeypatch, AHEAD, *args, **ROW)
    print("stats", got["stats"])
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, ROW_CALLS)
    assert got["stats"]["stopped"] >= 1


# 0.5 and seed 1: flags 00010000 with L = 53714aa2: every proposal is rejected (the flagged step is an L = 1
# step, which runs no leapfrog and keeps the state).
NONE = dict(step_size=0.5, seed=1)


def test_nothing_moves(monkeypatch):
    args = (40, 32, 10, [8])
    ref = _ref(monkeypatch, "none", *args, **NONE)
    moved, L, _ = _pattern(ref, [8])
    assert not moved.any() and (L > 3).sum() >= 3, (ref["accepted"], L)
    got = _traj(monkeypatch, AHEAD, *args, **NONE)
    _assert_equal(ref, got)
    assert got["stats"] == {"redone": 0, "stopped": 0, "skipped": 0}


# 0.02 and seed 3: flags 11000101 with L = 19899272: the stop pair of step 5 (L = 2 then 7).
UNEVEN = dict(step_size=0.02, seed=3)


def test_uneven_ownership(monkeypatch):
    """B = 64, D = 49, K = 3 (classes padded to 16, ragged feature slices): members that own no features
    publish a header, and with it the flag, but no data."""
    args = (64, 49, 3, [8])
    ref = _ref(monkeypatch, "uneven", *args, **UNEVEN)
    assert _stop_pairs(ref, [8]), (ref["accepted"], ref["L"])
    got = _traj(monkeypatch, AHEAD, *args, **UNEVEN)
    print("stats", got["stats"])
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, [8])
    assert got["stats"]["stopped"] >= 1


# 0.02 and seed 3: flags 100001000000 with L = 1989927264aa: the stop pair of step 5 (L = 2 then 7).
C2 = dict(step_size=0.02, seed=3)


def test_config2_shape_folded_instantiation(monkeypatch):
    """B = 500, D = 784, K = 10, 12 steps: the 8x16 plan's folded kernel, two lanes of 128 workgroups."""
    args = (500, 784, 10, [12])
    ref = _ref(monkeypatch, "c2", *args, **C2)
    assert _stop_pairs(ref, [12]), (ref["accepted"], ref["L"])
    got = _traj(monkeypatch, AHEAD, *args, **C2)
    print("stats", got["stats"])
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, [12])
    assert got["stats"]["stopped"] >= 1


def test_stats_before_any_launch_are_zero():
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    ctx = nat.Context(torch.device("cuda:0"))
    assert ctx.sghmc_ahead_stats() == {"redone": 0, "stopped": 0, "skipped": 0}
