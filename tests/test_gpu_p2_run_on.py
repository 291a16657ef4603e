"""Parked steps of the look-ahead launch (csrc/hmcx_persist2.hip, DESIGN §5.1 round 11, HMCX_P2_RUNON).

A speculative run of step s that ends while the other lane's verdict V(s − 1) is still unknown to its whole
lane, and that leaves the state as it was, is parked: the lane starts step s + 2 at once and resolves the
verdict while that runs ("unchanged": step s is final; "changed": step s and the run started on it are run
again from the true state).  Whether a step is parked depends on timing, results never do: every output must be
bit-equal to the plain launch (HMCX_P2_AHEAD=0 HMCX_P2_HELP=0), no launch may be re-run, `redone` is the number
of moved steps that have a successor in their call, and the counters of hmcx_sghmc_run_on_stats show that the
path ran.  float64, Philox noise, path 2 (persistent only).

Step sizes and seeds were picked by running the PLAIN launch alone over a grid (step sizes 0.02 … 0.5, seeds
1 … 40) and keeping pairs whose own flags hold the patterns asserted below; each test asserts its pattern on
the reference and fails, never skips, when it is lost.  With a path length of 5 step sizes L = ceil(10 u) runs
over 1 … 10, and a step runs L − 1 leapfrogs.  A margin of five leapfrogs between the two lanes' runs makes the
timing-dependent counters safe to assert."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_p2_ahead import KEYS, PLAIN  # noqa: E402
from test_gpu_p2_stop import C2, UNEVEN, _pattern, _redone_expected, _ref, _traj  # noqa: E402

RUN_ON = {"HMCX_P2_AHEAD": "1", "HMCX_P2_RUNON": "1"}
RUN_ON_OFF = {"HMCX_P2_AHEAD": "1", "HMCX_P2_RUNON": "0"}
CALLS = [8, 5, 7]


def _run(monkeypatch, env, *args, **kw):
    """_traj of test_gpu_p2_stop under `env`, with the parked-step counters added over the calls (read where
    _traj reads the look-ahead counters: after every call)."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    monkeypatch.delenv("HMCX_P2_RUNON", raising=False)
    total = {"ran_on": 0, "voided": 0}
    ahead_stats = nat.Context.sghmc_ahead_stats

    def both(self):
        for k, v in self.sghmc_run_on_stats().items():
            total[k] += v
        return ahead_stats(self)

    monkeypatch.setattr(nat.Context, "sghmc_ahead_stats", both)
    got = _traj(monkeypatch, env, *args, **kw)
    monkeypatch.setattr(nat.Context, "sghmc_ahead_stats", ahead_stats)
    got["run_on"] = total
    return got


def _plain(monkeypatch, key, *args, **kw):
    monkeypatch.delenv("HMCX_P2_RUNON", raising=False)
    return _ref(monkeypatch, key, *args, **kw)


def _assert_equal(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


def _in_call(calls):
    """first[s], last[s]: the first and the last step of the call that holds step s."""
    ends = np.cumsum(calls)
    first = np.repeat(ends - np.array(calls), calls)
    return first, np.repeat(ends - 1, calls)


def _park_steps(ref, calls):
    """Steps s that end at least five leapfrogs before step s − 1 of the same call does, neither of which moves
    the state, with a step s + 2 of at least two leapfrogs in the call: the lane of s parks it."""
    moved, L, _ = _pattern(ref, calls)
    first, last = _in_call(calls)
    return [int(s) for s in range(1, len(L)) if s - 1 >= first[s] and s + 2 <= last[s] and not moved[s - 1] and
            not moved[s] and L[s - 1] >= L[s] + 5 and L[s + 2] >= 3]


def _void_steps(ref, calls):
    """Steps s behind a moved step s − 1 of the same call that runs at least five leapfrogs longer, with s + 2 in
    the call: when the void run's own decision is a reject the step is parked, and the verdict voids it."""
    moved, L, _ = _pattern(ref, calls)
    first, last = _in_call(calls)
    return [int(s) for s in range(1, len(L)) if s - 1 >= first[s] and s + 2 <= last[s] and moved[s - 1] and
            L[s - 1] >= L[s] + 5 and L[s + 2] >= 2]


def _pending_steps(ref, calls):
    """Steps s whose predecessor runs at least five leapfrogs longer than steps s and s + 2 together: the lane
    reaches the accept round of s + 2 with s still parked."""
    moved, L, _ = _pattern(ref, calls)
    first, last = _in_call(calls)
    return [int(s) for s in range(1, len(L)) if s - 1 >= first[s] and s + 2 <= last[s] and not moved[s] and
            L[s + 2] >= 2 and L[s - 1] >= L[s] + L[s + 2] + 5]


def _sure_void_steps(ref, calls, in_flight):
    """The void steps that run no leapfrog (L = 1: their own decision is "state unchanged" whatever the state,
    so they are parked), split by where V(s − 1) lands: inside the run of s + 2 with three leapfrogs to spare
    (`in_flight`), or five leapfrogs behind its end."""
    _, L, _ = _pattern(ref, calls)
    if in_flight:
        return [s for s in _void_steps(ref, calls) if L[s] == 1 and L[s + 2] >= L[s - 1] - L[s] + 3]
    return [s for s in _void_steps(ref, calls) if L[s] == 1 and L[s - 1] >= L[s] + L[s + 2] + 5]


# B = 40, D = 32, K = 10: the 2x2 plan (one row-team member owns no softmax rows).  The plain launch gives
# (flags, L in hex; a step moved the state when it is flagged and L > 1):
#  0.5, seed 18:  00000000 00000 0000000, L = a2692a69 59865 2775789: park steps 1 (L = 10 then 2, step 3 has 9) and 4.
#  0.5, seed 32:  00000000 00000 0000010, L = 69a3525a 46882 6a53918: step 3 (L = 10, then 3, step 5 has 2) is
#                 still parked when the run of step 5 ends.
#  0.02, seed 33: moved 10101100 10001 0000001, L = a1813a74 3a8a6 3a3a8a4: step 2 moved after 7 leapfrogs, step 3
#                 runs none and step 5 runs 9, so V(2) = changed lands inside the run of step 5.
#  0.02, seed 15: moved 11001101 01111 1111001, L = 9a1126a4 142a7 4325193: step 1 moved after 9 leapfrogs, step 2
#                 runs none and step 4 one, so the run of step 4 ends with step 2 parked and V(1) = changed.
SHAPE = (40, 32, 10, CALLS)
REJECT = dict(step_size=0.5, seed=18)
PENDING = dict(step_size=0.5, seed=32)
VOID_IN_FLIGHT = dict(step_size=0.02, seed=33)
VOID_AT_END = dict(step_size=0.02, seed=15)


def test_all_reject_schedule_parks(monkeypatch):
    """Nothing moves: every verdict is "unchanged", so a parked step is never voided and nothing is redone."""
    ref = _plain(monkeypatch, ("run_on", "reject"), *SHAPE, **REJECT)
    moved, L, _ = _pattern(ref, CALLS)
    steps = _park_steps(ref, CALLS)
    assert not moved.any() and steps, (ref["accepted"], L)
    got = _run(monkeypatch, RUN_ON, *SHAPE, **REJECT)
    print("stats", got["stats"], got["run_on"], "park steps", steps)
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, CALLS) == 0
    assert got["run_on"]["ran_on"] >= 1 and got["run_on"]["voided"] == 0


def test_parked_step_voided_in_flight(monkeypatch):
    """A moved step at least five leapfrogs longer than its successor, which runs no leapfrog and is parked; the
    verdict lands inside the run started on it, the lane leaves that run on the flag, gathers the true state,
    redoes the parked step on its tile and runs the next one again.  (`voided` >= 1 held in five consecutive
    runs of this test.)"""
    ref = _plain(monkeypatch, ("run_on", "void"), *SHAPE, **VOID_IN_FLIGHT)
    steps = _sure_void_steps(ref, CALLS, True)
    assert steps, (ref["accepted"], ref["L"])
    got = _run(monkeypatch, RUN_ON, *SHAPE, **VOID_IN_FLIGHT)
    print("stats", got["stats"], got["run_on"], "void steps", steps)
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, CALLS)
    assert 1 <= got["run_on"]["voided"] <= min(got["run_on"]["ran_on"], got["stats"]["redone"])


def test_parked_step_voided_at_the_end_of_the_next_run(monkeypatch):
    """The same with a run of s + 2 that ends at least five leapfrogs before V(s − 1) = changed lands: it waits
    before its accept round, and the parked step and the run are void.  (`voided` >= 1 held in five
    consecutive runs of this test.)"""
    ref = _plain(monkeypatch, ("run_on", "void_end"), *SHAPE, **VOID_AT_END)
    steps = _sure_void_steps(ref, CALLS, False)
    assert steps and set(steps) <= set(_pending_steps(ref, CALLS)), (ref["accepted"], ref["L"])
    got = _run(monkeypatch, RUN_ON, *SHAPE, **VOID_AT_END)
    print("stats", got["stats"], got["run_on"], "void steps", steps)
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, CALLS)
    assert 1 <= got["run_on"]["voided"] <= min(got["run_on"]["ran_on"], got["stats"]["redone"])


def test_one_pending_step_waits_before_the_accept_round(monkeypatch):
    """Step s − 1 outlasts steps s and s + 2 together and nothing moves: the run of s + 2 ends with s still
    parked, waits for V(s − 1) = unchanged and only then loads the next tile into the parked step's buffer."""
    ref = _plain(monkeypatch, ("run_on", "pending"), *SHAPE, **PENDING)
    moved, L, _ = _pattern(ref, CALLS)
    steps = _pending_steps(ref, CALLS)
    assert steps and not moved.any(), (ref["accepted"], L)
    got = _run(monkeypatch, RUN_ON, *SHAPE, **PENDING)
    print("stats", got["stats"], got["run_on"], "pending steps", steps)
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, CALLS) == 0
    assert got["run_on"]["ran_on"] >= 1 and got["run_on"]["voided"] == 0


def test_ragged_ownership(monkeypatch):
    """B = 64, D = 49, K = 3: classes padded to 16, ragged feature slices."""
    args = (64, 49, 3, [8])
    ref = _plain(monkeypatch, "uneven", *args, **UNEVEN)
    got = _run(monkeypatch, RUN_ON, *args, **UNEVEN)
    print("stats", got["stats"], got["run_on"])
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, [8])
    assert got["run_on"]["voided"] <= got["run_on"]["ran_on"]


def test_config2_shape_folded_instantiation(monkeypatch):
    """B = 500, D = 784, K = 10, 12 steps: the 8x16 plan's folded kernel, two lanes of 128 workgroups."""
    args = (500, 784, 10, [12])
    ref = _plain(monkeypatch, "c2", *args, **C2)
    got = _run(monkeypatch, RUN_ON, *args, **C2)
    print("stats", got["stats"], got["run_on"])
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, [12])
    assert got["run_on"]["voided"] <= got["run_on"]["ran_on"]


def test_switched_off(monkeypatch):
    """HMCX_P2_RUNON=0: the lanes wait for every verdict, nothing is parked."""
    ref = _plain(monkeypatch, ("run_on", "reject"), *SHAPE, **REJECT)
    got = _run(monkeypatch, RUN_ON_OFF, *SHAPE, **REJECT)
    _assert_equal(ref, got)
    assert got["stats"]["redone"] == _redone_expected(ref, CALLS)
    assert got["run_on"] == {"ran_on": 0, "voided": 0}


def test_plain_launch_counts_nothing(monkeypatch):
    got = _run(monkeypatch, PLAIN, *SHAPE, **REJECT)
    assert got["run_on"] == {"ran_on": 0, "voided": 0}
