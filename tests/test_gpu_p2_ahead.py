"""Look-ahead of the persistent single-chain SGHMC kernel (csrc/hmcx_persist2.hip, HMCX_P2_AHEAD,
hmcx_set_sghmc_ahead).

With look-ahead the launch carries two chain lanes: lane 0 runs the even steps, lane 1 the odd ones, each
at first from its own last state (assuming the other lane's step before it rejects) and again from the
true state when that step accepted.  Every step that counts performs the arithmetic of the plain
launch in the same order, so every output must be bit-equal to a run with HMCX_P2_AHEAD=0 HMCX_P2_HELP=0
(and to the helper launch, HMCX_P2_AHEAD=0 HMCX_P2_HELP=2), and no launch may time out (a timed-out
hand-off is re-run on the kernel-per-phase path, which would hide a protocol error behind a correct
result).

Both variables are read per call.  float64, Philox noise, path 2 (persistent only)."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import inputs as gi  # noqa: E402

PLAIN = {"HMCX_P2_AHEAD": "0", "HMCX_P2_HELP": "0"}      # the reference of every case
HELPERS = {"HMCX_P2_AHEAD": "0", "HMCX_P2_HELP": "2"}
AHEAD = {"HMCX_P2_AHEAD": "1"}
KEYS = ("W", "b", "mom", "A", "accepted", "ll", "E", "L")


def _sampler(B, D, K, path_length, step_size, seed=5, alpha=0.01):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
    m = softmax({"alpha": alpha}, dtype=torch.float64, device="cuda:0")
    m.ctx.set_sghmc_path(2)
    s = sghmc(m, {"weights": np.full((D, K), 0.01), "bias": np.zeros(K)}, path_length=path_length,
              step_size=step_size, noise="philox", seed=seed)
    s.out = io.StringIO()
    s.trace = None
    return s


_DATA = {}


def _dataset(B, D, K):
    if (B, D, K) not in _DATA:
        _DATA[(B, D, K)] = gi.dataset(23, 3 * B, D, K)
    return _DATA[(B, D, K)]


def _traj(monkeypatch, env, B, D, K, calls, path_length=5e-3, step_size=1e-3, seed=5, alpha=0.01, ctx_mode=None):
    """Every output of `calls` (a list of step counts) consecutive sampler calls under the environment
    `env` (and the context's look-ahead mode `ctx_mode`, when given); asserts that no call was re-run."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    for k in ("HMCX_P2_AHEAD", "HMCX_P2_HELP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    X, Y = _dataset(B, D, K)
    s = _sampler(B, D, K, path_length, step_size, seed=seed, alpha=alpha)
    if ctx_mode is not None:
        s.model.ctx.set_sghmc_ahead(ctx_mode)
    data = s._upload_data(X, Y)
    st = s._init_state()
    before = dict(nat.recoveries_all())
    out = {k: [] for k in ("A", "accepted", "ll", "E", "L", "mom")}
    step = 0
    s._want_mom = True
    for n in calls:
        rows = [((step + i) % 3) * B for i in range(n)]
        step += n
        res = s._run(st, data, rows, [step_size] * n, None, B)
        for k in ("A", "accepted", "ll", "E", "L"):
            out[k].append(np.array(getattr(res, k)))
        out["mom"].append(res.mom.cpu().numpy())
    torch.cuda.synchronize()
    assert dict(nat.recoveries_all()) == before
    got = {k: np.concatenate([np.atleast_1d(v) for v in vs]) for k, vs in out.items()}
    host = s._state_to_host(st)
    got["W"], got["b"] = np.array(host["weights"]), np.array(host["bias"])
    return got


_REF = {}


def _ref(monkeypatch, key, *args, **kw):
    """The plain run (HMCX_P2_AHEAD=0 HMCX_P2_HELP=0) of a case, computed once and shared."""
    if key not in _REF:
        _REF[key] = _traj(monkeypatch, PLAIN, *args, **kw)
    return _REF[key]


def _assert_equal(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("calls", [(12,), (6, 6), (1,), (2,), (3,)])
def test_config2_shape_bit_equal(monkeypatch, calls):
    """B = 500, D = 784, K = 10, 1,500 rows (plan 8x16: two lanes of 128 workgroups, the folded
    instantiation).  (1,) leaves lane 1 nothing to do; (2,) ends on lane 1's only step, whose verdict and
    state lane 0 commits; (3,) and (12,) are an odd and an even end; (6, 6) starts a second launch from W
    and b in global memory with new epochs and step tags."""
    args = (500, 784, 10, list(calls))
    ref = _ref(monkeypatch, ("c2", calls), *args)
    assert ref["L"].sum() > len(ref["L"]) or len(ref["L"]) == 1            # leapfrogs were run
    _assert_equal(ref, _traj(monkeypatch, AHEAD, *args))
    if calls == (12,):
        _assert_equal(_traj(monkeypatch, HELPERS, *args), _traj(monkeypatch, AHEAD, *args))


@pytest.mark.parametrize("shape", [(40, 32, 10), (64, 49, 3)])
def test_generic_kernel_uneven_ownership_bit_equal(monkeypatch, shape):
    """The generic kernel at small shapes: B = 40, D = 32, K = 10 is the 2x2 plan in which one row-team
    member owns no softmax rows; B = 64, D = 49, K = 3 pads the classes to 16 and leaves ragged feature
    slices (members that own no features publish zeros in the state hand-off)."""
    args = shape + ([8],)
    ref = _ref(monkeypatch, shape, *args)
    assert ref["L"].sum() > len(ref["L"])
    _assert_equal(ref, _traj(monkeypatch, AHEAD, *args))
    _assert_equal(_traj(monkeypatch, HELPERS, *args), _traj(monkeypatch, AHEAD, *args))


# The decision mix: B = 40, D = 32, K = 10, path length 2.5 step sizes (L = ceil(5u) in 1 … 5, so L = 1
# steps, which run no leapfrog and keep the state, occur), calls of 8, 5 and 7 steps.  Step size and seed
# were picked by running the PLAIN launch alone over a grid (step sizes 0.02 … 0.5, seeds 1 … 40: accept
# rates from 1.0 down to 0.5) and keeping a pair whose flags satisfy _assert_mix; at 0.07 and seed 4 the plain
# launch gives flags 11101111 10100 1110110 with L = 53223313 14235 3115114 (14 flagged accepted, 6 rejected).
MIX_EPS, MIX_SEED = 0.07, 4
MIX = dict(path_length=2.5 * MIX_EPS, step_size=MIX_EPS, seed=MIX_SEED)
MIX_CALLS = [8, 5, 7]


def _assert_mix(ref, calls):
    """The reference's own decisions hold every hand-off the two lanes have: a step that MOVED the state
    is an accepted one with L > 1 (an L = 1 step is flagged accepted and keeps the state)."""
    acc, L = ref["accepted"].astype(bool), ref["L"].astype(int)
    moved = acc & (L > 1)
    assert acc.sum() >= 3 and (~acc).sum() >= 3
    assert moved.sum() >= 3
    assert np.any(acc[1:] & acc[:-1]) and np.any(moved[1:] & moved[:-1])       # two consecutive accepts
    starts = np.cumsum([0] + list(calls[:-1]))
    ends = np.cumsum(calls) - 1
    assert np.any(moved[starts])                                               # an accept at step 0 of a call
    assert np.any(moved[ends])                                                 # ... and at the last step of one
    assert np.any(moved[:-1] & (L[1:] == 1))                                   # an L = 1 step right after an accept
    assert np.any(~acc[:-1] & moved[1:]) and np.any(moved[:-1] & ~acc[1:])     # both changes of regime


def test_decision_mix_bit_equal(monkeypatch):
    """Accepts and rejects in every order: a voided run is redone from the gathered state (also twice in
    a row, at the first and the last step of a call, and for a step without leapfrogs), a confirmed one
    is kept.  Fails, and does not skip, when the reference's flags lose the mix."""
    args = (40, 32, 10, MIX_CALLS)
    ref = _ref(monkeypatch, "mix", *args, **MIX)
    _assert_mix(ref, MIX_CALLS)
    got = _traj(monkeypatch, AHEAD, *args, **MIX)
    _assert_equal(ref, got)
    _assert_equal(_traj(monkeypatch, HELPERS, *args, **MIX), got)


def test_context_modes_bit_equal(monkeypatch):
    """hmcx_set_sghmc_ahead without the environment variables: off, on, and auto — twice, so that the second
    run starts with the first one's 20 reported flags (14 accepted: above the rule's 0.4) — give the plain
    launch's outputs; a mode outside 0 … 2 is refused."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    args = (40, 32, 10, MIX_CALLS)
    ref = _ref(monkeypatch, "mix", *args, **MIX)
    ctx = nat.context(torch.device("cuda:0"))
    try:
        for mode in (0, 1, 2, 2):
            _assert_equal(ref, _traj(monkeypatch, {}, *args, ctx_mode=mode, **MIX))
        with pytest.raises(nat.HmcxError):
            ctx.set_sghmc_ahead(3)
    finally:
        ctx.set_sghmc_ahead(2)


@pytest.mark.allow_recovery
@pytest.mark.parametrize("step", [1, 2])
def test_forced_abort_in_either_lane_is_recovered(monkeypatch, capfd, step):
    """HMCX_P2_FORCE_ABORT=<step> (the cooperative early return of a lane's last workgroup at that step;
    step 1 is lane 1's, step 2 lane 0's): the lane's other workgroups leave from their polls, the twin
    lane from its verdict wait, nothing is committed, and the call is re-run on the kernel-per-phase path
    with the reference's results, counted once."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    from test_gpu_recovery import _restore_path
    B, D, K = 500, 784, 10
    calls = [4]
    ref = _ref(monkeypatch, ("c2", (4,)), B, D, K, calls)
    for k, v in AHEAD.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("HMCX_P2_HELP", raising=False)
    monkeypatch.setenv("HMCX_P2_FORCE_ABORT", str(step))
    try:
        X, Y = _dataset(B, D, K)
        s = _sampler(B, D, K, 5e-3, 1e-3)
        s._want_mom = True
        data = s._upload_data(X, Y)
        st = s._init_state()
        W0, b0 = st["weights"].clone(), st["bias"].clone()
        before = nat.recoveries_all()["persistent_sghmc"]
        h = s._enqueue(st, data, [0, B, 2 * B, 0], [1e-3] * 4, None, B)
        torch.cuda.synchronize()
        assert torch.equal(st["weights"], W0) and torch.equal(st["bias"], b0)      # the aborted launch wrote nothing
        res = s._collect(h)
        torch.cuda.synchronize()
        assert nat.recoveries_all()["persistent_sghmc"] == before + 1
        host = s._state_to_host(st)
    finally:
        _restore_path()
    assert "hand-off timed out" in capfd.readouterr().err
    # the kernel-per-phase path reduces in another order: decisions and path lengths are exact, the float64
    # state and energies agree to rounding (as tests/test_gpu_recovery.py asks of a recovered run)
    assert np.array_equal(np.array(res.accepted), ref["accepted"]) and np.array_equal(np.array(res.L), ref["L"])
    np.testing.assert_allclose(np.array(res.A), ref["A"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(np.array(res.ll), ref["ll"], rtol=1e-9)
    np.testing.assert_allclose(np.array(host["weights"]), ref["W"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(np.array(host["bias"]), ref["b"], rtol=1e-9, atol=1e-12)
