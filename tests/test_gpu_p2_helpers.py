"""Helper workgroups of the persistent single-chain SGHMC kernel (csrc/hmcx_persist2.hip, HMCX_P2_HELP).

With helpers on, workgroup G + b computes E_current's log-likelihood ll(q_s; batch s) for chain
workgroup b — the same A-gemm, A-RS exchange, log-softmax and row order as the chain's own it = -1
round, from the state the chain publishes after the previous accept — and the helpers of a feature
team draw the step's momentum p0 for it, with the chain's own Philox calls, so every output must be
bit-equal to a run with HMCX_P2_HELP=0, and no launch may time out (a timed-out hand-off is re-run
on the kernel-per-phase path, which would hide a protocol error behind a correct result).

HMCX_P2_HELP is read per call.  float64, Philox noise, path 2 (persistent only) unless said."""
import io
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import inputs as gi  # noqa: E402

MODES = (2,)            # the helper modes that ship


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


def _traj(monkeypatch, help_mode, B, D, K, calls, path_length=5e-3, step_size=1e-3):
    """Every output of `calls` (a list of step counts) consecutive sampler calls under HMCX_P2_HELP=help_mode;
    asserts that no call was re-run."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    monkeypatch.setenv("HMCX_P2_HELP", str(help_mode))
    X, Y = _dataset(B, D, K)
    s = _sampler(B, D, K, path_length, step_size)
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
    """The HMCX_P2_HELP=0 run of a case, computed once and shared."""
    if key not in _REF:
        _REF[key] = _traj(monkeypatch, 0, *args, **kw)
    return _REF[key]


def _assert_equal(a, b):
    assert a["L"].sum() > len(a["L"])                       # leapfrogs were run
    for k in ("W", "b", "mom", "A", "accepted", "ll", "E", "L"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("calls", [(12,), (6, 6)])
def test_config2_shape_bit_equal(monkeypatch, mode, calls):
    """B = 500, D = 784, K = 10, 1,500 rows (plan 8x16: 128 chain + 128 helper workgroups; the folded
    instantiation): 12 steps in one call, and two calls of 6 steps (step 0 of the second call reads W and
    b from global memory again, with the epochs and parities of a new launch)."""
    args = (500, 784, 10, list(calls))
    _assert_equal(_ref(monkeypatch, ("c2", calls), *args), _traj(monkeypatch, mode, *args))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(40, 32, 10), (64, 49, 3)])
def test_generic_kernel_uneven_ownership_bit_equal(monkeypatch, mode, shape):
    """The generic kernel at small shapes: B = 40, D = 32, K = 10 is the 2x2 plan in which one row-team
    member owns no softmax rows (its helper publishes ll0 = 0 and polls nothing in A-RS); B = 64, D = 49,
    K = 3 pads the classes to 16 and leaves ragged feature slices."""
    args = shape + ([8],)
    _assert_equal(_ref(monkeypatch, shape, *args), _traj(monkeypatch, mode, *args))


@pytest.mark.parametrize("mode", MODES)
def test_short_steps_bit_equal(monkeypatch, mode):
    """Path length = step size: L = ceil(2u) is 1 or 2, so a step has n = 0 or 1 leapfrog iterations and
    the chain reaches its accept before or with its helper (a step with n = 0 still needs ll0)."""
    args = (40, 32, 10, [30])
    kw = dict(path_length=1e-3, step_size=1e-3)
    a, b = _ref(monkeypatch, "short", *args, **kw), _traj(monkeypatch, mode, *args, **kw)
    n = b["L"].astype(int) - 1
    assert set(n.tolist()) == {0, 1}                        # the schedule really holds both
    for k in ("W", "b", "mom", "A", "accepted", "ll", "E", "L"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", MODES)
def test_traced_call_rows_equal_one_step_calls(monkeypatch, mode):
    """out_trace over 6 steps with helpers on: every row is the state that six one-step calls reach."""
    monkeypatch.setenv("HMCX_P2_HELP", str(mode))
    N, B, D, K = 400, 50, 40, 6
    X, Y = gi.dataset(63, N, D, K)
    rows = list(range(0, 6 * B, B))

    def make():
        s = _sampler(B, D, K, 0.05, 0.01, alpha=0.1)
        s.trace = []
        return s

    g = make()
    g.record_steps = True
    data = g._upload_data(X, Y)
    st = g._init_state()
    res = g._run(st, data, rows, [g.step_size] * len(rows), None, B)
    assert res.steps.shape == (len(rows), 1, D * K + K)

    h = make()
    data_h = h._upload_data(X, Y)
    st_h = h._init_state()
    A, acc, ll = [], [], []
    for i, r in enumerate(rows):
        ri = h._run(st_h, data_h, [r], [h.step_size], None, B)
        A.append(ri.A[0]); acc.append(ri.accepted[0]); ll.append(ri.ll[0])
        sh = h._state_to_host(st_h)
        np.testing.assert_array_equal(res.steps[i, 0, :D * K], np.asarray(sh["weights"]).reshape(-1))
        np.testing.assert_array_equal(res.steps[i, 0, D * K:], np.asarray(sh["bias"]))
    np.testing.assert_array_equal(res.A, np.array(A))
    np.testing.assert_array_equal(res.accepted, np.array(acc))
    np.testing.assert_array_equal(res.ll, np.array(ll))
    assert [t["L"] for t in g.trace] == [t["L"] for t in h.trace]
    assert 0 < np.sum(res.accepted) and len(np.unique(res.steps[:, 0, 0])) > 1   # the chain moves


@pytest.mark.allow_recovery
@pytest.mark.parametrize("mode", MODES)
def test_forced_abort_with_helpers_is_recovered(monkeypatch, capfd, mode):
    """HMCX_P2_FORCE_ABORT=1 (the cooperative early return of the last chain workgroup at step 1) with
    helpers on: chain workgroups leave from their polls, helpers from theirs, nothing is committed, and
    the call is re-run on the kernel-per-phase path — the oracle's results, counted once per re-run call."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    from test_gpu_recovery import _check_vs_oracle, _restore_path
    from test_gpu_samplers import _run_gpu
    monkeypatch.setenv("HMCX_P2_HELP", str(mode))
    monkeypatch.setenv("HMCX_P2_FORCE_ABORT", "1")
    try:
        # one call, by hand: W and b are untouched when the aborted launch has ended, and the recovery of
        # that one call is counted once
        B, D, K = 500, 784, 10
        X, Y = _dataset(B, D, K)
        s = _sampler(B, D, K, 5e-3, 1e-3)
        data = s._upload_data(X, Y)
        st = s._init_state()
        W0, b0 = st["weights"].clone(), st["bias"].clone()
        before = nat.recoveries_all()["persistent_sghmc"]
        h = s._enqueue(st, data, [0, B, 2 * B, 0], [1e-3] * 4, None, B)
        torch.cuda.synchronize()
        assert torch.equal(st["weights"], W0) and torch.equal(st["bias"], b0)
        res = s._collect(h)
        assert nat.recoveries_all()["persistent_sghmc"] == before + 1
        assert not torch.equal(st["weights"], W0) or not res.accepted.any()
        # a whole sample() run against the oracle
        _restore_path()
        capfd.readouterr()
        c = gi.TRAJ_CONFIGS["sghmc_mnist"]
        before = nat.recoveries_all()["persistent_sghmc"]
        got = _run_gpu(c, path=2)
    finally:
        _restore_path()
    err = capfd.readouterr().err
    assert "hand-off timed out" in err
    rerun = sum(int(n) for n in re.findall(r"re-running (\d+) call", err))
    assert rerun >= 1
    assert nat.recoveries_all()["persistent_sghmc"] == before + rerun
    _check_vs_oracle(c, got)
