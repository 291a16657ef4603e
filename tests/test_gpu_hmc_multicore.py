"""Multi-chain full-batch HMC (hmc_multicore.sample_multicore, hmcx_hmc_chains_run) against the NumPy
oracle: chain c of a noise='numpy' run reproduces oracle.samplers.hmc.sample(niter_w, burnin,
RandomState(c)) started from the global np.random state at entry; explicit ragged schedules against
oracle.samplers.hmc.step per chain; chain tilings (full + partial chain tiles); chain isolation; the
Philox mode against single-chain runs; the MVN route with the device diagnostics; the per-chain
fallback.

Tolerances are those of tests/test_gpu_hmc.py: float64 — path lengths and accept flags equal, states
rtol 1e-9 / atol 1e-12 (GEMM summation order only), losses rtol 1e-10, printed loss lines equal;
float32 — states rtol 1e-4 / atol 1e-5, losses rtol 1e-4 while no accept flips.  Every float64 test
first asserts on the oracle side that |A − u| > 1e-6 for every step and chain, so a seed that puts an
accept decision on the edge shows up as such."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import inputs as gi  # noqa: E402
from oracle import models as om  # noqa: E402
from oracle import samplers as osm  # noqa: E402

NP_SEED = 9


@pytest.fixture(scope="module", autouse=True)
def _no_recoveries():
    """No test of this file may have run through a recovery (re-run) path, as smoke() asserts."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    yield
    rec = nat.recoveries_all()
    assert not any(rec.values()), rec


def _mc(model, start, **kw):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc_multicore import hmc_multicore
    s = hmc_multicore(model, start, verbose=True, **kw)
    s.trace, s.out = [], io.StringIO()
    return s


def _flat(q):
    return np.concatenate([np.reshape(q["weights"], -1), np.reshape(q["bias"], -1)])


def _global_u(entry, n_steps):
    """The accept uniforms the global stream hands every chain (hmc.py:46 then :61 per step)."""
    keep = np.random.get_state()
    np.random.set_state(entry)
    u = np.array([(np.random.rand(), np.random.rand())[1] for _ in range(n_steps)])
    np.random.set_state(keep)
    return u


def _oracle_chains(model_o, start, X, Y, C, niter_w, burnin, **kw):
    """Per chain: oracle hmc.sample(niter_w, burnin, RandomState(c)) from the seeded global state."""
    np.random.seed(NP_SEED)
    entry = np.random.get_state()
    u = _global_u(entry, burnin + niter_w)
    runs = []
    for c in range(C):
        o = osm.hmc(model_o, start, verbose=True, **kw)
        o.trace, o.out = [], io.StringIO()
        np.random.set_state(entry)
        post, loss, pos, mom = o.sample(niter_w, burnin, np.random.RandomState(c), X_train=X, y_train=Y)
        A = np.array([t["A"] for t in o.trace])
        assert np.all(np.abs(A - u) > 1e-6), (c, A, u)          # no accept decision on the edge
        runs.append((post, loss, pos, mom, o))
    return entry, runs


def _compare_numpy_mode(model_g, model_o, start, X, Y, C, niter_w, burnin, f32=False, **kw):
    entry, runs = _oracle_chains(model_o, start, X, Y, C, niter_w, burnin, **kw)
    g = _mc(model_g, start, **kw)
    np.random.set_state(entry)
    post, positions, momentums, logp = g.sample_multicore(niter_w * C, burnin, C, X_train=X, y_train=Y)
    after = np.random.get_state()
    assert after[0] == entry[0] and np.array_equal(after[1], entry[1]) and after[2:] == entry[2:]
    # shapes and chain-major concatenation of the four returned objects
    for v in start:
        assert post[v].shape == (C * niter_w,) + np.shape(start[v])
    assert logp.shape == (C * niter_w,)
    assert len(positions) == C and len(momentums) == C
    assert all(len(p) == niter_w for p in positions) and all(len(m) == niter_w for m in momentums)
    assert len(g.chain_traces) == C and len(g.trace) == C * (burnin + niter_w)
    lines_g = g.out.getvalue().splitlines()
    lines_o = []
    for c, (po, lo, pos_o, mom_o, o) in enumerate(runs):
        sl = slice(c * niter_w, (c + 1) * niter_w)
        tg = g.chain_traces[c]
        assert [t["L"] for t in tg] == [t["L"] for t in o.trace]
        lines_o += o.out.getvalue().splitlines()
        if f32:
            if [t["accepted"] for t in tg] != [t["accepted"] for t in o.trace]:
                continue
            np.testing.assert_allclose(post["weights"][sl], po["weights"], rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(logp[sl], lo, rtol=1e-4)
            continue
        assert [t["accepted"] for t in tg] == [t["accepted"] for t in o.trace]
        for v in start:
            np.testing.assert_allclose(post[v][sl], po[v], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(logp[sl], lo, rtol=1e-10)
        for i in range(niter_w):
            for v in start:
                np.testing.assert_array_equal(momentums[c][i][0][v], mom_o[i][0][v])
                np.testing.assert_allclose(positions[c][i][0][v], pos_o[i][0][v], rtol=1e-9, atol=1e-12)
    if not f32:
        # per chain, in chain order, the lines that chain's sample prints (4-decimal losses identical)
        assert [l for l in lines_g if "loss" in l] == [l for l in lines_o if "loss" in l]
        assert sum("adapted step size" in l for l in lines_g) == C
    return g


def _softmax_problem(N=60, D=24, K=10, seed=3):
    X, Y = gi.dataset(seed, N, D, K)
    return X, Y, {"weights": np.zeros((D, K)), "bias": np.zeros(K)}


# ---------------------------------------------------------------------- 1. numpy mode against the oracle
@pytest.mark.parametrize("step,path", [(1e-2, 0.05), (5e-3, 1e-3)])
def test_numpy_mode_vs_oracle(step, path):
    """7 chains of K = 10 (chain tiles 6 + 1), N = 60 and D = 24 (partial last row / feature blocks);
    the second pair gives L = 1 on every step (no leapfrog, A = 1)."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    X, Y, start = _softmax_problem()
    g = _compare_numpy_mode(softmax({"alpha": 0.01}, dtype=torch.float64), om.softmax({"alpha": 0.01}), start, X, Y,
                            C=7, niter_w=6, burnin=2, path_length=path, step_size=step)
    if path == 1e-3:
        assert all(t["L"] == 1.0 for tr in g.chain_traces for t in tr)


# ---------------------------------------------------------------------- 2. ragged schedules, explicit inputs
EPS, LAM, ALPHA = 1e-2, 0.05, 0.01
N_ITER = np.array([[0, 1, 2, 9, 1, 3, 0],
                   [8, 0, 1, 2, 3, 1, 1],
                   [1, 1, 0, 0, 2, 7, 1],
                   [2, 3, 1, 0, 0, 1, 9]], dtype=np.int32)
U = np.array([[0.31, 0.9990, 0.52, 0.07, 0.9995, 0.44, 0.63],
              [0.12, 0.85, 0.9992, 0.38, 0.71, 0.9997, 0.05],
              [0.9993, 0.27, 0.66, 0.93, 0.18, 0.49, 0.9991],
              [0.58, 0.03, 0.9996, 0.74, 0.36, 0.9994, 0.22]])
_RAGGED = {}


class _StubRng:
    """rng.normal hands out one chain's momentum row of a step, variable by variable."""

    def __init__(self, row):
        self.row, self.at = row, 0

    def normal(self, loc, scale, size):
        n = int(np.prod(size))
        out = self.row[self.at:self.at + n].reshape(size).copy()
        self.at += n
        return out


def _ragged_inputs():
    X, Y, start = _softmax_problem()
    S, C = N_ITER.shape
    D, K = start["weights"].shape
    rs = np.random.RandomState(77)
    W0 = rs.normal(0, 0.05, (C, D, K))
    b0 = rs.normal(0, 0.05, (C, K))
    noise = rs.normal(0, 1, (S, C, D * K + K))
    return X, Y, start, W0, b0, noise


def _ragged_oracle(monkeypatch):
    """oracle.samplers.hmc.step per chain: np.random.rand returns the value that yields the wanted L,
    r = (L − 0.5)·ε/(2λ), then the hand-written u."""
    if "o" in _RAGGED:
        return _RAGGED["o"]
    X, Y, start, W0, b0, noise = _ragged_inputs()
    S, C = N_ITER.shape
    P = noise.shape[2]
    out = dict(A=np.empty((S, C)), acc=np.empty((S, C), bool), nlp=np.empty((S, C)), E=np.empty((S, C, 2)),
               trace=np.empty((S, C, P)))
    o = osm.hmc(om.softmax({"alpha": ALPHA}), start, path_length=LAM, step_size=EPS)
    o.trace = []
    for c in range(C):
        q = {"weights": W0[c].copy(), "bias": b0[c].copy()}
        for s in range(S):
            L = int(N_ITER[s, c]) + 1
            vals = iter([(L - 0.5) * EPS / (2 * LAM), U[s, c]])
            with monkeypatch.context() as mp:
                mp.setattr(np.random, "rand", lambda: next(vals))
                q, _, _, _, A = o.step(q, None, _StubRng(noise[s, c]), X_train=X, y_train=Y)
            assert o.trace[-1]["L"] == float(L)
            out["A"][s, c], out["acc"][s, c], out["E"][s, c] = A, o.trace[-1]["accepted"], o._E
            out["nlp"][s, c] = o.model.negative_log_posterior(q, X_train=X, y_train=Y)
            out["trace"][s, c] = _flat(q)
    assert np.all(np.abs(out["A"] - U) > 1e-6)
    assert out["acc"].any() and not out["acc"].all()             # both branches of the commit
    _RAGGED["o"] = out
    return out


def _ragged_gpu(W0, b0, n_iter):
    """hmcx_hmc_chains_run in BUFFER mode on explicit inputs; chain c starts at (W0[c], b0[c])."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    X, Y, start, _, _, noise = _ragged_inputs()
    S, C = n_iter.shape
    D, K = start["weights"].shape
    P = D * K + K
    g = _mc(softmax({"alpha": ALPHA}, dtype=torch.float64), start, path_length=LAM, step_size=EPS)
    dev = g.model.device
    W = torch.as_tensor(np.ascontiguousarray(W0.transpose(1, 0, 2).reshape(D, C * K))).to(dev)
    b = torch.as_tensor(b0.reshape(-1).copy()).to(dev)
    tr = torch.full((S, C, P), -7.0, dtype=torch.float64, device=dev)
    data = g._linear_data({"X_train": X, "y_train": Y})
    A, acc, nlp, E = g._hmc_chains_call(W, b, data, n_iter, U, torch.as_tensor(noise.reshape(-1)).to(dev), 0, tr, None)
    Wf = W.cpu().numpy().reshape(D, C, K).transpose(1, 0, 2)
    return dict(A=A, acc=acc, nlp=nlp, E=E, trace=tr.cpu().numpy(), W=Wf, b=b.cpu().numpy().reshape(C, K))


def test_ragged_schedule_vs_oracle_step(monkeypatch):
    """n_iter mixes 0, 1 and one chain ≥ 5 iterations longer than the rest (a different chain each
    step): every chain takes its own kicks/drifts from (evaluation index, n_iter) and stops writing
    after its last evaluation."""
    exp = _ragged_oracle(monkeypatch)
    _, _, start, W0, b0, _ = _ragged_inputs()
    got = _ragged_gpu(W0, b0, N_ITER)
    D, K = start["weights"].shape
    np.testing.assert_array_equal(got["acc"], exp["acc"])
    np.testing.assert_allclose(got["A"], exp["A"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got["nlp"], exp["nlp"], rtol=1e-10)
    np.testing.assert_allclose(got["E"], exp["E"], rtol=1e-10)
    np.testing.assert_allclose(got["trace"], exp["trace"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got["W"].reshape(7, -1), exp["trace"][-1][:, :D * K], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got["b"], exp["trace"][-1][:, D * K:], rtol=1e-9, atol=1e-12)
    # the final state is the last trace row, bit for bit
    np.testing.assert_array_equal(got["W"].reshape(7, -1), got["trace"][-1][:, :D * K])
    np.testing.assert_array_equal(got["b"], got["trace"][-1][:, D * K:])
    assert np.all(got["A"][N_ITER == 0] == 1.0)                   # n_iter = 0: q kept, A = 1


# ---------------------------------------------------------------------- 3. chain tilings
def test_chain_tiling_softmax_k3():
    """K = 3: 21 chains per tile, C = 22 → tiles 21 + 1."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    X, Y, start = _softmax_problem(N=40, D=20, K=3)
    _compare_numpy_mode(softmax({"alpha": 0.01}, dtype=torch.float64), om.softmax({"alpha": 0.01}), start, X, Y,
                        C=22, niter_w=2, burnin=1, path_length=0.05, step_size=1e-2)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_chain_tiling_logistic(dtype):
    """Logistic, K = 1: 64 chains per tile, C = 70 → tiles 64 + 6; float32 compared while no accept flips."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.logistic import logistic
    X, y, _, _ = gi.logistic_inputs(11, 120, 4)
    start = {"weights": np.full((4, 1), 0.3), "bias": np.array([0.1])}
    _compare_numpy_mode(logistic({"alpha": 0.25}, dtype=dtype), om.logistic({"alpha": 0.25}), start, X, y,
                        C=70, niter_w=2, burnin=1, f32=dtype == torch.float32, path_length=0.005, step_size=1e-3)


# ---------------------------------------------------------------------- 4. chain isolation
def test_chain_isolation_and_nan_chain():
    """Chain 3 with another start and schedule, then with an all-NaN start: every other chain's outputs
    stay bit-identical; the NaN chain reports A = 1 and is accepted (Python's min(1, nan) = 1)."""
    _, _, start, W0, b0, _ = _ragged_inputs()
    D, K = start["weights"].shape
    base = _ragged_gpu(W0, b0, N_ITER)
    W1, b1, n1 = W0.copy(), b0.copy(), N_ITER.copy()
    W1[3] = np.random.RandomState(5).normal(0, 0.2, (D, K))
    b1[3] = 0.3
    n1[:, 3] = [1, 12, 4, 0]
    other = _ragged_gpu(W1, b1, n1)
    W2, b2 = W0.copy(), b0.copy()
    W2[3], b2[3] = np.nan, np.nan
    nan = _ragged_gpu(W2, b2, N_ITER)
    keep = [c for c in range(7) if c != 3]
    for run in (other, nan):
        for k in ("A", "acc", "nlp", "E", "trace", "W", "b"):
            a, b = base[k], run[k]
            if k in ("W", "b"):
                np.testing.assert_array_equal(a[keep], b[keep], err_msg=k)
            else:
                np.testing.assert_array_equal(a[:, keep], b[:, keep], err_msg=k)
    assert not np.array_equal(base["trace"][:, 3], other["trace"][:, 3])
    assert np.all(nan["A"][:, 3] == 1.0) and np.all(nan["acc"][:, 3])
    assert np.all(np.isnan(nan["trace"][:, 3])) and np.all(np.isnan(nan["nlp"][:, 3]))
    assert np.all(np.isfinite(nan["trace"][:, keep]))


# ---------------------------------------------------------------------- 5. Philox
def test_philox_chains_vs_single_chain():
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc import hmc
    X, Y, start = _softmax_problem(N=200, D=784)
    model = softmax({"alpha": 0.01}, dtype=torch.float64)
    kw = dict(path_length=0.01, step_size=1e-3, noise="philox")
    C = 8
    runs = []
    for seed in (4, 4, 5):
        g = _mc(model, start, seed=seed, **kw)
        post, pos, mom, logp = g.sample_multicore(80, 2, C, X_train=X, y_train=Y)
        runs.append((post, logp, g.chain_traces, mom))
    for v in start:
        np.testing.assert_array_equal(runs[0][0][v], runs[1][0][v])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert not np.array_equal(runs[0][0]["weights"], runs[2][0]["weights"])
    Ls = [[t["L"] for t in tr] for tr in runs[0][2]]
    assert len({tuple(l) for l in Ls}) > 1                         # ragged: the chains' path lengths differ
    post, logp, traces, mom = runs[0]
    for c in range(C):
        h = hmc(model, start, verbose=True, seed=4, chain=c, **kw)
        h.trace, h.out = [], io.StringIO()
        p1, l1, _, m1 = h.sample(10, 2, X_train=X, y_train=Y)
        assert [t["L"] for t in traces[c]] == [t["L"] for t in h.trace]
        assert [t["accepted"] for t in traces[c]] == [t["accepted"] for t in h.trace]
        sl = slice(c * 10, (c + 1) * 10)
        for v in start:
            np.testing.assert_allclose(post[v][sl], p1[v], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(logp[sl], l1, rtol=1e-10)
        for i in range(10):
            np.testing.assert_array_equal(mom[c][i][0]["weights"], m1[i][0]["weights"])


# ---------------------------------------------------------------------- 6. MVN
MVN_SEED = 2024


def test_mvn_chains_diagnostics_and_mean():
    """Config 1 (μ = 0, Σ = [[1, .8], [.8, 1]], ε = 0.1, λ = 1), 64 Philox chains of 250 draws:
    chain_diagnostics() equals the host split-R̂ / ESS on the returned draws (rtol 1e-9, the tolerance
    of tests/test_gpu_diagnostics.py) and the pooled mean is within 3·MCSE of 0 (MCSE = sd/√ESS, the
    criterion of tests/test_gpu_statistics.py).  A host replay of these chains (the oracle's step fed
    from the Philox host twins) with this seed stays within the same bound: |mean|/MCSE = 1.74, 1.60."""
    from dropout_hamiltonian_montecarlo_amd import diagnostics
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mvn_gaussian import mvn_gaussian
    c = gi.MVN_CONFIG
    m = mvn_gaussian({"mu": np.array(c["mu"]), "cov": np.array(c["cov"])}, device="cuda:0")
    s = _mc(m, {"x": np.zeros(2)}, path_length=c["path_length"], step_size=c["step_size"], noise="philox",
            seed=MVN_SEED)
    with pytest.raises(HmcxError):
        s.chain_diagnostics()                                      # before any sample_multicore call
    C, T = 64, 250
    post, pos, mom, logp = s.sample_multicore(C * T, 100, C)
    assert post["x"].shape == (C * T, 2) and logp.shape == (C * T,) and len(pos) == C and len(mom) == C
    x = post["x"].reshape(C, T, 2)
    np.testing.assert_array_equal(pos[5][7][0]["x"], x[5, 6])      # position before draw 7 = draw 6
    srhat, ess = s.chain_diagnostics()
    np.testing.assert_allclose(srhat, diagnostics.split_rhat(x), rtol=1e-9)
    np.testing.assert_allclose(ess, diagnostics.ess(x), rtol=1e-9)
    flat = x.reshape(-1, 2)
    mcse = flat.std(axis=0, ddof=1) / np.sqrt(ess)
    print("pooled mean", flat.mean(axis=0), "mcse", mcse, "ess", ess, "split-rhat", srhat)
    assert np.all(np.abs(flat.mean(axis=0)) <= 3 * mcse)
    s.sample_multicore(C * 3, 0, C)
    with pytest.raises(HmcxError):
        s.chain_diagnostics()                                      # T = 3 < 4


# ---------------------------------------------------------------------- 7. fallback
def test_fallback_one_sample_per_chain():
    """GPU-prior softmax has no chain-batched entry: sample_multicore runs sample once per chain, chain c
    with RandomState(c) from the entry state of the global stream, which is restored afterwards."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc import hmc
    X, Y, _ = _softmax_problem(N=40, D=12, K=4)
    start = {"weights": np.full((12, 4), 0.05), "bias": np.linspace(-0.1, 0.1, 4)}
    model = softmax({"alpha": 0.5}, prior="gpu")
    kw = dict(path_length=0.03, step_size=1e-2)
    np.random.seed(NP_SEED)
    entry = np.random.get_state()
    g = _mc(model, start, **kw)
    post, pos, mom, logp = g.sample_multicore(8, 1, 2, X_train=X, y_train=Y)
    after = np.random.get_state()
    assert np.array_equal(after[1], entry[1]) and after[2:] == entry[2:]
    lines = []
    for c in range(2):
        h = hmc(model, start, verbose=True, **kw)
        h.trace, h.out = [], io.StringIO()
        np.random.set_state(entry)
        p1, l1, pos1, m1 = h.sample(4, 1, np.random.RandomState(c), X_train=X, y_train=Y)
        lines += h.out.getvalue().splitlines()
        sl = slice(c * 4, (c + 1) * 4)
        for v in start:
            np.testing.assert_array_equal(post[v][sl], p1[v])
        np.testing.assert_array_equal(logp[sl], l1)
        assert g.chain_traces[c] == h.trace
        assert len(pos[c]) == len(pos1) == 4
        for i in range(4):
            np.testing.assert_array_equal(mom[c][i][0]["weights"], m1[i][0]["weights"])
    assert g.out.getvalue().splitlines() == lines
    assert not np.array_equal(post["weights"][:4], post["weights"][4:])   # RandomState(0) vs RandomState(1)
    np.random.set_state(entry)
