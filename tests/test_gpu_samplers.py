"""GPU parity of the fused samplers against the NumPy oracle and the reference's golden runs.

Integer bookkeeping (path lengths, accept flags) must be bit-exact; float64 states within
rel 1e-9 (GEMM summation order only); float32 runs are compared statistically/loosely, except
test_sgld_f32_paths_vs_oracle: float32 SGLD at ragged shapes on the kernel-per-phase path and both forms of
the wide path, within max(16·d, 1e-5·s) of the float64 oracle (d: the oracle run in float32 against itself
in float64; tests/_linear_cases.py).  Measured on MI355X, largest err/d over the seven shapes:
  states   1.0 on all three paths, at (K, D, B) = (2, 1, 1): err = d = 3.7e-9; err/tolerance at most 0.046
           (kernel-per-phase, (38, 2000, 130): err 1.4e-6, d 1.9e-6), 0.021 on the wide paths
  logp     1.8 kernel-per-phase, 2.3 wide, both at (64, 300, 40): err 1.1e-7 / 1.4e-7, d 5.9e-8;
           err/tolerance at most 0.002
  ll       the same ratios (ll is logp without the prior's constant); err/tolerance at most 0.047
The fused and the three-launch wide path agree to every printed digit.  16·d is the bound on the states at
D = 785 and D = 2000; no output came near it."""
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import inputs as gi  # noqa: E402
from oracle import models as om  # noqa: E402
from oracle import samplers as osm  # noqa: E402

import _linear_cases as lc  # noqa: E402


def _gpu_classes():
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sgld import sgld
    return softmax, sghmc, sgld


def _run_oracle(c):
    X, Y = gi.dataset(c["data_seed"], c["N"], c["D"], c["K"])
    cls = osm.sghmc if c["kind"] == "sghmc" else osm.sgld
    s = cls(om.softmax({"alpha": c["alpha"]}), {"weights": np.zeros((c["D"], c["K"])), "bias": np.zeros(c["K"])},
            path_length=c["path_length"], step_size=c["step_size"], verbose=True)
    s.trace = []
    s.out = io.StringIO()
    np.random.seed(c["np_seed"])
    post, logp = s.sample(epochs=c["epochs"], burnin=c["burnin"], batch_size=c["B"],
                          rng=np.random.RandomState(c["rng_seed"]), X_train=X, y_train=Y)
    return post, logp, s.trace, s.out.getvalue()


def _run_gpu(c, dtype=torch.float64, noise="numpy", seed=0, path=0):
    softmax, sghmc, sgld = _gpu_classes()
    X, Y = gi.dataset(c["data_seed"], c["N"], c["D"], c["K"])
    cls = sghmc if c["kind"] == "sghmc" else sgld
    m = softmax({"alpha": c["alpha"]}, dtype=dtype, device="cuda:0")
    m.ctx.set_sghmc_path(path)
    s = cls(m,
            {"weights": np.zeros((c["D"], c["K"])), "bias": np.zeros(c["K"])},
            path_length=c["path_length"], step_size=c["step_size"], verbose=True, noise=noise, seed=seed)
    s.trace = []
    s.out = io.StringIO()
    np.random.seed(c["np_seed"])
    post, logp = s.sample(epochs=c["epochs"], burnin=c["burnin"], batch_size=c["B"],
                          rng=np.random.RandomState(c["rng_seed"]), X_train=X, y_train=Y)
    return post, logp, s.trace, s.out.getvalue()


_PATHS = [(n, p) for n in sorted(gi.TRAJ_CONFIGS) for p in ((1, 2) if gi.TRAJ_CONFIGS[n]["kind"] == "sghmc" else (0,))]


@pytest.mark.parametrize("name,path", _PATHS)
def test_trajectory_f64_vs_oracle_and_golden(name, path, golden_dir):
    """path 1 = kernel-per-phase, 2 = persistent 2-D kernel (both must agree with NumPy)."""
    c = gi.TRAJ_CONFIGS[name]
    post_r, logp_r, tr_r, log_r = _run_oracle(c)
    post_g, logp_g, tr_g, log_g = _run_gpu(c, path=path)
    # integer bookkeeping: bit-exact
    if c["kind"] == "sghmc":
        assert [t["L"] for t in tr_g] == [t["L"] for t in tr_r]
        assert [t["accepted"] for t in tr_g] == [t["accepted"] for t in tr_r]
        assert [t["eps"] for t in tr_g] == [t["eps"] for t in tr_r]
    # float64 state: GEMM summation order only
    for v in ("weights", "bias"):
        np.testing.assert_allclose(post_g[v], post_r[v], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(logp_g, logp_r, rtol=1e-11)
    if c["kind"] == "sghmc":
        A_r = np.array([t["A"] for t in tr_r])
        A_g = np.array([t["A"] for t in tr_g])
        np.testing.assert_allclose(A_g, A_r, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose([t["E"] for t in tr_g], [t["E"] for t in tr_r], rtol=1e-10, atol=1e-9)
    # the printed log lines (4 decimals) are identical to the reference's
    ref_lines = [l for l in log_r.splitlines() if "loss" in l]
    gpu_lines = [l for l in log_g.splitlines() if "loss" in l]
    assert gpu_lines == ref_lines
    # and against the reference's own stored run
    d = np.load(os.path.join(golden_dir, "traj_%s.npz" % name))
    np.testing.assert_allclose(logp_g, d["logp"], rtol=1e-11)
    if c["kind"] == "sghmc":
        np.testing.assert_array_equal([t["accepted"] for t in tr_g], d["trace"][:, 2].astype(bool))
        np.testing.assert_array_equal([max(0, t["L"] - 1) for t in tr_g], d["trace"][:, 0])
    if "post_weights" in d.files:
        np.testing.assert_allclose(post_g["weights"], d["post_weights"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name,path", [("sghmc_small", 1), ("sghmc_small", 2), ("sgld_small", 0),
                                       ("sghmc_hot", 1), ("sghmc_hot", 2), ("sghmc_mnist", 2)])
def test_trajectory_f32(name, path):
    c = gi.TRAJ_CONFIGS[name]
    post_r, logp_r, tr_r, _ = _run_oracle(c)
    post_g, logp_g, tr_g, _ = _run_gpu(c, dtype=torch.float32, path=path)
    if c["kind"] == "sghmc":
        assert [t["L"] for t in tr_g] == [t["L"] for t in tr_r]
    scale = np.abs(post_r["weights"]).max() + 1e-3
    assert np.abs(post_g["weights"] - post_r["weights"]).max() <= 1e-3 * scale
    np.testing.assert_allclose(logp_g, logp_r, rtol=1e-4)


@pytest.mark.parametrize("path", [1, 2])
def test_philox_mode_runs_and_is_deterministic(path):
    c = dict(gi.TRAJ_CONFIGS["sghmc_mnist"])
    p1, l1, t1, _ = _run_gpu(c, noise="philox", seed=11, path=path)
    p2, l2, t2, _ = _run_gpu(c, noise="philox", seed=11, path=path)
    p3, l3, t3, _ = _run_gpu(c, noise="philox", seed=12, path=path)
    np.testing.assert_array_equal(p1["weights"], p2["weights"])
    assert [t["L"] for t in t1] == [t["L"] for t in t2]
    assert not np.array_equal(p1["weights"], p3["weights"])
    assert np.all(np.isfinite(l1))


@pytest.mark.parametrize("path", [2])
def test_philox_paths_agree(path):
    """Every SGHMC implementation consumes the same Philox streams: same trajectory (f64)."""
    c = dict(gi.TRAJ_CONFIGS["sghmc_mnist"])
    p1, l1, t1, _ = _run_gpu(c, noise="philox", seed=5, path=1)
    p2, l2, t2, _ = _run_gpu(c, noise="philox", seed=5, path=path)
    assert [t["accepted"] for t in t1] == [t["accepted"] for t in t2]
    assert [t["L"] for t in t1] == [t["L"] for t in t2]
    np.testing.assert_allclose(p1["weights"], p2["weights"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(p1["bias"], p2["bias"], rtol=1e-9, atol=1e-12)


def test_philox_paths_agree_long_run():
    """A long config-2 run (B = 500, D = 784, 150 steps, the folded k_sghmc_p2<double,10,1> the bench
    times) against the kernel-per-phase path on the same Philox streams: every path length and accept
    flag equal, the accept-test energies within rel 1e-9 and the final state within rel 1e-8.  The
    persistent kernel's B-gemm sums its k values in another grouping than k_grad,
    so only floating-point summation order separates the two."""
    c = dict(gi.TRAJ_CONFIGS["sghmc_mnist"], N=25000, burnin=0, epochs=3)
    p1, _, t1, _ = _run_gpu(c, noise="philox", seed=17, path=1)
    p2, _, t2, _ = _run_gpu(c, noise="philox", seed=17, path=2)
    assert len(t1) == 150
    assert [t["L"] for t in t1] == [t["L"] for t in t2]
    assert [t["accepted"] for t in t1] == [t["accepted"] for t in t2]
    np.testing.assert_allclose(np.array([t["E"] for t in t2]), np.array([t["E"] for t in t1]), rtol=1e-9)
    np.testing.assert_allclose(p2["weights"], p1["weights"], rtol=1e-8, atol=1e-11)


def test_philox_noise_statistics():
    """Device momentum in philox mode is N(0,1): one SGHMC step with 0 leapfrog iterations
    leaves q unchanged and A = 1 (the n_iter == 0 branch), and SGLD noise has std 2ε."""
    softmax, sghmc, sgld = _gpu_classes()
    D, K, B = 256, 10, 64
    X, Y = gi.dataset(5, B, D, K)
    s = sgld(softmax({"alpha": 0.0}), {"weights": np.zeros((D, K)), "bias": np.zeros(K)},
             step_size=1e-3, noise="philox", seed=3)
    s.out = io.StringIO()
    post, _ = s.sample(epochs=1, burnin=0, batch_size=B, X_train=X, y_train=Y)
    # q = 2ε·ξ − ½ε·∇U(0) (one step): remove the deterministic part and check the noise std
    g = om.softmax({"alpha": 0.0}).grad({"weights": np.zeros((D, K)), "bias": np.zeros(K)}, X_train=X, y_train=Y)
    xi = (post["weights"][0] + 0.5 * 1e-3 * g["weights"]) / (2e-3)
    assert abs(xi.std() - 1.0) < 0.05 and abs(xi.mean()) < 0.05


def test_hmc_mvn_vs_golden(golden_dir):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mvn_gaussian import mvn_gaussian
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc import hmc
    c = gi.MVN_CONFIG
    d = np.load(os.path.join(golden_dir, "hmc_mvn.npz"))
    m = mvn_gaussian({"mu": np.array(c["mu"]), "cov": np.array(c["cov"])}, device="cuda:0")
    h = hmc(m, {"x": np.zeros(2)}, path_length=c["path_length"], step_size=c["step_size"], verbose=True)
    h.out = io.StringIO()
    h.trace = []
    np.random.seed(c["np_seed"])
    post, loss, pos, mom = h.sample(c["niter"], c["burnin"], np.random.RandomState(c["rng_seed"]))
    acc = np.array([t["accepted"] for t in h.trace])[c["burnin"]:]
    ref_acc = d["trace"][c["burnin"]:, 2].astype(bool)
    # the leapfrog is chaotic-free here, but a 1-ulp difference can flip a near-tie accept
    # eventually: require bit-exact flags/positions over the first 500 sampling steps
    np.testing.assert_array_equal(acc[:500], ref_acc[:500])
    np.testing.assert_allclose(post["x"][:500], d["post_x"][:500], rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(np.array([p[0]["x"] for p in mom]), d["mom0"])
    C = np.cov(post["x"].T)
    assert abs(C[0, 1] / np.sqrt(C[0, 0] * C[1, 1]) - 0.8) < 0.06


def test_hmc_generic_softmax_vs_golden(golden_dir):
    softmax, _, _ = _gpu_classes()
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc import hmc
    c = gi.HMC_SOFTMAX_CONFIG
    d = np.load(os.path.join(golden_dir, "hmc_softmax.npz"))
    X, Y = gi.dataset(c["data_seed"], c["N"], c["D"], c["K"])
    h = hmc(softmax({"alpha": c["alpha"]}), {"weights": np.zeros((c["D"], c["K"])), "bias": np.zeros(c["K"])},
            path_length=c["path_length"], step_size=c["step_size"], verbose=True)
    h.out = io.StringIO()
    h.trace = []
    np.random.seed(c["np_seed"])
    post, loss, _, _ = h.sample(c["niter"], c["burnin"], np.random.RandomState(c["rng_seed"]), X_train=X, y_train=Y)
    np.testing.assert_array_equal([t["accepted"] for t in h.trace], d["trace"][:, 2].astype(bool))
    np.testing.assert_allclose(post["weights"], d["post_weights"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(loss, d["loss"], rtol=1e-10)


@pytest.mark.parametrize("path", [1, 2])
def test_full_size_mnist_shape_properties(path):
    """BASELINE config 2 size (N=60000 would be slow for the oracle; use N=5000, B=500, D=784):
    every step accepted or rejected consistently with its own A and u; logp finite; the state
    after sampling equals the last posterior sample."""
    softmax, sghmc, _ = _gpu_classes()
    X, Y = gi.dataset(0, 5000, 784, 10)
    m = softmax({"alpha": 0.01})
    m.ctx.set_sghmc_path(path)
    s = sghmc(m, {"weights": np.zeros((784, 10)), "bias": np.zeros(10)},
              path_length=1e-2, step_size=1e-3, noise="philox", seed=1)
    s.out = io.StringIO()
    s.trace = []
    post, logp = s.sample(epochs=2, burnin=1, batch_size=500, X_train=X, y_train=Y)
    assert np.all(np.isfinite(logp)) and post["weights"].shape == (2, 784, 10)
    np.testing.assert_array_equal(s.last_state["weights"].cpu().numpy(), post["weights"][-1])
    assert all(0.0 <= t["A"] <= 1.0 for t in s.trace)


def test_sgld_wide_features_split_forward_vs_oracle(monkeypatch):
    """Config-5-like shape (D = 1536 features, K = 38 classes, one chain) on the kernel-per-phase
    path (HMCX_SGLD_WIDE=0): the forward's D reduction is split over several workgroups per tile
    (slab mode); trajectory within rel 1e-9 of the oracle."""
    monkeypatch.setenv("HMCX_SGLD_WIDE", "0")
    c = dict(kind="sgld", N=300, B=100, D=1536, K=38, alpha=0.01, step_size=1e-4, path_length=1.0,
             burnin=1, epochs=2, data_seed=31, np_seed=8, rng_seed=9)
    post_r, logp_r, _, _ = _run_oracle(c)
    post_g, logp_g, _, _ = _run_gpu(c)
    for v in ("weights", "bias"):
        np.testing.assert_allclose(post_g[v], post_r[v], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(logp_g, logp_r, rtol=1e-10)


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("K,D,B", [(38, 2048, 500), (10, 131, 77), (64, 300, 40), (17, 8, 5), (38, 2000, 130)])
def test_sgld_wide_path_vs_oracle(K, D, B, fuse, monkeypatch):
    """The wide SGLD path (hmcx_wide.hip), forced here for every shape, as two launches per step
    (fuse=1: forward + softmax fused by a team round, k_wfwd_sm) or three (fuse=0: k_wfwd, k_wsoft,
    k_wgrad): float64 trajectory within rel 1e-9 of the oracle, printed loss lines identical.
    Covers BASELINE config 5's shape (D=2048, K=38, B=500), a ragged shape (D not a multiple of the
    vector width, partial row block), the largest class count, a D smaller than one MFMA k-step group,
    and ragged row and feature blocks at config-5 width."""
    monkeypatch.setenv("HMCX_SGLD_WIDE", "1")
    monkeypatch.setenv("HMCX_WIDE_FUSE", fuse)
    c = dict(kind="sgld", N=2 * B, B=B, D=D, K=K, alpha=0.01, step_size=1e-4, path_length=1.0,
             burnin=1, epochs=2, data_seed=41, np_seed=2, rng_seed=3)
    post_r, logp_r, _, log_r = _run_oracle(c)
    post_g, logp_g, _, log_g = _run_gpu(c)
    for v in ("weights", "bias"):
        np.testing.assert_allclose(post_g[v], post_r[v], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(logp_g, logp_r, rtol=1e-10)
    assert [l for l in log_g.splitlines() if "loss" in l] == [l for l in log_r.splitlines() if "loss" in l]


@pytest.mark.allow_recovery
def test_sgld_wide_fused_timeout_reruns_unfused(monkeypatch, capfd):
    """A timed-out team round of the fused forward (forced: HMCX_WIDE_FORCE_ABORT=<step> raises the
    abort word in that step's launch) makes the call put its start state back and run again on the
    three-launch path: the trajectory is still the oracle's, and the re-run is reported on stderr."""
    monkeypatch.setenv("HMCX_SGLD_WIDE", "1")
    monkeypatch.setenv("HMCX_WIDE_FUSE", "1")
    monkeypatch.setenv("HMCX_WIDE_FORCE_ABORT", "1")
    c = dict(kind="sgld", N=1000, B=500, D=2048, K=38, alpha=0.01, step_size=1e-4, path_length=1.0,
             burnin=1, epochs=2, data_seed=41, np_seed=2, rng_seed=3)
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    post_r, logp_r, _, _ = _run_oracle(c)
    before = nat.recoveries_all()["sgld_wide_fused"]
    post_g, logp_g, _, _ = _run_gpu(c)
    for v in ("weights", "bias"):
        np.testing.assert_allclose(post_g[v], post_r[v], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(logp_g, logp_r, rtol=1e-10)
    assert "re-run on the three-launch path" in capfd.readouterr().err
    # one forced abort per call (step 1 of every epoch's call, burn-in included), each counted once
    assert nat.recoveries_all()["sgld_wide_fused"] == before + c["burnin"] + c["epochs"]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sgld_wide_equals_kernel_path_philox(dtype, monkeypatch):
    """Config 5 (D=2048, K=38, B=500): the wide path and the kernel-per-phase path consume the same
    Philox noise, so they produce the same trajectory up to summation order (f64: rel 1e-9;
    f32: rel 1e-4 + 1e-7 absolute)."""
    c = dict(kind="sgld", N=1500, B=500, D=2048, K=38, alpha=0.01, step_size=1e-4, path_length=1.0,
             burnin=0, epochs=2, data_seed=43, np_seed=0, rng_seed=0)
    dt = torch.float64 if dtype == "f64" else torch.float32
    monkeypatch.setenv("HMCX_SGLD_WIDE", "1")
    pw, lw, _, _ = _run_gpu(c, dtype=dt, noise="philox", seed=9)
    monkeypatch.setenv("HMCX_SGLD_WIDE", "0")
    ps, ls, _, _ = _run_gpu(c, dtype=dt, noise="philox", seed=9)
    tol = dict(rtol=1e-9, atol=1e-12) if dtype == "f64" else dict(rtol=1e-4, atol=1e-7)
    for v in ("weights", "bias"):
        np.testing.assert_allclose(pw[v], ps[v], **tol)
    np.testing.assert_allclose(lw, ls, rtol=1e-9 if dtype == "f64" else 1e-4)


@pytest.mark.parametrize("wide,fuse", lc.SGLD_PATHS, ids=["kernels", "wide-fused", "wide-3-launches"])
@pytest.mark.parametrize("K,D,B", lc.SGLD_SHAPES)
def test_sgld_f32_paths_vs_oracle(K, D, B, wide, fuse, monkeypatch):
    """float32 SGLD on the kernel-per-phase path and on both forms of the wide path at ragged shapes (one
    row and one feature; K < 16, K one past a class tile, K = 64; D not a multiple of 4, of 16, of the
    128-feature slice; partial row blocks) against oracle.samplers.sgld in float64 on the float32-rounded
    data.  step_size 1e-2: from the zero start a smaller step leaves the state almost pure noise and a wrong
    gradient within the tolerance.  States, logp and the log-likelihood inside logp within max(16·d, 1e-5·s)
    (tests/_linear_cases.py::sgld_tolerances; d from the oracle run in float32 throughout)."""
    monkeypatch.setenv("HMCX_SGLD_WIDE", wide)
    if fuse is None:
        monkeypatch.delenv("HMCX_WIDE_FUSE", raising=False)
    else:
        monkeypatch.setenv("HMCX_WIDE_FUSE", fuse)
    c = lc.sgld_config(K, D, B)
    s_r, logp_r = lc.sgld_reference(K, D, B)
    tol, d = lc.sgld_tolerances(K, D, B)
    post_g, logp_g, _, _ = _run_gpu(c, dtype=torch.float32)
    s_g = np.concatenate([post_g["weights"].reshape(c["epochs"], -1), post_g["bias"]], axis=1)
    err = {"states": float(np.max(np.abs(s_g - s_r))), "logp": float(np.max(np.abs(logp_g - logp_r))),
           "ll": float(np.max(np.abs(lc.sgld_loglik(K, D, B, logp_g) - lc.sgld_loglik(K, D, B, logp_r))))}
    for o in ("states", "logp", "ll"):
        print("sgld f32 K %d D %d B %d wide %s fuse %s %s: err %.3e, d %.3e, err/d %.3g, allowed %.3e" % (
            K, D, B, wide, fuse, o, err[o], d[o], err[o] / d[o] if d[o] > 0 else float("inf"), tol[o]))
    for o in ("states", "logp", "ll"):
        assert err[o] <= tol[o], (o, err[o], tol[o])


def _run_variant_oracle(c):
    X, Y = gi.dataset(c["data_seed"], c["N"], c["D"], c["K"])
    s = osm.sgld_gpu_variant(om.softmax({"alpha": c["alpha"]}),
                             {"weights": np.zeros((c["D"], c["K"])), "bias": np.zeros(c["K"])},
                             path_length=1.0, step_size=c["step_size"], verbose=True)
    s.out = io.StringIO()
    post, logp = s.sample(epochs=c["epochs"], burnin=c["burnin"], batch_size=c["B"],
                          rng=np.random.RandomState(c["rng_seed"]), X_train=X, y_train=Y)
    return post, logp, s.out.getvalue()


@pytest.mark.parametrize("wide", ["0", "1"])
@pytest.mark.parametrize("K,D,B", [(10, 40, 100), (38, 300, 64), (3, 7, 5)])
def test_sgld_gpu_variant_vs_oracle(K, D, B, wide, monkeypatch):
    """variant='gpu' (gpu/sgld.py:11-20): p = ν⊙p_prev − ½ε∇U carried across steps,
    on both SGLD paths (wide single-workgroup-row kernels and kernel-per-phase).  float64
    trajectory within rel 1e-9 of the oracle's sgld_gpu_variant; the printed loss lines match.
    Parity is against the oracle restatement only: the CuPy reference is not importable here."""
    monkeypatch.setenv("HMCX_SGLD_WIDE", wide)
    softmax, _, sgld = _gpu_classes()
    c = dict(N=3 * B, B=B, D=D, K=K, alpha=0.01, step_size=0.05, burnin=1, epochs=3, data_seed=51, rng_seed=4)
    post_r, logp_r, log_r = _run_variant_oracle(c)
    X, Y = gi.dataset(c["data_seed"], c["N"], c["D"], c["K"])
    s = sgld(softmax({"alpha": c["alpha"]}, dtype=torch.float64, device="cuda:0"),
             {"weights": np.zeros((D, K)), "bias": np.zeros(K)}, step_size=c["step_size"], verbose=True,
             variant="gpu")
    s.out = io.StringIO()
    post_g, logp_g = s.sample(epochs=c["epochs"], burnin=c["burnin"], batch_size=B,
                              rng=np.random.RandomState(c["rng_seed"]), X_train=X, y_train=Y)
    for v in ("weights", "bias"):
        np.testing.assert_allclose(post_g[v], post_r[v], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(logp_g, logp_r, rtol=1e-10)
    assert [l for l in s.out.getvalue().splitlines() if "loss" in l] == \
        [l for l in log_r.splitlines() if "loss" in l]
    # the variant differs from the CPU update (the momentum carries)
    post_c, _, _, _ = _run_oracle(dict(c, kind="sgld", path_length=1.0, np_seed=0))
    assert not np.allclose(post_c["weights"], post_r["weights"], rtol=1e-6)


def test_sgld_gpu_variant_step_api():
    """step(state, momentum, rng) of variant='gpu' returns (q, p) and threads p through."""
    softmax, _, sgld = _gpu_classes()
    D, K, B = 20, 4, 30
    X, Y = gi.dataset(3, B, D, K)
    start = {"weights": np.zeros((D, K)), "bias": np.zeros(K)}
    o = osm.sgld_gpu_variant(om.softmax({"alpha": 0.1}), start, step_size=0.1)
    g = sgld(softmax({"alpha": 0.1}, dtype=torch.float64, device="cuda:0"), start, step_size=0.1, variant="gpu")
    r1, r2 = np.random.RandomState(7), np.random.RandomState(7)
    qo, po = start, {v: np.zeros_like(start[v]) for v in start}
    qg, pg = start, None
    for _ in range(3):
        qo, po = o.step(qo, po, r1, X_train=X, y_train=Y)
        qg, pg = g.step(qg, pg, r2, X_train=X, y_train=Y)
    for v in start:
        np.testing.assert_allclose(qg[v].cpu().numpy(), qo[v], rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(pg[v].cpu().numpy(), po[v], rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("name", ["sghmc_hot", "sghmc_mnist"])
def test_persistent_small_shapes_finish_without_recovery(name, capfd):
    """The persistent kernel finishes every call itself (no timed-out hand-off and kernel-per-phase
    re-run) on shapes where some row-team member owns no rows (sghmc_hot: B = 40, plan 2x2, row team 1
    holds 8 of its 32 rows).  Round 3's kernel chose round B's protocol per member there and one member
    waited out the 4 s timeout; the recovery hid it behind a correct result."""
    c = gi.TRAJ_CONFIGS[name]
    post_r, _, tr_r, _ = _run_oracle(c)
    post_g, _, tr_g, _ = _run_gpu(c, path=2)
    assert [t["accepted"] for t in tr_g] == [t["accepted"] for t in tr_r]
    np.testing.assert_allclose(post_g["weights"], post_r["weights"], rtol=1e-9, atol=1e-11)
    assert "timed out" not in capfd.readouterr().err


@pytest.mark.parametrize("path", [1, 2])
def test_sghmc_step_api_returns_momentum(path):
    """sghmc.step(state, momentum, rng) returns (q, p, acceptprob) like cpu/sghmc.py:19-39 (A1
    completion): p is the final momentum of an accepted proposal, else the freshly drawn one.  The
    hot config (ε = 0.05) rejects some proposals; both cases must match the oracle's step."""
    softmax, sghmc, _ = _gpu_classes()
    c = gi.TRAJ_CONFIGS["sghmc_hot"]
    X, Y = gi.dataset(c["data_seed"], c["N"], c["D"], c["K"])
    Xb, Yb = X[:c["B"]], Y[:c["B"]]
    start = {"weights": np.zeros((c["D"], c["K"])), "bias": np.zeros(c["K"])}
    o = osm.sghmc(om.softmax({"alpha": c["alpha"]}), start, path_length=c["path_length"], step_size=c["step_size"])
    o.trace = []
    m = softmax({"alpha": c["alpha"]}, dtype=torch.float64, device="cuda:0")
    m.ctx.set_sghmc_path(path)
    try:
        g = sghmc(m, start, path_length=c["path_length"], step_size=c["step_size"])
        r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
        qo, qg = dict(start), dict(start)
        for i in range(8):
            np.random.seed(100 + i)
            qo, po, Ao = o.step(qo, None, r1, X_train=Xb, y_train=Yb)
            np.random.seed(100 + i)
            qg, pg, Ag = g.step(qg, None, r2, X_train=Xb, y_train=Yb)
            assert abs(Ag - Ao) <= 1e-9 * max(1.0, abs(Ao))
            for v in start:
                np.testing.assert_allclose(qg[v].cpu().numpy(), qo[v], rtol=1e-9, atol=1e-12)
                np.testing.assert_allclose(pg[v].cpu().numpy(), po[v], rtol=1e-9, atol=1e-12)
        acc = [t["accepted"] for t in o.trace]
        assert any(acc) and not all(acc), acc            # both branches exercised
    finally:
        m.ctx.set_sghmc_path(0)
