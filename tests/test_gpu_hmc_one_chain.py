"""The one-chain full-batch HMC entry points are the C = 1 case of the chain-batched ones.

A. hmcx_hmc_run against hmcx_hmc_chains_run with C = 1 through ctypes on identical inputs: every output
   and the final state bit for bit, at the smallest shapes that reach each path of the GEMM kernels, in
   BUFFER and PHILOX noise mode, with and without the optional outputs.
B. hmc.sample with rng = the global np.random stream itself (a case the reference supports) against the
   NumPy oracle run the same way: the draws interleave per step (momentum, path length, accept uniform).
   Tolerances are those of tests/test_gpu_hmc.py: path lengths and accept flags equal, states
   rtol 1e-9 / atol 1e-12, losses rtol 1e-10, momenta equal.
C. hmc.sample on the MVN model (noise='philox') against chain 0 of sample_multicore with C = 3: equal.
"""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import inputs as gi  # noqa: E402
from oracle import models as om  # noqa: E402
from oracle import samplers as osm  # noqa: E402

# ---------------------------------------------------------------------- A. hmcx_hmc_run = chains run, C = 1
S = 5
N_ITER = np.array([0, 2, 1, 0, 3], dtype=np.int32)      # an unmoved first step exercises the carried state
U = np.array([0.5, 0.0, 1.0, 0.5, 1.0])                 # acc = u < A, A ≤ 1: u = 0 accepts, u = 1 rejects
EPS = 1e-2
SENTINEL = -7.0

# (model, dtype, N, D, K): partial 16-row and 16-feature blocks with vector loads (D % 4 = 0) and scalar
# loads (D = 19); float32 at K = 10; logistic (K = 1) in both precisions
SHAPES = [("softmax", "f64", 33, 20, 3), ("softmax", "f64", 33, 19, 3), ("softmax", "f32", 60, 24, 10),
          ("logistic", "f64", 33, 5, 1), ("logistic", "f32", 33, 5, 1)]


def _inputs(model, dt, N, D, K):
    if model == "softmax":
        X, Y = gi.dataset(3, N, D, K)
    else:
        X, Y, _, _ = gi.logistic_inputs(11, N, D)
    rs = np.random.RandomState(77)
    W0 = rs.normal(0, 0.05, (D, K))
    b0 = rs.normal(0, 0.05, K)
    noise = rs.normal(0, 1, (S, D * K + K))
    npdt = np.float64 if dt == "f64" else np.float32
    return X.astype(npdt), Y.astype(npdt), W0.astype(npdt), b0.astype(npdt), noise


def _run(entry, model, dt, N, D, K, philox, full):
    """One call of `entry` ('run': hmcx_hmc_run, 'chains': hmcx_hmc_chains_run with C = 1) on the inputs
    of _inputs; every output buffer starts at SENTINEL."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    ptr = nat.ptr
    dev = torch.device("cuda:0")
    ctx = nat.context(dev)
    Xh, Yh, W0, b0, noise = _inputs(model, dt, N, D, K)
    tdt = torch.float64 if dt == "f64" else torch.float32
    P = D * K + K
    X, Y = torch.as_tensor(Xh).to(dev), torch.as_tensor(Yh).to(dev)
    W, b = torch.as_tensor(W0).to(dev), torch.as_tensor(b0).to(dev)
    noise_d = torch.as_tensor(noise.reshape(-1)).to(dev)
    noff = (np.arange(S, dtype=np.int64)[::-1] * P).copy()          # not in step order
    eps = np.full(S, EPS)
    out = dict(A=torch.full((S,), SENTINEL, dtype=torch.float64, device=dev),
               acc=torch.full((S,), int(SENTINEL), dtype=torch.int32, device=dev),
               nlp=torch.full((S,), SENTINEL, dtype=torch.float64, device=dev))
    if full:
        out.update(E=torch.full((S, 2), SENTINEL, dtype=torch.float64, device=dev),
                   trace=torch.full((S, P), SENTINEL, dtype=tdt, device=dev),
                   mom=torch.full((S, P), SENTINEL, dtype=tdt, device=dev))
    a = nat.HmcArgs() if entry == "run" else nat.HmcChainsArgs()
    a.dtype = nat.HMCX_F64 if dt == "f64" else nat.HMCX_F32
    a.model = nat.MODEL_LOGISTIC if model == "logistic" else nat.MODEL_SOFTMAX
    a.B, a.D, a.K, a.n_steps = N, D, K, S
    a.alpha, a.log_prior = (0.25, 0.0) if model == "logistic" else (0.01, -1.234)
    a.lp_const[0], a.lp_const[1] = -0.7, -0.2
    a.X, a.Y = ptr(X), ptr(Y)
    a.eps, a.n_iter, a.u_accept = eps.ctypes.data_as(nat.c_dblp), N_ITER.ctypes.data_as(nat.c_i32p), \
        U.ctypes.data_as(nat.c_dblp)
    if philox:
        a.noise_mode, a.seed, a.step_base = nat.NOISE_PHILOX, 11, 5
    else:
        a.noise_mode, a.noise, a.noise_off = nat.NOISE_BUFFER, ptr(noise_d), noff.ctypes.data_as(nat.c_i64p)
    if entry == "run":
        a.chain = 3
        fn = ctx.lib.hmcx_hmc_run
    else:
        a.C, a.chain0 = 1, 3
        fn = ctx.lib.hmcx_hmc_chains_run
    a.W, a.b = ptr(W), ptr(b)
    a.out_A, a.out_accepted, a.out_nlp = ptr(out["A"]), ptr(out["acc"]), ptr(out["nlp"])
    a.out_E, a.out_trace, a.out_mom = ptr(out.get("E")), ptr(out.get("trace")), ptr(out.get("mom"))
    ctx.check(fn(ctx.h, a), entry)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(W=W.cpu().numpy(), b=b.cpu().numpy())
    return res, W0, b0, noise, noff


@pytest.mark.parametrize("full", [True, False], ids=["outputs", "null-outputs"])
@pytest.mark.parametrize("philox", [False, True], ids=["buffer", "philox"])
@pytest.mark.parametrize("model,dt,N,D,K", SHAPES, ids=["%s-%s-N%d-D%d-K%d" % s for s in SHAPES])
def test_one_chain_run_is_chains_run_c1(model, dt, N, D, K, philox, full):
    one, W0, b0, noise, noff = _run("run", model, dt, N, D, K, philox, full)
    ch, _, _, _, _ = _run("chains", model, dt, N, D, K, philox, full)
    assert set(one) == set(ch)
    for k in one:
        np.testing.assert_array_equal(one[k], ch[k], err_msg=k)
    # every element was written, and the schedule did what it is meant to exercise
    for k in one:
        assert not np.any(one[k] == SENTINEL), k
    moved = N_ITER > 0
    acc = one["acc"].astype(bool)
    assert acc[moved].any() and not acc[moved].all()              # an accepted and a rejected moved step
    assert np.all(one["A"][~moved] == 1.0) and np.all(acc[~moved])
    assert not np.array_equal(one["W"], W0)                       # the accepted step moved the state
    if full:
        P = D * K + K
        np.testing.assert_array_equal(one["trace"][-1], np.concatenate([one["W"].reshape(-1), one["b"]]))
        np.testing.assert_array_equal(one["trace"][0], np.concatenate([W0.reshape(-1), b0]))   # n_iter = 0
        assert np.all(np.isfinite(one["E"]))
        if not philox:                                            # step s read its own noise row
            exp = np.stack([noise.reshape(-1)[o:o + P] for o in noff]).astype(one["mom"].dtype)
            np.testing.assert_array_equal(one["mom"], exp)


# ---------------------------------------------------------------------- B. aliased stream
NP_SEED = 9


def test_sample_with_the_global_stream_as_rng(monkeypatch):
    """rng = np.random.mtrand._rand: per step the momentum (weights, bias), the path length and the
    accept uniform come from one stream, in that order, after the discarded first momentum."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc import hmc
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    N, D, K = 33, 20, 3
    X, Y = gi.dataset(3, N, D, K)
    start = {"weights": np.zeros((D, K)), "bias": np.zeros(K)}
    kw = dict(path_length=0.05, step_size=1e-2)
    o = osm.hmc(om.softmax({"alpha": 0.01}), start, verbose=True, **kw)
    o.trace, o.out = [], io.StringIO()
    drawn = []
    rand = np.random.rand
    with monkeypatch.context() as mp:
        mp.setattr(np.random, "rand", lambda: drawn.append(rand()) or drawn[-1])
        np.random.seed(NP_SEED)
        po, lo, pos_o, mom_o = o.sample(6, 2, np.random.mtrand._rand, X_train=X, y_train=Y)
    u = np.array(drawn[1::2])                                     # hmc.py:46 then :61 per step
    A = np.array([t["A"] for t in o.trace])
    assert len(u) == 8 and np.all(np.abs(A - u) > 1e-6), (A, u)   # no accept decision on the edge
    assert [t["L"] for t in o.trace] == [6, 10, 10, 9, 1, 5, 1, 3]
    g = hmc(softmax({"alpha": 0.01}, dtype=torch.float64), start, verbose=True, **kw)
    g.trace, g.out = [], io.StringIO()
    np.random.seed(NP_SEED)
    pg, lg, pos_g, mom_g = g.sample(6, 2, np.random.mtrand._rand, X_train=X, y_train=Y)
    assert [t["L"] for t in g.trace] == [t["L"] for t in o.trace]
    assert [t["accepted"] for t in g.trace] == [t["accepted"] for t in o.trace]
    for v in start:
        np.testing.assert_allclose(pg[v], po[v], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(lg, lo, rtol=1e-10)
    assert len(mom_g) == len(mom_o) == 6
    for i in range(6):
        for v in start:
            np.testing.assert_array_equal(mom_g[i][0][v], mom_o[i][0][v])
            np.testing.assert_allclose(pos_g[i][0][v], pos_o[i][0][v], rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------- C. MVN route, C = 1 against C = 3
def test_mvn_sample_is_chain0_of_sample_multicore():
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc import hmc
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc_multicore import hmc_multicore
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mvn_gaussian import mvn_gaussian
    c = gi.MVN_CONFIG
    m = mvn_gaussian({"mu": np.array(c["mu"]), "cov": np.array(c["cov"])}, device="cuda:0")
    kw = dict(path_length=c["path_length"], step_size=c["step_size"], noise="philox", seed=2024)
    C, T = 3, 10
    h = hmc(m, {"x": np.zeros(2)}, **kw)
    h.trace, h.out = [], io.StringIO()
    p1, l1, pos1, m1 = h.sample(T, 2)
    s = hmc_multicore(m, {"x": np.zeros(2)}, **kw)
    s.trace, s.out = [], io.StringIO()
    post, pos, mom, logp = s.sample_multicore(T * C, 2, C)
    assert p1["x"].shape == (T, 2) and l1.shape == (T,) and len(m1) == T and len(h.trace) == 2 + T
    np.testing.assert_array_equal(p1["x"], post["x"][:T])
    np.testing.assert_array_equal(l1, logp[:T])
    for i in range(T):
        np.testing.assert_array_equal(m1[i][0]["x"], mom[0][i][0]["x"])
        np.testing.assert_array_equal(pos1[i][0]["x"], pos[0][i][0]["x"])
    assert [t["accepted"] for t in h.trace] == [t["accepted"] for t in s.chain_traces[0]]
    assert not np.array_equal(post["x"][:T], post["x"][T:2 * T])     # the chains differ
