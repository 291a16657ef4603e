"""Random-walk Metropolis on the device (hamiltonian.inference.gpu.metropolis.MH, hmcx_mh_run,
hmcx_mh_mvn_run) against the NumPy restatement tests/_mh_ref.py and the golden files of the reference's
own sampler.

noise='numpy': chain c reproduces the restatement's chain c (RandomState(c), shared global accept
uniforms).  Tolerances: float64 — accept flags and tuned scales equal, A rtol 1e-9 with non-finite entries
equal, draws rtol 1e-9 / atol 1e-12 (GEMM summation order only), logp rtol 1e-10, printed lines equal;
float32 — draws rtol 1e-4 / atol 1e-5 while no accept flips.  Every comparison first asserts on the
reference side that |A − u| > 1e-6 for every finite A, so a seed that puts an accept decision on the edge
shows up as such."""
import ctypes
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import inputs as gi  # noqa: E402
from oracle import models as om  # noqa: E402

import _mh_ref  # noqa: E402

NP_SEED = 0
MVN_HYPER = {"mu": np.zeros(2), "cov": np.array([[1.0, 0.8], [0.8, 1.0]])}


@pytest.fixture(scope="module", autouse=True)
def _no_recoveries():
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    yield
    rec = nat.recoveries_all()
    assert not any(rec.values()), rec


def _MH(*a, **kw):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.metropolis import MH
    s = MH(*a, **kw)
    s.out = io.StringIO()
    return s


def _softmax_g(dtype=torch.float64):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    return softmax({"alpha": 0.01}, dtype=dtype)


def _logistic_g():
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.logistic import logistic
    return logistic({"alpha": 0.25}, dtype=torch.float64)


def _mvn_g():
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mvn_gaussian import mvn_gaussian
    return mvn_gaussian(MVN_HYPER, device="cuda:0")


def _softmax_problem():
    X, Y = gi.dataset(3, 60, 24, 10)
    return X, Y, {"weights": np.zeros((24, 10)), "bias": np.zeros(10)}


def _logistic_problem():
    X, y, _, _ = gi.logistic_inputs(3, 77, 33)
    return X, y, {"weights": np.zeros((33, 1)), "bias": np.zeros(1)}


def _assert_off_edge(rec):
    A, u = np.array(rec.A), np.array(rec.u)
    fin = np.isfinite(A)
    assert np.all(np.abs(A[fin] - u[fin]) > 1e-6), (A, u)


_REF_CACHE = {}


def _reference(key, model_o, X, y, start, C, niter_w, burnin, scale, seq):
    """The restatement's C chains from the seeded global state, computed once per configuration."""
    if key not in _REF_CACHE:
        np.random.seed(NP_SEED)
        entry = np.random.get_state()
        r = _mh_ref.MH(X, y, model_o, start, model_o.hyper, scale=scale, update_sequential=seq)
        post = r.multicore_sample(niter_w * C, burnin, C)
        for rec in r.records:
            _assert_off_edge(rec)
        _REF_CACHE[key] = (entry, r, post)
    return _REF_CACHE[key]


def _compare_numpy_mode(key, model_g, model_o, X, y, start, C, niter_w, burnin, scale, seq, f32=False):
    entry, r, post_r = _reference(key, model_o, X, y, start, C, niter_w, burnin, scale, seq)
    g = _MH(X, y, model_g, start, None, scale=scale, update_sequential=seq)
    ctx = model_g.ctx
    ctx.set_timing(True)
    np.random.set_state(entry)
    post = g.multicore_sample(niter_w * C, burnin, C)
    calls = ctx.get_timing()[1]
    ctx.set_timing(False)
    assert calls == (1 if burnin else 0) + 1                      # one library call per phase
    after = np.random.get_state()
    assert after[0] == entry[0] and np.array_equal(after[1], entry[1]) and after[2:] == entry[2:]
    lines_r = []
    for v in start:
        assert post[v].shape == (C * niter_w, np.asarray(start[v]).size)
    assert g.accepted.shape == (niter_w, C) and len(g.chain_traces) == C
    for c, rec in enumerate(r.records):
        sl = slice(c * niter_w, (c + 1) * niter_w)
        tg = g.chain_traces[c]
        assert len(tg) == burnin + niter_w
        lines_r += rec.lines
        acc_g, acc_r = np.array([t["accepted"] for t in tg]), np.array(rec.accepted)
        A_g, A_r = np.array([t["A"] for t in tg]), np.array(rec.A)
        lp_g, lp_r = np.array([t["logp"] for t in tg]), np.array(rec.logp)
        ok = np.isfinite(A_r) & np.isfinite(A_g) & (A_r != 0)
        print("chain", c, "max rel dA", np.max(np.abs(A_g[ok] - A_r[ok]) / np.abs(A_r[ok]), initial=0.0),
              "flags equal", np.array_equal(acc_g, acc_r))
        if f32:
            # compare while no accept has flipped (a burn-in flip may change the tuned scale)
            same = acc_g == acc_r
            n_ok = len(same) if same.all() else int(np.argmin(same))
            k = max(0, n_ok - burnin)
            for v in start:
                np.testing.assert_allclose(post[v][sl][:k], post_r[v][sl][:k], rtol=1e-4, atol=1e-5)
            continue
        assert np.array_equal(acc_g, acc_r)
        assert np.array_equal(g.accepted[:, c], acc_r[burnin:])
        assert g.scales[c] == rec.scale
        assert [t["site"] for t in tg] == rec.site
        np.testing.assert_allclose(np.array([t["mult"] for t in tg]), np.array(rec.mult), rtol=0, atol=0)
        fin = np.isfinite(A_r)
        assert np.array_equal(np.isfinite(A_g), fin) and np.array_equal(A_g[~fin], A_r[~fin])
        np.testing.assert_allclose(A_g[fin], A_r[fin], rtol=1e-9)
        np.testing.assert_allclose(lp_g, lp_r, rtol=1e-10)
        for v in start:
            np.testing.assert_allclose(post[v][sl], post_r[v][sl], rtol=1e-9, atol=1e-12)
    if not f32:
        assert g.out.getvalue().splitlines() == lines_r
    return g, post


# ---------------------------------------------------------------------- 1-3. softmax
def test_softmax_f64_vs_restatement():
    """7 chains of K = 10 (chain tiles 6 + 1), N = 60 and D = 24 (partial last row / feature blocks),
    8 + 12 steps; three tune branches fire (scales 0.09, 0.1, 0.01)."""
    X, Y, start = _softmax_problem()
    g, _ = _compare_numpy_mode("softmax_seq", _softmax_g(), om.softmax({"alpha": 0.01}), X, Y, start, 7, 12, 8,
                               0.1, True)
    assert sorted(set(np.round(g.scales, 12))) == [0.01, 0.09, 0.1]


def test_softmax_single_site():
    """update_sequential=False: one coordinate per variable and step."""
    X, Y, start = _softmax_problem()
    g, post = _compare_numpy_mode("softmax_site", _softmax_g(), om.softmax({"alpha": 0.01}), X, Y, start, 7, 12, 8,
                                  0.5, False)
    for c in range(7):
        for v in start:
            d = post[v][c * 12:(c + 1) * 12]
            assert np.all(np.sum(d[1:] != d[:-1], axis=1) <= 1)
        assert all(0 <= t["site"][0] < 240 and 0 <= t["site"][1] < 10 for t in g.chain_traces[c])


def test_softmax_f32():
    """float32 chains on the same inputs: draws rtol 1e-4 / atol 1e-5 while no accept flips (the reference
    side's smallest |A − u| is 1.4e-3)."""
    X, Y, start = _softmax_problem()
    _compare_numpy_mode("softmax_seq", _softmax_g(torch.float32), om.softmax({"alpha": 0.01}), X, Y, start, 7, 12,
                        8, 0.1, True, f32=True)


# ---------------------------------------------------------------------- 4. logistic
def test_logistic_f64_vs_restatement():
    """5 chains, N = 77, D = 33: the Σθ² partials of the proposal feed the log prior."""
    X, y, start = _logistic_problem()
    _compare_numpy_mode("logistic", _logistic_g(), om.logistic({"alpha": 0.25}), X, y, start, 5, 12, 8, 0.05, True)


# ---------------------------------------------------------------------- 5. sample() against the golden files
def _golden(golden_dir, fname, group):
    z = np.load(os.path.join(golden_dir, fname))
    return {k[len(group) + 1:]: z[k] for k in z.files if k.startswith(group + "_")}


@pytest.mark.parametrize("name", ["softmax_seq", "softmax_site", "logistic", "mvn_near", "mvn_far"])
def test_sample_vs_golden(golden_dir, name):
    """sample() (C = 1) against what the reference's own MH produced, one library call per phase."""
    if name.startswith("softmax"):
        X, y, start = _softmax_problem()
        model, fname = _softmax_g(), "mh_softmax.npz"
        group, scale, seq, burnin, niter = ("seq", 0.1, True, 8, 12) if name == "softmax_seq" else \
            ("site", 0.5, False, 8, 12)
    elif name == "logistic":
        X, y, start = _logistic_problem()
        model, fname, group, scale, seq, burnin, niter = _logistic_g(), "mh_logistic.npz", "seq", 0.05, True, 8, 12
    else:
        X = y = None
        model, fname, seq = _mvn_g(), "mh_mvn.npz", True
        group, start, scale, burnin, niter = ("near", {"x": np.zeros(2)}, 1.0, 50, 200) if name == "mvn_near" else \
            ("far", {"x": np.array([60.0, -60.0])}, 30.0, 0, 40)
    gd = _golden(golden_dir, fname, group)
    fin = np.isfinite(gd["A"])
    assert np.all(np.abs(gd["A"] - gd["u"])[fin] > 1e-6)
    s = _MH(X, y, model, start, None, scale=scale, update_sequential=seq)
    model.ctx.set_timing(True)
    np.random.seed(0)
    post = s.sample(niter, burnin, np.random.RandomState(0))
    calls = model.ctx.get_timing()[1]
    model.ctx.set_timing(False)
    assert calls == (1 if burnin else 0) + 1
    tg = s.chain_traces[0]
    assert np.array_equal(np.array([t["accepted"] for t in tg]), gd["accepted"])
    A = np.array([t["A"] for t in tg])
    assert np.array_equal(A[~fin], gd["A"][~fin])
    np.testing.assert_allclose(A[fin], gd["A"][fin], rtol=1e-9)
    np.testing.assert_allclose(np.array([t["logp"] for t in tg]), gd["logp"], rtol=1e-10)
    assert s.scale == float(gd["scale"]) and s._scale == s.scale
    assert s.out.getvalue().splitlines() == [str(l) for l in gd["lines"]]
    for v in start:
        assert post[v].shape == gd["post_" + v].shape
        np.testing.assert_allclose(post[v], gd["post_" + v], rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------- 6. MVN, C = 4
@pytest.mark.parametrize("row", ["near", "far"])
def test_mvn_vs_restatement(row):
    """Both golden configurations with 4 chains; the far start pins inf → reject."""
    start, scale, burnin, niter = ({"x": np.zeros(2)}, 1.0, 50, 200) if row == "near" else \
        ({"x": np.array([60.0, -60.0])}, 30.0, 0, 40)
    g, _ = _compare_numpy_mode("mvn_" + row, _mvn_g(), om.mvn_gaussian(MVN_HYPER), None, None, start, 4, niter,
                               burnin, scale, True)
    if row == "far":
        r = _REF_CACHE["mvn_far"][1]
        for c in range(4):
            A_r = np.array(r.records[c].A)
            A_g = np.array([t["A"] for t in g.chain_traces[c]])
            inf = np.isposinf(A_r)
            assert 11 <= inf.sum() <= 23
            assert np.array_equal(np.isposinf(A_g), inf)
            assert not np.array([t["accepted"] for t in g.chain_traces[c]])[inf].any()


# ---------------------------------------------------------------------- 7. direct hmcx_mh_run, BUFFER mode
def _direct_call(nat, model, X, Y, W0, b0, mult, site, u, z, want_E=True):
    """W0 [C, D, K], b0 [C, K] per-chain starting states; returns A, acc, logp, E, trace, W, b (host)."""
    C, D, K = W0.shape
    n = u.shape[0]
    P = D * K + K
    dev = model.device
    Xd, Yd = model._xy({"X_train": X, "y_train": Y})
    W = torch.as_tensor(np.ascontiguousarray(W0.transpose(1, 0, 2).reshape(D, C * K))).to(dev)
    b = torch.as_tensor(np.ascontiguousarray(b0.reshape(C * K))).to(dev)
    zd = torch.as_tensor(np.ascontiguousarray(z.reshape(-1))).to(dev)
    noff = np.arange(n * C, dtype=np.int64) * P
    out_A = torch.empty(n * C, dtype=torch.float64, device=dev)
    out_lp = torch.empty(n * C, dtype=torch.float64, device=dev)
    out_E = torch.empty(n * C * 2, dtype=torch.float64, device=dev)
    out_acc = torch.empty(n * C, dtype=torch.int32, device=dev)
    tr = torch.empty((n, C, P), dtype=torch.float64, device=dev)
    mult = np.ascontiguousarray(mult, dtype=np.float64)
    site = np.ascontiguousarray(site, dtype=np.int32)
    u = np.ascontiguousarray(u, dtype=np.float64)
    a = nat.MhArgs()
    a.dtype, a.model = nat.HMCX_F64, nat.MODEL_SOFTMAX
    a.B, a.D, a.K, a.C, a.n_steps = X.shape[0], D, K, C, n
    a.alpha = model.alpha
    a.log_prior = model.log_prior_const([(D, K), (K,)])
    a.X, a.Y = nat.ptr(Xd.contiguous()), nat.ptr(Yd.contiguous())
    a.mult, a.site = mult.ctypes.data_as(nat.c_dblp), site.ctypes.data_as(nat.c_i32p)
    a.u_accept = u.ctypes.data_as(nat.c_dblp)
    a.noise_mode, a.noise, a.noise_off = nat.NOISE_BUFFER, nat.ptr(zd), noff.ctypes.data_as(nat.c_i64p)
    a.W, a.b = nat.ptr(W), nat.ptr(b)
    a.out_A, a.out_accepted, a.out_logp = nat.ptr(out_A), nat.ptr(out_acc), nat.ptr(out_lp)
    a.out_E = nat.ptr(out_E) if want_E else None
    a.out_trace = nat.ptr(tr)
    ctx = nat.context(dev)
    ctx.check(ctx.lib.hmcx_mh_run(ctx.h, a), "hmcx_mh_run")
    return (out_A.cpu().numpy().reshape(n, C), out_acc.cpu().numpy().astype(bool).reshape(n, C),
            out_lp.cpu().numpy().reshape(n, C), out_E.cpu().numpy().reshape(n, C, 2), tr.cpu().numpy(),
            W.cpu().numpy().reshape(D, C, K).transpose(1, 0, 2), b.cpu().numpy().reshape(C, K))


def test_direct_call_buffer_mode():
    """hmcx_mh_run with distinct starting states per chain (3 chains, N = 37, D = 19, K = 4), five steps:
    ordinary, every chain rejects (u = 1 against a far proposal, A = 0), every chain accepts (u = 0, tiny
    proposal, finite A), a single-site step, and a last ordinary one.  Trace rows, final W / b, out_E, A,
    flags and logp against a NumPy evaluation with the oracle model."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    model = _softmax_g()
    mo = om.softmax({"alpha": 0.01})
    N, D, K, C, n = 37, 19, 4, 3, 5
    X, Y = gi.dataset(5, N, D, K)
    rs = np.random.RandomState(17)
    W0, b0 = rs.normal(0, 0.3, (C, D, K)), rs.normal(0, 0.3, (C, K))
    P = D * K + K
    z = rs.normal(0, 1, (n, C, P))
    mult = np.exp(rs.uniform(-1.5, 1.5, (n, C, 2))) * 0.05
    mult[1] = 40.0
    mult[2] = 1e-4
    site = np.full((n, C, 2), -1, dtype=np.int32)
    site[3, :, 0] = [0, D * K - 1, 31]
    site[3, :, 1] = [K - 1, 0, 2]
    u = rs.rand(n, C)
    u[1], u[2] = 1.0, 0.0
    lpc = mo.log_prior({"weights": W0[0], "bias": b0[0]})
    q = [np.concatenate([W0[c].reshape(-1), b0[c]]) for c in range(C)]
    exp_tr = np.empty((n, C, P)); exp_A = np.empty((n, C)); exp_acc = np.empty((n, C), dtype=bool)
    exp_E = np.empty((n, C, 2)); exp_lp = np.empty((n, C))

    def logp(flat):
        return mo.log_likelihood({"weights": flat[:D * K].reshape(D, K), "bias": flat[D * K:]}, X_train=X,
                                 y_train=Y) + lpc

    for s in range(n):
        for c in range(C):
            qn = q[c].copy()
            for k, (o, dim) in enumerate(((0, D * K), (D * K, K))):
                if site[s, c, k] < 0:
                    qn[o:o + dim] += mult[s, c, k] * z[s, c, o:o + dim]
                else:
                    qn[o + site[s, c, k]] += mult[s, c, k] * z[s, c, o + site[s, c, k]]
            E, En = -logp(q[c]), -logp(qn)
            with np.errstate(over="ignore"):
                A = np.exp(E - En)
            acc = bool(np.isfinite(A) and u[s, c] < A)
            assert not np.isfinite(A) or abs(A - u[s, c]) > 1e-6
            exp_A[s, c], exp_acc[s, c], exp_E[s, c] = A, acc, (E, En)
            if acc:
                q[c] = qn
            exp_lp[s, c] = -(En if acc else E)
            exp_tr[s, c] = q[c]
    assert not exp_acc[1].any() and exp_acc[2].all() and np.all(np.isfinite(exp_A[2]))
    A, acc, lp, E, tr, W, b = _direct_call(nat, model, X, Y, W0, b0, mult, site, u, z)
    assert np.array_equal(acc, exp_acc)
    np.testing.assert_allclose(A, exp_A, rtol=1e-9, atol=1e-300)
    np.testing.assert_allclose(E, exp_E, rtol=1e-10)
    np.testing.assert_allclose(lp, exp_lp, rtol=1e-10)
    np.testing.assert_allclose(tr, exp_tr, rtol=1e-9, atol=1e-12)
    for c in range(C):
        np.testing.assert_allclose(W[c].reshape(-1), q[c][:D * K], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(b[c], q[c][D * K:], rtol=1e-9, atol=1e-12)
        np.testing.assert_array_equal(tr[-1, c], np.concatenate([W[c].reshape(-1), b[c]]))
    # the same call without out_E
    A2, acc2, _, _, tr2, _, _ = _direct_call(nat, model, X, Y, W0, b0, mult, site, u, z, want_E=False)
    assert np.array_equal(A2, A) and np.array_equal(acc2, acc) and np.array_equal(tr2, tr)


def test_validation_errors():
    """A bad model, C < 1 and an out-of-range site return HMCX_EINVAL with a message, before any launch."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    ctx = nat.context()
    a = nat.MhArgs()
    a.dtype, a.model, a.B, a.D, a.K, a.C, a.n_steps = nat.HMCX_F64, 7, 4, 3, 2, 1, 1
    assert ctx.lib.hmcx_mh_run(ctx.h, ctypes.byref(a)) == -1 and b"model" in ctx.lib.hmcx_last_error(ctx.h)
    a.model, a.C = nat.MODEL_SOFTMAX, 0
    assert ctx.lib.hmcx_mh_run(ctx.h, ctypes.byref(a)) == -1 and ctx.lib.hmcx_last_error(ctx.h)
    a.model, a.C, a.K = nat.MODEL_LOGISTIC, 1, 2
    assert ctx.lib.hmcx_mh_run(ctx.h, ctypes.byref(a)) == -1 and b"K = 1" in ctx.lib.hmcx_last_error(ctx.h)
    m = nat.MhMvnArgs()
    m.dim, m.C, m.n_steps = 2, 0, 1
    assert ctx.lib.hmcx_mh_mvn_run(ctx.h, ctypes.byref(m)) == -1 and ctx.lib.hmcx_last_error(ctx.h)


# ---------------------------------------------------------------------- 8. Philox mode
def test_philox_chains_equal_single_chain_calls():
    """A C = 6 call equals six C = 1 calls with chain = c: softmax rtol 1e-9 (chain tiling changes the GEMM
    summation order only), MVN bit-equal."""
    X, Y, start = _softmax_problem()
    model = _softmax_g()
    C, niter_w, burnin = 6, 6, 4
    g = _MH(X, Y, model, start, None, scale=0.1, noise="philox", seed=5, chain=2)
    post = g.multicore_sample(niter_w * C, burnin, C)
    for c in range(C):
        s = _MH(X, Y, model, start, None, scale=0.1, noise="philox", seed=5, chain=2 + c)
        p1 = s.sample(niter_w, burnin)
        assert [t["accepted"] for t in s.chain_traces[0]] == [t["accepted"] for t in g.chain_traces[c]]
        assert [t["mult"] for t in s.chain_traces[0]] == [t["mult"] for t in g.chain_traces[c]]
        assert s.scale == g.scales[c]
        for v in start:
            np.testing.assert_allclose(post[v][c * niter_w:(c + 1) * niter_w], p1[v], rtol=1e-9, atol=1e-12)
    mvn = _mvn_g()
    g = _MH(None, None, mvn, {"x": np.zeros(2)}, None, scale=1.0, noise="philox", seed=9, update_sequential=False)
    post = g.multicore_sample(40 * C, 10, C)
    for c in range(C):
        s = _MH(None, None, mvn, {"x": np.zeros(2)}, None, scale=1.0, noise="philox", seed=9, chain=c,
                update_sequential=False)
        p1 = s.sample(40, 10)
        np.testing.assert_array_equal(post["x"][c * 40:(c + 1) * 40], p1["x"])
        assert [t["A"] for t in s.chain_traces[0]] == [t["A"] for t in g.chain_traces[c]]


# ---------------------------------------------------------------------- 9. law
def test_mvn_law_vs_restatement_ensemble():
    """64 device Philox chains (100 + 400 steps) against a restatement ensemble of the same size with a
    disjoint seed: tests/_stats.compare then assert_same_moments (tests/test_mh_cpu.py shows two
    restatement ensembles passing the same criterion at these sizes)."""
    import _stats
    C, T = 64, 400
    g = _MH(None, None, _mvn_g(), {"x": np.zeros(2)}, None, scale=1.0, verbose=False, noise="philox", seed=303)
    post = g.multicore_sample(C * T, 100, C)
    a = post["x"].reshape(C, T, 2)
    b = _mh_ref.mvn_ensemble(seed=101, C=C, burnin=100, niter=T)
    z = _stats.compare(a, b)
    print(_stats.summary(z))
    _stats.assert_same_moments(z)


# ---------------------------------------------------------------------- 10. diagnostics
def test_chain_diagnostics_equal_host():
    from dropout_hamiltonian_montecarlo_amd import diagnostics
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    C, T = 16, 120
    g = _MH(None, None, _mvn_g(), {"x": np.zeros(2)}, None, scale=1.0, verbose=False, noise="philox", seed=77)
    with pytest.raises(HmcxError):
        g.chain_diagnostics()
    post = g.multicore_sample(C * T, 20, C)
    x = post["x"].reshape(C, T, 2)
    srhat, ess = g.chain_diagnostics()
    np.testing.assert_allclose(srhat, diagnostics.split_rhat(x), rtol=1e-9)
    np.testing.assert_allclose(ess, diagnostics.ess(x), rtol=1e-9)
    X, Y, start = _softmax_problem()
    s = _MH(X, Y, _softmax_g(), start, None, scale=0.05, verbose=False, noise="philox", seed=3)
    post = s.multicore_sample(4 * 8, 2, 4)
    flat = np.concatenate([post["weights"], post["bias"]], axis=1).reshape(4, 8, 250)
    srhat, ess = s.chain_diagnostics()
    np.testing.assert_allclose(srhat, diagnostics.split_rhat(flat), rtol=1e-9)
    np.testing.assert_allclose(ess, diagnostics.ess(flat), rtol=1e-9)
