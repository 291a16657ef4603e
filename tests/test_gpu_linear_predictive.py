"""GPU tests of the linear models' posterior predictive (hmcx_linear_predictive, hmcx_lin_pred.hip) against
the float64 reference tests/_linear_predictive_ref.py (oracle.models.softmax.net / logistic.net + NumPy), on
the general path (path 1) and the fused row-block kernel (path 2), for the softmax and logistic models.

Tolerances are those of tests/test_gpu_mlp_predictive.py.  float64 `mean` and `draw_nll`: rtol 1e-11, atol
1e-14 (summation order only); the entropies and lppd, each a sum of K terms of such quantities: rtol 1e-10,
atol 1e-12.  float32 against the reference at float32-rounded inputs: 2e-4 of the largest reference entry
(one GEMM here where the MLP has three, so its bound carries over).  `pred` and `draw_correct` exact: the
cases' seeds keep every reference decision's gap above 1e-6 (float64) / 1e-3 (float32), asserted on the
reference alone in test_linear_predictive_cpu.py.

Besides the shared cases, LAUNCH_CASES (every launch branch of lin_predictive_t, see the inventory in the
reference module) run on both paths in the mode their branch needs, the two paths are held to each other in
float64, and SAT_CASES put logits beyond the clip and, in float32, where a float32 sigmoid rounds to 1.

The float32 test compares mean, entropy, expected_entropy, lppd and draw_nll and prints err / bound for each.
Measured on an MI355X over all cases, paths and modes (the saturated ones included), largest err / bound:
mean 1.3e-3, entropy 6.5e-4, expected_entropy 6.2e-4 (softmax 33x24x38x2x2, path 1, no dropout), lppd 8.9e-4 and
draw_nll 8.9e-4 (softmax 1x1x2x1x1); saturated logistic draw_nll 2.1e-4.  A logit error of about 1e-5 enters nll
linearly, and a bound of 2e-4 · max |reference| is 1e-4 or more here.  Before the general path took the float32
sigmoid from the clipped logit, test_saturated_logits[logistic-*-1-f32] failed with draw_nll NaN in 10 of 12
draws and inf in 2 (dropout), NaN in 6 of 6 (no dropout); everything else passed on that library too."""
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _linear_predictive_ref as lr  # noqa: E402
from oracle import inputs as gi, models as om  # noqa: E402

FUSED = [c for c in lr.CASES if lr.eligible(c)]
INELIGIBLE = [c for c in lr.CASES if not lr.eligible(c)] + [lr.LDS_EDGE]
# every (case, path) that exists: the general path everywhere, the fused one where the shape is eligible
CASE_PATHS = [(c, 1) for c in lr.CASES] + [(c, 2) for c in FUSED]
MODELS = ['softmax', 'logistic']
# the shared cases with and without dropout, the launch cases in the mode their branch needs
RUNS = [(c, p, d) for c, p in CASE_PATHS for d in (True, False)] + \
       [(c, p, c.dropout) for c in lr.LAUNCH_CASES for p in ((1, 2) if lr.eligible(c) else (1,))]
RUN_IDS = ["%s-path%d-%s" % (lr.case_id(c), p, "fixed" if d else "off") for c, p, d in RUNS]


def _model(kind, dtype=None):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.logistic import logistic
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    cls = logistic if kind == 'logistic' else softmax
    return cls({"alpha": 0.01}, dtype=dtype or torch.float64, device="cuda:0")


def _run_pb(kind, pb, T, path, dropout=True, dtype=None, y=True, **kw):
    if dropout:
        kw = dict(n_dropout=T, Z=pb.masks, **kw)
    return _model(kind, dtype).posterior_predictive(lr.posterior(pb), pb.X, y=pb.y if y else None, path=path, **kw)


def _run(c, path, dropout=True, dtype=None, rounded=False, y=True, **kw):
    return _run_pb(c.model, lr.problem(c, rounded), c.shape[4], path, dropout, dtype, y, **kw)


def _check64(r, ref):
    np.testing.assert_allclose(r.mean, ref.mean, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(r.draw_nll, ref.draw_nll, rtol=1e-11, atol=1e-14)
    for name in ("entropy", "expected_entropy", "lppd"):
        np.testing.assert_allclose(getattr(r, name), getattr(ref, name), rtol=1e-10, atol=1e-12, err_msg=name)
    np.testing.assert_allclose(r.mutual_information, r.entropy - r.expected_entropy, rtol=0, atol=0)
    np.testing.assert_allclose(r.mutual_information, ref.mutual_information, rtol=0, atol=1e-10)
    np.testing.assert_array_equal(r.pred, ref.pred)
    np.testing.assert_array_equal(r.draw_accuracy, ref.draw_accuracy)


def _same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


F32_QUANTITIES = ("mean", "entropy", "expected_entropy", "lppd", "draw_nll")


def _check32(r, ref, label):
    """2e-4 of the largest reference entry for every real-valued quantity; each err / bound is printed."""
    worst = {}
    for name in F32_QUANTITIES:
        got, want = getattr(r, name), getattr(ref, name)
        assert got.dtype == np.float64
        assert np.all(np.isfinite(got)), "%s: %d entries not finite, e.g. %r" % (
            name, int((~np.isfinite(got)).sum()), got[~np.isfinite(got)][:4])
        err, bound = np.abs(got - want).max(), 2e-4 * np.abs(want).max()
        worst[name] = err / bound
        print("f32 %s %s: max abs err %.3e, bound %.3e, err/bound %.3g" % (label, name, err, bound, err / bound))
    for name in F32_QUANTITIES:
        assert worst[name] <= 1.0, "%s: err / bound %.3g" % (name, worst[name])
    np.testing.assert_array_equal(r.pred, ref.pred)
    np.testing.assert_array_equal(r.draw_accuracy, ref.draw_accuracy)


@pytest.mark.parametrize("c,path,dropout", RUNS, ids=RUN_IDS)
def test_f64_matches_reference(c, path, dropout):
    _check64(_run(c, path, dropout), lr.case_ref(c, dropout))


@pytest.mark.parametrize("c,path,dropout", RUNS, ids=RUN_IDS)
def test_f32_close_to_reference_at_rounded_inputs(c, path, dropout, request):
    r, ref = _run(c, path, dropout, torch.float32, True), lr.case_ref(c, dropout, True)
    _check32(r, ref, request.node.callspec.id)


@pytest.mark.parametrize("c", lr.LAUNCH_CASES, ids=lr.case_id)
def test_paths_agree_on_launch_cases(c):
    """The general path and the fused kernel against each other, float64, at the reference's tolerances."""
    _check64(_run(c, 2, c.dropout), _run(c, 1, c.dropout))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("dropout", [True, False], ids=["fixed", "off"])
@pytest.mark.parametrize("kind", MODELS)
def test_saturated_logits(kind, dropout, path, dtype, request):
    """Logits in the bands of tests/_linear_predictive_ref.py (ordinary, beyond the clip on both sides and, in
    float32, where a float32 sigmoid rounds to 1): every output finite and within the tolerances above."""
    f32 = dtype == torch.float32
    c = lr.sat_case(kind, f32)
    r = _run_pb(kind, lr.sat_problem(c, f32), c.shape[4], path, dropout, dtype)
    ref = lr.sat_ref(c, dropout, f32)
    for name in F32_QUANTITIES + ("mutual_information", "draw_accuracy"):
        got = getattr(r, name)
        assert np.all(np.isfinite(got)), "%s: %d entries not finite, e.g. %r" % (
            name, int((~np.isfinite(got)).sum()), got[~np.isfinite(got)][:4])
    if f32:
        _check32(r, ref, request.node.callspec.id)
        np.testing.assert_allclose(r.mutual_information, r.entropy - r.expected_entropy, rtol=0, atol=0)
    else:
        _check64(r, ref)


def test_single_draw_is_predict():
    """S = T = 1 without masks reproduces predict(prob=True), on both paths and both models."""
    for kind in MODELS:
        c = lr.MULTIBLOCK[kind]
        pb, N = lr.problem(c), c.shape[0]
        m = _model(kind)
        par = {'weights': pb.W[0], 'bias': pb.b[0]}
        want = m.predict(par, pb.X, prob=True, **({'batchsize': N} if kind == 'logistic' else {}))
        for path in (1, 2):
            r = m.posterior_predictive(par, pb.X, path=path)
            np.testing.assert_allclose(r.mean.reshape(want.shape), want, rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("kind", MODELS)
def test_philox_equals_injected_api_masks(kind, path, dtype):
    """PHILOX draw d uses the values hmcx_input_masks writes for step d (global element index, whatever the
    kernel's row tiling): injecting those masks gives the same bits."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import input_masks
    c = lr.MULTIBLOCK[kind]
    N, D, _, S, T = c.shape
    pb = lr.problem(c)
    m = _model(kind, dtype)
    r_philox = m.posterior_predictive(lr.posterior(pb), pb.X, y=pb.y, n_dropout=T, p=0.7, seed=11, path=path)
    Z = torch.stack([input_masks("cuda:0", N, D, 0.7, 11, d) for d in range(S * T)])
    assert Z.dtype == torch.uint8 and 0.6 < float(Z.double().mean()) < 0.8
    r_fixed = m.posterior_predictive(lr.posterior(pb), pb.X, y=pb.y, n_dropout=T, Z=Z, path=path)
    _same(r_philox, r_fixed)
    other = m.posterior_predictive(lr.posterior(pb), pb.X, y=pb.y, n_dropout=T, p=0.7, seed=12, path=path)
    assert np.abs(other.mean - r_philox.mean).max() > 1e-6


def test_input_masks_are_the_sgd_dropout_stream():
    """hmcx_input_masks is the draw k_xdrop makes for sgd.fit_dropout (hmcx_sgd_run, PHILOX): element i of the
    mask of (seed, step) is philox_uniform(seed, 0, step, 0xFFFFFFFC, i) < p.  The host hmcx_philox_uniforms
    indexes elements the same way (0 … n − 1 of one slot), so it is compared through it."""
    from dropout_hamiltonian_montecarlo_amd._native import philox_uniforms
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import input_masks
    N, D, p = 37, 29, 0.3
    for seed, step in ((5, 0), (2 ** 40 + 3, 7)):
        got = input_masks("cuda:0", N, D, p, seed, step).cpu().numpy()
        want = (philox_uniforms(seed, 0, step, 0xFFFFFFFC, N * D) < p).astype(np.uint8).reshape(N, D)
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("kind", MODELS)
def test_matches_existing_device_code(kind, path):
    """Without dropout: `mean` is the row-wise mean of hmcx_softmax_predict / hmcx_logistic_predict over the
    sets, draw_nll is −hmcx_*_loglik / N per set."""
    c = lr.MULTIBLOCK[kind]
    pb, N, K, S = lr.problem(c), c.shape[0], c.shape[2], c.shape[3]
    m = _model(kind)
    r = m.posterior_predictive(lr.posterior(pb), pb.X, y=pb.y, path=path)
    sets = [{'weights': pb.W[s], 'bias': pb.b[s]} for s in range(S)]
    if kind == 'logistic':
        probs = [m.predict(p_, pb.X, prob=True, batchsize=N).reshape(N, 1) for p_ in sets]
        ll = [m.log_likelihood(p_, X_train=pb.X, y_train=pb.y) for p_ in sets]
    else:
        probs = [m.predict(p_, pb.X, prob=True) for p_ in sets]
        ll = [m.log_likelihood(p_, X_train=pb.X, y_train=om.one_hot(pb.y, K)) for p_ in sets]
    np.testing.assert_allclose(r.mean, np.mean(probs, axis=0), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(r.draw_nll, -np.asarray(ll) / N, rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("c,path", [(lr.CASES[1], 1), (lr.CASES[2], 1), (lr.CASES[2], 2), (lr.CASES[7], 2)],
                         ids=["general", "multiblock-path1", "multiblock-path2", "logistic-path2"])
def test_two_calls_are_bit_equal(c, path):
    _same(_run(c, path, True, torch.float32), _run(c, path, True, torch.float32))


def test_path0_selection_rule():
    """path 0 is the fused kernel where the shape is eligible and, with input dropout, the call has at least 32
    draws; without, at least 4 units and either 1536 row-block x unit pairs or 200 parameter sets — the general
    path otherwise.  Its bits are those of the path it names, on both sides of every bound."""
    def run(c, path, dropout, dtype=torch.float32):
        pb = lr.problem(c)
        return _model(c.model, dtype).posterior_predictive(lr.posterior(pb), pb.X, y=pb.y, path=path,
                                                           **(dict(n_dropout=c.shape[4], Z=pb.masks) if dropout else {}))

    seen = set()
    for c, dropout in ((lr.CASES[2], True), (lr.CASES[7], True), (lr.CASES[2], False), (lr.CASES[8], False),
                       (lr.CASES[5], True), (lr.LDS_EDGE, False)):
        N, D, K, S, T = c.shape
        named = 2 if lr.path0_is_fused(N, D, K, 4, S, T, dropout) else 1
        seen.add((dropout, named))
        _same(run(c, 0, dropout), run(c, named, dropout))
    assert (True, 1) in seen and (True, 2) in seen              # 18 and 40 draws
    # without dropout the bounds need rows: K = 16 (4 sets per unit), D = 8
    rs = np.random.RandomState(2)
    m = _model('softmax', torch.float32)
    for N, S, named in ((6144, 16, 2), (6128, 16, 1), (8192, 12, 1), (32, 200, 2), (32, 199, 1)):
        assert named == (2 if lr.path0_is_fused(N, 8, 16, 4, S, 1, False) else 1)
        post = {'weights': rs.normal(0, 0.3, (S, 8, 16)), 'bias': rs.normal(0, 0.3, (S, 16))}
        X, y = rs.rand(N, 8), rs.randint(0, 16, N)
        _same(m.posterior_predictive(post, X, y=y, path=0), m.posterior_predictive(post, X, y=y, path=named))
        other = m.posterior_predictive(post, X, y=y, path=3 - named)
        assert not np.array_equal(other.mean, m.posterior_predictive(post, X, y=y, path=0).mean)
    # float64 at the LDS edge: D = 945 is eligible in float32 only
    assert lr.fused_eligible(945, 3, 4) and not lr.fused_eligible(945, 3, 8)
    _same(run(lr.LDS_EDGE, 0, False, torch.float64), run(lr.LDS_EDGE, 1, False, torch.float64))


@pytest.mark.parametrize("c", INELIGIBLE, ids=lr.case_id)
def test_path2_rejects_ineligible_shape_and_path0_serves_it(c):
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    with pytest.raises(HmcxError, match="not eligible"):
        _run(c, 2, False)
    _check64(_run(c, 0, False), lr.case_ref(c, False))


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("c", [lr.CASES[4], lr.CASES[3], lr.CASES[7]], ids=lr.case_id)
def test_nan_in_one_parameter_set_stays_in_its_draws(c, path):
    """A NaN parameter set reaches the per-row outputs (which average over it) and its own draws only — also
    when it shares a column tile with other sets (20x16x10x40x1: six sets per unit on the fused path)."""
    S, T = c.shape[3], c.shape[4]
    pb = lr.problem(c)
    m = _model(c.model)
    bad = 2
    W = pb.W.copy()
    W[bad, 0, 0] = np.nan
    kw = dict(n_dropout=T, Z=pb.masks) if T > 1 else {}
    r = m.posterior_predictive({'weights': W, 'bias': pb.b}, pb.X, y=pb.y, path=path, **kw)   # returns normally
    assert np.all(np.isnan(r.mean))
    mine = np.arange(S * T) // T == bad
    assert np.all(np.isnan(r.draw_nll[mine])) and np.all(np.isfinite(r.draw_nll[~mine]))
    # the other draws are what a run without the bad set gives
    keep = [s for s in range(S) if s != bad]
    kw2 = dict(n_dropout=T, Z=pb.masks[~mine]) if T > 1 else {}
    r2 = m.posterior_predictive({'weights': pb.W[keep], 'bias': pb.b[keep]}, pb.X, y=pb.y, path=1, **kw2)
    np.testing.assert_allclose(r.draw_nll[~mine], r2.draw_nll, rtol=1e-11, atol=1e-14)
    np.testing.assert_array_equal(r.draw_accuracy[~mine], r2.draw_accuracy)
    assert np.all(np.isfinite(r2.mean))


def test_python_surface():
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    c = lr.CASES[1]                                             # softmax (19, 50, 7, 3, 2)
    N, D, K, S, T = c.shape
    pb = lr.problem(c)
    post = lr.posterior(pb)
    m = _model('softmax', torch.float32)
    r = m.posterior_predictive(post, pb.X, y=pb.y, n_dropout=T, seed=5)
    DR = S * T
    assert r.mean.shape == (N, K) and r.mean.dtype == np.float64
    assert r.pred.shape == (N,) and r.pred.dtype == np.int32
    for a in (r.entropy, r.expected_entropy, r.mutual_information, r.lppd):
        assert a.shape == (N,) and a.dtype == np.float64
    assert r.draw_nll.shape == (DR,) and r.draw_accuracy.shape == (DR,)
    # 6 draws: path 0 is the general path, whose probabilities are k_fwd's float32 softmax (exp, sum and divide
    # each within a few float32 ulps of a value <= 1), averaged in float64; the fused kernel's softmax is float64
    np.testing.assert_allclose(r.mean.sum(axis=1), 1.0, rtol=0, atol=8 * 2.0 ** -24)
    r2 = m.posterior_predictive(post, pb.X, y=pb.y, n_dropout=T, seed=5, path=2)
    np.testing.assert_allclose(r2.mean.sum(axis=1), 1.0, rtol=1e-12)
    assert r.mutual_information.min() >= -1e-12
    _same(r, m.posterior_predictive(post, pb.X, y=pb.y, n_dropout=T, seed=5))      # the seed names the masks
    # one-hot labels are integer labels; without labels the three label outputs are None
    _same(r, m.posterior_predictive(post, pb.X, y=om.one_hot(pb.y, K), n_dropout=T, seed=5))
    r0 = m.posterior_predictive(post, pb.X, n_dropout=T, seed=5)
    assert r0.lppd is None and r0.draw_nll is None and r0.draw_accuracy is None
    np.testing.assert_array_equal(r0.mean, r.mean)
    with pytest.raises(ValueError):
        m.posterior_predictive(post, pb.X, n_dropout=0, Z=pb.masks)
    with pytest.raises(HmcxError):
        m.posterior_predictive(post, pb.X, n_dropout=T, Z=pb.masks[:-1])
    with pytest.raises(HmcxError):
        m.posterior_predictive({'weights': pb.W, 'bias': pb.b[:-1]}, pb.X)
    with pytest.raises(HmcxError):
        _model('logistic').posterior_predictive(post, pb.X)      # K = 7 is not a logistic posterior
    # logistic.predict_posterior: the flattened mean, or mean > 0.5
    cl = lr.CASES[7]
    pl, ref = lr.problem(cl), lr.case_ref(cl, False)
    ml = _model('logistic')
    np.testing.assert_allclose(ml.predict_posterior(lr.posterior(pl), pl.X, prob=True), ref.mean.reshape(-1),
                               rtol=1e-11, atol=1e-14)
    np.testing.assert_array_equal(ml.predict_posterior(lr.posterior(pl), pl.X), ref.pred)
    # softmax.predict_posterior keeps its own (host-averaged) route and agrees within rounding
    np.testing.assert_allclose(_model('softmax').predict_posterior(post, pb.X, prob=True),
                               lr.case_ref(c, False).mean, rtol=1e-11, atol=1e-14)


def test_c_api_rejects_invalid_arguments():
    """T != 1 without dropout, label outputs without y and K != 1 for logistic return a negative code with
    hmcx_last_error set, and launch nothing (the outputs keep their bytes)."""
    from dropout_hamiltonian_montecarlo_amd._native import (LinearPredictiveArgs, MLP_MASKS_NONE, MODEL_LOGISTIC,
                                                            MODEL_SOFTMAX, context)
    ctx = context("cuda:0")
    dev = dict(device="cuda:0")
    X, W, b = torch.rand(4, 3, dtype=torch.float64, **dev), torch.rand(2, 3, 2, dtype=torch.float64, **dev), \
        torch.rand(2, 2, dtype=torch.float64, **dev)
    y = torch.zeros(4, dtype=torch.int32, **dev)
    out = torch.full((4, 2), -7.0, dtype=torch.float64, **dev)
    nll = torch.full((2,), -7.0, dtype=torch.float64, **dev)

    def call(**over):
        a = LinearPredictiveArgs()
        a.dtype, a.model, a.N, a.D, a.K, a.S, a.T, a.mask_mode, a.path = 1, MODEL_SOFTMAX, 4, 3, 2, 2, 1, MLP_MASKS_NONE, 0
        a.X, a.W, a.b, a.y, a.out_mean, a.out_draw_nll = X.data_ptr(), W.data_ptr(), b.data_ptr(), y.data_ptr(), \
            out.data_ptr(), nll.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        rc = ctx.lib.hmcx_linear_predictive(ctx.h, ctypes.byref(a))
        torch.cuda.synchronize()
        return rc, ctx.lib.hmcx_last_error(ctx.h).decode()

    for over, word in ((dict(T=2), "T must be 1"), (dict(y=None), "need labels"),
                       (dict(model=MODEL_LOGISTIC), "K = 1"), (dict(path=3), "path")):
        rc, msg = call(**over)
        assert rc < 0 and word in msg, (over, rc, msg)
        assert float(out.min()) == -7.0 and float(nll.min()) == -7.0
    rc, _ = call()
    assert rc == 0 and float(out.min()) >= 0.0 and float(nll.min()) > 0.0


def test_leading_dimensions_flatten_row_major():
    c = lr.CASES[1]
    N, D, K, _, _ = c.shape
    rs = np.random.RandomState(3)
    W, b = rs.normal(0, 0.3, (6, D, K)), rs.normal(0, 0.3, (6, K))
    X, y = rs.rand(N, D), rs.randint(0, K, N)
    m = _model('softmax')
    r_flat = m.posterior_predictive({'weights': W, 'bias': b}, X, y=y)
    r_nest = m.posterior_predictive({'weights': W.reshape(2, 3, D, K), 'bias': b.reshape(2, 3, K)}, X, y=y)
    _same(r_flat, r_nest)
    ref = lr.predictive_ref('softmax', W, b, X, y)              # draw d is set d: the order matters
    np.testing.assert_allclose(r_nest.draw_nll, ref.draw_nll, rtol=1e-11, atol=1e-14)


def test_sampler_posteriors_go_straight_in():
    """A posterior from sghmc.sample (softmax) and from hmc.sample (logistic) is the argument as returned,
    on a 40-row problem."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc import hmc
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
    X, Y = gi.dataset(4, 40, 24, 5)
    m = _model('softmax')
    s = sghmc(m, {"weights": np.zeros((24, 5)), "bias": np.zeros(5)}, path_length=1e-2, step_size=1e-3)
    s.out, s.trace = io.StringIO(), []
    np.random.seed(0)
    post, _ = s.sample(epochs=3, burnin=1, batch_size=20, rng=np.random.RandomState(1), X_train=X, y_train=Y)
    W, b = np.asarray(post['weights'], dtype=np.float64), np.asarray(post['bias'], dtype=np.float64)
    assert W.shape[1:] == (24, 5) and W.shape[0] >= 2
    ref = lr.predictive_ref('softmax', W, b, X, Y.argmax(axis=1))
    r = m.posterior_predictive(post, X, y=Y)                    # one-hot labels, as the sampler takes them
    np.testing.assert_allclose(r.mean, ref.mean, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(r.draw_nll, ref.draw_nll, rtol=1e-11, atol=1e-14)

    Xl, yl, _, _ = gi.logistic_inputs(11, 40, 4)
    ml = _model('logistic')
    h = hmc(ml, {"weights": np.full((4, 1), 0.3), "bias": np.array([0.1])}, path_length=0.005, step_size=1e-3)
    h.out, h.trace = io.StringIO(), []
    np.random.seed(9)
    postl = h.sample(6, 1, np.random.RandomState(10), X_train=Xl, y_train=yl)[0]
    Wl = np.asarray(postl['weights'], dtype=np.float64)
    S = Wl.shape[0]
    refl = lr.predictive_ref('logistic', Wl.reshape(S, 4, 1), np.asarray(postl['bias'], dtype=np.float64).reshape(S, 1),
                             Xl, yl)
    rl = ml.posterior_predictive(postl, Xl, y=yl)
    np.testing.assert_allclose(rl.mean, refl.mean, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(rl.draw_nll, refl.draw_nll, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(ml.predict_posterior(postl, Xl, prob=True), refl.mean.reshape(-1), rtol=1e-11, atol=1e-14)
