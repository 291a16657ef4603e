"""GPU tests of the MLP posterior predictive (hmcx_mlp_predictive, hmcx_mlp_pred.hip) against the float64
reference tests/_predictive_ref.py (oracle.models.mlp._forward + NumPy), on the general path (path 1) and
the fused row-block kernel (path 2).

Tolerances.  float64 `mean` and `draw_nll`: rtol 1e-11, atol 1e-14 (test_predict_matches_oracle /
test_grad_f64_matches_oracle: summation order only); the entropies and lppd, each a sum of n_out terms of
such quantities: rtol 1e-10, atol 1e-12.  float32 against the oracle at float32-rounded inputs: 2e-4 of the
largest reference entry (test_grad_f32_close_to_oracle).  `pred` and `draw_correct` exact: the cases'
seeds keep every reference top-two gap above 1e-6 (float64) / 1e-3 (float32), asserted on the oracle alone
in test_mlp_predictive_cpu.py."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _predictive_ref as pr  # noqa: E402
from oracle import models as om  # noqa: E402

IDS = lambda c: "x".join(map(str, c.shape))  # noqa: E731
FUSED = [c for c in pr.CASES if c.fused]
# every (case, path) that exists: the general path everywhere, the fused one where the shape is eligible
CASE_PATHS = [(c, 1) for c in pr.CASES] + [(c, 2) for c in FUSED]
CP_IDS = ["%s-path%d" % (IDS(c), p) for c, p in CASE_PATHS]


def _model(shape, dtype=None, seed=0):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp
    return mlp({"alpha": 0.01}, shape[1], shape[2], shape[3], dtype=dtype or torch.float64, device="cuda:0", seed=seed)


def _check64(r, ref):
    np.testing.assert_allclose(r.mean, ref.mean, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(r.draw_nll, ref.draw_nll, rtol=1e-11, atol=1e-14)
    for name in ("entropy", "expected_entropy", "lppd"):
        np.testing.assert_allclose(getattr(r, name), getattr(ref, name), rtol=1e-10, atol=1e-12, err_msg=name)
    np.testing.assert_allclose(r.mutual_information, r.entropy - r.expected_entropy, rtol=0, atol=0)
    np.testing.assert_allclose(r.mutual_information, ref.mutual_information, rtol=0, atol=1e-10)
    np.testing.assert_array_equal(r.pred, ref.pred)
    np.testing.assert_array_equal(r.draw_accuracy, ref.draw_accuracy)


@pytest.mark.parametrize("dropout", [True, False], ids=["fixed", "off"])
@pytest.mark.parametrize("c,path", CASE_PATHS, ids=CP_IDS)
def test_f64_matches_reference(c, path, dropout):
    pb, ref = pr.problem(c.shape, c.seed), pr.case_ref(c.shape, c.seed, dropout)
    m = _model(c.shape)
    if dropout:
        r = m.posterior_predictive(pr.stack(pb.par_sets), pb.X, y=pb.y, masks=pb.masks, n_dropout=c.shape[5], path=path)
    else:
        r = m.posterior_predictive(pr.stack(pb.par_sets), pb.X, y=pb.y, masks='off', path=path)
    _check64(r, ref)


def test_path0_is_some_valid_path_and_labels_are_optional():
    c = FUSED[0]
    pb, ref = pr.problem(c.shape, c.seed), pr.case_ref(c.shape, c.seed)
    r = _model(c.shape).posterior_predictive(pr.stack(pb.par_sets), pb.X, masks=pb.masks, n_dropout=c.shape[5])
    assert r.lppd is None and r.draw_nll is None and r.draw_accuracy is None
    np.testing.assert_allclose(r.mean, ref.mean, rtol=1e-11, atol=1e-14)
    np.testing.assert_array_equal(r.pred, ref.pred)


def test_path0_selection_rule():
    """path 0 is the fused kernel where the shape is eligible and there are at least two draws, the general
    path otherwise: its bits are those of the path it names."""
    def run(c, path, sets=None):
        pb = pr.problem(c.shape, c.seed)
        post = pr.stack(pb.par_sets[:sets] if sets else pb.par_sets)
        return _model(c.shape, torch.float32).posterior_predictive(post, pb.X, y=pb.y, masks='off', path=path)

    def same(a, b):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    same(run(pr.MULTIBLOCK, 0), run(pr.MULTIBLOCK, 2))          # eligible, two sets
    same(run(pr.MULTIBLOCK, 0, sets=1), run(pr.MULTIBLOCK, 1, sets=1))   # eligible, a single draw
    same(run(pr.CASES[0], 0), run(pr.CASES[0], 1))              # not eligible


@pytest.mark.parametrize("c", [c for c in pr.CASES if not c.fused], ids=IDS)
def test_path2_rejects_ineligible_shape(c):
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    pb = pr.problem(c.shape, c.seed)
    with pytest.raises(HmcxError, match="not eligible"):
        _model(c.shape).posterior_predictive(pr.stack(pb.par_sets), pb.X, masks='off', path=2)


@pytest.mark.parametrize("c,path", CASE_PATHS, ids=CP_IDS)
def test_f32_close_to_reference_at_rounded_inputs(c, path):
    pb, ref = pr.problem(c.shape, c.seed, True), pr.case_ref(c.shape, c.seed, True, True)
    m = _model(c.shape, torch.float32)
    r = m.posterior_predictive(pr.stack(pb.par_sets), pb.X, y=pb.y, masks=pb.masks, n_dropout=c.shape[5], path=path)
    for name in ("mean", "entropy", "expected_entropy"):
        got, want = getattr(r, name), getattr(ref, name)
        assert got.dtype == np.float64
        err, bound = np.abs(got - want).max(), 2e-4 * np.abs(want).max()
        assert err <= bound, "%s: max abs err %.3e > %.3e" % (name, err, bound)
    np.testing.assert_array_equal(r.pred, ref.pred)
    np.testing.assert_array_equal(r.draw_accuracy, ref.draw_accuracy)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("path", [1, 2])
def test_philox_equals_injected_api_masks(path, dtype):
    """PHILOX draw d uses the values hmcx_mlp_masks writes for slot0 + d (global row index, whatever the
    kernel's row tiling): injecting those masks gives the same bits."""
    c = pr.MULTIBLOCK
    N, T = c.shape[0], c.shape[5]
    pb = pr.problem(c.shape, c.seed)
    post, D = pr.stack(pb.par_sets), c.shape[4] * T
    a = _model(c.shape, dtype, seed=11)
    a.draw_masks(N)                                             # slot0 past 0
    r_philox = a.posterior_predictive(post, pb.X, y=pb.y, n_dropout=T, path=path)
    b = _model(c.shape, dtype, seed=11)
    b.draw_masks(N)
    masks = torch.stack([b.draw_masks(N) for _ in range(D)])    # slots slot0 … slot0 + D − 1
    assert a._mask_calls == b._mask_calls == 1 + D
    assert 0.05 < float((masks == 0).double().mean()) < 0.15
    r_fixed = b.posterior_predictive(post, pb.X, y=pb.y, masks=masks, n_dropout=T, path=path)
    for x, y in zip(r_philox, r_fixed):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("path", [1, 2])
def test_matches_existing_device_forward(path):
    c = pr.MULTIBLOCK
    T = c.shape[5]
    pb = pr.problem(c.shape, c.seed)
    m = _model(c.shape)
    r = m.posterior_predictive(pr.stack(pb.par_sets), pb.X, y=pb.y, masks=pb.masks, n_dropout=T, path=path)
    D = c.shape[4] * T
    probs = [m.predict(pb.par_sets[d // T], pb.X, prob=True, masks=list(pb.masks[d])) for d in range(D)]
    np.testing.assert_allclose(r.mean, np.mean(probs, axis=0), rtol=1e-11, atol=1e-14)
    nll = [m.log_likelihood(pb.par_sets[d // T], masks=list(pb.masks[d]), X_train=pb.X, y_train=pb.y) for d in range(D)]
    np.testing.assert_allclose(r.draw_nll, nll, rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("c,path", [(pr.CASES[0], 1), (pr.MULTIBLOCK, 1), (pr.MULTIBLOCK, 2)],
                         ids=["general", "multiblock-path1", "multiblock-path2"])
def test_two_calls_are_bit_equal(c, path):
    pb = pr.problem(c.shape, c.seed)
    m = _model(c.shape, torch.float32)
    kw = dict(y=pb.y, masks=pb.masks, n_dropout=c.shape[5], path=path)
    r1 = m.posterior_predictive(pr.stack(pb.par_sets), pb.X, **kw)
    r2 = m.posterior_predictive(pr.stack(pb.par_sets), pb.X, **kw)
    for x, y in zip(r1, r2):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("path", [1, 2])
def test_nan_in_one_parameter_set_stays_in_its_draws(path):
    c = pr.CASES[4]                                             # S = 5, T = 2
    S, T = c.shape[4], c.shape[5]
    pb = pr.problem(c.shape, c.seed)
    m = _model(c.shape)
    bad = 2
    post = pr.stack(pb.par_sets)
    post['/l3/W'] = post['/l3/W'].copy()
    post['/l3/W'][bad, 0, 0] = np.nan
    r = m.posterior_predictive(post, pb.X, y=pb.y, masks=pb.masks, n_dropout=T, path=path)   # returns normally
    assert np.all(np.isnan(r.mean))
    draws = np.arange(S * T)
    mine = draws // T == bad
    assert np.all(np.isnan(r.draw_nll[mine])) and np.all(np.isfinite(r.draw_nll[~mine]))
    # the other draws are what a run without the bad set gives
    keep = [s for s in range(S) if s != bad]
    good = pr.stack([pb.par_sets[s] for s in keep])
    r2 = m.posterior_predictive(good, pb.X, y=pb.y, masks=pb.masks[~mine], n_dropout=T, path=path)
    np.testing.assert_array_equal(r.draw_nll[~mine], r2.draw_nll)
    np.testing.assert_array_equal(r.draw_accuracy[~mine], r2.draw_accuracy)
    assert np.all(np.isfinite(r2.mean))


def test_python_surface():
    c = pr.CASES[3]                                             # (20, 16, 32, 5, 4, 3)
    N, _, n_mid, K, S, T = c.shape
    pb = pr.problem(c.shape, c.seed)
    post = pr.stack(pb.par_sets)
    m = _model(c.shape, torch.float32, seed=5)
    r = m.posterior_predictive(post, pb.X, y=pb.y, n_dropout=T)
    D = S * T
    assert r.mean.shape == (N, K) and r.mean.dtype == np.float64
    assert r.pred.shape == (N,) and r.pred.dtype == np.int32
    for a in (r.entropy, r.expected_entropy, r.mutual_information, r.lppd):
        assert a.shape == (N,) and a.dtype == np.float64
    assert r.draw_nll.shape == (D,) and r.draw_accuracy.shape == (D,)
    np.testing.assert_allclose(r.mean.sum(axis=1), 1.0, rtol=1e-12)
    assert r.mutual_information.min() >= -1e-12
    # two consecutive Philox calls differ; a fresh model with the same seed reproduces the first
    r_next = m.posterior_predictive(post, pb.X, y=pb.y, n_dropout=T)
    assert np.abs(r_next.mean - r.mean).max() > 1e-6
    assert m._mask_calls == 2 * D
    r_again = _model(c.shape, torch.float32, seed=5).posterior_predictive(post, pb.X, y=pb.y, n_dropout=T)
    for x, y in zip(r, r_again):
        np.testing.assert_array_equal(x, y)
    # predict_posterior: mean or pred
    m2 = _model(c.shape, torch.float32, seed=5)
    np.testing.assert_array_equal(m2.predict_posterior(post, pb.X, prob=True, n_dropout=T), r.mean)
    np.testing.assert_array_equal(m.predict_posterior(post, pb.X, masks='off'),
                                  m.posterior_predictive(post, pb.X, masks='off').pred)
    with pytest.raises(ValueError):
        m.posterior_predictive(post, pb.X, masks='off', n_dropout=2)
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    with pytest.raises(HmcxError):
        m.posterior_predictive({k: v for k, v in post.items() if k != '/l2/b'}, pb.X)
    with pytest.raises(HmcxError):
        m.posterior_predictive(post, pb.X, masks=pb.masks[:-1], n_dropout=T)


def test_leading_dimensions_flatten_row_major():
    c = pr.CASES[3]
    N, n_in, n_mid, K, _, _ = c.shape
    rs = np.random.RandomState(3)
    sets = [{k: rs.normal(0, 0.3, s) for k, s in om.mlp_param_shapes(n_in, n_mid, K).items()} for _ in range(6)]
    flat = pr.stack(sets)
    nested = {k: v.reshape((2, 3) + v.shape[1:]) for k, v in flat.items()}
    X, y = rs.rand(N, n_in), rs.randint(0, K, N)
    masks = np.stack([np.stack(om.dropout_masks(rs, N, n_mid, dtype=np.float64)) for _ in range(6)])
    m = _model(c.shape)
    r_flat = m.posterior_predictive(flat, X, y=y, masks=masks)
    r_nest = m.posterior_predictive(nested, X, y=y, masks=masks)
    for a, b in zip(r_flat, r_nest):
        np.testing.assert_array_equal(a, b)
    ref = pr.predictive_ref(sets, X, y, masks, 1)               # draw d is set d: the order matters
    np.testing.assert_allclose(r_nest.draw_nll, ref.draw_nll, rtol=1e-11, atol=1e-14)


def test_predict_stochastic_is_one_set_predictive():
    c = pr.CASES[3]
    pb = pr.problem(c.shape, c.seed)
    a, b = _model(c.shape, torch.float32, seed=2), _model(c.shape, torch.float32, seed=2)
    p = a.predict_stochastic(pb.par_sets[0], pb.X, prob=True, n_dropout=4)
    r = b.posterior_predictive(pb.par_sets[0], pb.X, n_dropout=4)
    np.testing.assert_array_equal(p, r.mean)
    np.testing.assert_array_equal(_model(c.shape, torch.float32, seed=2).predict_stochastic(pb.par_sets[0], pb.X, n_dropout=4),
                                  r.pred)


def test_sghmc_posterior_goes_straight_into_predict_posterior():
    """Two epochs of sghmc.sample on the w32_b20-sized MLP; the returned posterior dict is the argument."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
    import _mlp_fixtures as fx
    f = fx.BY_NAME["w32_b20"]
    X, y, start = fx.problem(f.n_in, f.n_mid, f.n_out, f.B)
    m = _model((0, f.n_in, f.n_mid, f.n_out))
    s = sghmc(m, start, noise='philox', seed=3, **fx.KW)
    s.trace, s.out = [], io.StringIO()
    post, _ = s.sample(epochs=2, burnin=0, batch_size=f.B, rng=np.random.RandomState(8), X_train=X, y_train=y)
    assert post['/l1/W'].shape == (2, f.n_mid, f.n_in)
    Xt, yt = X[:f.B], y[:f.B]
    sets = [{k: np.asarray(post[k][e], dtype=np.float64) for k in om.MLP_PARAM_NAMES} for e in range(2)]
    ref = pr.predictive_ref(sets, Xt, yt, None, 1)
    mean = m.predict_posterior(post, Xt, prob=True, masks='off')
    np.testing.assert_allclose(mean, ref.mean, rtol=1e-11, atol=1e-14)
    if ref.mean_gap > pr.GAP64:
        np.testing.assert_array_equal(m.predict_posterior(post, Xt, masks='off'), ref.pred)
    r = m.posterior_predictive(post, Xt, y=yt, masks='off')
    np.testing.assert_allclose(r.draw_nll, ref.draw_nll, rtol=1e-11, atol=1e-14)
