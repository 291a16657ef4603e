"""Momentum SGD on the dropout MLP (sgd.fit on the mlp model: one hmcx_mlp_sgd_run per fit) against
oracle.samplers.sgd over oracle.models.mlp with the same masks (tests/_mlp_sgd_ref.py).

Problems: the four tests/_mlp_fixtures shapes with three rows appended (N = 6·B + 3, the tail is dropped),
alpha = 0.01, step_size = 0.05, gamma = 0.9, 3 epochs = 18 steps.  Bounds: float64 parameters rtol 1e-8 /
atol 1e-10 and losses rtol 1e-10 (test_gpu_mlp.py's for MLP SGHMC trajectories of this length); float32
each variable within 2e-5 of the largest entry of the float64 oracle (test_gpu_mlp.py's float32 MLP-state
bound) and loss_val rtol 1e-4.  Measured float32 worst ratios (error / largest entry): DESIGN.md §5.3.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _mlp_fixtures as fx  # noqa: E402
import _mlp_sgd_ref as ref  # noqa: E402

F32_REL = 2e-5


def _classes():
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sgd import sgd
    return mlp, sgd


def _model(f, dtype):
    mlp, _ = _classes()
    return mlp({"alpha": ref.ALPHA}, f.n_in, f.n_mid, f.n_out, dtype=dtype, device="cuda:0")


def _gpu_fit(f, dtype, order=None, provider="stream", seed=0, masks=None):
    """sgd.fit on the fixture's problem; returns (sampler, par, loss_val)."""
    _, sgd = _classes()
    X, y, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    if order is not None:
        start = {k: start[k] for k in order}
    s = sgd(_model(f, dtype), start, step_size=ref.STEP_SIZE, seed=seed)
    if provider == "stream":
        s.mask_provider = ref.stream_masks(f.B, f.n_mid)[0]
    kw = {} if masks is None else {"masks": masks}
    par, loss_val = s.fit(epochs=ref.EPOCHS, batch_size=f.B, gamma=ref.GAMMA, X_train=X, y_train=y, **kw)
    return s, par, loss_val


def _check_f64(s, par, loss_val, r):
    assert list(par.keys()) == list(r.par.keys())
    for k in r.par:
        np.testing.assert_allclose(par[k], r.par[k], rtol=1e-8, atol=1e-10, err_msg=k)
        np.testing.assert_allclose(s.last_momentum[k].cpu().numpy(), r.momentum[k], rtol=1e-8, atol=1e-10, err_msg=k)
    np.testing.assert_allclose(loss_val, r.loss_val, rtol=1e-10)
    np.testing.assert_allclose(s.loss_trace, r.loss_trace, rtol=1e-10)


# ----------------------------------------------------------------------------- 1. float64, injected masks
@pytest.mark.parametrize("f", fx.FIXTURES, ids=[f.name for f in fx.FIXTURES])
def test_f64_matches_oracle(f):
    s, par, loss_val = _gpu_fit(f, torch.float64)
    _check_f64(s, par, loss_val, ref.fixture_fit(f))
    assert s.global_step == 18 and s.loss_trace.shape == (18,)


def test_f64_permuted_start_order():
    f = fx.BY_NAME["w32_b20"]
    s, par, loss_val = _gpu_fit(f, torch.float64, order=fx.PERMUTED)
    assert list(par.keys()) == fx.PERMUTED
    _check_f64(s, par, loss_val, ref.fixture_fit(f, order=fx.PERMUTED))


# ----------------------------------------------------------------------------- 2. float32
@pytest.mark.parametrize("name", ["w32_b20", "w256_b4"])
def test_f32_within_state_bound(name):
    f = fx.BY_NAME[name]
    s, par, loss_val = _gpu_fit(f, torch.float32)
    r = ref.fixture_fit(f, kind="f32")
    ratios = {k: np.abs(par[k] - r.par[k]).max() / np.abs(r.par[k]).max() for k in r.par}
    print("float32 %s: worst ratio %.3e (%s); loss_val rel %.3e; loss_trace rel %.3e" % (
        name, max(ratios.values()), max(ratios, key=ratios.get),
        np.max(np.abs(loss_val - r.loss_val) / np.abs(r.loss_val)),
        np.max(np.abs(s.loss_trace - r.loss_trace) / np.abs(r.loss_trace))))
    for k, v in ratios.items():
        assert v <= F32_REL, (k, v)
    np.testing.assert_allclose(loss_val, r.loss_val, rtol=1e-4)


# ----------------------------------------------------------------------------- 3. Philox masks
def _philox_mask_fn(m, B, seed):
    """mask_fn over the public entry: forward f of global step k is hmcx_mlp_masks(seed, chain 0, step k,
    slot 0x80000000 + f)."""
    cache = {}

    def mask_fn(k, f):
        if (k, f) not in cache:
            out = torch.empty((3, B, m.n_mid), dtype=m.dtype, device=m.device)
            ctx = m.ctx
            ctx.check(ctx.lib.hmcx_mlp_masks(ctx.h, m.code, B, m.n_mid, seed, 0, k, 0x80000000 + f, out.data_ptr()),
                      "hmcx_mlp_masks")
            cache[(k, f)] = out.cpu().numpy().astype(np.float64)
        return list(cache[(k, f)])
    return mask_fn


def test_philox_masks_reproducible_through_public_entry():
    f = fx.BY_NAME["w32_b20"]
    s, par, loss_val = _gpu_fit(f, torch.float64, provider=None, seed=5)
    r = ref.oracle_fit((f.n_in, f.n_mid, f.n_out), f.B, _philox_mask_fn(s.model, f.B, 5))
    _check_f64(s, par, loss_val, r)
    s2, par2, loss_val2 = _gpu_fit(f, torch.float64, provider=None, seed=5)
    for k in par:
        np.testing.assert_array_equal(par[k], par2[k])
    np.testing.assert_array_equal(loss_val, loss_val2)
    np.testing.assert_array_equal(s.loss_trace, s2.loss_trace)
    _, par3, _ = _gpu_fit(f, torch.float64, provider=None, seed=6)
    assert not np.array_equal(par["/l1/W"], par3["/l1/W"])


# ----------------------------------------------------------------------------- 4. call splitting (C ABI)
def _c_fit(m, Xd, yd, start, B, splits, seed):
    """hmcx_mlp_sgd_run in PHILOX mode over 18 steps, as len(splits) calls that carry par / mom and advance
    step_base; returns (par, mom, out_loss) as host arrays."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import MLP_PARAM_NAMES
    par = [m._dev(start[k]).clone() for k in MLP_PARAM_NAMES]
    mom = [torch.zeros_like(t) for t in par]
    rows = np.tile(np.arange(0, Xd.shape[0] - B + 1, B, dtype=np.int64), ref.EPOCHS)
    assert rows.size == sum(splits) == 18
    out_loss = torch.empty(rows.size, dtype=torch.float64, device=m.device)
    base = 0
    for n in splits:
        row0 = np.ascontiguousarray(rows[base:base + n])
        a = nat.MlpSgdArgs()
        a.dtype = m.code
        a.B, a.n_in, a.n_mid, a.n_out, a.n_steps = B, m.n_in, m.n_mid, m.n_out, n
        a.alpha, a.step_size, a.gamma = ref.ALPHA, ref.STEP_SIZE, ref.GAMMA
        a.X, a.y = Xd.data_ptr(), yd.data_ptr()
        a.row0 = row0.ctypes.data_as(nat.c_i64p)
        a.mask_mode = nat.MLP_MASKS_PHILOX
        a.seed, a.chain, a.step_base = seed, 0, 100 + base
        for i in range(6):
            a.par.p[i], a.mom.p[i] = par[i].data_ptr(), mom[i].data_ptr()
        a.out_loss = out_loss[base:].data_ptr()
        m.ctx.check(m.ctx.lib.hmcx_mlp_sgd_run(m.ctx.h, ctypes.byref(a)), "hmcx_mlp_sgd_run")
        base += n
    return [t.cpu().numpy() for t in par], [t.cpu().numpy() for t in mom], out_loss.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_one_call_equals_three_calls_bitwise(dtype):
    f = fx.BY_NAME["w96_b36"]
    m = _model(f, dtype)
    X, y, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    Xd, yd = m._xy({"X_train": X, "y_train": y})
    one = _c_fit(m, Xd, yd, start, f.B, [18], seed=9)
    three = _c_fit(m, Xd, yd, start, f.B, [6, 6, 6], seed=9)
    for a, b in zip(one[0] + one[1], three[0] + three[1]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(one[2], three[2])
    assert np.all(np.isfinite(one[2])) and not np.array_equal(one[0][0], m._dev(start["/l1/W"]).cpu().numpy())


# ----------------------------------------------------------------------------- 5. masks='off'
def test_masks_off_matches_undropped_oracle():
    f = fx.BY_NAME["w20_b30"]
    s, par, loss_val = _gpu_fit(f, torch.float64, provider=None, masks="off")
    _check_f64(s, par, loss_val, ref.fixture_fit(f, kind="off"))


# ----------------------------------------------------------------------------- 6. surface
def test_surface():
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    _, sgd = _classes()
    f = fx.BY_NAME["w32_b20"]
    m = _model(f, torch.float64)
    X, y, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    with pytest.raises(HmcxError):
        sgd(m, {k: start[k] for k in list(start)[:-1]})
    s = sgd(m, {k: start[k] for k in fx.PERMUTED}, step_size=ref.STEP_SIZE)
    with pytest.raises(HmcxError, match="fit_dropout"):
        s.fit_dropout(epochs=1, batch_size=f.B, X_train=X, y_train=y)
    with pytest.raises(ValueError):
        s.fit(epochs=1, batch_size=X.shape[0] + 1, X_train=X, y_train=y)
    assert s.global_step == 0
    s.mask_provider = ref.stream_masks(f.B, f.n_mid)[0]
    par, loss_val = s.fit(epochs=ref.EPOCHS, batch_size=f.B, gamma=ref.GAMMA, X_train=X, y_train=y)
    assert list(par.keys()) == fx.PERMUTED and loss_val.shape == (ref.EPOCHS,)
    for k in par:
        assert par[k].shape == start[k].shape and par[k].dtype == np.float64
    r = ref.fixture_fit(f, order=fx.PERMUTED)
    for k in par:
        np.testing.assert_allclose(s.last_momentum[k].cpu().numpy(), r.momentum[k], rtol=1e-8, atol=1e-10, err_msg=k)
        assert s.last_state[k].is_cuda and s.last_momentum[k].is_cuda
    # MC dropout of the fitted state, straight from the device tensors the fit left behind
    pred = m.predict_stochastic(s.last_state, X, n_dropout=4)
    assert pred.shape == (X.shape[0],) and pred.min() >= 0 and pred.max() < f.n_out
    np.testing.assert_array_equal(m.predict_stochastic(par, X, n_dropout=4, masks=None).shape, pred.shape)
