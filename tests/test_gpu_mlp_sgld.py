"""SGLD on the dropout MLP (sgld on the mlp model: one hmcx_mlp_sgld_run per epoch) against
oracle.samplers.sgld / sgld_gpu_variant over oracle.models.mlp with the same masks and noise
(tests/_mlp_sgld_ref.py).

Problems: the four tests/_mlp_fixtures shapes with three rows appended (N = 6·B + 3, the tail is dropped),
alpha = 0.01, step_size = 0.05, burnin = 1, epochs = 2: 18 steps.  Bounds (test_gpu_mlp_sgd.py's, the trajectory
is the same length): float64 parameters and momentum rtol 1e-8 / atol 1e-10, losses and logp_samples rtol 1e-10;
float32 each variable within 2e-5 of the largest entry of the float64 oracle and losses rtol 1e-4.  Printed loss
lines are compared as parsed numbers: both sides print four decimals, so two lines of values that agree to
1e-10 differ by at most one unit of the fourth decimal.  tests/test_mlp_sgld_cpu.py asserts on the oracle alone
that the noise moves the final state by at least 2e-4 of its largest entry.  Measured float32 worst ratios
(error / largest entry): DESIGN.md §5.3.
"""
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _mlp_fixtures as fx  # noqa: E402
import _mlp_sgld_ref as ref  # noqa: E402

F32_REL = 2e-5
PRINT_ATOL = 1.0001e-4


def _classes():
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sgld import sgld
    return mlp, sgld


def _model(f, dtype):
    mlp, _ = _classes()
    return mlp({"alpha": ref.ALPHA}, f.n_in, f.n_mid, f.n_out, dtype=dtype, device="cuda:0")


class Run:
    """One sgld.sample on a fixture's problem: the sampler, its results and what every epoch's call returned."""

    def __init__(self, f, dtype, variant="cpu", order=None, provider="stream", noise="numpy", seed=0, chain=0,
                 masks=None, keep_every=None, data=None, epochs=ref.EPOCHS, burnin=ref.BURNIN):
        _, sgld = _classes()
        X, y, start = data if data is not None else ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
        if order is not None:
            start = {k: start[k] for k in order}
        self.X, self.y, self.start = X, y, start
        s = sgld(_model(f, dtype), start, step_size=ref.STEP_SIZE, noise=noise, seed=seed, chain=chain,
                 variant=variant, keep_every=keep_every)
        if provider == "stream":
            s.mask_provider = ref.stream_masks(f.B, f.n_mid)[0]
        s.out = io.StringIO()
        self.loss_trace, self.log = [], []
        inner = s._run_mlp

        def recording(*a, **kw):
            res = inner(*a, **kw)
            self.loss_trace.extend(s.loss_trace)
            self.log.extend(v for v in res.ll if not np.isnan(v))
            return res
        s._run_mlp = recording
        kw = {} if masks is None else {"masks": masks}
        self.post, self.logp = s.sample(epochs=epochs, burnin=burnin, batch_size=f.B,
                                        rng=np.random.RandomState(ref.NOISE_SEED), X_train=X, y_train=y, **kw)
        self.s = s
        self.lines = ref.parse_lines(s.out.getvalue())
        self.last = {k: v.cpu().numpy() for k, v in s.last_state.items()}
        self.mom = None if s.last_momentum is None else {k: v.cpu().numpy() for k, v in s.last_momentum.items()}


def _check_lines(got, want):
    assert [g[:3] for g in got] == [w[:3] for w in want] and len(got) > 0
    np.testing.assert_allclose([g[3] for g in got], [w[3] for w in want], rtol=0, atol=PRINT_ATOL)


def _check_f64(g, r, variant="cpu"):
    assert list(g.post.keys()) == list(r.post.keys())
    for k in r.post:
        np.testing.assert_allclose(g.post[k], r.post[k], rtol=1e-8, atol=1e-10, err_msg=k)
        np.testing.assert_allclose(g.last[k], r.q[k], rtol=1e-8, atol=1e-10, err_msg=k)
        if variant == "gpu":
            np.testing.assert_allclose(g.mom[k], r.p[k], rtol=1e-8, atol=1e-10, err_msg=k)
    assert (g.mom is None) == (variant != "gpu")
    np.testing.assert_allclose(g.logp, r.logp, rtol=1e-10)
    np.testing.assert_allclose(g.loss_trace, r.loss_trace, rtol=1e-10)
    np.testing.assert_allclose(g.log, r.log_trace, rtol=1e-10)
    _check_lines(g.lines, r.lines)


# ----------------------------------------------------------------------------- 1. float64, cpu variant
@pytest.mark.parametrize("f", fx.FIXTURES, ids=[f.name for f in fx.FIXTURES])
def test_f64_cpu_variant_matches_oracle(f):
    g = Run(f, torch.float64)
    _check_f64(g, ref.fixture_run(f))
    assert g.s.global_step == 18 and len(g.loss_trace) == 18


# ----------------------------------------------------------------------------- 2. float64, gpu variant
@pytest.mark.parametrize("name", ["w32_b20", "w96_b36"])
def test_f64_gpu_variant_matches_oracle(name):
    f = fx.BY_NAME[name]
    g = Run(f, torch.float64, variant="gpu")
    _check_f64(g, ref.fixture_run(f, "gpu"), variant="gpu")
    assert g.s.global_step == 18


# ----------------------------------------------------------------------------- 3. permuted start order
def test_f64_permuted_start_order():
    f = fx.BY_NAME["w32_b20"]
    g = Run(f, torch.float64, order=fx.PERMUTED)
    assert list(g.post.keys()) == fx.PERMUTED
    r = ref.fixture_run(f, order=fx.PERMUTED)
    _check_f64(g, r)
    # the noise layout follows the order: the canonical-order oracle is another trajectory
    assert ref.state_distance(r.q, ref.fixture_run(f).q) > 2e-4


# ----------------------------------------------------------------------------- 4. float32
@pytest.mark.parametrize("variant", ["cpu", "gpu"])
@pytest.mark.parametrize("name", ["w32_b20", "w256_b4"])
def test_f32_within_state_bound(name, variant):
    f = fx.BY_NAME[name]
    g = Run(f, torch.float32, variant=variant)
    r = ref.fixture_run(f, variant, kind="f32")
    ratios = {k: np.abs(g.last[k] - r.q[k]).max() / np.abs(r.q[k]).max() for k in r.q}
    post = {k: np.abs(g.post[k] - r.post[k]).max() / np.abs(r.post[k]).max() for k in r.q}
    mom = {k: np.abs(g.mom[k] - r.p[k]).max() / np.abs(r.p[k]).max() for k in r.q} if variant == "gpu" else {}
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - b) / np.abs(b)))  # noqa: E731
    print("float32 %s %s: worst ratio %.3e (%s), posterior %.3e, momentum %.3e; logp rel %.3e; loss_trace rel %.3e; "
          "log lines rel %.3e" % (name, variant, max(ratios.values()), max(ratios, key=ratios.get), max(post.values()),
                                  max(mom.values()) if mom else float("nan"), rel(g.logp, r.logp),
                                  rel(g.loss_trace, r.loss_trace), rel(g.log, r.log_trace)))
    for k in ratios:
        assert ratios[k] <= F32_REL, (k, ratios[k])
        assert post[k] <= F32_REL, (k, post[k])
        if mom:
            assert mom[k] <= F32_REL, (k, mom[k])
    np.testing.assert_allclose(g.logp, r.logp, rtol=1e-4)
    np.testing.assert_allclose(g.loss_trace, r.loss_trace, rtol=1e-4)
    np.testing.assert_allclose(g.log, r.log_trace, rtol=1e-4)


# ----------------------------------------------------------------------------- 5. Philox noise and masks
def _philox_mask_fn(m, B, seed, chain):
    """mask_fn over the public entry: forward f of global step k is hmcx_mlp_masks(seed, chain, step k,
    slot 0x80000000 + f)."""
    cache = {}

    def mask_fn(k, f):
        if (k, f) not in cache:
            out = torch.empty((3, B, m.n_mid), dtype=m.dtype, device=m.device)
            ctx = m.ctx
            ctx.check(ctx.lib.hmcx_mlp_masks(ctx.h, m.code, B, m.n_mid, seed, chain, k, 0x80000000 + f,
                                             out.data_ptr()), "hmcx_mlp_masks")
            cache[(k, f)] = out.cpu().numpy().astype(np.float64)
        return list(cache[(k, f)])
    return mask_fn


def _philox_source(start, seed, chain, n_steps):
    """The noise of steps 0 .. n_steps − 1 through the public host entry: P float64 normals per step, element
    e = offset of the variable in start's order + index."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    P = sum(int(np.prod(v.shape)) for v in start.values())
    return ref.array_source(np.concatenate([nat.philox_normals(seed, chain, k, 0, 0, P, dtype="f64")
                                            for k in range(n_steps)]))


@pytest.mark.parametrize("variant", ["cpu", "gpu"])
def test_philox_noise_and_masks_rebuilt_through_public_entries(variant):
    f = fx.BY_NAME["w32_b20"]
    kw = dict(variant=variant, provider=None, noise="philox")
    g = Run(f, torch.float64, seed=5, chain=2, **kw)
    r = ref.oracle_run((f.n_in, f.n_mid, f.n_out), f.B, _philox_mask_fn(g.s.model, f.B, 5, 2), variant,
                       _philox_source(g.start, 5, 2, 18))
    _check_f64(g, r, variant=variant)
    if variant == "gpu":
        return
    g2 = Run(f, torch.float64, seed=5, chain=2, **kw)
    for k in g.post:
        np.testing.assert_array_equal(g.post[k], g2.post[k])
    np.testing.assert_array_equal(g.logp, g2.logp)
    np.testing.assert_array_equal(g.loss_trace, g2.loss_trace)
    assert not np.array_equal(g.last["/l1/W"], Run(f, torch.float64, seed=6, chain=2, **kw).last["/l1/W"])
    assert not np.array_equal(g.last["/l1/W"], Run(f, torch.float64, seed=5, chain=3, **kw).last["/l1/W"])


# ----------------------------------------------------------------------------- 6. call splitting (C ABI)
def _c_run(m, Xd, yd, start, B, splits, seed, variant):
    """hmcx_mlp_sgld_run with PHILOX noise and masks over 18 steps, as len(splits) calls that carry par / mom
    and advance step_base and the draw pointers; every third step is kept.  Returns host arrays
    (par, mom, out_loss, draws)."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import MLP_PARAM_NAMES
    par = [m._dev(start[k]).clone() for k in MLP_PARAM_NAMES]
    mom = [torch.zeros_like(t) for t in par]
    rows = np.tile(np.arange(0, Xd.shape[0] - B + 1, B, dtype=np.int64), 3)
    assert rows.size == sum(splits) == 18
    flags = (np.arange(18) % 3 == 2).astype(np.uint8)
    draws = [torch.zeros((int(flags.sum()),) + tuple(t.shape), dtype=t.dtype, device=t.device) for t in par]
    out_loss = torch.empty(rows.size, dtype=torch.float64, device=m.device)
    eps = ref.STEP_SIZE / (1.0 + 0.01 * np.arange(18))            # a step size of its own per step
    base = 0
    for n in splits:
        row0, ep = np.ascontiguousarray(rows[base:base + n]), np.ascontiguousarray(eps[base:base + n])
        wd = np.ascontiguousarray(flags[base:base + n])
        a = nat.MlpSgldArgs()
        a.dtype = m.code
        a.B, a.n_in, a.n_mid, a.n_out, a.n_steps = B, m.n_in, m.n_mid, m.n_out, n
        for i in range(6):
            a.order[i] = i
        a.variant, a.alpha = variant, ref.ALPHA
        a.X, a.y = Xd.data_ptr(), yd.data_ptr()
        a.row0 = row0.ctypes.data_as(nat.c_i64p)
        a.eps = ep.ctypes.data_as(nat.c_dblp)
        a.noise_mode, a.mask_mode = nat.NOISE_PHILOX, nat.MLP_MASKS_PHILOX
        a.seed, a.chain, a.step_base = seed, 1, 100 + base
        d0 = int(flags[:base].sum())
        for i in range(6):
            a.par.p[i] = par[i].data_ptr()
            if variant == 1:
                a.mom.p[i] = mom[i].data_ptr()
            a.draws.p[i] = draws[i][d0:].data_ptr() if d0 < draws[i].shape[0] else draws[i].data_ptr()
        a.want_draw = wd.ctypes.data_as(nat.c_u8p)
        a.out_loss = out_loss[base:].data_ptr()
        m.ctx.check(m.ctx.lib.hmcx_mlp_sgld_run(m.ctx.h, ctypes.byref(a)), "hmcx_mlp_sgld_run")
        base += n
    host = lambda ts: [t.cpu().numpy() for t in ts]  # noqa: E731
    return host(par), host(mom), out_loss.cpu().numpy(), host(draws)


@pytest.mark.parametrize("variant", [0, 1], ids=["cpu", "gpu"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_one_call_equals_three_calls_bitwise(dtype, variant):
    f = fx.BY_NAME["w96_b36"]
    m = _model(f, dtype)
    X, y, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    Xd, yd = m._xy({"X_train": X, "y_train": y})
    one = _c_run(m, Xd, yd, start, f.B, [18], seed=9, variant=variant)
    three = _c_run(m, Xd, yd, start, f.B, [6, 6, 6], seed=9, variant=variant)
    for a, b in zip(one[0] + one[1] + one[3], three[0] + three[1] + three[3]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(one[2], three[2])
    assert np.all(np.isfinite(one[2])) and not np.array_equal(one[0][0], m._dev(start["/l1/W"]).cpu().numpy())
    for p, d in zip(one[0], one[3]):                              # step 17 is kept: the last draw is the state
        np.testing.assert_array_equal(d[-1], p)
        assert d.shape[0] == 6 and not np.array_equal(d[0], d[1])
    assert (np.abs(one[1][0]).max() > 0) == (variant == 1)


# ----------------------------------------------------------------------------- 7. masks='off'
def test_masks_off_matches_undropped_oracle():
    f = fx.BY_NAME["w20_b30"]
    g = Run(f, torch.float64, provider=None, masks="off")
    _check_f64(g, ref.fixture_run(f, kind="off"))


# ----------------------------------------------------------------------------- 8. two evaluations on one step
def test_log_line_and_epoch_end_on_the_same_step():
    """11 minibatches, burnin 0, one epoch: minibatch 10 is a log line and the epoch's last, so the step takes
    forwards 1 (log line) and 2 (negative_log_posterior) behind its gradient forward."""
    f = fx.BY_NAME["w32_b20"]
    data = fx.problem(f.n_in, f.n_mid, f.n_out, f.B, n_batches=11)
    asked = []
    _, sgld = _classes()
    g0, mask_fn = ref.stream_masks(f.B, f.n_mid)
    r = ref.oracle_run((f.n_in, f.n_mid, f.n_out), f.B, mask_fn, "cpu", ref.numpy_source(), epochs=1, burnin=0,
                       data=data)
    s = sgld(_model(f, torch.float64), data[2], step_size=ref.STEP_SIZE)
    s.mask_provider = lambda k, n: (asked.append((k, n)), g0(k, n))[1]
    s.out = io.StringIO()
    post, logp = s.sample(epochs=1, burnin=0, batch_size=f.B, rng=np.random.RandomState(ref.NOISE_SEED),
                          X_train=data[0], y_train=data[1])
    assert asked == [(0, 2)] + [(k, 1) for k in range(1, 10)] + [(10, 3)] and s.global_step == 11
    for k in r.post:
        np.testing.assert_allclose(post[k], r.post[k], rtol=1e-8, atol=1e-10, err_msg=k)
    np.testing.assert_allclose(logp, r.logp, rtol=1e-10)
    lines = ref.parse_lines(s.out.getvalue())
    assert [ln[:3] for ln in lines] == [("epoch", 0, 0), ("epoch", 0, 10), (None, None, None)]
    _check_lines(lines, r.lines)
    np.testing.assert_allclose(s.loss_trace, r.loss_trace, rtol=1e-10)


# ----------------------------------------------------------------------------- 9. draws
def test_keep_every_draws_feed_the_device_predictive():
    f = fx.BY_NAME["w32_b20"]
    g3 = Run(f, torch.float64, keep_every=3)
    g1 = Run(f, torch.float64, keep_every=1)
    assert Run(f, torch.float64).s.device_draws is None
    for k, shape in g3.s.model.shapes.items():
        d3, d1 = g3.s.device_draws[k], g1.s.device_draws[k]
        assert d3.is_cuda and tuple(d3.shape) == (4,) + shape and tuple(d1.shape) == (12,) + shape
        np.testing.assert_array_equal(d3.cpu().numpy(), d1.cpu().numpy()[[2, 5, 8, 11]])
        np.testing.assert_array_equal(d1.cpu().numpy()[[5, 11]], g1.post[k])      # the epochs' last states
    m = g3.s.model
    dev = m.posterior_predictive(g3.s.device_draws, g3.X, g3.y, masks="off")
    host = m.posterior_predictive({k: v.cpu().numpy() for k, v in g3.s.device_draws.items()}, g3.X, g3.y, masks="off")
    for name, a, b in zip(dev._fields, dev, host):
        assert np.all(np.isfinite(a)), name
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert dev.draw_nll.shape == (4,) and dev.mean.shape == (g3.X.shape[0], f.n_out)


# ----------------------------------------------------------------------------- 10. surface
def test_surface():
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    _, sgld = _classes()
    f = fx.BY_NAME["w32_b20"]
    m = _model(f, torch.float64)
    X, y, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    with pytest.raises(HmcxError):
        sgld(m, {k: start[k] for k in list(start)[:-1]})
    with pytest.raises(HmcxError):
        sgld(m, start, chains=2)
    s = sgld(m, start, step_size=ref.STEP_SIZE)
    s.out = io.StringIO()
    with pytest.raises(ValueError):
        s.sample(epochs=1, burnin=0, batch_size=X.shape[0] + 1, X_train=X, y_train=y)
    assert s.global_step == 0


@pytest.mark.parametrize("variant", ["cpu", "gpu"])
def test_step_matches_oracle_step(variant):
    _, sgld = _classes()
    f = fx.BY_NAME["w32_b20"]
    X, y, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    start = {k: start[k] for k in fx.PERMUTED}
    Xb, yb = X[:f.B], y[:f.B]
    rs = np.random.RandomState(2)
    mom0 = {k: 0.3 * rs.standard_normal(v.shape) for k, v in start.items()}
    provider, mask_fn = ref.stream_masks(f.B, f.n_mid)
    from oracle import models as om
    o = ref.sampler_class(variant)(ref.MaskedSgldMLP(om.mlp({"alpha": ref.ALPHA}, f.n_in, f.n_mid, f.n_out), mask_fn),
                                   start, step_size=ref.STEP_SIZE)
    q_r, p_r = o.step(start, mom0, ref.StreamRng(ref.numpy_source()), X_train=Xb, y_train=yb)
    s = sgld(_model(f, torch.float64), start, step_size=ref.STEP_SIZE, variant=variant)
    s.mask_provider = provider
    q, p = s.step(start, mom0, np.random.RandomState(ref.NOISE_SEED), X_train=Xb, y_train=yb)
    assert list(q.keys()) == fx.PERMUTED and s.global_step == 1
    for k in start:
        assert q[k].is_cuda
        np.testing.assert_allclose(q[k].cpu().numpy(), q_r[k], rtol=1e-8, atol=1e-10, err_msg=k)
        assert not np.array_equal(q[k].cpu().numpy(), start[k])
    if variant == "cpu":
        assert p is None
    else:
        for k in start:
            np.testing.assert_allclose(p[k].cpu().numpy(), p_r[k], rtol=1e-8, atol=1e-10, err_msg=k)
