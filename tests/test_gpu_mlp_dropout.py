"""The dropout ratio of the MLP through every device path: mlp(..., dropout=r) and the context setting behind it
(hmcx_set_mlp_dropout).

1. hmcx_mlp_masks at several ratios against the host twin of the keep law (tests/_mlp_dropout.py).
2. Philox ≡ fixed, entry by entry, at r = 0.5 and r = 0.9: a run that draws its masks from Philox at ratio r against
   the same run fed the values hmcx_mlp_masks writes at ratio r for the same (seed, chain, step, slot).  Both runs are
   device runs of the same kernels that read the mask values from a buffer (the one-chain SGHMC reads keep flags in
   Philox mode and is pinned bit for bit against values at 0.1 already), the fixed blocks start at multiples of
   3·B·n_mid elements of 256-byte aligned allocations, so vector and scalar mask reads are chosen alike: the
   comparison is bit for bit, except where the entry's existing Philox test holds a bound against the NumPy oracle
   (SGD, SGLD: float64 rtol 1e-8 / atol 1e-10 on parameters, rtol 1e-10 on losses) — there that bound is used.
3. dropout=0.1 is byte-identical to a model built without the keyword, and a context set to 0.1 explicitly to one that
   never called the setter.
4. Two models of different ratios interleaved on one device.
5. predict_stochastic at 0.5 against posterior_predictive fed the ratio-0.5 masks.
6. An invalid ratio raises and leaves the context's ratio as it was.

Shapes: the mask entry at B = 19, n_mid = 37 (n3 = 2109: a ragged last group, about 8 ties per forward); every
sampler entry on the smallest case of its own test file."""
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _mlp_dropout as md  # noqa: E402
import _mlp_fixtures as fx  # noqa: E402
import _mlp_hmc_ref as hmcref  # noqa: E402
import _mlp_sgd_ref as sgdref  # noqa: E402
import _mlp_sghmc_chains_ref as scref  # noqa: E402
import _mlp_sgld_ref as sgldref  # noqa: E402
import test_gpu_mlp_hmc_chains as hc  # noqa: E402
import test_gpu_mlp_sghmc_chains as sc  # noqa: E402

SLOT0 = 0x80000000
RATIOS = [0.5, 0.9]
DT = {"f64": torch.float64, "f32": torch.float32}


def _nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    return _native


def _mlp_mod():
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu import mlp
    return mlp


def _force_ratio(ctx, ratio):
    """Through the library, whatever the wrapper believes."""
    ctx.check(ctx.lib.hmcx_set_mlp_dropout(ctx.h, float(ratio)), "hmcx_set_mlp_dropout")
    ctx.mlp_dropout = float(ratio)


@pytest.fixture(autouse=True)
def _default_ratio_afterwards():
    """No test of this file leaks a ratio into the files that run after it."""
    yield
    _force_ratio(_nat().context(0), 0.1)


def _model(n_in, n_mid, n_out, dtype, alpha=0.01, seed=0, **kw):
    return _mlp_mod().mlp({"alpha": alpha}, n_in, n_mid, n_out, dtype=dtype, device="cuda:0", seed=seed, **kw)


def _api_masks(ctx, dtype, B, n_mid, seed, chain, step, slot):
    """What hmcx_mlp_masks writes at the context's present ratio: a device tensor [3, B, n_mid]."""
    nat = _nat()
    out = torch.empty((3, B, n_mid), dtype=dtype, device="cuda:0")
    ctx.check(ctx.lib.hmcx_mlp_masks(ctx.h, nat.dtype_code(dtype), B, n_mid, seed, chain, step & 0xFFFFFFFF,
                                     slot & 0xFFFFFFFF, nat.ptr(out)), "hmcx_mlp_masks")
    return out


def _provider(m, B, seed, chain):
    """A mask_provider over the public entry at the model's ratio: forward f of global step k is
    hmcx_mlp_masks(seed, chain, k, 0x80000000 + f)."""
    def provider(k, nf):
        ctx = _mlp_mod().mlp_context(m)
        return torch.stack([_api_masks(ctx, m.dtype, B, m.n_mid, seed, chain, k, SLOT0 + f)
                            for f in range(nf)]).cpu().numpy()
    return provider


def _same(a, b, what=""):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg="%s[%d]" % (what, i))


# ----------------------------------------------------------------------------- 1. the mask entry
MASK_KEY = dict(seed=0x123456789AB, chain=7, step=11, slot=SLOT0 + 5)
B1, NMID1 = 19, 37
N3 = 3 * B1 * NMID1


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("ratio", [0.05, 0.5, 0.9])
def test_masks_entry_equals_the_host_twin(ratio, dt):
    ctx = _nat().context(0)
    ctx.set_mlp_dropout(ratio)
    assert ctx.get_mlp_dropout() == ratio
    got = _api_masks(ctx, DT[dt], B1, NMID1, **MASK_KEY).cpu().numpy().reshape(-1)
    want = md.keep_group_host(ratio, MASK_KEY["seed"], N3, MASK_KEY["slot"], MASK_KEY["step"], MASK_KEY["chain"])
    assert want.any() and not want.all()
    np.testing.assert_array_equal(got != 0, want)
    scale = got.dtype.type(1.0 / (1.0 - ratio))                     # computed in double, then cast
    assert set(np.unique(got)) == {got.dtype.type(0), scale}


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_masks_entry_at_ratio_zero_is_all_ones(dt):
    ctx = _nat().context(0)
    ctx.set_mlp_dropout(0.0)
    got = _api_masks(ctx, DT[dt], B1, NMID1, **MASK_KEY).cpu().numpy()
    np.testing.assert_array_equal(got, np.ones_like(got))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_explicit_default_equals_a_context_that_never_set_it(dt):
    nat = _nat()
    fresh, other = nat.Context(0), nat.Context(0)
    for c in (fresh, other):
        c.bind_stream()
    assert fresh.get_mlp_dropout() == 0.1
    _force_ratio(other, 0.5)
    _force_ratio(other, 0.1)
    a = _api_masks(fresh, DT[dt], B1, NMID1, **MASK_KEY).cpu().numpy()
    b = _api_masks(other, DT[dt], B1, NMID1, **MASK_KEY).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    want = md.keep_group_host_default(MASK_KEY["seed"], N3, MASK_KEY["slot"], MASK_KEY["step"], MASK_KEY["chain"])
    np.testing.assert_array_equal(a.reshape(-1) != 0, want)
    assert set(np.unique(a)) == {a.dtype.type(0), a.dtype.type(1 / 0.9)}


# ----------------------------------------------------------------------------- the runs of sections 2 to 4
def _sghmc_run(dtype, fuse=True, provider=False, **mkw):
    """test_gpu_mlp.py's fwdr-f32 case (w96_b36): two epochs of one-chain SGHMC with Philox noise."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
    f = fx.BY_NAME["w96_b36"]
    X, y, start = fx.problem(f.n_in, f.n_mid, f.n_out, f.B, n_batches=2)
    m = _model(f.n_in, f.n_mid, f.n_out, dtype, **mkw)
    m.ctx.set_mlp_fuse(fuse)
    try:
        s = sghmc(m, start, path_length=5e-3, step_size=1e-3, verbose=False, noise='philox', seed=5, chain=3)
        s.mask_provider = _provider(m, f.B, 5, 3) if provider else None
        s.trace, s.out = [], io.StringIO()
        post, logp = s.sample(epochs=2, burnin=1, batch_size=f.B, X_train=X, y_train=y)
    finally:
        m.ctx.set_mlp_fuse(True)
    assert max(t["L"] for t in s.trace) >= 3
    return [post[k] for k in post] + [logp, [t["L"] for t in s.trace], [t["accepted"] for t in s.trace]]


def _hmc_run(monkeypatch, host, **mkw):
    """test_gpu_mlp.py's leapfrog case: four HMC steps, the trajectory in one hmcx_mlp_hmc_leapfrog call (Philox masks
    per gradient call) or as the host loop whose every grad() is handed the values hmcx_mlp_masks writes."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc import hmc
    if host:
        monkeypatch.setenv("HMCX_HMC_HOST_LOOP", "1")
    else:
        monkeypatch.delenv("HMCX_HMC_HOST_LOOP", raising=False)
    n_in, n_mid, n_out, N = 24, 20, 5, 60
    rs = np.random.RandomState(21)
    X, y = rs.rand(N, n_in), rs.randint(0, n_out, N)
    shapes = _mlp_mod().mlp_param_shapes(n_in, n_mid, n_out)
    start = {k: rs.normal(0, 0.2, shapes[k]) for k in ['/l2/W', '/l1/b', '/l3/b', '/l1/W', '/l3/W', '/l2/b']}
    m = _model(n_in, n_mid, n_out, torch.float64, seed=5, **mkw)
    s = hmc(m, start, path_length=0.03, step_size=0.005, verbose=True)
    s.trace, s.out = [], io.StringIO()
    np.random.seed(3)
    post, loss, _, _ = s.sample(4, 1, np.random.RandomState(4), X_train=X, y_train=y)
    assert max(t["L"] for t in s.trace) >= 3
    return [np.asarray(post[k]) for k in start] + [loss, [t["L"] for t in s.trace], m._mask_calls]


def _sgd_run(provider=False, **mkw):
    """test_gpu_mlp_sgd.py's Philox case (w32_b20, float64): (parameters, [loss_val, loss_trace])."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sgd import sgd
    f = fx.BY_NAME["w32_b20"]
    X, y, start = sgdref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    m = _model(f.n_in, f.n_mid, f.n_out, torch.float64, alpha=sgdref.ALPHA, **mkw)
    s = sgd(m, start, step_size=sgdref.STEP_SIZE, seed=5)
    s.mask_provider = _provider(m, f.B, 5, 0) if provider else None
    par, loss_val = s.fit(epochs=sgdref.EPOCHS, batch_size=f.B, gamma=sgdref.GAMMA, X_train=X, y_train=y)
    return [par[k] for k in par], [np.asarray(loss_val), np.asarray(s.loss_trace)]


def _sgld_sampler(m, start, provider=None, seed=5, chain=2):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sgld import sgld
    s = sgld(m, start, step_size=sgldref.STEP_SIZE, noise="philox", seed=seed, chain=chain, variant="cpu")
    s.mask_provider = provider
    s.out = io.StringIO()
    return s


def _sgld_run(provider=False, **mkw):
    """test_gpu_mlp_sgld.py's Philox case (w32_b20, float64, variant cpu): (draws and last state, [logp])."""
    f = fx.BY_NAME["w32_b20"]
    X, y, start = sgldref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    m = _model(f.n_in, f.n_mid, f.n_out, torch.float64, alpha=sgldref.ALPHA, **mkw)
    s = _sgld_sampler(m, start, _provider(m, f.B, 5, 2) if provider else None)
    post, logp = s.sample(epochs=sgldref.EPOCHS, burnin=sgldref.BURNIN, batch_size=f.B,
                          rng=np.random.RandomState(sgldref.NOISE_SEED), X_train=X, y_train=y)
    return [post[k] for k in post] + [v.cpu().numpy() for v in s.last_state.values()], [np.asarray(logp)]


def _predictive_run(dtype, path, fixed=False, **mkw):
    """test_gpu_mlp_predictive.py's Philox case: PHILOX draws against the same slots injected as values."""
    import _predictive_ref as pr
    c = pr.MULTIBLOCK
    N, T = c.shape[0], c.shape[5]
    pb = pr.problem(c.shape, c.seed)
    post, D = pr.stack(pb.par_sets), c.shape[4] * T
    m = _model(c.shape[1], c.shape[2], c.shape[3], dtype, seed=11, **mkw)
    m.draw_masks(N)                                                 # slot0 past 0
    masks = torch.stack([m.draw_masks(N) for _ in range(D)]) if fixed else None
    r = m.posterior_predictive(post, pb.X, y=pb.y, masks=masks, n_dropout=T, path=path)
    assert m._mask_calls == 1 + D
    return list(r), masks


# ----------------------------------------------------------------------------- 2. Philox ≡ fixed, entry by entry
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("dt,fuse", [("f32", True), ("f64", True), ("f64", False)], ids=["fwdr-f32", "fused-f64", "unfused-f64"])
def test_sghmc_philox_equals_fixed(dt, fuse, ratio):
    _same(_sghmc_run(DT[dt], fuse, dropout=ratio), _sghmc_run(DT[dt], fuse, provider=True, dropout=ratio), "sghmc")


@pytest.mark.parametrize("ratio", RATIOS)
def test_leapfrog_philox_equals_fixed(monkeypatch, ratio):
    _same(_hmc_run(monkeypatch, False, dropout=ratio), _hmc_run(monkeypatch, True, dropout=ratio), "hmc")


@pytest.mark.parametrize("ratio", RATIOS)
def test_sgd_philox_equals_fixed(ratio):
    (pp, lp), (pf, lf) = _sgd_run(dropout=ratio), _sgd_run(provider=True, dropout=ratio)
    for a, b in zip(pp, pf):
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=1e-10)
    for a, b in zip(lp, lf):
        np.testing.assert_allclose(a, b, rtol=1e-10)


@pytest.mark.parametrize("ratio", RATIOS)
def test_sgld_philox_equals_fixed(ratio):
    (pp, lp), (pf, lf) = _sgld_run(dropout=ratio), _sgld_run(provider=True, dropout=ratio)
    for a, b in zip(pp, pf):
        np.testing.assert_allclose(a, b, rtol=1e-8, atol=1e-10)
    for a, b in zip(lp, lf):
        np.testing.assert_allclose(a, b, rtol=1e-10)


def _sgld_chains_call(m, Xd, yd, par, B, C, S, chain0, masks):
    """hmcx_mlp_sgld_chains_run, variant 0, PHILOX noise, S steps from step_base 100 under seed 9; masks None (PHILOX)
    or a device tensor [S, 3, B, n_mid] (FIXED, step s at s·3·B·n_mid).  Returns out_loss [S, C]."""
    nat = _nat()
    rows = np.ascontiguousarray(np.tile(np.arange(0, Xd.shape[0] - B + 1, B, dtype=np.int64), S)[:S])
    eps = np.full(S, sgldref.STEP_SIZE)
    a = nat.MlpSgldChainsArgs()
    a.dtype = m.code
    a.B, a.n_in, a.n_mid, a.n_out, a.n_steps, a.C = B, m.n_in, m.n_mid, m.n_out, S, C
    for i in range(6):
        a.order[i] = i
        a.par.p[i] = par[i].data_ptr()
    a.variant, a.alpha = 0, sgldref.ALPHA
    a.X, a.y = Xd.data_ptr(), yd.data_ptr()
    a.row0, a.eps = rows.ctypes.data_as(nat.c_i64p), eps.ctypes.data_as(nat.c_dblp)
    a.noise_mode, a.mask_mode = nat.NOISE_PHILOX, nat.MLP_MASKS_PHILOX
    a.seed, a.chain0, a.step_base = 9, chain0, 100
    moff = np.arange(S, dtype=np.int64) * 3 * B * m.n_mid
    if masks is not None:
        a.mask_mode, a.masks, a.mask_off = nat.MLP_MASKS_FIXED, masks.data_ptr(), moff.ctypes.data_as(nat.c_i64p)
    out_loss = torch.empty((S, C), dtype=torch.float64, device=m.device)
    a.out_loss = out_loss.data_ptr()
    m.ctx.check(m.ctx.lib.hmcx_mlp_sgld_chains_run(m.ctx.h, ctypes.byref(a)), "hmcx_mlp_sgld_chains_run")
    return out_loss.cpu().numpy()


@pytest.mark.parametrize("ratio", RATIOS)
def test_sgld_chains_philox_equals_fixed(ratio):
    """Chain c of a C = 2 Philox call against the C = 1 call under Philox chain chain0 + c fed that chain's masks (a
    FIXED block is shared by the chains of a call, so the fixed side runs chain by chain)."""
    names = _mlp_mod().MLP_PARAM_NAMES
    f = fx.BY_NAME["w32_b20"]
    X, y, start = sgldref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    m = _model(f.n_in, f.n_mid, f.n_out, torch.float64, alpha=sgldref.ALPHA)
    Xd, yd = m._xy({"X_train": X, "y_train": y})
    C, S = 2, 6
    m.ctx.set_mlp_dropout(ratio)
    starts = [[m._dev(start[k] * (1.0 + 0.25 * c)) for k in names] for c in range(C)]
    par = [torch.stack([starts[c][i] for c in range(C)]).contiguous() for i in range(6)]
    loss = _sgld_chains_call(m, Xd, yd, par, f.B, C, S, 1, None)
    for c in range(C):
        masks = torch.stack([_api_masks(m.ctx, m.dtype, f.B, m.n_mid, 9, 1 + c, 100 + s, SLOT0) for s in range(S)])
        assert abs(float((masks == 0).double().mean()) - ratio) < 0.05
        one = [t.clone().unsqueeze(0).contiguous() for t in starts[c]]
        loss1 = _sgld_chains_call(m, Xd, yd, one, f.B, 1, S, 1 + c, masks)
        np.testing.assert_array_equal(loss[:, c], loss1[:, 0])
        for i in range(6):
            np.testing.assert_array_equal(par[i][c].cpu().numpy(), one[i][0].cpu().numpy())
            assert not np.array_equal(one[i][0].cpu().numpy(), starts[c][i].cpu().numpy())


@pytest.mark.parametrize("ratio", RATIOS)
def test_hmc_chains_philox_equals_fixed(ratio):
    shape, C, S, step_base, chain0 = hmcref.SHAPES[0], 2, 2, 2, 4
    B, n_mid = shape[3], shape[1]
    _, _, start = hmcref.chain_start(shape)
    starts = [{k: (1.0 - 0.1 * c) * v for k, v in start.items()} for c in range(C)]
    n_iter, u = np.array([[0, 3], [2, 1]]), np.random.RandomState(5).rand(S, C)
    runs = []
    for fixed in (False, True):
        g = hc.Call(shape, torch.float64, starts, seed=13, chain0=chain0)
        g.m.ctx.set_mlp_dropout(ratio)
        masks = 'philox'
        if fixed:                                                  # forwards 0 … 6n + 3 of every (step, chain)
            blocks, off = [], np.zeros((S, C), dtype=np.int64)
            for s in range(S):
                for c in range(C):
                    off[s, c] = sum(b.numel() for b in blocks)
                    blocks += [_api_masks(g.m.ctx, g.m.dtype, B, n_mid, 13, chain0 + c, step_base + s, SLOT0 + fw)
                               for fw in range(6 * int(n_iter[s, c]) + 4)]
            masks = (torch.cat([b.reshape(-1) for b in blocks]), off)
        out = g.run(n_iter, u, masks=masks, step_base=step_base)
        runs.append([out[k] for k in ('A', 'acc', 'E', 'loss', 'sumsq')] + [t.cpu().numpy() for t in g.par])
    assert runs[0][1].sum() > 0 and np.all(np.isfinite(runs[0][0]))
    _same(runs[0], runs[1], "hmc chains")


@pytest.mark.parametrize("ratio", RATIOS)
def test_sghmc_chains_philox_equals_fixed(ratio):
    name, C, S, step_base, chain0 = "w32_b20", 2, 2, 2, 4
    n_in, n_mid, n_out, B = scref.dims(name)[:4]
    _, _, start = scref.chain_start(name)
    starts = [{k: (1.0 - 0.1 * c) * v for k, v in start.items()} for c in range(C)]
    n_iter, u = np.array([[0, 3], [2, 1]]), np.random.RandomState(5).rand(S, C)   # the chains' path lengths differ
    runs = []
    for fixed in (False, True):
        g = sc.Call(name, torch.float64, starts, seed=13, chain0=chain0)
        g.m.ctx.set_mlp_dropout(ratio)
        masks = 'philox'
        if fixed:                                                  # forwards 0 … 6n + 1 of every (step, chain)
            masks = [[torch.stack([_api_masks(g.m.ctx, g.m.dtype, B, n_mid, 13, chain0 + c, step_base + s, SLOT0 + fw)
                                   for fw in range(6 * int(n_iter[s, c]) + 2)]).cpu().numpy()
                      for c in range(C)] for s in range(S)]
        out = g.run(n_iter, u, sc.EPS, scref.rows(name, S), masks=masks, step_base=step_base)
        runs.append([out[k] for k in ('A', 'acc', 'E', 'loss', 'nlp')] + [t.cpu().numpy() for t in g.par])
    assert np.all(np.isfinite(runs[0][0]))
    _same(runs[0], runs[1], "sghmc chains")


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("dt,path", [("f64", 1), ("f64", 2), ("f32", 2)])
def test_predictive_philox_equals_fixed(dt, path, ratio):
    r_philox, _ = _predictive_run(DT[dt], path, dropout=ratio)
    r_fixed, masks = _predictive_run(DT[dt], path, fixed=True, dropout=ratio)
    assert abs(float((masks == 0).double().mean()) - ratio) < 0.02
    _same(r_philox, r_fixed, "predictive")


# ----------------------------------------------------------------------------- 3. the default is unchanged
def test_keyword_default_is_byte_identical(monkeypatch):
    """dropout=0.1 against no keyword, after another ratio has run on the device."""
    _nat().context(0).set_mlp_dropout(0.5)
    for run in (lambda **kw: _sghmc_run(torch.float32, **kw), lambda **kw: _sghmc_run(torch.float64, **kw),
                lambda **kw: _hmc_run(monkeypatch, False, **kw), lambda **kw: sum(_sgd_run(**kw), []),
                lambda **kw: sum(_sgld_run(**kw), []), lambda **kw: _predictive_run(torch.float64, 2, **kw)[0],
                lambda **kw: _predictive_run(torch.float32, 1, **kw)[0]):
        a = run()
        _nat().context(0).set_mlp_dropout(0.5)                      # what a model of another ratio leaves behind
        b = run(dropout=0.1)
        _same(a, b, "default")
        for x, y in zip(a, b):
            if isinstance(x, np.ndarray):
                assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("entry", ["sgld", "hmc", "sghmc"])
def test_chain_entries_at_explicit_default_equal_a_fresh_context(entry):
    """The three chain entries under a context set to 0.5 and back to 0.1 through the library against a context that
    never called the setter."""
    nat = _nat()
    runs = []
    for fresh in (True, False):
        ctx = nat.Context(0)
        ctx.bind_stream()
        if not fresh:
            _force_ratio(ctx, 0.5)
            _force_ratio(ctx, 0.1)
        n_iter, u = np.array([[0, 3], [2, 1]]), np.random.RandomState(5).rand(2, 2)
        if entry == "sgld":
            f = fx.BY_NAME["w32_b20"]
            X, y, start = sgldref.problem(f.n_in, f.n_mid, f.n_out, f.B)
            m = _model(f.n_in, f.n_mid, f.n_out, torch.float64, alpha=sgldref.ALPHA)
            Xd, yd = m._xy({"X_train": X, "y_train": y})
            m.ctx = ctx
            par = [torch.stack([m._dev(start[k] * (1.0 + 0.25 * c)) for c in range(2)]).contiguous()
                   for k in _mlp_mod().MLP_PARAM_NAMES]
            out = [_sgld_chains_call(m, Xd, yd, par, f.B, 2, 6, 1, None)] + [t.cpu().numpy() for t in par]
        elif entry == "hmc":
            shape = hmcref.SHAPES[0]
            _, _, start = hmcref.chain_start(shape)
            g = hc.Call(shape, torch.float64, [{k: (1.0 - 0.1 * c) * v for k, v in start.items()} for c in range(2)],
                        seed=13, chain0=4)
            g.m.ctx = ctx
            o = g.run(n_iter, u, step_base=2)
            out = [o[k] for k in ('A', 'acc', 'E', 'loss', 'sumsq')] + [t.cpu().numpy() for t in g.par]
        else:
            _, _, start = scref.chain_start("w32_b20")
            g = sc.Call("w32_b20", torch.float64, [{k: (1.0 - 0.1 * c) * v for k, v in start.items()} for c in range(2)],
                        seed=13, chain0=4)
            g.m.ctx = ctx
            o = g.run(n_iter, u, sc.EPS, scref.rows("w32_b20", 2), step_base=2)
            out = [o[k] for k in ('A', 'acc', 'E', 'loss', 'nlp')] + [t.cpu().numpy() for t in g.par]
        torch.cuda.synchronize()
        runs.append(out)
    _same(runs[0], runs[1], entry)
    for x, y in zip(*runs):
        assert x.tobytes() == y.tobytes()


# ----------------------------------------------------------------------------- 4. two ratios on one device
def _sgld_epochs(models, schedule):
    """One SGLD sample() (three epochs) per entry of `schedule` (indices into models), each model's sampler continuing its own chain;
    returns per model the states after each of its epochs."""
    f = fx.BY_NAME["w32_b20"]
    X, y, start = sgldref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    samplers = [_sgld_sampler(m, start) for m in models]
    states = [[] for _ in models]
    for i in schedule:
        s = samplers[i]
        s.sample(epochs=sgldref.EPOCHS, burnin=sgldref.BURNIN, batch_size=f.B, rng=np.random.RandomState(1), X_train=X,
                 y_train=y)
        states[i] += [v.cpu().numpy() for v in s.last_state.values()]
        samplers[i] = _sgld_sampler(models[i], {k: v.cpu().numpy() for k, v in s.last_state.items()},
                                    seed=5, chain=2 + len(states[i]))
    return states


def test_two_ratios_interleaved_on_one_device():
    f = fx.BY_NAME["w32_b20"]

    def models():
        return [_model(f.n_in, f.n_mid, f.n_out, torch.float64, alpha=sgldref.ALPHA),
                _model(f.n_in, f.n_mid, f.n_out, torch.float64, alpha=sgldref.ALPHA, dropout=0.5)]
    mixed = _sgld_epochs(models(), [0, 1, 0, 1])
    alone0 = _sgld_epochs(models(), [0, 0])
    _nat().context(0).set_mlp_dropout(0.9)                          # neither model's ratio
    alone1 = _sgld_epochs(models(), [1, 1])
    assert len(mixed[0]) == len(mixed[1]) == 12
    _same(mixed[0], alone0[0], "default model")
    _same(mixed[1], alone1[1], "dropout=0.5 model")
    assert not np.array_equal(mixed[0][0], mixed[1][0])


# ----------------------------------------------------------------------------- 5. MC dropout
def test_predict_stochastic_follows_the_models_ratio():
    import _predictive_ref as pr
    c = pr.MULTIBLOCK
    N, T = c.shape[0], 4
    pb = pr.problem(c.shape, c.seed)
    par = pb.par_sets[0]
    a = _model(c.shape[1], c.shape[2], c.shape[3], torch.float64, seed=11, dropout=0.5)
    got = a.predict_stochastic(par, pb.X, prob=True, n_dropout=T)
    b = _model(c.shape[1], c.shape[2], c.shape[3], torch.float64, seed=11, dropout=0.5)
    masks = torch.stack([b.draw_masks(N) for _ in range(T)])
    values = np.unique(masks.cpu().numpy())
    np.testing.assert_array_equal(values, [0.0, 2.0])
    assert abs(float((masks == 0).double().mean()) - 0.5) < 0.02
    want = b.posterior_predictive(par, pb.X, masks=masks, n_dropout=T)
    np.testing.assert_array_equal(got, want.mean)
    default = _model(c.shape[1], c.shape[2], c.shape[3], torch.float64, seed=11)
    assert not np.array_equal(got, default.predict_stochastic(par, pb.X, prob=True, n_dropout=T))


# ----------------------------------------------------------------------------- 6. an invalid ratio
@pytest.mark.parametrize("bad", [1.0, 1.5, -1e-9, float("nan"), float("inf")])
def test_invalid_ratio_raises_and_keeps_the_old_one(bad):
    nat = _nat()
    ctx = nat.context(0)
    ctx.set_mlp_dropout(0.25)
    with pytest.raises(nat.HmcxError, match="mlp dropout: ratio must satisfy"):
        ctx.set_mlp_dropout(bad)
    assert ctx.get_mlp_dropout() == 0.25 and ctx.mlp_dropout == 0.25
    got = _api_masks(ctx, torch.float32, B1, NMID1, **MASK_KEY).cpu().numpy().reshape(-1)
    np.testing.assert_array_equal(got != 0, md.keep_group_host(0.25, MASK_KEY["seed"], N3, MASK_KEY["slot"],
                                                               MASK_KEY["step"], MASK_KEY["chain"]))
