"""Several SGLD chains on the dropout MLP in one device call (sgld(mlp, chains=C): one hmcx_mlp_sgld_chains_run
per epoch, the chains as the problems of batched launches in groups of at most six).

Problems, run length and bounds are those of tests/test_gpu_mlp_sgld.py: the tests/_mlp_fixtures shapes with
N = 6·B + 3, alpha = 0.01, step_size = 0.05, burnin 1 + 2 epochs = 18 steps; float64 parameters and momentum
rtol 1e-8 / atol 1e-10, losses rtol 1e-10; float32 each variable within 2e-5 of the largest entry of the float64
oracle, losses rtol 1e-4.  With Philox noise and masks chain c must equal the one-chain sampler under Philox chain
chain0 + c bit for bit (both dtypes); with injected noise and masks the chains are replicas apart from their
start, and tests/test_mlp_sgld_chains_cpu.py asserts on the oracle alone that the two starts used here end at
least 2e-4 apart.  Measured float32 worst ratios (error / largest entry): DESIGN.md §5.3.
"""
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _mlp_fixtures as fx  # noqa: E402
import _mlp_sgld_ref as ref  # noqa: E402
import test_gpu_mlp_sgld as one  # noqa: E402
import test_mlp_sgld_chains_cpu as cpu_side  # noqa: E402

F32_REL = one.F32_REL
WIDE = fx.Fixture("w32_o40_b20", 16, 32, 40, 20, 0.01, 51, False)      # n_out > 32: layer 3 by k_l3_wide


class ChainRun:
    """One sgld(chains=C).sample on a fixture's problem; loss_trace [18, C], log (the log lines' values) [3, C]."""

    def __init__(self, f, dtype, C, variant="cpu", order=None, provider=None, noise="philox", seed=0, chain=0,
                 keep_every=None, starts=None, epochs=ref.EPOCHS, burnin=ref.BURNIN):
        _, sgld = one._classes()
        X, y, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
        if order is not None:
            start = {k: start[k] for k in order}
        self.X, self.y, self.start = X, y, start
        sp = start if starts is None else {k: np.stack([s[k] for s in starts]) for k in start}
        s = sgld(one._model(f, dtype), sp, step_size=ref.STEP_SIZE, noise=noise, seed=seed, chain=chain, chains=C,
                 variant=variant, keep_every=keep_every)
        if provider == "stream":
            s.mask_provider = ref.stream_masks(f.B, f.n_mid)[0]
        s.out = io.StringIO()
        loss_trace, log = [], []
        inner = s._run_mlp

        def recording(*a, **kw):
            res = inner(*a, **kw)
            loss_trace.extend(s.loss_trace)
            log.extend(row for row in res.ll if not np.isnan(row).any())
            return res
        s._run_mlp = recording
        self.post, self.logp = s.sample(epochs=epochs, burnin=burnin, batch_size=f.B,
                                        rng=np.random.RandomState(ref.NOISE_SEED), X_train=X, y_train=y)
        self.s, self.C = s, C
        self.loss_trace, self.log = np.asarray(loss_trace), np.asarray(log)
        self.lines = ref.parse_lines(s.out.getvalue())
        self.last = {k: v.cpu().numpy() for k, v in s.last_state.items()}
        self.mom = None if s.last_momentum is None else {k: v.cpu().numpy() for k, v in s.last_momentum.items()}
        n = (burnin + epochs) * fx.STEPS_PER_CALL
        assert s.global_step == n and self.loss_trace.shape == (n, C) and self.logp.shape == (C, epochs)
        for k, v in start.items():
            assert self.post[k].shape == (C, epochs) + v.shape and self.last[k].shape == (C,) + v.shape


def _check_chain_f64(g, c, r, variant):
    """Chain c of g against its oracle run r at the float64 bounds."""
    assert list(g.post.keys()) == list(r.post.keys())
    for k in r.post:
        np.testing.assert_allclose(g.post[k][c], r.post[k], rtol=1e-8, atol=1e-10, err_msg=k)
        np.testing.assert_allclose(g.last[k][c], r.q[k], rtol=1e-8, atol=1e-10, err_msg=k)
        if variant == "gpu":
            np.testing.assert_allclose(g.mom[k][c], r.p[k], rtol=1e-8, atol=1e-10, err_msg=k)
    assert (g.mom is None) == (variant != "gpu")
    np.testing.assert_allclose(g.logp[c], r.logp, rtol=1e-10)
    np.testing.assert_allclose(g.loss_trace[:, c], r.loss_trace, rtol=1e-10)
    np.testing.assert_allclose(g.log[:, c], r.log_trace, rtol=1e-10)
    if c == 0:                                                 # the printed lines show chain 0
        one._check_lines(g.lines, r.lines)


def _philox_oracle(g, f, seed, chain, variant, order=None):
    return ref.oracle_run((f.n_in, f.n_mid, f.n_out), f.B, one._philox_mask_fn(g.s.model, f.B, seed, chain), variant,
                          one._philox_source(g.start, seed, chain, 18), order=order)


# ----------------------------------------------------------------------------- 1. per-chain oracle parity, Philox
@pytest.mark.parametrize("variant", ["cpu", "gpu"])
@pytest.mark.parametrize("name", ["w32_b20", "w20_b30"])
def test_f64_every_chain_matches_its_philox_oracle(name, variant):
    f = fx.BY_NAME[name]
    g = ChainRun(f, torch.float64, 3, variant=variant, seed=5, chain=2)
    for c in range(3):
        _check_chain_f64(g, c, _philox_oracle(g, f, 5, 2 + c, variant), variant)


# ----------------------------------------------------------------------------- 2. bit equality with one chain
@pytest.mark.parametrize("variant", ["cpu", "gpu"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("f,C", [(fx.BY_NAME["w32_b20"], 7), (fx.BY_NAME["w96_b36"], 2), (fx.BY_NAME["w256_b4"], 2),
                                 (WIDE, 2)], ids=["w32_b20-C7", "w96_b36-C2", "w256_b4-C2", "n_out40-C2"])
def test_every_chain_equals_the_one_chain_sampler_bitwise(f, C, dtype, variant):
    kw = dict(variant=variant, noise="philox", seed=11, keep_every=3)
    g = ChainRun(f, dtype, C, chain=1, **kw)
    assert g.s.device_draws["/l1/W"].shape[:2] == (C, 4)
    for c in range(C):
        r = one.Run(f, dtype, provider=None, chain=1 + c, **kw)
        for k in r.post:
            np.testing.assert_array_equal(g.post[k][c], r.post[k], err_msg=k)
            np.testing.assert_array_equal(g.last[k][c], r.last[k], err_msg=k)
            np.testing.assert_array_equal(g.s.device_draws[k][c].cpu().numpy(), r.s.device_draws[k].cpu().numpy(),
                                          err_msg=k)
            if variant == "gpu":
                np.testing.assert_array_equal(g.mom[k][c], r.mom[k], err_msg=k)
        np.testing.assert_array_equal(g.logp[c], r.logp)
        np.testing.assert_array_equal(g.loss_trace[:, c], r.loss_trace)
        np.testing.assert_array_equal(g.log[:, c], r.log)
        assert np.all(np.isfinite(r.loss_trace))
        if c == 0:                                             # the printed lines show chain 0
            assert g.lines == r.lines and len(g.lines) > 0


# ----------------------------------------------------------------------------- 3. distinct starts, replicas mode
def _replica_run(f, dtype, variant):
    starts = [ref.problem(f.n_in, f.n_mid, f.n_out, f.B)[2]]
    starts.append(cpu_side.second_start(starts[0]))
    return ChainRun(f, dtype, 2, variant=variant, provider="stream", noise="numpy", starts=starts), starts


@pytest.mark.parametrize("variant", ["cpu", "gpu"])
@pytest.mark.parametrize("name", ["w32_b20", "w20_b30"])
def test_f64_replicas_from_two_starts_match_their_oracles(name, variant):
    f = fx.BY_NAME[name]
    g, starts = _replica_run(f, torch.float64, variant)
    for c in range(2):
        _check_chain_f64(g, c, cpu_side.replica_oracle(f, variant, starts[c]), variant)


@pytest.mark.parametrize("variant", ["cpu", "gpu"])
def test_f32_replicas_within_state_bound(variant):
    f = fx.BY_NAME["w32_b20"]
    g, starts = _replica_run(f, torch.float32, variant)
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - b) / np.abs(b)))  # noqa: E731
    for c in range(2):
        r = cpu_side.replica_oracle(f, variant, starts[c], f32=True)
        ratios = {k: np.abs(g.last[k][c] - r.q[k]).max() / np.abs(r.q[k]).max() for k in r.q}
        post = {k: np.abs(g.post[k][c] - r.post[k]).max() / np.abs(r.post[k]).max() for k in r.q}
        mom = ({k: np.abs(g.mom[k][c] - r.p[k]).max() / np.abs(r.p[k]).max() for k in r.q} if variant == "gpu" else {})
        print("float32 replicas %s chain %d: worst ratio %.3e (%s), posterior %.3e, momentum %.3e; logp rel %.3e; "
              "loss_trace rel %.3e; log lines rel %.3e"
              % (variant, c, max(ratios.values()), max(ratios, key=ratios.get), max(post.values()),
                 max(mom.values()) if mom else float("nan"), rel(g.logp[c], r.logp),
                 rel(g.loss_trace[:, c], r.loss_trace), rel(g.log[:, c], r.log_trace)))
        for k in ratios:
            assert ratios[k] <= F32_REL, (k, ratios[k])
            assert post[k] <= F32_REL, (k, post[k])
            if mom:
                assert mom[k] <= F32_REL, (k, mom[k])
        np.testing.assert_allclose(g.logp[c], r.logp, rtol=1e-4)
        np.testing.assert_allclose(g.loss_trace[:, c], r.loss_trace, rtol=1e-4)
        np.testing.assert_allclose(g.log[:, c], r.log_trace, rtol=1e-4)


# ----------------------------------------------------------------------------- 4. permuted start order
def test_f64_permuted_start_order():
    f = fx.BY_NAME["w32_b20"]
    g = ChainRun(f, torch.float64, 2, order=fx.PERMUTED, seed=5, chain=2)
    assert list(g.post.keys()) == fx.PERMUTED
    for c in range(2):
        r = _philox_oracle(g, f, 5, 2 + c, "cpu", order=fx.PERMUTED)
        _check_chain_f64(g, c, r, "cpu")
        # the noise layout follows the order: the canonical-order oracle is another trajectory
        canon = ref.oracle_run((f.n_in, f.n_mid, f.n_out), f.B, one._philox_mask_fn(g.s.model, f.B, 5, 2 + c), "cpu",
                               one._philox_source(g.start, 5, 2 + c, 18))
        assert ref.state_distance(r.q, canon.q) > 2e-4


# ----------------------------------------------------------------------------- 5. the C ABI
N_STEPS, KEPT = 18, 6


def _chains_args(m, nat, Xd, yd, B, C, n, variant, seed, chain0, step_base):
    a = nat.MlpSgldChainsArgs()
    a.dtype = m.code
    a.B, a.n_in, a.n_mid, a.n_out, a.n_steps, a.C = B, m.n_in, m.n_mid, m.n_out, n, C
    for i in range(6):
        a.order[i] = i
    a.variant, a.alpha = variant, ref.ALPHA
    a.X, a.y = Xd.data_ptr(), yd.data_ptr()
    a.noise_mode, a.mask_mode = nat.NOISE_PHILOX, nat.MLP_MASKS_PHILOX
    a.seed, a.chain0, a.step_base = seed, chain0, step_base
    return a


def _c_run(m, Xd, yd, start, B, C, splits, seed, variant):
    """hmcx_mlp_sgld_chains_run with PHILOX noise and masks over 18 steps, as len(splits) calls that carry par /
    mom and advance step_base and the draw pointers; every third step is kept in one [C][6][shape] buffer per
    variable.  Chain c starts at (1 + c/4)·start.  Returns host arrays (par, mom, out_loss [18, C], draws)."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import MLP_PARAM_NAMES
    par = [torch.stack([m._dev(start[k] * (1.0 + 0.25 * c)) for c in range(C)]).contiguous() for k in MLP_PARAM_NAMES]
    mom = [torch.zeros_like(t) for t in par]
    rows = np.tile(np.arange(0, Xd.shape[0] - B + 1, B, dtype=np.int64), 3)
    assert rows.size == sum(splits) == N_STEPS
    flags = (np.arange(N_STEPS) % 3 == 2).astype(np.uint8)
    draws = [torch.zeros((C, KEPT) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in par]
    out_loss = torch.empty((N_STEPS, C), dtype=torch.float64, device=m.device)
    eps = ref.STEP_SIZE / (1.0 + 0.01 * np.arange(N_STEPS))       # a step size of its own per step
    after_kept = []
    base = 0
    for n in splits:
        row0, ep = np.ascontiguousarray(rows[base:base + n]), np.ascontiguousarray(eps[base:base + n])
        wd = np.ascontiguousarray(flags[base:base + n])
        a = _chains_args(m, nat, Xd, yd, B, C, n, variant, seed, 1, 100 + base)
        a.row0 = row0.ctypes.data_as(nat.c_i64p)
        a.eps = ep.ctypes.data_as(nat.c_dblp)
        d0 = int(flags[:base].sum())
        for i in range(6):
            a.par.p[i] = par[i].data_ptr()
            if variant == 1:
                a.mom.p[i] = mom[i].data_ptr()
            a.draws.p[i] = draws[i][:, min(d0, KEPT - 1):].data_ptr()
        a.want_draw = wd.ctypes.data_as(nat.c_u8p)
        a.draw_stride = KEPT
        a.out_loss = out_loss[base:].data_ptr()
        m.ctx.check(m.ctx.lib.hmcx_mlp_sgld_chains_run(m.ctx.h, ctypes.byref(a)), "hmcx_mlp_sgld_chains_run")
        base += n
        if flags[base - 1]:                                        # the call ended on a kept step
            after_kept.append((int(flags[:base].sum()) - 1, [t.cpu().numpy() for t in par]))
    host = lambda ts: [t.cpu().numpy() for t in ts]  # noqa: E731
    return host(par), host(mom), out_loss.cpu().numpy(), host(draws), after_kept


@pytest.mark.parametrize("variant", [0, 1], ids=["cpu", "gpu"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_one_call_equals_three_calls_bitwise(dtype, variant):
    f = fx.BY_NAME["w96_b36"]
    m = one._model(f, dtype)
    X, y, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    Xd, yd = m._xy({"X_train": X, "y_train": y})
    C = 3
    whole = _c_run(m, Xd, yd, start, f.B, C, [18], seed=9, variant=variant)
    parts = _c_run(m, Xd, yd, start, f.B, C, [7, 5, 6], seed=9, variant=variant)
    for a, b in zip(whole[0] + whole[1] + whole[3], parts[0] + parts[1] + parts[3]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(whole[2], parts[2])
    assert np.all(np.isfinite(whole[2])) and whole[2].shape == (18, C)
    for p, d in zip(whole[0], whole[3]):                          # step 17 is kept: the last draw is the state
        assert d.shape[:2] == (C, KEPT)
        np.testing.assert_array_equal(d[:, -1], p)
        for c in range(C):
            assert not np.array_equal(d[c, 0], d[c, 1]) and not np.array_equal(d[c, 0], d[(c + 1) % C, 0])
    # the draw layout (c·draw_stride + d): the split run's state after a call that ended on kept step d
    ends = [7 + 5, 18]
    assert [d for d, _ in parts[4]] == [int((np.arange(e) % 3 == 2).sum()) - 1 for e in ends if e % 3 == 0]
    for d, state in parts[4]:
        for p, dr in zip(state, whole[3]):
            np.testing.assert_array_equal(dr[:, d], p)
    assert (np.abs(whole[1][0]).max() > 0) == (variant == 1)
    # chain c of the call is the one-chain entry under Philox chain 1 + c
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import MLP_PARAM_NAMES
    for c in range(C):
        sc = {k: start[k] * (1.0 + 0.25 * c) for k in MLP_PARAM_NAMES}
        r = _one_chain_c_run(m, Xd, yd, sc, f.B, seed=9, variant=variant, chain=1 + c)
        for i in range(6):
            np.testing.assert_array_equal(whole[0][i][c], r[0][i])
            np.testing.assert_array_equal(whole[3][i][c], r[3][i])
        np.testing.assert_array_equal(whole[2][:, c], r[2])


def _one_chain_c_run(m, Xd, yd, start, B, seed, variant, chain):
    """test_gpu_mlp_sgld._c_run's single call with the Philox chain of its own."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import MLP_PARAM_NAMES
    par = [m._dev(start[k]).clone() for k in MLP_PARAM_NAMES]
    mom = [torch.zeros_like(t) for t in par]
    rows = np.tile(np.arange(0, Xd.shape[0] - B + 1, B, dtype=np.int64), 3)
    flags = (np.arange(N_STEPS) % 3 == 2).astype(np.uint8)
    draws = [torch.zeros((KEPT,) + tuple(t.shape), dtype=t.dtype, device=t.device) for t in par]
    out_loss = torch.empty(N_STEPS, dtype=torch.float64, device=m.device)
    eps = ref.STEP_SIZE / (1.0 + 0.01 * np.arange(N_STEPS))
    a = nat.MlpSgldArgs()
    a.dtype = m.code
    a.B, a.n_in, a.n_mid, a.n_out, a.n_steps = B, m.n_in, m.n_mid, m.n_out, N_STEPS
    for i in range(6):
        a.order[i] = i
        a.par.p[i] = par[i].data_ptr()
        if variant == 1:
            a.mom.p[i] = mom[i].data_ptr()
        a.draws.p[i] = draws[i].data_ptr()
    a.variant, a.alpha = variant, ref.ALPHA
    a.X, a.y = Xd.data_ptr(), yd.data_ptr()
    a.row0 = rows.ctypes.data_as(nat.c_i64p)
    a.eps = eps.ctypes.data_as(nat.c_dblp)
    a.noise_mode, a.mask_mode = nat.NOISE_PHILOX, nat.MLP_MASKS_PHILOX
    a.seed, a.chain, a.step_base = seed, chain, 100
    a.want_draw = flags.ctypes.data_as(nat.c_u8p)
    a.out_loss = out_loss.data_ptr()
    m.ctx.check(m.ctx.lib.hmcx_mlp_sgld_run(m.ctx.h, ctypes.byref(a)), "hmcx_mlp_sgld_run")
    host = lambda ts: [t.cpu().numpy() for t in ts]  # noqa: E731
    return host(par), host(mom), out_loss.cpu().numpy(), host(draws)


def test_invalid_arguments_leave_the_state_untouched():
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import MLP_PARAM_NAMES
    f = fx.BY_NAME["w32_b20"]
    m = one._model(f, torch.float64)
    X, y, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    Xd, yd = m._xy({"X_train": X, "y_train": y})
    C = 2
    par = [torch.stack([m._dev(start[k])] * C).contiguous() for k in MLP_PARAM_NAMES]
    before = [t.clone() for t in par]
    row0, eps = np.zeros(1, dtype=np.int64), np.full(1, ref.STEP_SIZE)
    out_loss = torch.full((1, C), -7.0, dtype=torch.float64, device=m.device)

    def call(C_=C, chain0=0, step_base=0, n=1, null_par=False):
        a = _chains_args(m, nat, Xd, yd, f.B, C_, n, 0, 3, chain0, step_base)
        a.row0 = row0.ctypes.data_as(nat.c_i64p)
        a.eps = eps.ctypes.data_as(nat.c_dblp)
        for i in range(6):
            a.par.p[i] = par[i].data_ptr()
        if null_par:
            a.par.p[3] = None
        a.out_loss = out_loss.data_ptr()
        return m.ctx.lib.hmcx_mlp_sgld_chains_run(m.ctx.h, ctypes.byref(a))

    for kw in (dict(C_=0), dict(C_=65), dict(chain0=0xFFFFFFFF), dict(step_base=0xFFFFFFFF, n=2), dict(null_par=True)):
        assert call(**kw) < 0, kw
        assert len(m.ctx.lib.hmcx_last_error(m.ctx.h)) > 0
    assert call(n=0) == 0
    torch.cuda.synchronize()
    for t, b in zip(par, before):
        assert torch.equal(t, b)
    assert float(out_loss.min()) == -7.0
    assert call(chain0=0xFFFFFFFE) == 0                           # chain0 + C = 2^32 exactly: the last two chains
    torch.cuda.synchronize()
    assert not torch.equal(par[0][0], before[0][0]) and not torch.equal(par[0][0], par[0][1])
    assert np.all(np.isfinite(out_loss.cpu().numpy())) and float(out_loss.min()) > 0


# ----------------------------------------------------------------------------- 6. draws: predictive, diagnostics
def test_draws_feed_the_predictive_and_the_chain_diagnostics():
    from dropout_hamiltonian_montecarlo_amd import diagnostics
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    f = fx.BY_NAME["w32_b20"]
    g = ChainRun(f, torch.float64, 4, seed=3, keep_every=1)
    d = g.s.device_draws
    host = {k: v.cpu().numpy() for k, v in d.items()}
    for k, shape in g.s.model.shapes.items():
        assert d[k].is_cuda and tuple(d[k].shape) == (4, 12) + shape
        np.testing.assert_array_equal(host[k][:, [5, 11]], g.post[k])         # the epochs' last states
    m = g.s.model
    dev = m.posterior_predictive(d, g.X, g.y, masks="off")
    hst = m.posterior_predictive(host, g.X, g.y, masks="off")
    for name, a, b in zip(dev._fields, dev, hst):
        assert np.all(np.isfinite(a)), name
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert dev.draw_nll.shape == (48,)
    diag = g.s.chain_diagnostics()
    assert list(diag.keys()) == list(d.keys())
    for k, (sr, es) in diag.items():
        assert sr.shape == g.s.model.shapes[k] == es.shape
        for got, want in ((sr, diagnostics.split_rhat(host[k])), (es, diagnostics.ess(host[k]))):
            assert np.array_equal(np.isnan(got), np.isnan(want)), k
            ok = ~np.isnan(want)
            assert ok.any()
            np.testing.assert_allclose(got[ok], want[ok], rtol=1e-9, err_msg=k)
    only = g.s.chain_diagnostics(vars=["/l3/b"])
    assert list(only.keys()) == ["/l3/b"]
    np.testing.assert_array_equal(only["/l3/b"][0], diag["/l3/b"][0])
    with pytest.raises(HmcxError):
        ChainRun(f, torch.float64, 2, keep_every=6).s.chain_diagnostics()     # T = 2 draws per chain
    with pytest.raises(HmcxError):
        ChainRun(f, torch.float64, 2).s.chain_diagnostics()                   # no draws


# ----------------------------------------------------------------------------- 7. independence
def test_chains_differ_and_follow_the_seed():
    f = fx.BY_NAME["w32_b20"]
    g = ChainRun(f, torch.float64, 3, seed=5)
    h = ChainRun(f, torch.float64, 3, seed=6)
    w = g.last["/l1/W"]
    for c in range(3):
        assert not np.array_equal(w[c], w[(c + 1) % 3])
        assert not np.array_equal(w[c], h.last["/l1/W"][c])
        assert not np.array_equal(g.loss_trace[:, c], g.loss_trace[:, (c + 1) % 3])
    g2 = ChainRun(f, torch.float64, 3, seed=5)
    for k in g.last:
        np.testing.assert_array_equal(g.last[k], g2.last[k])
