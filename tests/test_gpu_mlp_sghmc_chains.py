"""SGHMC on the dropout MLP, C chains per device call (hmcx_mlp_sghmc_chains_run; sghmc(mlp, chains=C) with
noise='philox').

Fixtures, recipe and preconditions: tests/_mlp_sghmc_chains_ref.py and tests/test_mlp_sghmc_chains_cpu.py (three
shapes, three chains, 3 epochs × 6 steps, n_iter 0 .. 4, accepts and rejects, every decision at least 1e-3 from
flipping: smallest |dE − ln u| 0.28).  Bounds, float64 against the restatement (test_gpu_mlp_hmc_chains.py's): flags
exact, A rtol 1e-9 / atol 1e-12, loss and nlp rtol 1e-10, states rtol 1e-8 / atol 1e-10, E within n·2⁻⁵³·Σ|terms| (n
the longest sum, the largest variable) plus 1e-10·|loss| of that energy's loss.  With PHILOX noise and masks every
comparison between calls is bit for bit.

float32 against the float64 restatement on the same float32-rounded noise and mask values: flags exact, each variable
within F32_TOL of its largest entry — F32_MARGIN × the worst error measured on an MI355X over the three fixtures, never
above F32_CAP (tests/_mlp_cases.py).  Measured worst (error / largest entry) per fixture, 18 steps: w32_b20 3.435e-7,
w96_b36 2.132e-7, w20_b30 1.104e-7; A differed by at most 4.4e-6 and no flag flipped.

Against the one-chain entry (hmcx_mlp_sghmc_run, fused launches off, w20_b30, float64, the same BUFFER noise and FIXED
masks): every output and the state came out bit-identical on the MI355X, so the test asserts that.
"""
import ctypes
import functools
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _mlp_cases as mc  # noqa: E402
import _mlp_fixtures as fx  # noqa: E402
import _mlp_sghmc_chains_ref as ref  # noqa: E402
import test_mlp_sghmc_chains_checks_cpu as checks  # noqa: E402

F32_WORST = 3.435e-7                                         # measured, see above
F32_TOL = min(mc.F32_MARGIN * F32_WORST, mc.F32_CAP)
NAMES = ref.NAMES
DT = {"f64": torch.float64, "f32": torch.float32}


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    return _native


def _model(name, dtype, seed=0):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp
    f = fx.BY_NAME[name]
    return mlp({"alpha": f.alpha}, f.n_in, f.n_mid, f.n_out, dtype=dtype, device="cuda:0", seed=seed)


def _nvars(name):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp_param_shapes
    return [int(np.prod(s)) for s in mlp_param_shapes(*ref.dims(name)[:3]).values()]


class Call:
    """One hmcx_mlp_sghmc_chains_run.  starts: per chain {name: array}; n_iter, u [S, C]; eps, row0 [S]; noise None
    (PHILOX) or per (step, chain) host blocks [S][C] of P·(n + 1) normals in `order` layout (BUFFER); masks 'philox',
    None or per (step, chain) host blocks [S][C] of [6n + 2, 3, B, n_mid] (FIXED).  The state is carried in self.par,
    so a second run() continues the first."""
    entry = "hmcx_mlp_sghmc_chains_run"

    def __init__(self, name, dtype, starts, order=NAMES, seed=7, chain0=0):
        self.nat = _nat()
        self.name, self.m, self.C = name, _model(name, dtype), len(starts)
        X, y, _ = ref.chain_start(name)
        self.X, self.y = self.m._xy(dict(X_train=X, y_train=y))
        self.par = [self.m._dev(np.stack([s[k] for s in starts])).contiguous() for k in NAMES]
        self.order = [NAMES.index(k) for k in order]
        self.seed, self.chain0 = seed, chain0

    def args(self, n_iter, u, eps, row0, noise=None, masks='philox', step_base=0, want_draw=None, draws=None,
             draw_stride=0, draw0=0):
        nat, m, C = self.nat, self.m, self.C
        n_iter = np.ascontiguousarray(n_iter, dtype=np.int32).reshape(-1, C)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, C)
        S = n_iter.shape[0]
        dev = m.device
        k = types_keep = {}
        k['eps'] = np.ascontiguousarray(np.broadcast_to(np.asarray(eps, dtype=np.float64), (S,)))
        k['row0'] = np.ascontiguousarray(row0, dtype=np.int64)
        assert k['row0'].shape == (S,)
        k['n_iter'], k['u'] = n_iter, u
        a = nat.MlpSghmcChainsArgs()
        a.dtype, a.B, a.n_in, a.n_mid, a.n_out, a.n_steps, a.C = m.code, ref.dims(self.name)[3], m.n_in, m.n_mid, m.n_out, S, C
        for i, v in enumerate(self.order):
            a.order[i] = v
        a.alpha = m.alpha
        a.X, a.y = self.X.data_ptr(), self.y.data_ptr()
        a.row0 = k['row0'].ctypes.data_as(nat.c_i64p)
        a.eps = k['eps'].ctypes.data_as(nat.c_dblp)
        a.n_iter = n_iter.ctypes.data_as(nat.c_i32p)
        a.u_accept = u.ctypes.data_as(nat.c_dblp)

        def blocks(bl):
            off, o = np.zeros((S, C), dtype=np.int64), 0
            flat = []
            for s in range(S):
                for c in range(C):
                    b = np.asarray(bl[s][c], dtype=np.float64).reshape(-1)
                    off[s, c] = o
                    o += b.size
                    flat.append(b)
            return np.concatenate(flat), off
        a.noise_mode = nat.NOISE_PHILOX
        if noise is not None:
            flat, k['noff'] = blocks(noise)
            k['noise'] = torch.from_numpy(flat).to(dev)
            a.noise_mode, a.noise = nat.NOISE_BUFFER, k['noise'].data_ptr()
            a.noise_off = k['noff'].ctypes.data_as(nat.c_i64p)
        if masks is None:
            a.mask_mode = nat.MLP_MASKS_NONE
        elif isinstance(masks, str):
            a.mask_mode = nat.MLP_MASKS_PHILOX
        else:
            flat, k['moff'] = blocks(masks)
            k['masks'] = m._dev(flat).contiguous()
            a.mask_mode, a.masks = nat.MLP_MASKS_FIXED, k['masks'].data_ptr()
            a.mask_off = k['moff'].ctypes.data_as(nat.c_i64p)
        a.seed, a.chain0, a.step_base = self.seed, self.chain0, step_base
        for i, t in enumerate(self.par):
            a.par.p[i] = t.data_ptr()
        f64 = dict(dtype=torch.float64, device=dev)
        o = dict(A=torch.full((S, C), np.nan, **f64), acc=torch.full((S, C), -1, dtype=torch.int32, device=dev),
                 E=torch.full((S, C, 2), np.nan, **f64), loss=torch.full((S, C), np.nan, **f64),
                 nlp=torch.full((S, C), np.nan, **f64))
        a.out_A, a.out_accepted, a.out_E = o['A'].data_ptr(), o['acc'].data_ptr(), o['E'].data_ptr()
        a.out_loss, a.out_nlp = o['loss'].data_ptr(), o['nlp'].data_ptr()
        if want_draw is not None:
            k['wd'] = np.ascontiguousarray(want_draw, dtype=np.uint8)
            a.want_draw, a.draw_stride = k['wd'].ctypes.data_as(nat.c_u8p), draw_stride
            for i, t in enumerate(draws):
                a.draws.p[i] = t.data_ptr() + draw0 * t[0, 0].numel() * t.element_size()
        return a, o, types_keep

    def run(self, *args, **kw):
        a, o, keep = self.args(*args, **kw)
        ctx = self.m.ctx
        ctx.check(getattr(ctx.lib, self.entry)(ctx.h, ctypes.byref(a)), self.entry)
        torch.cuda.synchronize()
        del keep
        return {k: v.cpu().numpy() for k, v in o.items()}

    def state(self, c):
        return {k: t[c].cpu().numpy() for k, t in zip(NAMES, self.par)}

    def buffers(self, T):
        return [torch.zeros((self.C, T) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in self.par]


@functools.lru_cache(maxsize=None)
def _restated(name, c, order, f32):
    return ref.restate_chain(name, c, list(order) if order else None, rnd=_f32 if f32 else None)


def _fixed_inputs(name, chains, order=None, f32=False):
    """BUFFER noise and FIXED mask blocks [S][C], n_iter and u [S, C], eps and row0 [S], the starts and the
    restatements of the listed chains of the three-chain recipe (chain j of the call = recipe chain chains[j]).  f32:
    noise and mask values (1/0.9) are rounded through float32 for the device and the restatement alike; X and the
    starts are float32-exact already (fx.problem, and the start scales ±1 and 0.5 keep them so)."""
    rnd = _f32 if f32 else np.asarray
    S = ref.NSTEPS
    runs = [ref.oracle_run(name, c, order) for c in chains]
    n_iter = np.stack([r.n_iter for r in runs], axis=1)
    u = np.stack([r.u for r in runs], axis=1)
    for r in runs:                                              # the chains share the steps' sizes
        np.testing.assert_array_equal(r.eps, runs[0].eps)
    zs = [ref.noise_blocks(name, c, runs[j].n_iter) for j, c in enumerate(chains)]
    ones = [ref.mask_of(name, c) for c in chains]
    noise = [[rnd(zs[j][s]) for j in range(len(chains))] for s in range(S)]
    masks = [[np.stack([rnd(ones[j](s, f)) for f in range(6 * int(n_iter[s, j]) + 2)]) for j in range(len(chains))]
             for s in range(S)]
    starts = [ref.chain_start(name, c, order)[2] for c in chains]
    rs = [_restated(name, c, tuple(order) if order else None, f32) for c in chains]
    return n_iter, u, runs[0].eps, ref.rows(name), noise, masks, starts, rs


# ----------------------------------------------------------------------------- 1. float64 against the restatement
def _check_f64(name, chains, order=None):
    n_iter, u, eps, row0, noise, masks, starts, rs = _fixed_inputs(name, chains, order)
    g = Call(name, torch.float64, starts, order=order or NAMES)
    T = ref.NSTEPS
    draws = g.buffers(T)
    out = g.run(n_iter, u, eps, row0, noise=noise, masks=masks, want_draw=np.ones(T), draws=draws, draw_stride=T)
    nlong = max(_nvars(name))
    for j in range(len(chains)):
        r = rs[j]
        np.testing.assert_array_equal(out['acc'][:, j], [int(s.accepted) for s in r])
        np.testing.assert_allclose(out['A'][:, j], [s.A for s in r], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(out['loss'][:, j], [s.loss for s in r], rtol=1e-10)
        np.testing.assert_allclose(out['nlp'][:, j], [s.nlp for s in r], rtol=1e-10)
        worst = 0.0
        for s in range(T):
            for w in (0, 1):                                   # E_current, E_new
                tol = nlong * 2.0 ** -53 * r[s].terms[w] + 1e-10 * r[s].eloss[w]
                d = abs(out['E'][s, j, w] - r[s].E[w])
                worst = max(worst, d / tol)
                assert d <= tol, (s, j, w, d, tol)
            for i, k in enumerate(NAMES):
                np.testing.assert_allclose(draws[i][j, s].cpu().numpy(), r[s].q[k], rtol=1e-8, atol=1e-10, err_msg=k)
        print("%s chain %d: worst |dE| / bound %.3e" % (name, chains[j], worst))
        for k in NAMES:
            np.testing.assert_allclose(g.state(j)[k], r[-1].q[k], rtol=1e-8, atol=1e-10, err_msg=k)


@pytest.mark.parametrize("chains", [(0,), (0, 1, 2)], ids=["C1", "C3"])
@pytest.mark.parametrize("name", ref.SHAPES)
def test_f64_matches_the_restatement(name, chains):
    _check_f64(name, chains)


def test_f64_matches_the_restatement_in_permuted_order():
    _check_f64("w32_b20", (0,), fx.PERMUTED)


# ----------------------------------------------------------------------------- 2. float32
@pytest.mark.parametrize("name", ref.SHAPES)
def test_f32_matches_the_restatement(name):
    n_iter, u, eps, row0, noise, masks, starts, rs = _fixed_inputs(name, (0,), f32=True)
    r = rs[0]
    assert [s.accepted for s in r] == [t['accepted'] for t in ref.oracle_run(name).trace]   # rounding flips nothing
    assert min(ref.margins(r, u[:, 0])) >= 1e-3
    g = Call(name, torch.float32, starts)
    T = ref.NSTEPS
    draws = g.buffers(T)
    out = g.run(n_iter, u, eps, row0, noise=noise, masks=masks, want_draw=np.ones(T), draws=draws, draw_stride=T)
    worst = 0.0
    for s in range(T):
        for i, k in enumerate(NAMES):
            worst = max(worst, np.abs(draws[i][0, s].cpu().numpy() - r[s].q[k]).max() / np.abs(r[s].q[k]).max())
    print("%s float32 worst state error / largest entry: %.3e; worst |dA| %.3e; tolerance %.3e"
          % (name, worst, np.abs(out['A'][:, 0] - [s.A for s in r]).max(), F32_TOL))
    np.testing.assert_array_equal(out['acc'][:, 0], [int(s.accepted) for s in r])
    for s in range(T):
        for i, k in enumerate(NAMES):
            assert np.abs(draws[i][0, s].cpu().numpy() - r[s].q[k]).max() <= F32_TOL * np.abs(r[s].q[k]).max(), (s, k)
    np.testing.assert_allclose(out['loss'][:, 0], [s.loss for s in r], rtol=1e-4)


# ----------------------------------------------------------------------------- 3. against the one-chain entry
def test_f64_matches_the_one_chain_entry_unfused():
    """hmcx_mlp_sghmc_run with the fused layer-2/3 launches off, on the shape where k_fwdr is not eligible: the same
    BUFFER noise, FIXED masks, n_iter and u as chain 0.  The two entries run the same GEMM bodies and the same
    element-wise statements here, and the results are bit-identical."""
    name = "w20_b30"
    nat = _nat()
    n_iter, u, eps, row0, noise, masks, starts, rs = _fixed_inputs(name, (0,))
    S = ref.NSTEPS
    g = Call(name, torch.float64, starts)
    out = g.run(n_iter, u, eps, row0, noise=noise, masks=masks)
    h = Call(name, torch.float64, starts)                       # the one-chain call on its own copy of the start
    a, o, keep = h.args(n_iter, u, eps, row0, noise=noise, masks=masks)
    b = nat.MlpSghmcArgs()
    for f in ("dtype", "B", "n_in", "n_mid", "n_out", "n_steps", "alpha", "X", "y", "row0", "eps", "n_iter", "u_accept",
              "noise_mode", "noise", "noise_off", "masks", "mask_off", "seed", "step_base", "out_A", "out_accepted",
              "out_loss", "out_nlp", "out_E"):
        setattr(b, f, getattr(a, f))
    for i in range(6):
        b.order[i] = a.order[i]
        b.par.p[i] = a.par.p[i]
    b.mask_mode, b.chain = nat.NOISE_BUFFER, 0
    ctx = h.m.ctx
    fuse = ctx.mlp_fuse
    ctx.set_mlp_fuse(False)
    try:
        ctx.check(ctx.lib.hmcx_mlp_sghmc_run(ctx.h, ctypes.byref(b)), "hmcx_mlp_sghmc_run")
        torch.cuda.synchronize()
    finally:
        ctx.set_mlp_fuse(fuse)
    one = {k: v.cpu().numpy() for k, v in o.items()}
    del keep
    assert 0 < out['acc'].sum() < S
    for k in ('acc', 'A', 'loss', 'nlp', 'E'):                  # measured bit-identical, so that is what is asserted
        np.testing.assert_array_equal(out[k], one[k], err_msg=k)
    for k in NAMES:
        np.testing.assert_array_equal(g.state(0)[k], h.state(0)[k], err_msg=k)
        assert not np.array_equal(g.state(0)[k], np.asarray(starts[0][k])), k


# ----------------------------------------------------------------------------- 4. chain invariance
def _ragged(S, C, seed):
    """n_iter [S, C] with a 0 and a value >= 3 in every chain, the chains' path lengths differing step by step."""
    rs = np.random.RandomState(seed)
    n_iter = rs.randint(0, 4, (S, C))
    for c in range(C):
        n_iter[c % S, c] = 0
        n_iter[(c + 1) % S, c] = 3 + c % 2
    return n_iter, rs.rand(S, C)


EPS = 0.005


def _philox_run(name, dt, starts, n_iter, u, chain0, masks='philox'):
    S = n_iter.shape[0]
    g = Call(name, DT[dt], starts, seed=13, chain0=chain0)
    draws = g.buffers(S)
    row0 = ref.rows(name, S)
    out = g.run(n_iter, u, EPS, row0, masks=masks, step_base=2, want_draw=np.ones(S), draws=draws, draw_stride=S)
    out['draws'] = [t.cpu().numpy() for t in draws]
    out['state'] = [t.cpu().numpy() for t in g.par]
    return out


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name,C", [("w32_b20", 7), ("w96_b36", 2), ("w20_b30", 2)])
def test_every_chain_equals_the_one_chain_call_bitwise(name, C, dt):
    S = 3
    _, _, start = ref.chain_start(name)
    starts = [{k: (1.0 - 0.1 * c) * v for k, v in start.items()} for c in range(C)]
    n_iter, u = _ragged(S, C, 5)
    assert all((n_iter[:, c] == 0).any() and (n_iter[:, c] >= 3).any() for c in range(C))
    g = _philox_run(name, dt, starts, n_iter, u, 4)
    assert 0 < g['acc'].sum() and np.all(np.isfinite(g['A']))
    for c in range(C):
        r = _philox_run(name, dt, [starts[c]], n_iter[:, c:c + 1], u[:, c:c + 1], 4 + c)
        for key in ('A', 'acc', 'E', 'loss', 'nlp'):
            np.testing.assert_array_equal(g[key][:, c], r[key][:, 0], err_msg="%s chain %d" % (key, c))
        for key in ('draws', 'state'):
            for i, k in enumerate(NAMES):
                np.testing.assert_array_equal(g[key][i][c], r[key][i][0], err_msg="%s %s chain %d" % (key, k, c))
    assert not np.array_equal(g['A'][:, 0], g['A'][:, 1])       # the chains are different runs


# ----------------------------------------------------------------------------- 5. split invariance
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_call_equals_its_splits_bitwise(dt):
    name, C, S = "w32_b20", 3, 6
    _, _, start = ref.chain_start(name)
    starts = [{k: (1.0 + 0.2 * c) * v for k, v in start.items()} for c in range(C)]
    n_iter, u = _ragged(S, C, 9)
    want_draw = np.array([0, 1, 0, 1, 0, 1], dtype=np.uint8)
    T = int(want_draw.sum())
    row0 = np.asarray(ref.rows(name, S))
    eps = EPS / (1.0 + 0.1 * np.arange(S))

    def run(splits):
        g = Call(name, DT[dt], starts, seed=21, chain0=1)
        draws = g.buffers(T)
        outs, s0, d0 = [], 0, 0
        for n in splits:
            sl = slice(s0, s0 + n)
            outs.append(g.run(n_iter[sl], u[sl], eps[sl], row0[sl], step_base=10 + s0, want_draw=want_draw[sl],
                              draws=draws, draw_stride=T, draw0=d0))
            s0, d0 = s0 + n, d0 + int(want_draw[sl].sum())
        out = {k: np.concatenate([o[k] for o in outs], axis=0) for k in outs[0]}
        out['draws'] = [t.cpu().numpy() for t in draws]
        out['state'] = [t.cpu().numpy() for t in g.par]
        return out
    a = run([6])
    assert np.all(np.isfinite(a['loss'])) and a['acc'].min() >= 0 and 0 < a['acc'].sum()
    for splits in ([1, 5], [2, 2, 2]):
        b = run(splits)
        for key in ('A', 'acc', 'E', 'loss', 'nlp'):
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        for key in ('draws', 'state'):
            for i in range(6):
                np.testing.assert_array_equal(a[key][i], b[key][i], err_msg=key)
    assert not np.array_equal(a['draws'][0][0, 0], a['draws'][0][0, -1])


# ----------------------------------------------------------------------------- 6. no masks, no steps
def test_masks_none_runs_and_zero_steps_do_nothing():
    name, C, S = "w20_b30", 2, 3
    _, _, start = ref.chain_start(name)
    starts = [start, {k: 0.5 * v for k, v in start.items()}]
    n_iter, u = _ragged(S, C, 3)
    u = np.zeros_like(u)                                         # every proposal is committed: the states move
    a = _philox_run(name, "f64", starts, n_iter, u, 0, masks=None)
    b = _philox_run(name, "f64", starts, n_iter, u, 0)
    assert np.all(np.isfinite(a['A'])) and np.all(np.isfinite(a['loss'])) and a['acc'].min() >= 0
    assert not np.array_equal(a['loss'], b['loss']) and not np.array_equal(a['state'][0], b['state'][0])
    # without dropout the two energy forwards of an n = 0 step see the same network: E_new = E_current, A = 1
    for s, c in zip(*np.nonzero(n_iter == 0)):
        assert a['A'][s, c] == 1.0 and a['E'][s, c, 0] == a['E'][s, c, 1]
        assert b['E'][s, c, 0] != b['E'][s, c, 1]
    g = Call(name, torch.float64, starts)
    before = [t.clone() for t in g.par]
    args, o, keep = g.args(n_iter, u, EPS, ref.rows(name, S))
    args.n_steps = 0
    assert g.m.ctx.lib.hmcx_mlp_sghmc_chains_run(g.m.ctx.h, ctypes.byref(args)) == 0
    torch.cuda.synchronize()
    assert torch.isnan(o['A']).all() and torch.isnan(o['loss']).all() and (o['acc'] == -1).all()
    assert all(torch.equal(t, x) for t, x in zip(g.par, before))
    del keep


# ----------------------------------------------------------------------------- 7. invalid arguments
def test_invalid_arguments_leave_the_state_untouched():
    """The cases of tests/test_mlp_sghmc_chains_checks_cpu.py against the entry point: its status and message, nothing
    launched, par bit-identical."""
    name, C, S = "w32_b20", 2, 3
    nat = _nat()
    _, _, start = ref.chain_start(name)
    g = Call(name, torch.float64, [start] * C)
    before = [t.clone() for t in g.par]
    lib, h = g.m.ctx.lib, g.m.ctx.h
    n_iter, u = np.ones((S, C), dtype=np.int32), np.full((S, C), 0.5)
    P = sum(_nvars(name))
    noise = [[np.zeros(2 * P)] * C for _ in range(S)]
    masks = [[np.ones((8, 3, ref.dims(name)[3], ref.dims(name)[1]))] * C for _ in range(S)]
    draws = g.buffers(S)
    neg = np.ones((S, C), dtype=np.int32)
    neg[-1, -1] = -1
    table = {r[0]: (r[2], r[3]) for r in checks.ROWS}
    cases = {
        "C 0": lambda a: setattr(a, "C", 0),
        "C 65": lambda a: setattr(a, "C", 65),
        "order repeats": lambda a: a.order.__setitem__(0, a.order[1]),
        "n_iter < 0 in the last entry": lambda a: setattr(a, "n_iter", neg.ctypes.data_as(nat.c_i32p)),
        "chain0 + C wraps": lambda a: setattr(a, "chain0", 0xFFFFFFFF),
        "step_base + n_steps wraps": lambda a: setattr(a, "step_base", 0xFFFFFFFE),
        "draw_stride below the flagged steps": lambda a: setattr(a, "draw_stride", 2),
        "BUFFER noise without noise_off": lambda a: setattr(a, "noise_off", None),
        "FIXED masks without mask_off": lambda a: setattr(a, "mask_off", None),
        "null out_loss": lambda a: setattr(a, "out_loss", None),
    }
    for case, mutate in cases.items():
        a, o, keep = g.args(n_iter, u, EPS, ref.rows(name, S), noise=noise, masks=masks, want_draw=np.ones(S), draws=draws,
                            draw_stride=S)
        mutate(a)
        rc = lib.hmcx_mlp_sghmc_chains_run(h, ctypes.byref(a))
        msg = lib.hmcx_last_error(h)
        torch.cuda.synchronize()
        status, text = table[case]
        assert status < 0 and rc == status and msg == text.encode(), (case, rc, msg)
        for t, b in zip(g.par, before):
            assert torch.equal(t, b), case
        assert torch.isnan(o['A']).all(), case                  # nothing was launched
        del keep
    assert lib.hmcx_mlp_sghmc_chains_run(None, None) == -1 and lib.hmcx_mlp_sghmc_chains_run(h, None) < 0
    # the valid block runs
    a, o, keep = g.args(n_iter, u, EPS, ref.rows(name, S), noise=noise, masks=masks, want_draw=np.ones(S), draws=draws,
                        draw_stride=S)
    assert table["valid"][0] == 0 and lib.hmcx_mlp_sghmc_chains_run(h, ctypes.byref(a)) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(o['A']).all()


# ----------------------------------------------------------------------------- 8. the Python route
def _sampler(name, dtype, start, **kw):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
    s = sghmc(_model(name, dtype), start, noise='philox', **fx.KW, **kw)
    s.out, s.trace = io.StringIO(), []
    return s


def test_python_route_runs_the_chains_in_one_call_per_epoch():
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    name, nat = "w32_b20", _nat()
    f = fx.BY_NAME[name]
    C, epochs, burnin, n = 3, 2, 1, fx.STEPS_PER_CALL
    X, y, start = ref.chain_start(name)
    s = _sampler(name, torch.float32, start, chains=C, seed=3, chain=3, keep_every=2)
    post, logp = s.sample(epochs=epochs, burnin=burnin, batch_size=f.B, X_train=X, y_train=y)
    T = epochs * n // 2
    assert list(post.keys()) == list(start.keys()) and logp.shape == (C, epochs) and np.all(np.isfinite(logp))
    d = s.device_draws
    for k, v in start.items():
        assert post[k].shape == (C, epochs) + v.shape and d[k].shape == (C, T) + v.shape and d[k].is_cuda
        assert s.last_state[k].shape == (C,) + v.shape and s.last_state[k].is_cuda
        np.testing.assert_array_equal(post[k][:, -1], s.last_state[k].cpu().numpy())
        np.testing.assert_array_equal(post[k][:, -1], d[k][:, -1].cpu().numpy())       # step 12 is a kept step
        np.testing.assert_array_equal(post[k][:, 0], d[k][:, n // 2 - 1].cpu().numpy())
    S = (burnin + epochs) * n
    assert len(s.trace) == S
    for t in s.trace:
        assert all(np.shape(t[key]) == (C,) for key in ('L', 'A', 'accepted')) and np.shape(t['E']) == (C, 2)
    lines = s.out.getvalue().splitlines()
    assert lines[0] == 'start burnin' and 'start sampling' in lines
    assert sum(ln.startswith("epoch") for ln in lines) == epochs        # log_every 10: step 0 of an epoch of 6
    # chain c is the C entry called with C = 1 under chain 3 + c: the schedule is philox_schedule's one-chain stream
    eps = np.array([t['eps'] for t in s.trace])
    row0 = ref.rows(name, S)
    for c in range(C):
        L, n_iter, u = nat.philox_schedule(3, 3 + c, 1, 0, fx.KW['path_length'], eps)
        np.testing.assert_array_equal(L[:, 0], [t['L'][c] for t in s.trace])
        g = Call(name, torch.float32, [start], seed=3, chain0=3 + c)
        outs = []
        for i in range(burnin + epochs):
            sl = slice(i * n, (i + 1) * n)
            outs.append(g.run(n_iter[sl], u[sl], eps[sl], row0[sl], step_base=i * n))
            if i >= burnin:
                for k in start:
                    np.testing.assert_array_equal(post[k][c, i - burnin], g.state(0)[k].astype(np.float64), err_msg=k)
                np.testing.assert_array_equal(logp[c, i - burnin], outs[-1]['nlp'][-1, 0])
        out = {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
        np.testing.assert_array_equal(out['A'][:, 0], [t['A'][c] for t in s.trace])
        np.testing.assert_array_equal(out['acc'][:, 0].astype(bool), [t['accepted'][c] for t in s.trace])
        np.testing.assert_array_equal(out['E'][:, 0], [t['E'][c] for t in s.trace])
        # the chains == 1 sampler runs other kernels (hmcx_mlp_sghmc_run): the float32 tolerance of the restatement test
        s1 = _sampler(name, torch.float32, start, seed=3, chain=3 + c)
        p1, l1 = s1.sample(epochs=epochs, burnin=burnin, batch_size=f.B, X_train=X, y_train=y)
        assert [t['L'] for t in s1.trace] == L[:, 0].tolist()
        mg = min(abs((t['E'][0] - t['E'][1]) - np.log(uu)) for t, uu in zip(s1.trace, u[:, 0]))
        print("chain %d: one-chain sampler accepts %d of %d, smallest |dE - ln u| %.3g, worst state error / largest "
              "entry %.3e" % (c, sum(t['accepted'] for t in s1.trace), S, mg,
                              max(np.abs(p1[k] - post[k][c]).max() / np.abs(post[k][c]).max() for k in start)))
        assert [t['accepted'] for t in s1.trace] == [bool(t['accepted'][c]) for t in s.trace]
        for k in start:
            assert np.abs(p1[k] - post[k][c]).max() <= F32_TOL * np.abs(post[k][c]).max(), (c, k)
    assert not np.array_equal(post['/l1/W'][0], post['/l1/W'][1])
    # diagnostics and the predictive read the device draws
    diag = s.chain_diagnostics()
    assert list(diag.keys()) == list(d.keys()) and T >= 4
    for k, (sr, es) in diag.items():
        sr, es = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in (sr, es))
        assert sr.shape == s.model.shapes[k] == es.shape
        assert np.all(np.isfinite(sr)) and np.all(np.isfinite(es)), k
    host = {k: v.cpu().numpy() for k, v in d.items()}
    ptrs = {k: v.data_ptr() for k, v in d.items()}
    dev = s.model.posterior_predictive(d, X, y, masks="off")
    hst = s.model.posterior_predictive(host, X, y, masks="off")
    assert {k: v.data_ptr() for k, v in s.device_draws.items()} == ptrs
    for fname, a, b in zip(dev._fields, dev, hst):
        assert np.all(np.isfinite(a)), fname
        np.testing.assert_array_equal(a, b, err_msg=fname)
    # masks='off' selects NONE: another run, and deterministic energies on the n = 0 steps
    s2 = _sampler(name, torch.float32, start, chains=C, seed=3, chain=3)
    p2, _ = s2.sample(epochs=1, burnin=0, batch_size=f.B, X_train=X, y_train=y, masks='off')
    assert s2.device_draws is None and not np.array_equal(p2['/l1/W'][:, 0], post['/l1/W'][:, 0])
    for t in s2.trace:
        for c in range(C):
            if t['L'][c] <= 1:
                assert t['A'][c] == 1.0
    # the refused combinations
    with pytest.raises(HmcxError, match="noise='philox'"):
        from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
        sghmc(s.model, start, chains=C, **fx.KW)
    with pytest.raises(HmcxError, match="at most 64"):
        _sampler(name, torch.float32, start, chains=65)
    with pytest.raises(HmcxError, match="keep_every"):
        _sampler(name, torch.float32, start, chains=1, keep_every=2)
    with pytest.raises(HmcxError, match="single-chain"):
        s.step(start, None, None, X_train=X[:f.B], y_train=y[:f.B])
    s.mask_provider = lambda k, nf: None
    with pytest.raises(HmcxError, match="mask_provider"):
        s.sample(epochs=1, burnin=0, batch_size=f.B, X_train=X, y_train=y)
