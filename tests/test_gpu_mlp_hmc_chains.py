"""Full-batch HMC on the dropout MLP, C chains per device call (hmcx_mlp_hmc_chains_run; hmc_multicore on the GPU
mlp with noise='philox').

Fixtures, recipe and preconditions: tests/_mlp_hmc_ref.py and tests/test_mlp_hmc_chains_cpu.py (three shapes, 1
burn-in + 8 steps, n_iter 0 .. 5, accepts and rejects, every decision at least 1e-3 from flipping: measured min
|A − u| 0.059).  Bounds, float64 against the oracle's restatement: flags and n_iter exact, A rtol 1e-9 / atol
1e-12, states rtol 1e-8 / atol 1e-10, losses rtol 1e-10 (test_hmc_mlp_generic_loop_matches_oracle's), E within
n·2⁻⁵³·Σ|terms| (n the longest sum, the largest variable: only summation order differs in the Σθ² / Σp² terms) plus
1e-10·|loss| of that energy's loss alone (the loss comes out of a forward, where more than summation order differs:
the rtol the losses get); measured worst |dE| 4.5e-13 against bounds of 2e-10 and more.  With PHILOX noise and masks
every comparison between calls is bit for bit.

float32 against the float64 restatement on the same float32-rounded inputs, momenta and mask values: flags exact,
each variable within F32_TOL of its largest entry — F32_MARGIN × the worst error measured on an MI355X over the three
fixtures, never above F32_CAP (tests/_mlp_cases.py).  Measured worst (error / largest entry) per fixture, 9 steps:
24-20-5-b60 1.587e-7, 16-32-17-b33 1.302e-7, 16-37-33-b19 1.698e-7; A differed by at most 3.7e-7 and no flag
flipped (smallest |A − u| 0.059).  The float32 momentum against its host twin: worst |difference| 1.311e-6 (the
device's hardware log / sin / cos), held to F32_MARGIN × that.
"""
import ctypes
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _mlp_cases as mc  # noqa: E402
import _mlp_fixtures as fx  # noqa: E402
import _mlp_hmc_ref as ref  # noqa: E402

F32_WORST = 1.698e-7                                       # measured, see above
F32_TOL = min(mc.F32_MARGIN * F32_WORST, mc.F32_CAP)
TWIN_F32_WORST = 1.311e-6                                   # worst |device normal − host twin|, float32, measured
NAMES = ref.NAMES
DT = {"f64": torch.float64, "f32": torch.float32}


def _nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    return _native


def _model(shape, dtype, seed=0):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp
    return mlp({"alpha": ref.ALPHA}, shape[0], shape[1], shape[2], dtype=dtype, device="cuda:0", seed=seed)


def _nvars(shape):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp_param_shapes
    return [int(np.prod(s)) for s in mlp_param_shapes(*shape[:3]).values()]


class Call:
    """One hmcx_mlp_hmc_chains_run.  starts: per chain {name: array}; n_iter, u [S, C]; noise None (PHILOX) or a host
    array [S, C, P] (BUFFER, laid out in `order`); masks 'philox', None or (host array, mask_off [S, C]) (FIXED).
    The state is carried in self.par, so a second run() continues the first."""

    def __init__(self, shape, dtype, starts, order=NAMES, seed=7, chain0=0, data=None):
        self.nat = _nat()
        self.shape, self.m, self.C = shape, _model(shape, dtype), len(starts)
        X, y, _ = ref.chain_start(shape) if data is None else data
        self.X, self.y = self.m._xy(dict(X_train=X, y_train=y))
        self.par = [self.m._dev(np.stack([s[k] for s in starts])).contiguous() for k in NAMES]
        self.order = [NAMES.index(k) for k in order]
        self.seed, self.chain0 = seed, chain0

    def args(self, n_iter, u, noise=None, masks='philox', step_base=0, eps=ref.STEP_SIZE, want_eval=None,
             want_draw=None, draws=None, mom=None, draw_stride=0, draw0=0):
        nat, m, C = self.nat, self.m, self.C
        n_iter = np.ascontiguousarray(n_iter, dtype=np.int32).reshape(-1, C)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1, C)
        S = n_iter.shape[0]
        dev = m.device
        k = types_keep = {}
        k['eps'] = np.full(S, eps, dtype=np.float64)
        k['n_iter'], k['u'] = n_iter, u
        a = nat.MlpHmcChainsArgs()
        a.dtype, a.B, a.n_in, a.n_mid, a.n_out, a.n_steps, a.C = m.code, self.shape[3], m.n_in, m.n_mid, m.n_out, S, C
        for i, v in enumerate(self.order):
            a.order[i] = v
        a.alpha = m.alpha
        a.X, a.y = self.X.data_ptr(), self.y.data_ptr()
        a.eps = k['eps'].ctypes.data_as(nat.c_dblp)
        a.n_iter = n_iter.ctypes.data_as(nat.c_i32p)
        a.u_accept = u.ctypes.data_as(nat.c_dblp)
        a.noise_mode = nat.NOISE_PHILOX
        if noise is not None:
            P = noise.shape[-1]
            k['noise'] = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64).reshape(-1)).to(dev)
            k['noff'] = np.arange(S * C, dtype=np.int64) * P
            a.noise_mode, a.noise = nat.NOISE_BUFFER, k['noise'].data_ptr()
            a.noise_off = k['noff'].ctypes.data_as(nat.c_i64p)
        if masks is None:
            a.mask_mode = nat.MLP_MASKS_NONE
        elif isinstance(masks, str):
            a.mask_mode = nat.MLP_MASKS_PHILOX
        else:
            k['masks'] = m._dev(masks[0]).contiguous()
            k['moff'] = np.ascontiguousarray(masks[1], dtype=np.int64)
            a.mask_mode, a.masks = nat.MLP_MASKS_FIXED, k['masks'].data_ptr()
            a.mask_off = k['moff'].ctypes.data_as(nat.c_i64p)
        a.seed, a.chain0, a.step_base = self.seed, self.chain0, step_base
        for i, t in enumerate(self.par):
            a.par.p[i] = t.data_ptr()
        f64 = dict(dtype=torch.float64, device=dev)
        we = np.ones(S, dtype=np.uint8) if want_eval is None else np.ascontiguousarray(want_eval, dtype=np.uint8)
        ne = int(we.sum())
        k['we'] = we
        o = dict(A=torch.full((S, C), np.nan, **f64), acc=torch.full((S, C), -1, dtype=torch.int32, device=dev),
                 E=torch.full((S, C, 2), np.nan, **f64), loss=torch.full((ne, C), np.nan, **f64),
                 sumsq=torch.full((ne, C, 6), np.nan, **f64))
        a.out_A, a.out_accepted, a.out_E = o['A'].data_ptr(), o['acc'].data_ptr(), o['E'].data_ptr()
        a.want_eval = we.ctypes.data_as(nat.c_u8p)
        a.out_eval_loss, a.out_eval_sumsq = o['loss'].data_ptr(), o['sumsq'].data_ptr()
        if want_draw is not None:
            k['wd'] = np.ascontiguousarray(want_draw, dtype=np.uint8)
            a.want_draw, a.draw_stride = k['wd'].ctypes.data_as(nat.c_u8p), draw_stride
            for i, t in enumerate(draws):
                a.draws.p[i] = t.data_ptr() + draw0 * t[0, 0].numel() * t.element_size()
            if mom is not None:
                for i, t in enumerate(mom):
                    a.out_mom.p[i] = t.data_ptr() + draw0 * t[0, 0].numel() * t.element_size()
        return a, o, types_keep

    def run(self, *args, **kw):
        a, o, keep = self.args(*args, **kw)
        ctx = self.m.ctx
        ctx.check(ctx.lib.hmcx_mlp_hmc_chains_run(ctx.h, ctypes.byref(a)), "hmcx_mlp_hmc_chains_run")
        torch.cuda.synchronize()
        del keep
        return {k: v.cpu().numpy() for k, v in o.items()}

    def state(self, c):
        return {k: t[c].cpu().numpy() for k, t in zip(NAMES, self.par)}

    def buffers(self, T):
        return [torch.zeros((self.C, T) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in self.par]


def _fixed_inputs(shape, chains, f32=False):
    """BUFFER noise [S, C, P], FIXED masks and mask_off [S, C], n_iter and u [S, C], the starts and the restatements
    of the listed chains of the three-chain recipe (chain j of the call = recipe chain chains[j]).  f32: momenta and
    mask values (1/0.9) are rounded through float32 for the device and the restatement alike; X and the starts are
    float32-exact already (fx.problem, and the start scales ±1 and 0.5 keep them so)."""
    B, n_mid = shape[3], shape[1]
    n3 = 3 * B * n_mid
    rnd = (lambda a: np.asarray(a).astype(np.float32).astype(np.float64)) if f32 else (lambda a: np.asarray(a))
    S, C = ref.NSTEPS, len(chains)
    runs = [ref.oracle_run(shape, c) for c in chains]
    n_iter = np.stack([r.n_iter for r in runs], axis=1)
    u = np.stack([r.u for r in runs], axis=1)
    noise = np.stack([np.stack([np.concatenate([rnd(t['p'][k]).reshape(-1) for k in NAMES]) for t in r.trace])
                      for r in runs], axis=1)
    blocks, moff, off = [], np.zeros((S, C), dtype=np.int64), 0
    for s in range(S):
        for j, c in enumerate(chains):
            one = ref.mask_of(shape, c)
            nf = 6 * int(n_iter[s, j]) + 4
            moff[s, j] = off
            blocks.append(np.stack([rnd(one(s, f)) for f in range(nf)]).reshape(-1))
            off += nf * n3
    starts = [ref.chain_start(shape, c)[2] for c in chains]
    rs = []
    for j, c in enumerate(chains):
        X, y, _ = ref.chain_start(shape, c)
        moms = [{k: rnd(t['p'][k]) for k in NAMES} for t in runs[j].trace]
        one = ref.mask_of(shape, c)
        rs.append(ref.restate(shape, X, y, starts[j], ref.STEP_SIZE, n_iter[:, j], u[:, j], moms,
                              lambda k, f, one=one: rnd(one(k, f))))
    return n_iter, u, noise, (np.concatenate(blocks), moff), starts, rs


# ----------------------------------------------------------------------------- 1. float64 against the oracle
@pytest.mark.parametrize("chains", [(0,), (0, 1, 2)], ids=["C1", "C3"])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_f64_matches_the_oracle(shape, chains):
    n_iter, u, noise, masks, starts, rs = _fixed_inputs(shape, chains)
    for c in chains:                                           # the precondition fails the test, it does not skip it
        o = ref.oracle_run(shape, c)
        assert min(abs(t['A'] - t['u']) for t in o.trace) >= 1e-3
        assert [s.accepted for s in rs[chains.index(c)]] == [t['accepted'] for t in o.trace]
    g = Call(shape, torch.float64, starts)
    T = ref.NSTEPS
    draws, mom = g.buffers(T), g.buffers(T)
    out = g.run(n_iter, u, noise=noise, masks=masks, want_draw=np.ones(T), draws=draws, mom=mom, draw_stride=T)
    nlong = max(_nvars(shape))
    for j in range(len(chains)):
        r = rs[j]
        np.testing.assert_array_equal(out['acc'][:, j], [int(s.accepted) for s in r])
        np.testing.assert_allclose(out['A'][:, j], [s.A for s in r], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(out['loss'][:, j], [s.loss for s in r], rtol=1e-10)
        np.testing.assert_allclose(out['sumsq'][:, j], [s.sumsq for s in r], rtol=1e-10)
        for s in range(T):
            for w in (0, 1):                                   # E_current, E_new
                tol = nlong * 2.0 ** -53 * r[s].terms[w] + 1e-10 * r[s].eloss[w]
                d = abs(out['E'][s, j, w] - r[s].E[w])
                print("step %d chain %d E[%d]: |dE| %.3e tol %.3e" % (s, j, w, d, tol))
                assert d <= tol, (s, j, w, d, tol)
            for i, k in enumerate(NAMES):
                np.testing.assert_allclose(draws[i][j, s].cpu().numpy(), r[s].q[k], rtol=1e-8, atol=1e-10, err_msg=k)
        e0 = 0
        for i, k in enumerate(NAMES):                          # the momenta stored are the momenta drawn
            n = int(np.prod(starts[0][k].shape))
            np.testing.assert_array_equal(mom[i][j].cpu().numpy().reshape(T, -1), noise[:, j, e0:e0 + n])
            e0 += n
            np.testing.assert_allclose(g.state(j)[k], r[-1].q[k], rtol=1e-8, atol=1e-10, err_msg=k)


# ----------------------------------------------------------------------------- 2. against the one-chain trajectory
@pytest.mark.parametrize("n", [0, 1, 3])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_committed_proposal_equals_the_leapfrog_entry_bitwise(dt, n):
    """u = 0 commits every proposal: the state after one step is hmcx_mlp_hmc_leapfrog's q from the same start and
    the same momentum, under the same Philox masks (slot0 = 0x80000000).  The momentum handed to the one-chain
    entry is the call's own record of what it drew (out_mom): the host twin of the stream (hmcx_philox_normals*)
    evaluates Box–Muller with the host's libm — sin / cos of 2π·u where the device takes sincospi — so it equals
    the device's draw to rounding, not bit for bit (measured: 43 % of the float64 elements differ in the last
    place), and is compared at that level here."""
    shape, nat = ref.SHAPES[1], _nat()
    order = fx.PERMUTED
    _, _, start = ref.chain_start(shape)
    seed, chain0, step_base, C = 11, 3, 5, 2
    g = Call(shape, DT[dt], [start] * C, order=order, seed=seed, chain0=chain0)
    m = g.m
    draws, mom = g.buffers(1), g.buffers(1)
    out = g.run(np.full((1, C), n), np.zeros((1, C)), step_base=step_base, want_draw=np.ones(1), draws=draws, mom=mom,
                draw_stride=1)
    assert out['acc'].tolist() == [[1] * C]
    P = sum(_nvars(shape))
    for c in range(C):
        z = nat.philox_normals(seed, chain0 + c, step_base, 0, 0, P, dtype=dt)
        q = {k: m._dev(start[k]).contiguous().clone() for k in NAMES}
        p, e0 = {}, 0
        for k in order:
            nk = int(np.prod(start[k].shape))
            p[k] = mom[NAMES.index(k)][c, 0].contiguous().clone()
            # float32: the device takes the hardware log / sin / cos approximations (hmcx_common.h, box_muller);
            # absolute, since the normals are O(1): F32_MARGIN × the worst difference measured (TWIN_F32_WORST)
            dz = np.abs(p[k].cpu().numpy().reshape(-1).astype(np.float64) - z[e0:e0 + nk]).max()
            print("%s n=%d chain %d %s: worst |device - host twin| %.3e" % (dt, n, c, k, dz))
            if dt == "f64":
                np.testing.assert_allclose(p[k].cpu().numpy().reshape(-1), z[e0:e0 + nk], rtol=1e-12, atol=1e-14, err_msg=k)
            else:
                assert dz <= mc.F32_MARGIN * TWIN_F32_WORST, (k, dz)
            e0 += nk
        a = nat.MlpLeapfrogArgs()
        a.dtype, a.B, a.n_in, a.n_mid, a.n_out, a.n_iter = m.code, shape[3], m.n_in, m.n_mid, m.n_out, n
        for i, k in enumerate(order):
            a.order[i] = NAMES.index(k)
        a.eps, a.alpha = ref.STEP_SIZE, m.alpha
        a.X, a.y = g.X.data_ptr(), g.y.data_ptr()
        gs = {k: torch.empty_like(q[k]) for k in NAMES}
        for i, k in enumerate(NAMES):
            a.q.p[i], a.p.p[i], a.g.p[i] = q[k].data_ptr(), p[k].data_ptr(), gs[k].data_ptr()
        scr = torch.empty((3, shape[3], m.n_mid), dtype=m.dtype, device=m.device)
        a.mask_mode, a.masks = nat.MLP_MASKS_PHILOX, scr.data_ptr()
        a.seed, a.chain, a.step, a.slot0 = seed, chain0 + c, step_base, 0x80000000
        m.ctx.check(m.ctx.lib.hmcx_mlp_hmc_leapfrog(m.ctx.h, ctypes.byref(a)), "hmcx_mlp_hmc_leapfrog")
        torch.cuda.synchronize()
        for k in NAMES:
            np.testing.assert_array_equal(g.state(c)[k], q[k].cpu().numpy(), err_msg="%s chain %d" % (k, c))
        if n > 0:
            assert not np.array_equal(g.state(c)['/l1/W'], m._dev(start['/l1/W']).cpu().numpy())


# ----------------------------------------------------------------------------- 3. chain invariance
def _ragged(S, C, seed):
    rs = np.random.RandomState(seed)
    n_iter = rs.randint(0, 4, (S, C))
    n_iter[0, :min(C, 3)] = [0, 3, 1][:min(C, 3)]
    if C > 2:
        n_iter[1, :3] = [2, 2, 5]
    return n_iter, rs.rand(S, C)


def _philox_run(shape, dt, starts, n_iter, u, chain0, T):
    g = Call(shape, DT[dt], starts, seed=13, chain0=chain0)
    draws, mom = g.buffers(T), g.buffers(T)
    out = g.run(n_iter, u, step_base=2, want_draw=np.ones(T), draws=draws, mom=mom, draw_stride=T)
    out['draws'] = [t.cpu().numpy() for t in draws]
    out['mom'] = [t.cpu().numpy() for t in mom]
    out['state'] = [t.cpu().numpy() for t in g.par]
    return out


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("shape,C", [(ref.SHAPES[0], 7), (ref.SHAPES[1], 2), (ref.SHAPES[2], 2)],
                         ids=["24-20-5-C7", "16-32-17-C2", "16-37-33-C2"])
def test_every_chain_equals_the_one_chain_call_bitwise(shape, C, dt):
    S = 3
    _, _, start = ref.chain_start(shape)
    starts = [{k: (1.0 - 0.1 * c) * v for k, v in start.items()} for c in range(C)]
    n_iter, u = _ragged(S, C, 5)
    g = _philox_run(shape, dt, starts, n_iter, u, 4, S)
    assert 0 < g['acc'].sum() and np.all(np.isfinite(g['A']))
    for c in range(C):
        r = _philox_run(shape, dt, [starts[c]], n_iter[:, c:c + 1], u[:, c:c + 1], 4 + c, S)
        for key in ('A', 'acc', 'E', 'loss', 'sumsq'):
            np.testing.assert_array_equal(g[key][:, c], r[key][:, 0], err_msg="%s chain %d" % (key, c))
        for key in ('draws', 'mom', 'state'):
            for i, k in enumerate(NAMES):
                np.testing.assert_array_equal(g[key][i][c], r[key][i][0], err_msg="%s %s chain %d" % (key, k, c))
    if C == 7:
        # the same chains in another C and at other positions of the launch group: chains 4, 5 (the first group's last
        # two) and 6 (alone in the second group) of the call above as positions 0, 1, 2 of one group of three
        sub = [4, 5, 6]
        h = _philox_run(shape, dt, [starts[c] for c in sub], n_iter[:, sub], u[:, sub], 4 + sub[0], S)
        for j, c in enumerate(sub):
            for key in ('A', 'acc', 'E', 'loss', 'sumsq'):
                np.testing.assert_array_equal(g[key][:, c], h[key][:, j], err_msg=key)
            for i in range(6):
                np.testing.assert_array_equal(g['draws'][i][c], h['draws'][i][j])


# ----------------------------------------------------------------------------- 4. split invariance
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_one_call_equals_its_splits_bitwise(dt):
    shape, C, S = ref.SHAPES[0], 3, 6
    _, _, start = ref.chain_start(shape)
    starts = [{k: (1.0 + 0.2 * c) * v for k, v in start.items()} for c in range(C)]
    n_iter, u = _ragged(S, C, 9)
    want_eval = np.array([1, 0, 1, 1, 0, 1], dtype=np.uint8)
    want_draw = np.array([0, 1, 1, 0, 1, 1], dtype=np.uint8)
    T = int(want_draw.sum())

    def run(splits):
        g = Call(shape, DT[dt], starts, seed=21, chain0=1)
        draws, mom = g.buffers(T), g.buffers(T)
        outs, s0, d0 = [], 0, 0
        for n in splits:
            sl = slice(s0, s0 + n)
            outs.append(g.run(n_iter[sl], u[sl], step_base=10 + s0, want_eval=want_eval[sl], want_draw=want_draw[sl],
                              draws=draws, mom=mom, draw_stride=T, draw0=d0))
            s0, d0 = s0 + n, d0 + int(want_draw[sl].sum())
        out = {k: np.concatenate([o[k] for o in outs], axis=0) for k in outs[0]}
        out['draws'] = [t.cpu().numpy() for t in draws]
        out['mom'] = [t.cpu().numpy() for t in mom]
        out['state'] = [t.cpu().numpy() for t in g.par]
        return out
    a, b = run([6]), run([1, 2, 3])
    assert a['loss'].shape == (4, C) and np.all(np.isfinite(a['loss'])) and a['acc'].min() >= 0
    for key in ('A', 'acc', 'E', 'loss', 'sumsq'):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    for key in ('draws', 'mom', 'state'):
        for i in range(6):
            np.testing.assert_array_equal(a[key][i], b[key][i], err_msg=key)
    assert not np.array_equal(a['draws'][0][0, 0], a['draws'][0][0, -1])


# ----------------------------------------------------------------------------- 5. float32
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_f32_matches_the_oracle(shape):
    n_iter, u, noise, masks, starts, rs = _fixed_inputs(shape, (0,), f32=True)
    r = rs[0]
    o = ref.oracle_run(shape)
    assert [s.accepted for s in r] == [t['accepted'] for t in o.trace]        # rounding the momenta flips nothing
    assert min(abs(s.A - uu) for s, uu in zip(r, u[:, 0])) >= 1e-3
    g = Call(shape, torch.float32, starts)
    T = ref.NSTEPS
    draws = g.buffers(T)
    out = g.run(n_iter, u, noise=noise, masks=masks, want_draw=np.ones(T), draws=draws, draw_stride=T)
    worst = 0.0
    for s in range(T):
        for i, k in enumerate(NAMES):
            worst = max(worst, np.abs(draws[i][0, s].cpu().numpy() - r[s].q[k]).max() / np.abs(r[s].q[k]).max())
    print("float32 worst state error / largest entry: %.3e; worst |dA| %.3e; tolerance %.3e"
          % (worst, np.abs(out['A'][:, 0] - [s.A for s in r]).max(), F32_TOL))
    np.testing.assert_array_equal(out['acc'][:, 0], [int(s.accepted) for s in r])
    for s in range(T):
        for i, k in enumerate(NAMES):
            assert np.abs(draws[i][0, s].cpu().numpy() - r[s].q[k]).max() <= F32_TOL * np.abs(r[s].q[k]).max(), (s, k)
    np.testing.assert_allclose(out['loss'][:, 0], [s.loss for s in r], rtol=1e-4)


# ----------------------------------------------------------------------------- 6. invalid arguments
def test_invalid_arguments_leave_the_state_untouched():
    shape, C = ref.SHAPES[0], 2
    _, _, start = ref.chain_start(shape)
    g = Call(shape, torch.float64, [start] * C)
    before = [t.clone() for t in g.par]
    lib, h = g.m.ctx.lib, g.m.ctx.h
    n_iter, u = np.ones((2, C), dtype=np.int32), np.full((2, C), 0.5)
    T = 2
    draws = g.buffers(T)

    def base(**kw):
        return g.args(n_iter, u, want_draw=np.ones(2), draws=draws, draw_stride=T, **kw)

    def bad(name, mutate, **kw):
        a, o, keep = base(**kw)
        mutate(a)
        rc = lib.hmcx_mlp_hmc_chains_run(h, ctypes.byref(a))
        msg = lib.hmcx_last_error(h)
        torch.cuda.synchronize()
        assert rc < 0 and msg and b"mlp hmc chains" in msg, (name, rc, msg)
        for t, b in zip(g.par, before):
            assert torch.equal(t, b), name
        assert torch.isnan(o['A']).all(), name                 # nothing was launched
        del keep
    bad("C = 0", lambda a: setattr(a, "C", 0))
    bad("C = 65", lambda a: setattr(a, "C", 65))
    bad("order", lambda a: a.order.__setitem__(0, a.order[1]))
    neg = np.array([[1, -1], [1, 1]], dtype=np.int32)
    bad("n_iter < 0", lambda a: setattr(a, "n_iter", neg.ctypes.data_as(g.nat.c_i32p)))
    big = np.array([[1, 1], [(0x7fffffff - 3) // 6 + 1, 1]], dtype=np.int32)
    bad("n_iter wraps", lambda a: setattr(a, "n_iter", big.ctypes.data_as(g.nat.c_i32p)))
    bad("chain0 wraps", lambda a: setattr(a, "chain0", 0xFFFFFFFF))
    bad("step_base wraps", lambda a: setattr(a, "step_base", 0xFFFFFFFF))
    bad("draw_stride", lambda a: setattr(a, "draw_stride", 1))
    bad("BUFFER without noise", lambda a: setattr(a, "noise_mode", g.nat.NOISE_BUFFER))
    bad("FIXED without masks", lambda a: setattr(a, "mask_mode", g.nat.MLP_MASKS_FIXED))
    bad("no out_A", lambda a: setattr(a, "out_A", None))
    bad("want_eval without out_eval_loss", lambda a: setattr(a, "out_eval_loss", None))
    assert lib.hmcx_mlp_hmc_chains_run(None, None) == -1 and lib.hmcx_mlp_hmc_chains_run(h, None) < 0
    a, o, keep = base()
    a.n_steps = 0                                               # zero steps: nothing happens
    assert lib.hmcx_mlp_hmc_chains_run(h, ctypes.byref(a)) == 0
    torch.cuda.synchronize()
    assert torch.isnan(o['A']).all() and all(torch.equal(t, b) for t, b in zip(g.par, before))


# ----------------------------------------------------------------------------- 7. the Python surface
def _multicore(shape, dtype, ncores, niter, chain=0, seed=3, masks=None, **kw):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc_multicore import hmc_multicore
    X, y, start = ref.chain_start(shape)
    s = hmc_multicore(_model(shape, dtype), start, path_length=ref.PATH_LENGTH, step_size=ref.STEP_SIZE, noise='philox',
                      seed=seed, chain=chain, **kw)
    s.out, s.trace = io.StringIO(), []
    extra = {} if masks is None else {'masks': masks}
    res = s.sample_multicore(niter, 2, ncores, X_train=X, y_train=y, **extra)
    return s, res, (X, y, start)


def test_sample_multicore_runs_the_chains_in_one_call_per_phase():
    from dropout_hamiltonian_montecarlo_amd import diagnostics
    shape, nat = ref.SHAPES[0], _nat()
    C, T = 3, 4
    s, (post, positions, momentums, logp), (X, y, start) = _multicore(shape, torch.float64, C, 12)
    assert list(post.keys()) == list(start.keys()) and logp.shape == (C * T,)
    d = s.device_draws
    for k, v in start.items():
        assert post[k].shape == (C * T,) + v.shape and d[k].shape == (C, T) + v.shape
        np.testing.assert_array_equal(post[k], d[k].cpu().numpy().reshape((C * T,) + v.shape))   # chain-major
        assert s.last_state[k].shape == (C,) + v.shape
        np.testing.assert_array_equal(s.last_state[k].cpu().numpy(), d[k][:, -1].cpu().numpy())
    assert len(positions) == C and len(momentums) == C and len(positions[0]) == T and len(momentums[0]) == T
    np.testing.assert_array_equal(positions[1][2][0]['/l2/W'], post['/l2/W'][T + 1])
    # the schedule is philox_schedule's
    L, n_iter, u = nat.philox_schedule(3, 0, C, 0, ref.PATH_LENGTH, np.full(2 + T, ref.STEP_SIZE))
    for c in range(C):
        assert [t['L'] for t in s.chain_traces[c]] == L[:, c].tolist() and len(s.chain_traces[c]) == 2 + T
        assert all(0.0 <= t['A'] <= 1.0 for t in s.chain_traces[c])
    assert len(s.trace) == C * (2 + T)
    assert s.out.getvalue().count("adapted step size") == C
    # chain c is the one-chain run under chain = c
    for c in range(C):
        s1, (p1, pos1, mom1, l1), _ = _multicore(shape, torch.float64, 1, T, chain=c)
        for k in start:
            np.testing.assert_array_equal(p1[k], post[k][c * T:(c + 1) * T], err_msg=k)
            np.testing.assert_array_equal(mom1[0][1][0][k], momentums[c][1][0][k], err_msg=k)
        np.testing.assert_array_equal(l1, logp[c * T:(c + 1) * T])
        assert s1.chain_traces[0] == s.chain_traces[c]
    # the chains differ from each other and follow the seed
    assert not np.array_equal(post['/l1/W'][0], post['/l1/W'][T])
    _, (p2, _, _, _), _ = _multicore(shape, torch.float64, C, 12, seed=4)
    assert not np.array_equal(p2['/l1/W'], post['/l1/W'])
    # diagnostics and the predictive read the device draws
    host = {k: v.cpu().numpy() for k, v in d.items()}
    diag = s.chain_diagnostics()
    assert list(diag.keys()) == list(d.keys())
    for k, (sr, es) in diag.items():
        sr, es = np.asarray(sr.cpu() if hasattr(sr, "cpu") else sr), np.asarray(es.cpu() if hasattr(es, "cpu") else es)
        assert sr.shape == s.model.shapes[k] == es.shape
        for got, want in ((sr, diagnostics.split_rhat(host[k])), (es, diagnostics.ess(host[k]))):
            assert np.array_equal(np.isnan(got), np.isnan(want)), k
            ok = ~np.isnan(want)
            np.testing.assert_allclose(got[ok], want[ok], rtol=1e-9, err_msg=k)
    dev = s.model.posterior_predictive(d, X, y, masks="off")
    hst = s.model.posterior_predictive(host, X, y, masks="off")
    for name, a, b in zip(dev._fields, dev, hst):
        assert np.all(np.isfinite(a)), name
        np.testing.assert_array_equal(a, b, err_msg=name)
    # the returned log-posterior values are the model's negative_log_posterior of the draws: with dropout off the
    # record forward is deterministic, so the host composition (loss − Σ ½α·Σθ²/dim in start order) is pinned
    s4, (p4, _, _, l4), _ = _multicore(shape, torch.float64, 2, 6, masks='off')
    for i in (0, 2, 5):
        want = s4.model.negative_log_posterior({k: p4[k][i] for k in start}, masks='off', X_train=X, y_train=y)
        np.testing.assert_allclose(l4[i], want, rtol=1e-10)
    lines = [float(x.split()[1]) for x in s4.out.getvalue().splitlines() if x.startswith("loss:")]
    assert len(lines) >= 2

    s3, (p3, _, mom3, _), _ = _multicore(shape, torch.float64, C, 12, keep_momentum=False)
    assert all(m == [] for m in mom3)
    np.testing.assert_array_equal(p3['/l3/W'], post['/l3/W'])
