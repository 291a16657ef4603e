"""Reference side of multi-chain full-batch HMC on the dropout MLP (hmcx_mlp_hmc_chains_run): the oracle runs of
the fixtures and a NumPy float64 restatement of the call.

The oracle is oracle.samplers.hmc over oracle.models.mlp with dropout masks injected in the sampler's call order
(tests/_mlp_fixtures.py's MaskedOracleMLP, as for SGHMC).  The restatement takes what the C call takes — host
momenta, per-forward masks in the call's numbering, explicit n_iter and u — and is checked against the oracle in
tests/test_mlp_hmc_chains_cpu.py, which also asserts the conditions the GPU tests rely on (accepts and rejects,
an n_iter of 0 and one >= 3, every decision at least 1e-3 from flipping).

Forwards of a step are numbered in call order: 0 the gradient at q, 1 + 6·it + i the gradient after the drift of
order[i] in iteration it, 6n + 1 the proposal's energy forward, 6n + 2 the current state's, 6n + 3 the record."""
import functools
import io
from collections import namedtuple

import numpy as np

import _mlp_fixtures as fx
from oracle import models as om
from oracle import samplers as osm

ALPHA, STEP_SIZE, PATH_LENGTH = 0.01, 0.2, 0.6
NBURN, NSAMP = 1, 8
NSTEPS = NBURN + NSAMP
SHAPES = [(24, 20, 5, 60), (16, 32, 17, 33), (16, 37, 33, 19)]          # n_in, n_mid, n_out, B
IDS = ["%d-%d-%d-b%d" % s for s in SHAPES]
NAMES = om.MLP_PARAM_NAMES
# chain c of the three-chain tests: its start is START_SCALE[c] × the fixture start, its global stream
# np.random.seed(3 + c), its momenta RandomState(4 + c), its masks the stream of steps MASK_K0·c + s
START_SCALE = (1.0, -1.0, 0.5)
MASK_K0 = 100


class RecordingOracleHmc(osm.hmc):
    """Records, per step, the drawn momentum, the accept uniform (the step's second global np.random.rand draw:
    hmc.py:46 draws the path length first, :61 the uniform), both energies and the state kept."""

    def step(self, state, momentum, rng, **args):
        self.model.in_step, self.model.f = True, 0
        draws = []
        real = np.random.rand

        def rand(*a):
            v = real(*a)
            draws.append(v)
            return v
        np.random.rand = rand
        try:
            out = super().step(state, momentum, rng, **args)
        finally:
            np.random.rand = real
        self.model.in_step = False
        self.model.k += 1
        assert len(draws) == 2
        t = self.trace[-1]
        t['u'] = float(draws[1])
        t['E'] = self._E                                       # (E_current, E_new)
        t['p'] = out[3][0]
        t['q'] = {k: np.array(v) for k, v in out[0].items()}
        return out


OracleRun = namedtuple("OracleRun", "trace n_iter u")


def chain_start(shape, c=0):
    n_in, n_mid, n_out, B = shape
    X, y, start = fx.problem(n_in, n_mid, n_out, B, 1)
    return X, y, {k: START_SCALE[c] * v for k, v in start.items()}


def mask_of(shape, c=0):
    """one(k, f) of chain c: the masks of forward f of step k."""
    one = fx.mask_stream(shape[3], shape[1])[1]
    return lambda k, f: one(MASK_K0 * c + k, f)


@functools.lru_cache(maxsize=None)
def oracle_run(shape, c=0):
    """The oracle's NBURN + NSAMP steps of chain c at `shape` (computed once per process: read-only)."""
    n_in, n_mid, n_out, B = shape
    X, y, start = chain_start(shape, c)
    model = fx.MaskedOracleMLP(om.mlp({"alpha": ALPHA}, n_in, n_mid, n_out), mask_of(shape, c))
    o = RecordingOracleHmc(model, start, path_length=PATH_LENGTH, step_size=STEP_SIZE, verbose=None)
    o.trace, o.out = [], io.StringIO()
    state = np.random.get_state()
    try:
        np.random.seed(3 + c)
        o.sample(niter=NSAMP, burnin=NBURN, rng=np.random.RandomState(4 + c), X_train=X, y_train=y)
    finally:
        np.random.set_state(state)
    n_iter = np.array([max(0, int(t['L']) - 1) for t in o.trace], dtype=np.int32)
    return OracleRun(o.trace, n_iter, np.array([t['u'] for t in o.trace]))


Step = namedtuple("Step", "A accepted E q loss sumsq terms eloss")


def restate(shape, X, y, start, eps, n_iter, u, moms, one, order=None, alpha=ALPHA):
    """The call, restated: per step (A, accepted, (E_cur, E_new), the kept state, the record's mean CE under forward
    6n + 3, Σθ² per canonical variable of the kept state, Σ|terms| of each energy and the |loss| in each, both as
    (current, new)).  moms[s]: the step's momentum per variable; one(s, f): the masks of forward f of step s (None: no dropout); order: the variables'
    names in the caller's order (default: start's)."""
    n_in, n_mid, n_out, B = shape
    m = om.mlp({"alpha": alpha}, n_in, n_mid, n_out)
    order = list(order or start.keys())
    args = dict(X_train=X, y_train=y)
    mk = (lambda s, f: None) if one is None else (lambda s, f: list(one(s, f)))
    q = {k: np.array(start[k], dtype=np.float64) for k in order}
    out = []
    for s in range(len(n_iter)):
        n = int(n_iter[s])
        p = {k: np.array(moms[s][k], dtype=np.float64) for k in order}
        qn, pn = {k: v.copy() for k, v in q.items()}, {k: v.copy() for k, v in p.items()}
        if n > 0:
            g = m.grad(q, masks=mk(s, 0), **args)
        for it in range(n):
            for i, var in enumerate(order):
                pn[var] -= (0.5 * eps) * g[var]
                qn[var] += eps * pn[var]
                g = m.grad(qn, masks=mk(s, 1 + 6 * it + i), **args)
                pn[var] -= eps * g[var]

        def energy(qq, pp, f):
            loss = m.log_likelihood(qq, masks=mk(s, f), **args)
            pri = [-0.5 * alpha * np.sum(np.square(qq[k])) / qq[k].size for k in order]
            kin = [0.5 * np.sum(np.square(pp[k])) for k in order]
            return (loss + sum(pri)) + sum(kin), abs(loss) + sum(abs(x) for x in pri) + sum(kin), abs(float(loss))
        E_new, t_new, l_new = energy(qn, pn, 6 * n + 1)
        E_cur, t_cur, l_cur = energy(q, p, 6 * n + 2)
        A = min(1, np.exp(E_cur - E_new))
        acc = bool(np.isfinite(A) and u[s] < A)
        if acc:
            q = qn
        loss = m.log_likelihood(q, masks=mk(s, 6 * n + 3), **args)
        out.append(Step(float(A), acc, (float(E_cur), float(E_new)), {k: v.copy() for k, v in q.items()}, float(loss),
                        np.array([np.sum(np.square(q[k])) for k in NAMES]), (t_cur, t_new), (l_cur, l_new)))
    return out


def restate_chain(shape, c=0):
    """The restatement of chain c's oracle run, from the oracle's recorded momenta, n_iter and u."""
    X, y, start = chain_start(shape, c)
    o = oracle_run(shape, c)
    return restate(shape, X, y, start, STEP_SIZE, o.n_iter, o.u, [t['p'] for t in o.trace], mask_of(shape, c))
