"""Reference side of multi-chain SGHMC on the dropout MLP (hmcx_mlp_sghmc_chains_run): the oracle runs of the
three-chain recipe and a NumPy float64 restatement of the call.

The oracle is oracle.samplers.sghmc over oracle.models.mlp with dropout masks injected in the sampler's call order
(tests/_mlp_fixtures.py: RecordingOracleSghmc over MaskedOracleMLP).  Chain c of a fixture: its start is
START_SCALE[c] × fx.problem's start, its momenta and noise RandomState(8 + c), its masks mask_stream's step
MASK_K0·c + k, its global stream np.random.seed(SEEDS[shape][c]); chain 0 is the committed fixture run.
tests/test_mlp_sghmc_chains_cpu.py asserts, on the oracle alone, the conditions the GPU tests rely on and is the
authority for the seeds (a seed that stops meeting a condition is searched again, the condition stays).

The restatement takes what the C call takes — host noise blocks (the momentum, then one block of P per iteration, laid
out variable after variable in `order`), per-forward masks in the call's numbering (f = 6·it + i the gradient
forwards, 6n the proposal's energy forward, 6n + 1 the current state's), explicit n_iter and u, and `order`."""
import functools
import io
from collections import namedtuple

import numpy as np

import _mlp_fixtures as fx
from oracle import models as om

NAMES = om.MLP_PARAM_NAMES
SHAPES = ["w32_b20", "w96_b36", "w20_b30"]
START_SCALE = (1.0, -1.0, 0.5)
MASK_K0 = 100
SEEDS = {"w32_b20": (51, 56, 53), "w96_b36": (1925, 1928, 1927), "w20_b30": (59, 60, 61)}
NSTEPS = fx.STEPS_PER_CALL * fx.EPOCHS


def dims(name):
    f = fx.BY_NAME[name]
    return f.n_in, f.n_mid, f.n_out, f.B


def chain_start(name, c=0, order=None):
    X, y, start = fx.problem(*dims(name))
    keys = list(order) if order is not None else list(start.keys())
    return X, y, {k: START_SCALE[c] * start[k] for k in keys}


def mask_of(name, c=0):
    """one(k, f) of chain c: the masks of forward f of global step k."""
    f = fx.BY_NAME[name]
    one = fx.mask_stream(f.B, f.n_mid)[1]
    return lambda k, fwd: one(MASK_K0 * c + k, fwd)


OracleRun = namedtuple("OracleRun", "trace post logp n_iter u eps")


@functools.lru_cache(maxsize=None)
def _oracle_run(name, c, order):
    f = fx.BY_NAME[name]
    X, y, start = chain_start(name, c, order)
    model = fx.MaskedOracleMLP(om.mlp({"alpha": f.alpha}, f.n_in, f.n_mid, f.n_out), mask_of(name, c))
    o = fx.RecordingOracleSghmc(model, start, **fx.KW)
    o.trace, o.out = [], io.StringIO()
    state = np.random.get_state()
    try:
        np.random.seed(SEEDS[name][c])
        post, logp = o.sample(epochs=fx.EPOCHS, burnin=0, batch_size=f.B, rng=np.random.RandomState(8 + c),
                              X_train=X, y_train=y)
    finally:
        np.random.set_state(state)
    n_iter = np.array([max(0, int(t['L']) - 1) for t in o.trace], dtype=np.int32)
    return OracleRun(o.trace, post, logp, n_iter, np.array([t['u'] for t in o.trace]),
                     np.array([t['eps'] for t in o.trace]))


def oracle_run(name, c=0, order=None):
    """The oracle's 3 epochs × 6 steps of chain c (computed once per process and shared: read-only)."""
    return _oracle_run(name, c, tuple(order) if order is not None else None)


def noise_blocks(name, c, n_iter):
    """The standard normals chain c's oracle run drew, per step: P·(n + 1) values in the draw order — the momentum of
    every variable in start order, then per iteration one block per variable (rng.normal(0, s) is s × the stream's
    standard normal, so the same RandomState replays them unscaled)."""
    P = sum(int(np.prod(s)) for s in om.mlp_param_shapes(*dims(name)[:3]).values())
    rs = np.random.RandomState(8 + c)
    return [rs.standard_normal(P * (1 + int(n))) for n in n_iter]


Step = namedtuple("Step", "A accepted E q loss nlp terms eloss")


def restate(name, X, y, start, eps, row0, n_iter, u, noise, one, order=None, alpha=None):
    """The call for one chain, restated: per step (A, accepted, (E_cur, E_new), the kept state, its mean CE and
    loss + log_prior under that state's energy forward, Σ|terms| of each energy and the |loss| in each, both as
    (current, new)).  noise[s]: the step's normals, [P·(n + 1)] in `order` layout; one(s, f): the masks of forward f of
    step s (None: no dropout); order: the variables' names in the caller's order (default: start's)."""
    n_in, n_mid, n_out, B = dims(name)
    alpha = fx.BY_NAME[name].alpha if alpha is None else alpha
    m = om.mlp({"alpha": alpha}, n_in, n_mid, n_out)
    order = list(order or start.keys())
    mk = (lambda s, f: None) if one is None else (lambda s, f: list(one(s, f)))
    q = {k: np.array(start[k], dtype=np.float64) for k in order}
    sizes = [q[k].size for k in order]
    off = dict(zip(order, np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)))
    P = int(sum(sizes))
    out = []
    for s in range(len(n_iter)):
        n, e = int(n_iter[s]), float(eps[s])
        args = dict(X_train=X[row0[s]:row0[s] + B], y_train=y[row0[s]:row0[s] + B])
        z = np.asarray(noise[s], dtype=np.float64)
        assert z.size == P * (n + 1)
        p = {k: z[off[k]:off[k] + q[k].size].reshape(q[k].shape).copy() for k in order}
        qn, pn = {k: v.copy() for k, v in q.items()}, {k: v.copy() for k, v in p.items()}
        for it in range(n):
            for i, var in enumerate(order):
                zz = z[P * (it + 1) + off[var]:P * (it + 1) + off[var] + q[var].size].reshape(q[var].shape)
                qn[var] += e * pn[var]
                g = m.grad(qn, masks=mk(s, 6 * it + i), **args)
                pn[var] = ((1 - e) * pn[var] + e * g[var]) + (2 * e) * zz

        def energy(qq, pp, f):
            loss = m.log_likelihood(qq, masks=mk(s, f), **args)
            pri = [-0.5 * alpha * np.sum(np.square(qq[k])) / qq[k].size for k in order]
            kin = [0.5 * np.sum(np.square(pp[k])) for k in order]
            nlp = loss + sum(pri)
            return nlp + sum(kin), abs(loss) + sum(abs(x) for x in pri) + sum(kin), float(loss), float(nlp)
        E_new, t_new, l_new, nlp_new = energy(qn, pn, 6 * n)
        E_cur, t_cur, l_cur, nlp_cur = energy(q, p, 6 * n + 1)
        A = min(1, np.exp(E_cur - E_new))
        acc = bool(np.isfinite(A) and u[s] < A)
        if acc:
            q = qn
        out.append(Step(float(A), acc, (float(E_cur), float(E_new)), {k: v.copy() for k, v in q.items()},
                        l_new if acc else l_cur, nlp_new if acc else nlp_cur, (t_cur, t_new), (abs(l_cur), abs(l_new))))
    return out


def rows(name, n_steps=NSTEPS):
    """row0 of the recipe's steps: six minibatches per epoch, in order."""
    B = dims(name)[3]
    return [(s % fx.STEPS_PER_CALL) * B for s in range(n_steps)]


def restate_chain(name, c=0, order=None, rnd=None):
    """The restatement of chain c's oracle run, from the oracle's recorded n_iter, u and eps and the replayed noise.
    rnd: rounding applied to the noise and the mask values (the float32 tests), default none."""
    rnd = rnd or (lambda a: np.asarray(a))
    X, y, start = chain_start(name, c, order)
    o = oracle_run(name, c, order)
    one = mask_of(name, c)
    noise = [rnd(z) for z in noise_blocks(name, c, o.n_iter)]
    return restate(name, X, y, start, o.eps, rows(name), o.n_iter, o.u, noise, lambda k, f: rnd(one(k, f)))


def margins(steps, u):
    """|dE − ln u| of every restated step (fx.margins on the restatement's energies)."""
    return fx.margins([{"E": s.E, "u": uu} for s, uu in zip(steps, u)])
