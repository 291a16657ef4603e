"""NumPy restatement of the reference's random-walk Metropolis sampler (hamiltonian/inference/cpu/
metropolis.py, class MH) for C chains — test infrastructure for tests/test_mh_cpu.py and
tests/test_gpu_mh.py.

Arithmetic is the reference's, operation for operation (metropolis.py:38-64): per variable
``factor = exp(rng.uniform(-1.5, 1.5))`` then ``q_new[var] += factor*scale*rng.normal(0, 1, dim)`` (or one
coordinate ``rng.randint(dim)`` with ``update_sequential=False``), ``A = exp(E - E_new)`` with
``E = -logp``, accepted iff ``isfinite(A) and u < A`` — no min(1, ·), so an overflowing ratio is rejected.

``logp`` is an oracle model (``oracle.models``: ``log_likelihood + log_prior``, or ``-negative_log_posterior``
for the MVN model) or any callable ``logp(X, y, q, hyper)``.

Stream convention (that of the library's MH class):

* ``noise='numpy'``: chain c draws factors, sites and normals from ``rngs[c]`` (``RandomState(c)`` in
  ``multicore_sample``); the accept uniform of a step is one ``np.random.rand()`` from the global stream,
  shared by the chains;
* ``noise='philox'``: factors / sites from ``philox_uniforms(seed, chain + c, step, SLOT_PATH, 4)``
  (u0, u1 → ``exp(-1.5 + 3u)`` of variable 0, 1; u2, u3 → ``floor(u·dim)``), the accept uniform from
  ``SLOT_ACCEPT``, the normals from the float64 host twin of the device stream (slot 0).

Per chain it records A, u, the accept flags, the factors, the multipliers, the sites, the kept state's
logp, the tuned scale and the printed lines.
"""
import numpy as np


def logp_of(model):
    """logp(X, y, q, hyper) of an oracle model instance (or the callable itself)."""
    if hasattr(model, "log_likelihood"):
        return lambda X, y, q, hyper: model.log_likelihood(q, X_train=X, y_train=y) + model.log_prior(q)
    if hasattr(model, "negative_log_posterior"):
        return lambda X, y, q, hyper: -model.negative_log_posterior(q)
    return model


def tune(scale, acc_rate, lines):                                           # metropolis.py:105-128
    new_scale = scale
    if acc_rate < 0.001:
        lines.append('reduce by 90 percent')
        new_scale *= 0.1
    elif acc_rate < 0.05:
        lines.append('reduce by 50 percent')
        new_scale *= 0.5
    elif acc_rate < 0.2:
        lines.append('reduce by ten percent')
        new_scale *= 0.9
    elif acc_rate > 0.95:
        lines.append('increase by factor of ten')
        new_scale *= 10.0
    elif acc_rate > 0.75:
        lines.append('increase by double')
        new_scale *= 2.0
    elif acc_rate > 0.5:
        lines.append('increase by ten percent')
        new_scale *= 1.1
    return new_scale


class ChainRecord:
    def __init__(self):
        self.A, self.u, self.accepted, self.factors, self.mult, self.site, self.logp = [], [], [], [], [], [], []
        self.lines = []
        self.scale = None
        self.posterior = None


class MH:
    def __init__(self, X, y, logp, start, hyper, scale=1.0, update_sequential=True, verbose=True,
                 noise='numpy', seed=0, chain=0):
        self.start, self.hyper = start, hyper
        self.logp = logp_of(logp)
        self._update_sequential = update_sequential
        self._scale = scale
        self._log_factor = 1.5
        self._verbose = verbose
        self.X, self.y = X, y
        self.noise, self.seed, self.chain = noise, int(seed), int(chain)
        self.global_step = 0

    def energy(self, q):                                                     # metropolis.py:49-50
        return -self.logp(self.X, self.y, q, self.hyper)

    # ------------------------------------------------------------------ one step of one chain
    def _philox(self, c, step):
        from dropout_hamiltonian_montecarlo_amd import _native as nat
        ch, st = (self.chain + c) & 0xFFFFFFFF, step & 0xFFFFFFFF
        P = sum(int(np.asarray(self.start[v]).size) for v in self.start)
        return (nat.philox_uniforms(self.seed, ch, st, nat.SLOT_PATH, 4),
                nat.philox_uniforms(self.seed, ch, st, nat.SLOT_ACCEPT, 1)[0],
                nat.philox_normals(self.seed, ch, st, 0, 0, P, dtype="f64"))

    def _step(self, q, scale, rng, c, step, rec):
        q_new = {var: q[var].flatten() for var in self.start.keys()}        # metropolis.py:54
        factors, mults, sites = [], [], []
        if self.noise == 'philox':
            pu, u_acc, z_all = self._philox(c, step)
        off = 0
        for k, var in enumerate(self.start.keys()):
            dim = (np.array(self.start[var])).size
            if self.noise == 'philox':
                factor = np.exp(-self._log_factor + 2 * self._log_factor * pu[k])
                ind = min(int(np.floor(pu[2 + k] * dim)), dim - 1)
                z = z_all[off:off + dim] if self._update_sequential else z_all[off + ind]
            else:
                factor = np.exp(rng.uniform(-self._log_factor, self._log_factor))
                if self._update_sequential:
                    z = rng.normal(0.0, 1.0, dim)
                else:
                    ind = rng.randint(dim)
                    z = rng.normal(0.0, 1.0)
            if self._update_sequential:
                q_new[var] += factor * scale * z                             # metropolis.py:59
                sites.append(-1)
            else:
                q_new[var][ind] += factor * scale * z                        # metropolis.py:62
                sites.append(int(ind))
            q_new[var] = q_new[var].reshape(np.shape(self.start[var]))
            factors.append(float(factor))
            mults.append(float(factor * scale))
            off += dim
        E_new = self.energy(q_new)                                           # metropolis.py:40-46
        E = self.energy(q)
        with np.errstate(over='ignore', invalid='ignore'):
            A = np.exp(E - E_new)
        g = u_acc if self.noise == 'philox' else np.random.rand()
        accepted = bool(np.isfinite(A) and (g < A))
        rec.A.append(float(A)); rec.u.append(float(g)); rec.accepted.append(accepted)
        rec.factors.append(factors); rec.mult.append(mults); rec.site.append(sites)
        rec.logp.append(float(-(E_new if accepted else E)))
        return (q_new if accepted else q), accepted

    # ------------------------------------------------------------------ C chains
    def run(self, niter, burnin, C, rngs, niter_print=None):
        """C chains, step-interleaved (every chain sees the same global accept uniform per step).
        niter_print: the raw niter of the print test ``i % (niter/10) == 0`` (default niter)."""
        niter_print = niter if niter_print is None else niter_print
        nburn, nit = int(burnin), int(niter)
        recs = [ChainRecord() for _ in range(C)]
        qs = [{v: np.array(self.start[v], dtype=np.float64) for v in self.start} for _ in range(C)]
        scales = [self._scale] * C
        step = self.global_step
        for i in range(nburn):
            u_state = np.random.get_state() if self.noise == 'numpy' else None
            for c in range(C):
                if u_state is not None:
                    np.random.set_state(u_state)
                qs[c], _ = self._step(qs[c], scales[c], rngs[c] if rngs else None, c, step, recs[c])
            step += 1
        for c in range(C):
            if nburn > 0:
                rate = np.sum(1.0 * np.array(recs[c].accepted)) / nburn
                recs[c].lines.append('burnin acceptance rate : {0:.4f}'.format(rate))
                scales[c] = tune(scales[c], rate, recs[c].lines)
            recs[c].scale = scales[c]
        draws = [[] for _ in range(C)]
        for i in range(nit):
            u_state = np.random.get_state() if self.noise == 'numpy' else None
            for c in range(C):
                if u_state is not None:
                    np.random.set_state(u_state)
                qs[c], _ = self._step(qs[c], scales[c], rngs[c] if rngs else None, c, step, recs[c])
                draws[c].append(np.concatenate([np.reshape(qs[c][v], -1) for v in self.start]))
                if self._verbose and (i % (niter_print / 10) == 0):
                    acc = recs[c].accepted[nburn:]
                    recs[c].lines.append('acceptance rate : {0:.4f}'.format(np.sum(1.0 * np.array(acc)) / len(acc)))
            step += 1
        self.global_step = step
        sizes = [int(np.asarray(self.start[v]).size) for v in self.start]
        for c in range(C):
            flat = np.array(draws[c]).reshape(nit, sum(sizes))
            o, post = 0, {}
            for v, n in zip(self.start, sizes):
                post[v] = flat[:, o:o + n].copy()
                o += n
            recs[c].posterior = post
            recs[c].flat = flat
        return recs

    def sample(self, niter=1e3, burnin=100, rng=None):                        # metropolis.py:67-96
        if rng is None:
            rng = np.random.RandomState(0)
        self.records = self.run(niter, burnin, 1, [rng])
        self._scale = self.records[0].scale
        return self.records[0].posterior

    def multicore_sample(self, niter=1e4, burnin=1e3, ncores=2):              # metropolis.py:98-103
        entry = np.random.get_state()
        try:
            rngs = [np.random.RandomState(i) for i in range(ncores)]
            self.records = self.run(int(niter / ncores), burnin, ncores, rngs)
        finally:
            np.random.set_state(entry)
        return {var: np.concatenate([r.posterior[var] for r in self.records], axis=0) for var in self.start.keys()}


MVN_LAW = {"mu": np.zeros(2), "cov": np.array([[1.0, 0.8], [0.8, 1.0]])}


def mvn_ensemble(seed, C, burnin, niter, scale=1.0, chain=0):
    """Draws [C, niter, 2] of C independent noise='philox' chains on the MVN target of the law tests
    (mu 0, cov [[1, .8], [.8, 1]], start 0): the restatement's steps with the model's
    −negative_log_posterior written out once (precision and constant precomputed), so that an ensemble
    takes seconds."""
    mu, cov = MVN_LAW["mu"], MVN_LAW["cov"]
    prec = np.linalg.inv(cov)
    const = mu.shape[0] * np.log(2 * np.pi) + np.log(np.linalg.det(cov))

    def logp(X, y, q, hyper):
        d = q['x'] - mu
        return -0.5 * (const + np.dot(np.dot(d, prec), d))

    r = MH(None, None, logp, {'x': np.zeros(2)}, None, scale=scale, verbose=False, noise='philox', seed=seed,
           chain=chain)
    recs = r.run(niter, burnin, C, None)
    return np.stack([rec.flat for rec in recs], axis=0)
