"""Random-walk Metropolis — drop-in for hamiltonian/inference/cpu/metropolis.py (class MH).

Reference: hamiltonian/inference/cpu/metropolis.py:14-128.  step (:27-32) proposes per variable
``q_new[var] += factor·scale·N(0, 1)`` with ``factor = exp(U(−1.5, 1.5))`` (every coordinate, or one
``randint(dim)`` coordinate with ``update_sequential=False``, :53-64) and accepts iff
``isfinite(A) and rand() < A`` with ``A = exp(E − E_new)``, ``E = −logp`` (:38-50) — there is no
min(1, ·), so an overflowing ratio is rejected.  sample (:67-96) runs the burn-in, tunes the scale once from
its acceptance rate (:105-128), then samples; multicore_sample (:98-103) runs one sample per worker
from ``RandomState(i)`` and concatenates.

``logp`` may be a libhmcx model (``logp = log_likelihood + log_prior``; ``−negative_log_posterior`` for the
MVN model; ``hyper`` may be None) or any callable ``logp(X, y, q, hyper)``.

* softmax (CPU prior), logistic and MVN models: a burn-in or sampling phase of C chains is ONE library
  call (hmcx_mh_run / hmcx_mh_mvn_run): proposal, energies, accept, commit and trace run on the device,
  the host draws the schedule (factors, sites, accept uniforms and, with noise='numpy', the normals) in
  the reference's order and tunes the scales between the phases.  ``sample`` is the C = 1 case of
  ``multicore_sample``'s code (_chains_fused).
* a callable, or any other model object (MLP, GPU-prior softmax): the reference's loop on the host.

Random streams (hmc_multicore's convention).  noise='numpy': chain c draws factors, sites and normals
from ``RandomState(c)`` (``sample``: the caller's rng); the accept uniforms come from the global
``np.random`` as it stands at entry, identically for every chain, and ``multicore_sample`` restores the
global state on return.  noise='philox': factors and sites from ``philox_uniforms(seed, chain + c, step,
SLOT_PATH, 4)`` (u0, u1 → ``exp(−1.5 + 3u)``; u2, u3 → ``floor(u·dim)``), the accept uniform from
SLOT_ACCEPT, the normals on the device (slot 0).
"""
import sys
from copy import deepcopy

import numpy as np
import torch

from dropout_hamiltonian_montecarlo_amd import _native as nat
from dropout_hamiltonian_montecarlo_amd import diagnostics
from dropout_hamiltonian_montecarlo_amd._native import HmcxError, ptr

from .hmc import hmc


def _tune(scale, acc_rate):
    """metropolis.py:105-128: the new scale and the message the reference prints (None: unchanged)."""
    for test, msg, f in ((acc_rate < 0.001, 'reduce by 90 percent', 0.1),
                         (acc_rate < 0.05, 'reduce by 50 percent', 0.5),
                         (acc_rate < 0.2, 'reduce by ten percent', 0.9),
                         (acc_rate > 0.95, 'increase by factor of ten', 10.0),
                         (acc_rate > 0.75, 'increase by double', 2.0),
                         (acc_rate > 0.5, 'increase by ten percent', 1.1)):
        if test:
            return scale * f, msg
    return scale, None


class MH:
    NOISE_CHUNK = hmc.NOISE_CHUNK      # float64 normals handed to one library call (noise='numpy')

    def __init__(self, X, y, logp, start, hyper, scale=1.0, update_sequential=True, verbose=True,
                 noise='numpy', seed=0, chain=0):
        self.start = start
        self.hyper = hyper
        self.model = logp if getattr(logp, '_hmcx_model', None) is not None else None
        if self.model is None and not callable(logp):
            raise HmcxError("MH: logp must be a libhmcx model or a callable logp(X, y, q, hyper)")
        self.logp = self._model_logp if self.model is not None else logp
        self._update_sequential = update_sequential
        self._scale = scale
        self._log_factor = 1.5
        self._verbose = verbose
        self.X = X
        self.y = y
        if noise not in ('numpy', 'philox'):
            raise ValueError("noise must be 'numpy' or 'philox'")
        self.noise = noise
        self.seed, self.chain = int(seed), int(chain)
        self.global_step = 0
        self.out = sys.stdout
        self.scale, self.scales, self.accepted, self.chain_traces = scale, None, None, None
        self._diag_trace = None

    # ------------------------------------------------------------------ the reference's host surface
    def _model_logp(self, X, y, q, hyper):
        m = self.model
        if m._hmcx_model == 'mvn_gaussian':
            return -m.negative_log_posterior(q)
        return m.log_likelihood(q, X_train=X, y_train=y) + m.log_prior(q)

    def energy(self, q):                                                     # metropolis.py:49-50
        return -self.logp(self.X, self.y, q, self.hyper)

    def acceptance_rate(self, accepted, samples):                            # metropolis.py:34-35
        return np.sum(1.0 * np.array(accepted)) / len(samples)

    def accept(self, current_q, proposal_q):                                 # metropolis.py:38-46
        accept = False
        E_new = self.energy(proposal_q)
        E = self.energy(current_q)
        with np.errstate(over='ignore', invalid='ignore'):
            A = np.exp(E - E_new)
        g = np.random.rand()
        if np.isfinite(A) and (g < A):
            accept = True
        return accept

    def random_walk(self, q, rng):                                           # metropolis.py:53-64
        q_new = {var: np.asarray(q[var]).flatten() for var in self.start.keys()}
        for var in self.start.keys():
            factor = np.exp(rng.uniform(-self._log_factor, self._log_factor))
            dim = (np.array(self.start[var])).size
            if self._update_sequential:
                q_new[var] += factor * self._scale * rng.normal(0.0, 1.0, dim)
            else:
                ind = rng.randint(dim)
                q_new[var][ind] += factor * self._scale * rng.normal(0.0, 1.0)
            q_new[var] = q_new[var].reshape(np.shape(self.start[var]))
        return q_new

    def step(self, q, rng):                                                  # metropolis.py:27-32
        q_new = self.random_walk(q, rng)
        accepted = self.accept(q, q_new)
        if accepted:
            q = deepcopy(q_new)
        return q, accepted

    def tune(self, acc_rate):                                                # metropolis.py:105-128
        new_scale, msg = _tune(self._scale, acc_rate)
        if msg:
            print(msg, file=self.out)
        return new_scale

    # ------------------------------------------------------------------ public sampling entry points
    def sample(self, niter=1e3, burnin=100, rng=None):                        # metropolis.py:67-96
        if rng is None:
            rng = np.random.RandomState(0)
        if self._route() is None:
            post, scale, rec = self._sample_host(niter, burnin, rng)
            self._note([rec], [scale], np.concatenate([post[v] for v in self.start], axis=1)[:, None, :])
        else:
            posts, scales = self._chains_fused(niter, burnin, 1, [rng], niter)
            post, scale = posts[0], scales[0]
        self._scale = self.scale = scale
        return post

    def multicore_sample(self, niter=1e4, burnin=1e3, ncores=2):              # metropolis.py:98-103
        ncores = int(ncores)
        if ncores < 1:
            raise ValueError("ncores must be >= 1")
        niter_w = int(niter / ncores)
        entry = np.random.get_state()
        try:
            if self._route() is None:
                posts, scales = self._chains_host(niter_w, burnin, ncores, entry)
            else:
                rngs = [np.random.RandomState(i) for i in range(ncores)] if self.noise == 'numpy' else None
                posts, scales = self._chains_fused(niter_w, burnin, ncores, rngs, niter_w)
        finally:
            np.random.set_state(entry)
        self.scales = np.array(scales, dtype=np.float64)
        return {var: np.concatenate([p[var] for p in posts], axis=0) for var in self.start.keys()}

    def chain_diagnostics(self):
        """(split_rhat, ess) per parameter over the chains of the last sampling phase, computed on the
        device from its [T, C, P] trace (diagnostics.device_diagnostics)."""
        tr = self._diag_trace
        if tr is None:
            raise HmcxError("chain_diagnostics: no sampling trace")
        if tr.shape[0] < 4:
            raise HmcxError("chain_diagnostics: need at least 4 draws per chain")
        if not isinstance(tr, torch.Tensor):                                 # the host loop's rows
            tr = torch.as_tensor(tr, dtype=torch.float64).to(nat.context().device)
        _, srhat, ess = diagnostics.device_diagnostics(tr.permute(1, 0, 2).to(torch.float64).contiguous())
        return srhat, ess

    # ------------------------------------------------------------------ routing
    def _route(self):
        """'linear', 'mvn' or None (the host loop)."""
        m = self.model
        if m is None:
            return None
        keys = list(self.start.keys())
        if m._hmcx_model == 'mvn_gaussian' and keys == ['x']:
            return 'mvn'
        if (m._hmcx_model in ('softmax', 'logistic') and getattr(m, 'prior', 'cpu') == 'cpu'
                and keys == ['weights', 'bias']):
            return 'linear'
        return None

    def _dims(self):
        return [int(np.asarray(self.start[v]).size) for v in self.start]

    def _note(self, recs, scales, trace):
        """chain_traces[c]: chain c's per-step records (burn-in, then sampling); accepted: the sampling
        phase's flags [niter, C]; scales; the [T, C, P] trace chain_diagnostics reads."""
        self.chain_traces = recs
        self.scales = np.array(scales, dtype=np.float64)
        self._diag_trace = trace

    # ------------------------------------------------------------------ host loop (callables, other models)
    def _sample_host(self, niter, burnin, rng):
        """metropolis.py:67-96 verbatim, for one chain; returns (posterior, tuned scale, step records)."""
        samples, burnin_samples, accepted, rec = [], [], [], []
        q = self.start
        scale0 = self._scale
        try:
            for i in range(int(burnin)):
                q, a = self.step(q, rng)
                burnin_samples.append(q)
                accepted.append(a)
                rec.append({'accepted': bool(a)})
                if i == burnin - 1:
                    acc_rate = self.acceptance_rate(accepted, burnin_samples)
                    print('burnin acceptance rate : {0:.4f}'.format(acc_rate), file=self.out)
                    del accepted[:]
                    del burnin_samples[:]
                    self._scale = self.tune(acc_rate)
            for i in range(int(niter)):
                q, a = self.step(q, rng)
                samples.append(q)
                accepted.append(a)
                rec.append({'accepted': bool(a)})
                if self._verbose and (i % (niter / 10) == 0):
                    print('acceptance rate : {0:.4f}'.format(self.acceptance_rate(accepted, samples)), file=self.out)
            scale = self._scale
        finally:
            self._scale = scale0
        posterior = {var: [] for var in self.start.keys()}
        for s in samples:
            for var in self.start.keys():
                posterior[var].append(np.asarray(s[var]).reshape(-1))
        for var, dim in zip(self.start.keys(), self._dims()):
            posterior[var] = np.array(posterior[var]).reshape(len(samples), dim)
        self.accepted = np.array(accepted, dtype=bool).reshape(-1, 1)
        return posterior, scale, rec

    def _chains_host(self, niter_w, burnin, C, entry):
        """One host-loop sample per chain, in sequence, each from the entry state of the global stream,
        chain c with RandomState(c)."""
        posts, scales, recs, acc = [], [], [], []
        for c in range(C):
            np.random.set_state(entry)
            post, scale, rec = self._sample_host(niter_w, burnin, np.random.RandomState(c))
            posts.append(post); scales.append(scale); recs.append(rec); acc.append(self.accepted[:, 0])
        self.accepted = np.stack(acc, axis=1) if acc else None
        trace = None
        if niter_w > 0:
            trace = np.stack([np.concatenate([p[v] for v in self.start], axis=1) for p in posts], axis=1)
        self._note(recs, scales, trace)
        return posts, scales

    # ------------------------------------------------------------------ fused routes: C chains per call
    def _schedule(self, n_steps, C, rngs, scales, step0, want_noise):
        """Steps step0.. of a phase for C chains: mult, site [n_steps, C, V] (V variables), accept
        uniforms u [n_steps, C], and with want_noise the normals [n_steps, C, P] (zero where no coordinate
        is updated).  noise='numpy': per step the reference's draw order — metropolis.py:56-62 per chain
        from its rng (variables in start order), then :43 one accept uniform from the global np.random,
        shared by the chains."""
        dims = self._dims()
        V, P = len(dims), sum(dims)
        mult = np.empty((n_steps, C, V), dtype=np.float64)
        site = np.full((n_steps, C, V), -1, dtype=np.int32)
        seq = self._update_sequential
        if self.noise == 'numpy':
            u = np.empty((n_steps, C), dtype=np.float64)
            z = np.zeros((n_steps, C, P), dtype=np.float64)
            for s in range(n_steps):
                for c in range(C):
                    rng, off = rngs[c], 0
                    for k, dim in enumerate(dims):
                        factor = np.exp(rng.uniform(-self._log_factor, self._log_factor))
                        if seq:
                            z[s, c, off:off + dim] = rng.normal(0.0, 1.0, dim)
                        else:
                            ind = rng.randint(dim)
                            z[s, c, off + ind] = rng.normal(0.0, 1.0)
                            site[s, c, k] = ind
                        mult[s, c, k] = factor * scales[c]
                        off += dim
                u[s, :] = np.random.rand()
            return mult, site, u, z
        g0 = self.global_step + step0
        steps = ((g0 + np.arange(n_steps, dtype=np.int64)) & 0xFFFFFFFF)[:, None]
        chains = ((self.chain + np.arange(C, dtype=np.int64)) & 0xFFFFFFFF)[None, :]
        sc = np.asarray(scales, dtype=np.float64)[None, :]
        for k, dim in enumerate(dims):
            uf = nat.philox_uniforms_chains(self.seed, chains, steps, nat.SLOT_PATH, k)
            mult[:, :, k] = np.exp(-self._log_factor + 2 * self._log_factor * uf) * sc
            if not seq:
                us = nat.philox_uniforms_chains(self.seed, chains, steps, nat.SLOT_PATH, 2 + k)
                site[:, :, k] = np.minimum(np.floor(us * dim).astype(np.int64), dim - 1)
        u = nat.philox_uniforms_chains(self.seed, chains, steps, nat.SLOT_ACCEPT, 0)
        return mult, site, np.ascontiguousarray(u), None

    def _linear_call(self, st, mult, site, u, noise, step_base, trace):
        """One hmcx_mh_run call; returns host A, accepted, logp [n_steps, C]."""
        W, b, data, D, K = st
        m = self.model
        n_steps, C = u.shape
        P = D * K + K
        dev = m.device
        nsc = n_steps * C
        mult = np.ascontiguousarray(mult, dtype=np.float64)
        site = np.ascontiguousarray(site, dtype=np.int32)
        u = np.ascontiguousarray(u, dtype=np.float64)
        noff = np.arange(nsc, dtype=np.int64) * P
        out_f = torch.empty(2 * nsc, dtype=torch.float64, device=dev)
        out_acc = torch.empty(nsc, dtype=torch.int32, device=dev)
        a = nat.MhArgs()
        a.dtype, a.model = m.code, nat.MODEL_LOGISTIC if m._hmcx_model == 'logistic' else nat.MODEL_SOFTMAX
        a.B, a.D, a.K, a.C, a.n_steps = data[0].shape[0], D, K, C, n_steps
        a.alpha = m.alpha
        if m._hmcx_model == 'logistic':                                        # logistic.py:15-21
            for i, dim in enumerate(self._dims()):
                a.lp_const[i] = dim * 0.5 * np.log(m.hyper['alpha'] / (2 * np.pi))
        else:
            a.log_prior = m.log_prior_const([np.shape(self.start[v]) for v in self.start])
        a.X, a.Y = ptr(data[0]), ptr(data[1])
        a.mult = mult.ctypes.data_as(nat.c_dblp)
        a.site = site.ctypes.data_as(nat.c_i32p)
        a.u_accept = u.ctypes.data_as(nat.c_dblp)
        a.noise_mode = nat.NOISE_BUFFER if noise is not None else nat.NOISE_PHILOX
        a.noise = ptr(noise)
        a.noise_off = noff.ctypes.data_as(nat.c_i64p)
        a.seed, a.chain0, a.step_base = self.seed, self.chain & 0xFFFFFFFF, step_base & 0xFFFFFFFF
        a.W, a.b = ptr(W), ptr(b)
        a.out_A, a.out_logp, a.out_accepted = ptr(out_f[:nsc]), ptr(out_f[nsc:]), ptr(out_acc)
        a.out_trace = ptr(trace)
        ctx = nat.context(dev)
        ctx.check(ctx.lib.hmcx_mh_run(ctx.h, a), "hmcx_mh_run")
        f = out_f.cpu().numpy()
        return (f[:nsc].reshape(n_steps, C), out_acc.cpu().numpy().astype(bool).reshape(n_steps, C),
                f[nsc:].reshape(n_steps, C))

    def _mvn_call(self, st, mult, site, u, noise, step_base, trace):
        """One hmcx_mh_mvn_run call; returns host A, accepted, logp [n_steps, C]."""
        x, dim = st
        m = self.model
        n_steps, C = u.shape
        dev = m.device
        nsc = n_steps * C
        mult = np.ascontiguousarray(mult.reshape(n_steps, C), dtype=np.float64)
        site = np.ascontiguousarray(site.reshape(n_steps, C), dtype=np.int32)
        u = np.ascontiguousarray(u, dtype=np.float64)
        noff = np.arange(nsc, dtype=np.int64) * dim
        out_f = torch.empty(2 * nsc, dtype=torch.float64, device=dev)
        out_acc = torch.empty(nsc, dtype=torch.int32, device=dev)
        a = nat.MhMvnArgs()
        a.dim, a.C, a.n_steps = dim, C, n_steps
        a.mu, a.prec, a.nlp_const = ptr(m.mu), ptr(m.prec), m.nlp_const
        a.mult = mult.ctypes.data_as(nat.c_dblp)
        a.site = site.ctypes.data_as(nat.c_i32p)
        a.u_accept = u.ctypes.data_as(nat.c_dblp)
        a.noise_mode = nat.NOISE_BUFFER if noise is not None else nat.NOISE_PHILOX
        a.noise = ptr(noise)
        a.noise_off = noff.ctypes.data_as(nat.c_i64p)
        a.seed, a.chain0, a.step_base = self.seed, self.chain & 0xFFFFFFFF, step_base & 0xFFFFFFFF
        a.x = ptr(x)
        a.out_A, a.out_logp, a.out_accepted = ptr(out_f[:nsc]), ptr(out_f[nsc:]), ptr(out_acc)
        a.out_trace = ptr(trace)
        ctx = nat.context(dev)
        ctx.check(ctx.lib.hmcx_mh_mvn_run(ctx.h, a), "hmcx_mh_mvn_run")
        f = out_f.cpu().numpy()
        return (f[:nsc].reshape(n_steps, C), out_acc.cpu().numpy().astype(bool).reshape(n_steps, C),
                f[nsc:].reshape(n_steps, C))

    def _phase(self, call, st, P, tdtype, n_steps, C, rngs, scales, record):
        """One burn-in / sampling phase: A, acc, logp, mult, site [n_steps, C(, V)] and the device trace
        [n_steps, C, P] when recording.  One library call, unless the host normals of noise='numpy' exceed
        NOISE_CHUNK values: then consecutive calls over consecutive steps, which changes no result."""
        dev = self.model.device
        host_noise = self.noise == 'numpy'
        tr = torch.empty((n_steps, C, P), dtype=tdtype, device=dev) if record else None
        chunk = max(1, self.NOISE_CHUNK // (C * P)) if host_noise else n_steps
        outs, mults, sites = [], [], []
        for s0 in range(0, n_steps, chunk):
            s1 = min(n_steps, s0 + chunk)
            mult, site, u, z = self._schedule(s1 - s0, C, rngs, scales, s0, host_noise)
            mults.append(mult); sites.append(site)
            noise = torch.from_numpy(z.reshape(-1)).to(dev) if host_noise else None
            outs.append(call(st, mult, site, u, noise, self.global_step + s0, tr[s0:s1] if record else None))
        self.global_step += n_steps
        A, acc, logp = (np.concatenate([o[i] for o in outs], axis=0) for i in range(3))
        return A, acc, logp, np.concatenate(mults, axis=0), np.concatenate(sites, axis=0), tr

    def _chains_fused(self, niter, burnin, C, rngs, niter_print):
        """C chains, one library call per phase; per chain, in chain order, what MH.sample prints and
        returns.  niter_print: the niter of the reference's print test ``i % (niter/10) == 0``."""
        m = self.model
        nit, nburn = int(niter), int(burnin)
        if self._route() == 'mvn':
            x0 = np.asarray(self.start['x'], dtype=np.float64).reshape(-1)
            x = torch.as_tensor(np.tile(x0, (C, 1))).to(m.device).contiguous()
            st, call, P, tdtype = (x, x0.size), self._mvn_call, x0.size, torch.float64
        else:
            data = tuple(t.contiguous() for t in m._xy({'X_train': self.X, 'y_train': self.y}))
            D, K = np.shape(self.start['weights'])
            W = m._dev(self.start['weights']).clone().repeat(1, C).contiguous()          # [D][C·K]
            b = m._dev(np.reshape(self.start['bias'], -1)).clone().repeat(C).contiguous()
            st, call, P, tdtype = (W, b, data, D, K), self._linear_call, D * K + K, m.dtype
            self.last_state = {'weights': W, 'bias': b}
        scales = [self._scale] * C
        recs = [[] for _ in range(C)]

        def note(ph):
            A, acc, logp, mult, site = ph[:5]
            for c in range(C):
                recs[c].extend({'A': float(A[i, c]), 'accepted': bool(acc[i, c]), 'logp': float(logp[i, c]),
                                'mult': mult[i, c].tolist(), 'site': site[i, c].tolist()} for i in range(A.shape[0]))

        burn = self._phase(call, st, P, tdtype, nburn, C, rngs, scales, False) if nburn > 0 else None
        lines = [[] for _ in range(C)]
        out = self.out
        if burn is not None:
            note(burn)
            for c in range(C):
                acc_rate = np.sum(1.0 * np.array(burn[1][:, c])) / nburn         # metropolis.py:35, :79
                lines[c].append('burnin acceptance rate : {0:.4f}'.format(acc_rate))
                scales[c], msg = _tune(scales[c], acc_rate)
                if msg:
                    lines[c].append(msg)
        samp = self._phase(call, st, P, tdtype, nit, C, rngs, scales, True) if nit > 0 else None
        tr = None
        if samp is not None:
            note(samp)
            tr = samp[5].cpu().numpy().astype(np.float64)                     # [niter, C, P]
            self.accepted = samp[1]
        else:
            self.accepted = np.zeros((0, C), dtype=bool)
        dims, posts = self._dims(), []
        for c in range(C):
            for line in lines[c]:
                print(line, file=out)
            if samp is not None and self._verbose:
                acc = samp[1][:, c]
                for i in range(nit):
                    if i % (niter_print / 10) == 0:
                        print('acceptance rate : {0:.4f}'.format(np.sum(1.0 * acc[:i + 1]) / (i + 1)), file=out)
            o, post = 0, {}
            for v, n in zip(self.start, dims):
                post[v] = tr[:, c, o:o + n].copy() if tr is not None else np.zeros((0, n))
                o += n
            posts.append(post)
        self._note(recs, scales, samp[5] if samp is not None else None)
        return posts, scales
