"""hmc_multicore — multi-chain full-batch HMC, the intent of hamiltonian/inference/cpu/hmc_multicore.py.

Reference: hamiltonian/inference/cpu/hmc_multicore.py:17-38 of the reference.  There,
``sample_multicore(niter, burnin, ncores, X_train=…, y_train=…)`` is meant to run one ``hmc.sample`` per
pool worker — worker i draws ``int(niter/ncores)`` samples after ``int(burnin)`` burn-in steps (burn-in
is not divided, line 30) from ``RandomState(i)`` — and to return the workers' results concatenated.  As
written it cannot run (the ``zip`` omits ``self``); this module serves the intent.

Here the ncores workers are ncores chains of ONE libhmcx call per phase:

* softmax (CPU prior) and logistic models: ``hmcx_hmc_chains_run`` — all chains share the two gradient
  GEMMs of every leapfrog evaluation (state in the [D][C·K] layout), each chain with its own path
  length, momentum and accept decision;
* the MVN model: ``hmcx_hmc_mvn_run`` with C = ncores (one thread per chain);
* anything else (MLP, GPU-prior softmax, a model that overrides grad): ``hmc.sample`` once per chain,
  in sequence.

Random streams.  ``noise='numpy'`` (hmc's default): chain c draws its momenta from ``RandomState(c)``
(including the discarded first draw of hmc.py:93); path lengths and accept uniforms come from the global
``np.random`` stream as it stands at entry, identically for every chain — what forked workers inherit
in the reference — and the global state is restored to its entry value on return (the reference's parent
process never draws from it).  Chain c therefore reproduces ``hmc.sample(niter_w, burnin,
RandomState(c))`` run from that global state.  ``noise='philox'``: chain c uses Philox chain id
``self.chain + c`` for momenta, path lengths (SLOT_PATH) and accept uniforms (SLOT_ACCEPT), so the
chains are independent and their trajectories ragged.

Return value: ``(posterior, sample_positions, sample_momentums, logp_samples)`` — the names of the
reference's return statement.  The reference fills them from mislabelled tuple indices of
``hmc.sample``'s ``(posterior, loss, positions, momentums)`` (its ``r[1]``, called sample_positions, is
the loss); here each name holds what it says: ``posterior[var]`` the chains' draws concatenated along
axis 0 (chain-major), ``sample_positions`` / ``sample_momentums`` one entry per chain (that chain's
``hmc.sample`` lists), ``logp_samples`` the chains' loss arrays concatenated.

BUFFER-mode momenta (noise='numpy') of one call are capped at NOISE_CHUNK float64 values (128 MiB); a
longer phase is split into several calls over consecutive steps, which changes no result (the carried
state of a call is recomputed by the same kernel on the same values).
"""
import numpy as np
import torch

from dropout_hamiltonian_montecarlo_amd import _native as nat
from dropout_hamiltonian_montecarlo_amd import diagnostics
from dropout_hamiltonian_montecarlo_amd._native import HmcxError, ptr

from .hmc import DualAveragingStepSize, hmc
from .multicore import cpu_count
from .sghmc import _n_iter


class hmc_multicore(hmc):
    NOISE_CHUNK = 1 << 24          # float64 momentum normals handed to one hmcx_hmc_chains_run call

    _diag_trace = None             # [T, C, P] trace of the last sampling phase (device tensor on the fused paths)

    def sample_multicore(self, niter=1e4, burnin=1e3, ncores=cpu_count(), **args):   # hmc_multicore.py:22-38
        ncores = int(ncores)
        if ncores < 1:
            raise ValueError("ncores must be >= 1")
        niter_w, nburn = int(niter / ncores), int(burnin)                   # hmc_multicore.py:29-30
        entry = np.random.get_state()
        try:
            if self.model._hmcx_model == 'mvn_gaussian':
                results = self._chains_fused(niter_w, nburn, ncores, None)
            elif self._linear_fused():
                results = self._chains_fused(niter_w, nburn, ncores, args)
            else:
                results = self._chains_sequential(niter_w, nburn, ncores, entry, args)
        finally:
            np.random.set_state(entry)
        posterior = {var: np.concatenate([r[0][var] for r in results], axis=0) for var in self.start.keys()}
        logp_samples = np.concatenate([r[1] for r in results], axis=0)
        sample_positions = [r[2] for r in results]
        sample_momentums = [r[3] for r in results]
        return posterior, sample_positions, sample_momentums, logp_samples

    def chain_diagnostics(self):
        """(split_rhat, ess) per parameter over the chains of the last sample_multicore call, computed on
        the device from the sampling phase's [C, T, P] trace (diagnostics.device_diagnostics)."""
        tr = self._diag_trace
        if tr is None:
            raise HmcxError("chain_diagnostics: no sample_multicore trace")
        if tr.shape[0] < 4:
            raise HmcxError("chain_diagnostics: need at least 4 draws per chain")
        if not isinstance(tr, torch.Tensor):                                 # the per-chain fallback's host rows
            tr = torch.as_tensor(tr, dtype=torch.float64).to(self.model.device)
        _, srhat, ess = diagnostics.device_diagnostics(tr.permute(1, 0, 2).to(torch.float64).contiguous())
        return srhat, ess

    # ------------------------------------------------------------------ schedules
    def _schedule(self, n_steps, C):
        """Path iterations and accept uniforms [n_steps, C], and the path lengths L."""
        if self.noise == 'numpy':
            n1 = np.empty(n_steps, dtype=np.int32)
            u1 = np.empty(n_steps, dtype=np.float64)
            L1 = np.empty(n_steps, dtype=np.float64)
            for s in range(n_steps):
                L1[s] = np.ceil(2 * np.random.rand() * self.path_length / self.step_size)   # hmc.py:46
                n1[s] = _n_iter(L1[s])
                u1[s] = np.random.rand()                                                    # hmc.py:61
            rep = lambda v: np.ascontiguousarray(np.repeat(v[:, None], C, axis=1))
            return rep(n1), rep(u1), rep(L1)
        eps = np.full(n_steps, self.step_size, dtype=np.float64)
        L, n_iter, u = nat.philox_schedule(self.seed, self.chain, C, self.global_step, self.path_length, eps)
        return n_iter, u, L

    def _momenta(self, n_steps, C, P, rngs, step0):
        """Host momenta [n_steps, C, P] of steps step0.. of the phase: per chain from its RandomState in
        step order (hmc.py:41), or the host twin of the device's float64 Philox stream (the MVN route;
        the linear models draw their Philox momenta on the device)."""
        noise = np.empty((n_steps, C, P), dtype=np.float64)
        if self.noise == 'numpy':
            for c in range(C):
                for s in range(n_steps):
                    mom = self.draw_momentum(rngs[c])
                    noise[s, c] = np.concatenate([np.reshape(mom[v], -1) for v in self.start])
        else:
            for s in range(n_steps):
                g = (self.global_step + step0 + s) & 0xFFFFFFFF
                for c in range(C):
                    noise[s, c] = nat.philox_normals(self.seed, self.chain + c, g, 0, 0, P, dtype="f64")
        return noise

    # ------------------------------------------------------------------ device calls
    def _hmc_chains_call(self, W, b, data, n_iter, u, noise=None, step_base=0, trace=None, mom=None):
        """One hmcx_hmc_chains_run call.  W [D, C·K], b [C·K] device tensors (updated in place); n_iter,
        u host [n_steps, C]; noise a device float64 tensor [n_steps, C, P] (BUFFER) or None (PHILOX);
        trace / mom device [n_steps, C, P] tensors in the model dtype or None.  Returns host arrays
        A, accepted, nlp [n_steps, C] and E [n_steps, C, 2]."""
        m = self.model
        Xd, Yd = data
        n_iter = np.ascontiguousarray(n_iter, dtype=np.int32)
        u = np.ascontiguousarray(u, dtype=np.float64)
        n_steps, C = n_iter.shape
        D = W.shape[0]
        K = W.shape[1] // C
        P = D * K + K
        dev = m.device
        eps = np.full(n_steps, self.step_size, dtype=np.float64)
        noff = np.arange(n_steps * C, dtype=np.int64) * P
        out_f = torch.empty(4 * n_steps * C, dtype=torch.float64, device=dev)     # A, nlp, E (2)
        out_acc = torch.empty(n_steps * C, dtype=torch.int32, device=dev)
        nsc = n_steps * C
        a = nat.HmcChainsArgs()
        self._linear_model_args(a, Xd, Yd, D, K, n_steps)
        a.C = C
        a.eps = eps.ctypes.data_as(nat.c_dblp)
        a.n_iter = n_iter.ctypes.data_as(nat.c_i32p)
        a.u_accept = u.ctypes.data_as(nat.c_dblp)
        a.noise_mode = nat.NOISE_BUFFER if noise is not None else nat.NOISE_PHILOX
        a.noise = ptr(noise)
        a.noise_off = noff.ctypes.data_as(nat.c_i64p)
        a.seed, a.chain0, a.step_base = self.seed, self.chain & 0xFFFFFFFF, step_base & 0xFFFFFFFF
        a.W, a.b = ptr(W), ptr(b)
        a.out_A, a.out_nlp, a.out_E = ptr(out_f[:nsc]), ptr(out_f[nsc:2 * nsc]), ptr(out_f[2 * nsc:])
        a.out_accepted = ptr(out_acc)
        a.out_trace, a.out_mom = ptr(trace), ptr(mom)
        ctx = nat.context(dev)
        ctx.check(ctx.lib.hmcx_hmc_chains_run(ctx.h, a), "hmcx_hmc_chains_run")
        f = out_f.cpu().numpy()
        return (f[:nsc].reshape(n_steps, C), out_acc.cpu().numpy().astype(bool).reshape(n_steps, C),
                f[nsc:2 * nsc].reshape(n_steps, C), f[2 * nsc:].reshape(n_steps, C, 2))

    def _linear_phase(self, st, n_steps, C, rngs, record):
        """One burn-in / sampling phase of the linear models: A, acc, nlp, L [n_steps, C] and, when
        recording, the host trace and momenta [n_steps, C, P]."""
        W, b, data, P = st
        n_iter, u, L = self._schedule(n_steps, C)
        dev, dt = self.model.device, self.model.dtype
        tr = torch.empty((n_steps, C, P), dtype=dt, device=dev) if record else None
        host_mom = self.noise == 'numpy'
        mo = torch.empty((n_steps, C, P), dtype=dt, device=dev) if (record and not host_mom) else None
        chunk = max(1, self.NOISE_CHUNK // (C * P)) if host_mom else n_steps
        outs, moms = [], []
        for s0 in range(0, n_steps, chunk):
            s1 = min(n_steps, s0 + chunk)
            noise = noise_d = None
            if host_mom:
                noise = self._momenta(s1 - s0, C, P, rngs, s0)
                noise_d = torch.from_numpy(noise.reshape(-1)).to(dev)
                if record:
                    moms.append(noise)
            outs.append(self._hmc_chains_call(W, b, data, n_iter[s0:s1], u[s0:s1], noise_d,
                                              self.global_step + s0, tr[s0:s1] if record else None,
                                              mo[s0:s1] if mo is not None else None))
        self.global_step += n_steps
        A, acc, nlp = (np.concatenate([o[i] for o in outs], axis=0) for i in range(3))
        trace = mom = None
        if record:
            self._diag_trace = tr
            trace = tr.cpu().numpy().astype(np.float64)
            mom = np.concatenate(moms, axis=0) if host_mom else mo.cpu().numpy().astype(np.float64)
        return A, acc, nlp, L, trace, mom

    def _mvn_phase(self, st, n_steps, C, rngs, record):
        """The same for the MVN model: hmcx_hmc_mvn_run with C chains, x [C, dim]."""
        x, dim = st
        m = self.model
        n_iter, u, L = self._schedule(n_steps, C)
        # both modes hand the device host-drawn momenta, as hmc._mvn_run does
        noise = self._momenta(n_steps, C, dim, rngs, 0)
        dev = m.device
        nsc = n_steps * C
        eps = np.full(n_steps, self.step_size, dtype=np.float64)
        noise_d = torch.from_numpy(noise.reshape(-1)).to(dev)
        noff = np.arange(nsc, dtype=np.int64) * dim
        out_A = torch.empty(nsc, dtype=torch.float64, device=dev)
        out_acc = torch.empty(nsc, dtype=torch.int32, device=dev)
        out_nlp = torch.empty(nsc, dtype=torch.float64, device=dev)
        out_tr = torch.empty((n_steps, C, dim), dtype=torch.float64, device=dev)
        a = nat.MvnArgs()
        a.dim, a.C, a.n_steps = dim, C, n_steps
        a.mu, a.prec, a.nlp_const = ptr(m.mu), ptr(m.prec), m.nlp_const
        a.eps = eps.ctypes.data_as(nat.c_dblp)
        a.n_iter = n_iter.ctypes.data_as(nat.c_i32p)
        a.u_accept = u.ctypes.data_as(nat.c_dblp)
        a.noise_mode = nat.NOISE_BUFFER
        a.noise = ptr(noise_d)
        a.noise_off = noff.ctypes.data_as(nat.c_i64p)
        a.seed, a.chain0, a.step_base = self.seed, self.chain & 0xFFFFFFFF, self.global_step & 0xFFFFFFFF
        a.x = ptr(x)
        a.out_A, a.out_accepted, a.out_nlp, a.out_trace = ptr(out_A), ptr(out_acc), ptr(out_nlp), ptr(out_tr)
        ctx = nat.context(dev)
        ctx.check(ctx.lib.hmcx_hmc_mvn_run(ctx.h, a), "hmcx_hmc_mvn_run")
        self.global_step += n_steps
        A = out_A.cpu().numpy().reshape(n_steps, C)
        acc = out_acc.cpu().numpy().astype(bool).reshape(n_steps, C)
        nlp = out_nlp.cpu().numpy().reshape(n_steps, C)
        trace = None
        if record:
            self._diag_trace = out_tr
            trace = out_tr.cpu().numpy()
        return A, acc, nlp, L, trace, noise

    # ------------------------------------------------------------------ chain-batched sampling
    def _chains_fused(self, niter_w, nburn, C, args):
        """All chains in one device call per phase; per chain, in chain order, what hmc.sample prints
        and returns.  args None: the MVN model."""
        m = self.model
        mvn = args is None
        rngs = [np.random.RandomState(c) for c in range(C)] if self.noise == 'numpy' else None
        if rngs:
            for r in rngs:
                self.draw_momentum(r)                                        # hmc.py:93 consumes RNG
        if mvn:
            x0 = np.asarray(self.start['x'], dtype=np.float64).reshape(-1)
            x = torch.as_tensor(np.tile(x0, (C, 1))).to(m.device).contiguous()
            st, phase = (x, x0.size), self._mvn_phase
            state = lambda: x.cpu().numpy().copy()                           # [C, dim]
            split = lambda flat: {'x': flat.reshape(np.shape(self.start['x'])).copy()}
        else:
            data = self._linear_data(args)
            D, K = np.shape(self.start['weights'])
            W = m._dev(self.start['weights']).clone().repeat(1, C).contiguous()          # [D][C·K]
            b = m._dev(np.reshape(self.start['bias'], -1)).clone().repeat(C).contiguous()
            st, phase = (W, b, data, D * K + K), self._linear_phase
            state = lambda: np.concatenate([W.cpu().numpy().reshape(D, C, K).transpose(1, 0, 2).reshape(C, D * K),
                                            b.cpu().numpy().reshape(C, K)], axis=1).astype(np.float64)
            split = self._split
        self._diag_trace = None
        burn = phase(st, nburn, C, rngs, False) if nburn > 0 else None
        before = state()
        samp = phase(st, niter_w, C, rngs, True) if niter_w > 0 else None
        if not mvn:
            self.last_state = {'weights': st[0], 'bias': st[1]}
        traces = [[] for _ in range(C)]
        results = []
        for c in range(C):
            p_accept = None
            if burn is not None:
                A, acc, nlp, L = burn[:4]
                for i in range(nburn):
                    if self.verbose is not None and (i % (nburn / 10) == 0):
                        print('loss: {0:.4f}'.format(nlp[i, c]), file=self.out)
                p_accept = A[-1, c]
                traces[c].extend({'L': float(L[i, c]), 'A': float(A[i, c]), 'accepted': bool(acc[i, c]),
                                  'eps': self.step_size} for i in range(nburn))
            _, avg_step_size = DualAveragingStepSize(self.step_size).update(p_accept)
            print('adapted step size : ', avg_step_size, file=self.out)
            if samp is None:
                results.append(({v: np.zeros((0,) + np.shape(self.start[v])) for v in self.start}, np.zeros(0), [], []))
                continue
            A, acc, nlp, L, tr, mom = samp
            traces[c].extend({'L': float(L[i, c]), 'A': float(A[i, c]), 'accepted': bool(acc[i, c]),
                              'eps': self.step_size} for i in range(niter_w))
            positions = [[split(before[c] if i == 0 else tr[i - 1, c])] for i in range(niter_w)]
            momentums = [[split(mom[i, c])] for i in range(niter_w)]
            for i in range(niter_w):
                if self.verbose and (i % (niter_w / 10) == 0):
                    print('loss: {0:.4f}'.format(nlp[i, c]), file=self.out)
            if mvn:
                posterior = {'x': tr[:, c].copy()}
            else:
                D, K = np.shape(self.start['weights'])
                posterior = {'weights': tr[:, c, :D * K].reshape((niter_w,) + np.shape(self.start['weights'])),
                             'bias': tr[:, c, D * K:].reshape((niter_w,) + np.shape(self.start['bias']))}
            results.append((posterior, nlp[:, c].copy(), positions, momentums))
        self._note_traces(traces)
        return results

    def _note_traces(self, traces):
        """chain_traces[c]: chain c's per-step records (L, A, accepted, eps); appended chain-major to
        self.trace when that is a list."""
        self.chain_traces = traces
        if self.trace is not None:
            for t in traces:
                self.trace.extend(t)

    # ------------------------------------------------------------------ one sample() per chain
    def _chains_sequential(self, niter_w, nburn, C, entry, args):
        """Models without a chain-batched entry: hmc.sample once per chain, in sequence, each from the
        entry state of the global stream, chain c with RandomState(c) and Philox chain id chain + c."""
        chain0, step0 = self.chain, self.global_step
        user_trace, traces, results = self.trace, [], []
        try:
            for c in range(C):
                np.random.set_state(entry)
                self.chain, self.global_step = chain0 + c, step0
                self.trace = []
                posterior, loss, positions, momentums = self.sample(niter_w, nburn, np.random.RandomState(c), **args)
                traces.append(self.trace)
                results.append((posterior, loss, positions, momentums))
        finally:
            self.chain, self.trace = chain0, user_trace
        self._diag_trace = None
        if niter_w > 0:
            flat = np.stack([np.concatenate([np.reshape(r[0][v], (niter_w, -1)) for v in self.start], axis=1)
                             for r in results], axis=1)                     # [T, C, P]
            self._diag_trace = flat                                          # host; uploaded on demand
        self._note_traces(traces)
        return results
