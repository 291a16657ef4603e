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

The schedule, the device calls and the per-chain assembly are hmc's (``hmc._chains_fused``, of which
``hmc.sample`` is the C = 1 case); this module adds what is about several chains: the per-chain streams,
the global stream's save / restore, concatenation, the diagnostics and the per-chain fallback.
"""
import numpy as np
import torch

from dropout_hamiltonian_montecarlo_amd import diagnostics
from dropout_hamiltonian_montecarlo_amd._native import HmcxError

from .hmc import hmc
from .multicore import cpu_count


class hmc_multicore(hmc):
    _diag_trace = None             # [T, C, P] trace of the last sampling phase (device tensor on the fused paths)

    def sample_multicore(self, niter=1e4, burnin=1e3, ncores=cpu_count(), **args):   # hmc_multicore.py:22-38
        ncores = int(ncores)
        if ncores < 1:
            raise ValueError("ncores must be >= 1")
        niter_w, nburn = int(niter / ncores), int(burnin)                   # hmc_multicore.py:29-30
        entry = np.random.get_state()
        try:
            if self.model._hmcx_model == 'mvn_gaussian':
                results = self._chains_batched(niter_w, nburn, ncores, None)
            elif self._linear_fused():
                results = self._chains_batched(niter_w, nburn, ncores, args)
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

    # ------------------------------------------------------------------ chain-batched sampling
    def _chains_batched(self, niter_w, nburn, C, args):
        """hmc._chains_fused with C chains: chain c draws from RandomState(c) (noise='numpy'), burn-in
        losses are printed every nburn / 10 steps, the trace records hold the drawn L.  args None: the
        MVN model."""
        rngs = None
        if self.noise == 'numpy':
            rngs = [np.random.RandomState(c) for c in range(C)]
            for r in rngs:
                self.draw_momentum(r)                                        # hmc.py:93 consumes RNG
        results, traces, self._diag_trace = self._chains_fused(niter_w, nburn, C, rngs, args, nburn / 10)
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
