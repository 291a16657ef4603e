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
* the GPU dropout MLP with ``noise='philox'``, its own ``grad`` (``leapfrog_device_ok()``) and ``masks`` absent,
  ``None`` (Philox masks) or ``'off'``: ``hmcx_mlp_hmc_chains_run`` — momentum draw, trajectory, energies, accept,
  commit and trace of every step on the device, the chains as the problems of batched launches, one call per
  phase and nothing read back inside it.  The draws stay on the device as ``device_draws[var]`` ([C, T, *shape],
  what ``mlp.posterior_predictive`` and ``chain_diagnostics`` read without a copy), the final states as
  ``last_state[var]`` ([C, *shape]).  The drawn momenta are kept as a second [C, T, P] device buffer of the model's
  dtype (C·T·P·4 bytes in float32: 12 chains × 1000 draws of the 784-256-256-10 net, P = 269,322, are 12.9 GB
  beside the draws' 12.9 GB); ``keep_momentum=False`` leaves it out and the chains' momentum lists empty;
* anything else (the MLP with ``noise='numpy'`` or explicit mask lists, GPU-prior softmax, a model that overrides
  grad): ``hmc.sample`` once per chain, in sequence.

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
import ctypes

import numpy as np
import torch

from dropout_hamiltonian_montecarlo_amd import _native as nat
from dropout_hamiltonian_montecarlo_amd import diagnostics
from dropout_hamiltonian_montecarlo_amd._native import HmcxError

from . import _mlp_call
from .hmc import hmc
from .multicore import cpu_count


class hmc_multicore(hmc):
    _diag_trace = None             # [T, C, P] trace of the last sampling phase (device tensor on the fused paths)
    device_draws = None            # the MLP route: {var: [C, T, *shape]} device tensors of the last sampling phase
    last_state = None

    def __init__(self, *a, keep_momentum=True, **kw):
        super().__init__(*a, **kw)
        self.keep_momentum = bool(keep_momentum)

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
            elif self._mlp_fused(args):
                results = self._chains_mlp(niter_w, nburn, ncores, args)
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
        """Split-R̂ and ESS per parameter over the chains of the last sample_multicore call, computed on the device
        (diagnostics.device_diagnostics).  The MLP route (``device_draws`` set): ``{var: (split_rhat, ess)}``, each of
        the variable's shape, from the [C, T, *shape] draws, as ``sgld.chain_diagnostics`` returns them.  Every other
        route: the tuple ``(split_rhat, ess)`` over the flat parameter vector, from the sampling phase's [C, T, P]
        trace."""
        if self.device_draws is not None:                                    # the MLP route: per variable
            return diagnostics.draws_diagnostics(self.device_draws,
                                                 lambda T: "chain_diagnostics: need at least 4 draws per chain")
        tr = self._diag_trace
        if tr is None:
            raise HmcxError("chain_diagnostics: no sample_multicore trace")
        if tr.shape[0] < 4:
            raise HmcxError("chain_diagnostics: need at least 4 draws per chain")
        if not isinstance(tr, torch.Tensor):                                 # the per-chain fallback's host rows
            tr = torch.as_tensor(tr, dtype=torch.float64).to(self.model.device)
        _, srhat, ess = diagnostics.device_diagnostics(tr.permute(1, 0, 2).to(torch.float64).contiguous())
        return srhat, ess

    # ------------------------------------------------------------------ the dropout MLP: C chains per device call
    def _mlp_fused(self, args):
        """hmcx_mlp_hmc_chains_run serves the GPU mlp with its own grad, Philox momenta and Philox or no masks."""
        m = self.model
        ok = getattr(m, 'leapfrog_device_ok', None)
        if getattr(m, '_hmcx_model', None) != 'mlp' or self.noise != 'philox' or ok is None or not ok():
            return False
        masks = args.get('masks', None)
        return masks is None or (isinstance(masks, str) and masks == 'off')

    def _mlp_phase(self, par, data, order, mask_mode, n_steps, C, want_eval, record):
        """One phase: n_steps steps of C chains in one hmcx_mlp_hmc_chains_run on par (six [C, *shape] device
        tensors, canonical order, updated in place).  Returns host A, accepted, L [n_steps, C], the evaluations'
        loss [n_evals, C] and Σθ² [n_evals, C, 6], and when recording the device draws and momenta
        ({var: [C, n_steps, *shape]}, momenta None without keep_momentum)."""
        from ...models.gpu.mlp import MLP_PARAM_NAMES
        m = self.model
        X, y = data
        dev, dt = m.device, m.dtype
        eps = np.full(n_steps, self.step_size, dtype=np.float64)
        L, n_iter, u = nat.philox_schedule(self.seed, self.chain, C, self.global_step, self.path_length, eps)
        want_eval = np.ascontiguousarray(want_eval, dtype=np.uint8)
        n_evals = int(want_eval.sum())
        nsc = n_steps * C
        out_f = torch.empty(3 * nsc + 7 * max(n_evals, 1) * C, dtype=torch.float64, device=dev)   # A, E, loss, Σθ²
        out_acc = torch.empty(nsc, dtype=torch.int32, device=dev)
        a = nat.MlpHmcChainsArgs()
        a.dtype, a.B, a.n_in, a.n_mid, a.n_out, a.n_steps, a.C = m.code, X.shape[0], m.n_in, m.n_mid, m.n_out, n_steps, C
        a.order[:] = order
        a.alpha = m.alpha
        a.X, a.y = X.data_ptr(), y.data_ptr()
        a.eps = eps.ctypes.data_as(nat.c_dblp)
        a.n_iter = n_iter.ctypes.data_as(nat.c_i32p)
        a.u_accept = u.ctypes.data_as(nat.c_dblp)
        a.noise_mode, a.mask_mode = nat.NOISE_PHILOX, mask_mode
        a.seed, a.chain0, a.step_base = self.seed, self.chain & 0xFFFFFFFF, self.global_step & 0xFFFFFFFF
        _mlp_call.fill_params(a.par, par)
        o_ev = 3 * nsc
        a.out_A, a.out_E, a.out_accepted = nat.ptr(out_f[:nsc]), nat.ptr(out_f[nsc:3 * nsc]), nat.ptr(out_acc)
        a.want_eval = want_eval.ctypes.data_as(nat.c_u8p)
        a.out_eval_loss = nat.ptr(out_f[o_ev:o_ev + n_evals * C]) if n_evals else nat.ptr(out_f[o_ev:o_ev + 1])
        a.out_eval_sumsq = nat.ptr(out_f[o_ev + max(n_evals, 1) * C:])
        draws = moms = want_draw = None
        if record:
            want_draw = np.ones(n_steps, dtype=np.uint8)
            draws = [torch.empty((C, n_steps) + m.shapes[k], dtype=dt, device=dev) for k in MLP_PARAM_NAMES]
            a.want_draw, a.draw_stride = want_draw.ctypes.data_as(nat.c_u8p), n_steps
            _mlp_call.fill_params(a.draws, draws)
            if self.keep_momentum:
                moms = [torch.empty((C, n_steps) + m.shapes[k], dtype=dt, device=dev) for k in MLP_PARAM_NAMES]
                _mlp_call.fill_params(a.out_mom, moms)
        ctx = _mlp_call.mlp_context(self.model)
        ctx.check(ctx.lib.hmcx_mlp_hmc_chains_run(ctx.h, ctypes.byref(a)), "hmcx_mlp_hmc_chains_run")
        self.global_step += n_steps
        f = out_f.cpu().numpy()
        A = f[:nsc].reshape(n_steps, C)
        acc = out_acc.cpu().numpy().astype(bool).reshape(n_steps, C)
        loss = f[o_ev:o_ev + n_evals * C].reshape(n_evals, C)
        o_sq = o_ev + max(n_evals, 1) * C
        sumsq = f[o_sq:o_sq + 6 * n_evals * C].reshape(n_evals, C, 6)
        named = lambda ts: None if ts is None else dict(zip(MLP_PARAM_NAMES, ts))   # noqa: E731
        return A, acc, L, loss, sumsq, named(draws), named(moms)

    def _chains_mlp(self, niter_w, nburn, C, args):
        """The MLP route: burn-in and sampling as one device call each; per chain, in chain order, what hmc.sample
        prints and returns (hmc._chains_fused's assembly)."""
        from ...models.gpu.mlp import MLP_PARAM_NAMES
        m = self.model
        keys = list(self.start.keys())
        order = [MLP_PARAM_NAMES.index(k) for k in keys]
        if sorted(order) != list(range(6)):
            raise HmcxError("mlp: start must hold the six parameters, got %s" % (keys,))
        masks = args.get('masks', None)
        mask_mode = nat.MLP_MASKS_NONE if masks == 'off' else nat.MLP_MASKS_PHILOX
        data = m._xy(args)
        par = [m._dev(self.start[k]).reshape(m.shapes[k]).unsqueeze(0).repeat((C,) + (1,) * len(m.shapes[k])).contiguous()
               for k in MLP_PARAM_NAMES]
        npdt = torch.empty(0, dtype=m.dtype).numpy().dtype
        nlp = lambda loss, sumsq: _mlp_call.nlp_from_eval(m, keys, loss, sumsq)   # noqa: E731
        burn = None
        burn_print = nburn / 10
        if nburn > 0:
            flags = np.array([self.verbose is not None and (i % burn_print == 0) for i in range(nburn)], dtype=np.uint8)
            A, acc, L, loss, sumsq, _, _ = self._mlp_phase(par, data, order, mask_mode, nburn, C, flags, False)
            burn = (A, acc, L, nlp(loss, sumsq))
        before = [t.cpu().numpy().astype(npdt) for t in par]                   # [C, *shape] per variable
        samp = None
        self.device_draws = None
        if niter_w > 0:
            A, acc, L, loss, sumsq, draws, moms = self._mlp_phase(par, data, order, mask_mode, niter_w, C,
                                                                  np.ones(niter_w, dtype=np.uint8), True)
            samp = (A, acc, L, nlp(loss, sumsq))
            self.device_draws = {k: draws[k] for k in keys}
            host = {k: draws[k].cpu().numpy() for k in keys}
            hmom = None if moms is None else {k: moms[k].cpu().numpy() for k in keys}
        self.last_state = {k: par[MLP_PARAM_NAMES.index(k)] for k in keys}
        self._diag_trace = None
        first = lambda c: {k: before[MLP_PARAM_NAMES.index(k)][c] for k in keys}   # noqa: E731
        results, traces = self._assemble_chains(
            C, nburn, niter_w, burn and burn[:3], burn and burn[3], samp,
            lambda c: {k: host[k][c] for k in keys},
            lambda c, i: first(c) if i == 0 else {k: host[k][c, i - 1] for k in keys},
            None if samp is None or hmom is None else lambda c, i: {k: hmom[k][c, i] for k in keys})
        self._note_traces(traces)
        return results

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
        self.device_draws = None
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
        self._diag_trace = self.device_draws = None
        if niter_w > 0:
            flat = np.stack([np.concatenate([np.reshape(r[0][v], (niter_w, -1)) for v in self.start], axis=1)
                             for r in results], axis=1)                     # [T, C, P]
            self._diag_trace = flat                                          # host; uploaded on demand
        self._note_traces(traces)
        return results
