"""SGLD sampler — drop-in for hamiltonian/inference/cpu/sgld.py.

Reference step: /root/reference/hamiltonian/inference/cpu/sgld.py:31-46:
    p = N(0, (2ε)²)  (draw_momentum, noise_scale = 2ε);  p += −½ε·∇U(q);  q += p.
The CuPy file's variant (gpu/sgld.py:11-20) is the named mode ``variant='gpu'``:
p = ν⊙p_prev − ½ε∇U(q) with ν ~ N(0, (2ε)²) and p carried from step to step (zeros at the start
of ``sample``, gpu/sgmcmc.py:48), q += p.  The momentum lives on the device next to the state
(hmcx_sampler_args.pW/pb); the kernels fuse the extra multiply and store.  Default
``variant='cpu'``: the NumPy semantics, the parity target.

One SGLD step = one k_fwd + one k_grad launch (hmcx_sgld_run); the log-likelihood the
reference prints every 10 minibatches costs one extra forward launch on those steps only.

The dropout MLP (``_run_mlp``): one epoch is one hmcx_mlp_sgld_run call — per step hmcx_mlp_grad's unfused
launches into a gradient workspace and one element-wise kernel that draws the noise and applies the update
(8 launches), plus one forward per log line and one for the epoch-end negative_log_posterior.  Dropout masks are
Philox keyed by (seed, chain, global step, forward), ``sample(..., masks='off')`` runs without dropout, and
``mask_provider`` injects them (parity).  ``keep_every=k`` keeps every k-th sampling step's state on the device
(``device_draws``, the stacked layout ``mlp.posterior_predictive`` reads).

Several MLP chains (``chains=C``, 1 < C ≤ 64): one hmcx_mlp_sgld_chains_run per epoch, the chains as the problems
of batched launches (groups of at most 6) on shared minibatches.  ``start_p[var]`` is the variable's shape (every
chain starts there) or ``[C, *shape]``; the device state, ``last_state`` and ``last_momentum`` are ``[C, *shape]``,
``posterior[var]`` is ``[C, epochs, *shape]``, ``logp`` ``[C, epochs]``, ``loss_trace`` ``[n_steps, C]`` and
``device_draws[var]`` ``[C, T, *shape]`` (one buffer, written in place).  With Philox noise and masks chain c is,
bit for bit, the one-chain sampler with ``chain=chain + c``; ``noise='numpy'`` and ``mask_provider`` feed every
chain the same values (replicas, a parity mode), so ``noise='numpy'`` takes per-chain starts only: one shared
start under one noise stream raises, as ``chains=2`` on the MLP always did.  ``chain_diagnostics`` gives split-R̂
and ESS of the kept draws on the device.
"""
import ctypes

import numpy as np
import torch

from dropout_hamiltonian_montecarlo_amd import _native as nat
from dropout_hamiltonian_montecarlo_amd._native import HmcxError, ptr

from . import _mlp_call
from .sgmcmc import RunResult, sgmcmc


class sgld(sgmcmc):

    mask_provider = None    # MLP parity hook: f(global_step, n_forwards) -> [n_fwd, 3, B, n_mid] masks

    def __init__(self, model, start_p, path_length=1.0, step_size=0.1, verbose=True,
                 noise='numpy', seed=0, chain=0, chains=1, variant='cpu', keep_every=None):
        if variant not in ('cpu', 'gpu'):
            raise ValueError("variant must be 'cpu' (cpu/sgld.py) or 'gpu' (gpu/sgld.py)")
        if keep_every is not None and int(keep_every) < 1:
            raise ValueError("keep_every must be None or >= 1")
        self.variant = variant
        self.keep_every = None if keep_every is None else int(keep_every)   # MLP: device_draws
        self.device_draws = None
        self._mom = None
        self._mlp_masks_off = False
        self._mlp_sampling = None          # inside sample(): [burn-in calls left, sampling steps done, draw chunks]
        self._mlp_draw_buf = None          # inside sample(), chains > 1: the [C, T, *shape] draw buffers
        super().__init__(model, start_p, path_length=path_length, step_size=step_size, verbose=verbose,
                         noise=noise, seed=seed, chain=chain, chains=chains)

    def sample(self, epochs=1, burnin=1, batch_size=1, rng=None, **args):
        self._mom = None                       # p = zeros (gpu/sgmcmc.py:48)
        if self.model._hmcx_model == 'mlp':
            return self._sample_mlp(epochs, burnin, batch_size, rng, args)
        return super().sample(epochs=epochs, burnin=burnin, batch_size=batch_size, rng=rng, **args)

    def _momentum(self, state):
        if self._mom is None or any(self._mom[v].shape != state[v].shape for v in state):
            self._mom = {v: torch.zeros_like(state[v]) for v in state}
        return self._mom

    def _check_vars(self):
        if self.model._hmcx_model == 'mlp':
            from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import MLP_PARAM_NAMES
            if sorted(self.start.keys()) != sorted(MLP_PARAM_NAMES):
                raise HmcxError("sgld(mlp): start_p must hold exactly %s" % (MLP_PARAM_NAMES,))
            C = self.chains
            if C > 64:
                raise HmcxError("sgld(mlp): at most 64 chains per sampler")
            for k in self.start:
                shape, want = tuple(self.start[k].shape), self.model.shapes[k]
                if shape != want and not (C > 1 and shape == (C,) + want):
                    raise HmcxError("sgld(mlp): %s has shape %s, expected %s%s"
                                    % (k, shape, want, " or %s" % ((C,) + want,) if C > 1 else ""))
            self._order = [MLP_PARAM_NAMES.index(k) for k in self.start.keys()]
            if C > 1 and self.noise == 'numpy' and all(tuple(v.shape) == self.model.shapes[k]
                                                       for k, v in self.start.items()):
                # the host noise stream drives every chain (replicas): from one shared start the chains would be
                # copies of one another in all but their dropout masks, which says nothing about convergence
                raise HmcxError("sgld(mlp): chains=%d with noise='numpy' replays one noise stream in every chain; "
                                "give per-chain starts [%d, *shape] or use noise='philox'" % (C, C))
            if C > 1:
                # one start per chain, [C, *shape]; self.start keeps the per-chain shapes (chain 0's values)
                self._mlp_start = {k: np.array(np.broadcast_to(v, (C,) + self.model.shapes[k]))
                                   for k, v in self.start.items()}
                self.start = {k: v[0] for k, v in self._mlp_start.items()}
            return
        if self.model._hmcx_model != 'softmax' or list(self.start.keys()) != ['weights', 'bias']:
            raise HmcxError("sgld: libhmcx implements the softmax model with start_p keys ['weights', 'bias']")

    def _mlp_chains(self):
        return self.model._hmcx_model == 'mlp' and self.chains > 1

    def _init_state(self):
        if not self._mlp_chains():
            return super()._init_state()
        dt, dev = self.model.dtype, self.model.device
        return {k: torch.as_tensor(v).to(dev, dt).contiguous().clone() for k, v in self._mlp_start.items()}

    def _state_to_host(self, state):
        if not self._mlp_chains():
            return super()._state_to_host(state)
        return {k: state[k].detach().cpu().numpy().astype(np.float64) for k in self.start}   # [C, *shape]

    def _run(self, state, data, rows, eps, rng, batch_size):
        if self.model._hmcx_model == 'mlp':
            return self._run_mlp(state, data, rows, eps, rng, batch_size)
        Xd, Yd = data
        W, b = state['weights'], state['bias']
        C = self.chains
        D, K = W.shape[0], W.shape[1] // C
        P = D * K + K
        n_steps = len(rows)
        dev = self.model.device
        # noise offsets [n_steps, C]; numpy mode: every chain replays the same stream (replicas)
        noise_off = np.repeat(np.arange(n_steps, dtype=np.int64) * P, C)
        noise_d = None
        if self.noise == 'numpy':
            # sgld.py:45: rng.normal(0, 2ε, shape) per var = 2ε·N(0,1) (scaled on the device)
            noise_d = torch.from_numpy(rng.standard_normal(P * n_steps)).to(dev)
        want = np.zeros(n_steps, dtype=np.uint8)
        want[::self.log_every] = 1
        want[-1] = 1
        out_ll = torch.zeros(n_steps * C, dtype=torch.float64, device=dev)
        row0 = np.asarray(rows, dtype=np.int64)
        eps_a = np.asarray(eps, dtype=np.float64)
        a = nat.SamplerArgs()
        a.dtype = self.model.code
        a.B, a.D, a.K, a.C = batch_size, D, K, C
        a.n_steps = n_steps
        a.alpha = self.model.alpha
        a.log_prior = self._log_prior()
        a.X, a.Y = ptr(Xd), ptr(Yd)
        a.row0 = nat.addr(row0)
        a.eps = nat.addr(eps_a)
        a.want_ll = nat.addr(want)
        a.noise_mode = nat.NOISE_BUFFER if self.noise == 'numpy' else nat.NOISE_PHILOX
        a.noise = ptr(noise_d)
        a.noise_off = nat.addr(noise_off)
        a.seed, a.chain0, a.step_base = self.seed, self.chain, self.global_step & 0xFFFFFFFF
        a.W, a.b = ptr(W), ptr(b)
        if self.variant == 'gpu':
            mom = self._momentum(state)
            a.pW, a.pb = ptr(mom['weights']), ptr(mom['bias'])
        a.out_ll = ptr(out_ll)
        out_steps = None
        if self.record_steps:
            out_steps = torch.empty((n_steps, C, P), dtype=self.model.dtype, device=dev)
            a.out_trace = ptr(out_steps)
        ctx = nat.context(dev)
        # the call's verdict (include/hmcx.h out_abort): a fused wide-SGLD call that timed out in a team
        # round leaves W / b invalid; the start state is kept here and the call re-run on the three
        # launches — same noise, same result — so the call itself never waits for its stream
        out_abort = torch.zeros(1, dtype=torch.int32, device=dev)
        a.out_abort = ptr(out_abort)
        saved = [t.clone() for t in ((W, b) if self.variant != 'gpu' else (W, b, mom['weights'], mom['bias']))]
        ctx.check(ctx.lib.hmcx_sgld_run(ctx.h, a), "hmcx_sgld_run")
        ll = out_ll.cpu().numpy()
        if int(out_abort.item()):
            import sys
            print("[hmcx] wide SGLD: a team round timed out; call re-run on the three-launch path", file=sys.stderr)
            for t, s0 in zip((W, b) if self.variant != 'gpu' else (W, b, mom['weights'], mom['bias']), saved):
                t.copy_(s0)
            ctx.set_sgld_fuse(False)
            try:
                ctx.check(ctx.lib.hmcx_sgld_run(ctx.h, a), "hmcx_sgld_run (unfused re-run)")
            finally:
                ctx.set_sgld_fuse(True)
            ctx.note_recovery("sgld_wide_fused")
            ll = out_ll.cpu().numpy()
        del saved
        self.global_step += n_steps
        if C > 1:
            ll = ll.reshape(n_steps, C)
        if self.trace is not None:
            self.trace.extend({'L': 1.0, 'A': 1.0, 'accepted': True, 'eps': float(e)} for e in eps)
        return RunResult(np.ones(n_steps), np.ones(n_steps, dtype=bool), ll,
                         steps=out_steps.cpu().numpy() if out_steps is not None else None)

    def step(self, state, momentum, rng, **args):                         # sgld.py:31-39
        """variant='cpu': returns (q, None) — the drawn momentum is not part of the result the
        reference's loop uses.  variant='gpu' (gpu/sgld.py:11-20): ``momentum`` is p_prev (None =
        zeros) and (q, p) is returned."""
        if self.chains != 1:
            raise HmcxError("step() is the reference's single-chain API; use sample() for chains > 1")
        if self.model._hmcx_model == 'mlp':
            return self._step_mlp(state, momentum, rng, args)
        X, y = args['X_train'], args['y_train']
        data = self._upload_data(X, y)
        dev, dt = self.model.device, self.model.dtype

        def dev_copy(v):
            return torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v) \
                .to(dev, dt).contiguous().clone()

        st = {var: dev_copy(state[var]) for var in self.start}
        if self.variant == 'gpu':
            self._mom = {var: (dev_copy(momentum[var]).reshape(st[var].shape) if momentum is not None
                               else torch.zeros_like(st[var])) for var in self.start}
        self._run(st, data, [0], [self.step_size], rng, data[0].shape[0])
        return st, (self._mom if self.variant == 'gpu' else None)

    # ------------------------------------------------------------------ the dropout MLP
    def _sample_mlp(self, epochs, burnin, batch_size, rng, args):
        """sgmcmc.sample on the MLP: its loop of one call per epoch, with the draws of ``keep_every`` collected
        from the sampling epochs' calls and the device state / momentum left behind."""
        self._mlp_masks_off = _mlp_call.masks_off(args.get('masks', None))
        self._mlp_sampling = [int(burnin), 0, []]
        self.device_draws = None
        buf = None
        if self.chains > 1 and self.keep_every is not None:
            # the draws of every chain in one buffer [C, T, *shape] the calls write in place
            n_rows = len(range(0, args['X_train'].shape[0] - int(batch_size) + 1, int(batch_size)))
            T = int(epochs) * n_rows // self.keep_every
            buf = {k: torch.empty((self.chains, T) + self.model.shapes[k], dtype=self.model.dtype,
                                  device=self.model.device) for k in self.start}
        self._mlp_draw_buf = buf
        try:
            out = super().sample(epochs=epochs, burnin=burnin, batch_size=batch_size, rng=rng, **args)
            chunks = self._mlp_sampling[2]
        finally:
            self._mlp_sampling = None
            self._mlp_masks_off = False
            self._mlp_draw_buf = None
        if buf is not None:
            self.device_draws = buf
        elif self.keep_every is not None:
            dev, dt = self.model.device, self.model.dtype
            self.device_draws = {k: (torch.cat([c[k] for c in chunks]) if chunks else
                                     torch.empty((0,) + self.model.shapes[k], dtype=dt, device=dev))
                                 for k in self.start}
        self.last_momentum = self._mom if self.variant == 'gpu' else None
        return out

    def _run_mlp(self, state, data, rows, eps, rng, batch_size, evals=True):
        """len(rows) SGLD steps as one hmcx_mlp_sgld_run.  RunResult.ll[j] is the log line's loss (the mean CE
        at the updated state under fresh masks) where j % log_every == 0, RunResult.nlp[-1] the epoch-end
        negative_log_posterior; ``evals=False`` (step()) runs neither.  chains > 1: one
        hmcx_mlp_sgld_chains_run on the stacked state, ll / nlp / loss_trace with a trailing chain axis."""
        m = self.model
        Xd, yd = data
        dev = m.device
        B = int(batch_size)
        P = sum(int(np.prod(self.start[k].shape)) for k in self.start)
        n_steps = len(rows)
        row0 = np.asarray(rows, dtype=np.int64)
        eps_a = np.asarray(eps, dtype=np.float64)
        noise_off = np.arange(n_steps, dtype=np.int64) * P
        noise_d = None
        if self.noise == 'numpy':
            # sgld.py:45: rng.normal(0, 2ε, shape) per variable in start order = 2ε·N(0,1) (scaled on the device)
            noise_d = torch.from_numpy(np.asarray(rng.standard_normal(P * n_steps), dtype=np.float64)).to(dev)
        want = np.zeros(n_steps, dtype=np.uint8)
        if evals:
            want[::self.log_every] |= 1
            want[-1] |= 2
        n_fwd = 1 + (want & 1) + (want >> 1)
        n_evals = int(n_fwd.sum()) - n_steps
        mode, host_masks, mask_off, eval_off = _mlp_call.mask_plan(
            'off' if self._mlp_masks_off else None, self.mask_provider, self.global_step, n_fwd, B, m.n_mid, "sgld(mlp)")
        masks_d = None if host_masks is None else torch.from_numpy(host_masks).to(dev, m.dtype)
        # keep_every: every k-th sampling step (burn-in calls keep nothing)
        C = self.chains
        draw, want_draw, d0 = None, None, 0
        smp = self._mlp_sampling
        if smp is not None:
            if smp[0] > 0:
                smp[0] -= 1
            else:
                if self.keep_every is not None:
                    idx = smp[1] + np.arange(n_steps)
                    want_draw = ((idx + 1) % self.keep_every == 0).astype(np.uint8)
                    nd = int(want_draw.sum())
                    if C == 1:
                        draw = {k: torch.empty((nd,) + m.shapes[k], dtype=m.dtype, device=dev) for k in self.start}
                    else:                      # draw d0 onward of every chain's row of the [C, T, *shape] buffer
                        draw, d0 = self._mlp_draw_buf, smp[1] // self.keep_every
                    if nd == 0:
                        want_draw = None
                smp[1] += n_steps
        # one chain's outputs are the chain call's with C = 1: [n_steps, C], [n_evals, C], [n_evals, C, 6]
        f64 = dict(dtype=torch.float64, device=dev)
        out_loss = torch.empty((n_steps, C), **f64)
        ev_loss, ev_ss = torch.empty((max(n_evals, 1), C), **f64), torch.empty((max(n_evals, 1), C, 6), **f64)
        if C == 1:
            a = nat.MlpSgldArgs()
            a.chain = self.chain
        else:
            a = nat.MlpSgldChainsArgs()
            a.C, a.chain0 = C, self.chain
        a.dtype = m.code
        a.B, a.n_in, a.n_mid, a.n_out, a.n_steps = B, m.n_in, m.n_mid, m.n_out, n_steps
        a.order[:] = self._order
        a.variant = 1 if self.variant == 'gpu' else 0
        a.alpha = m.alpha
        a.X, a.y = ptr(Xd), ptr(yd)
        a.row0 = row0.ctypes.data_as(nat.c_i64p)
        a.eps = eps_a.ctypes.data_as(nat.c_dblp)
        a.want_eval = want.ctypes.data_as(nat.c_u8p)
        a.noise_mode = nat.NOISE_BUFFER if self.noise == 'numpy' else nat.NOISE_PHILOX
        a.noise = ptr(noise_d)
        a.noise_off = noise_off.ctypes.data_as(nat.c_i64p)
        a.mask_mode, a.masks = mode, ptr(masks_d)
        a.mask_off = mask_off.ctypes.data_as(nat.c_i64p)
        a.eval_mask_off = eval_off.ctypes.data_as(nat.c_i64p)
        a.seed, a.step_base = self.seed, self.global_step & 0xFFFFFFFF
        _mlp_call.fill_params(a.par, state)
        if self.variant == 'gpu':
            _mlp_call.fill_params(a.mom, self._momentum(state))
        if want_draw is not None:
            a.want_draw = want_draw.ctypes.data_as(nat.c_u8p)
            _mlp_call.fill_params(a.draws, draw if C == 1 else {k: draw[k][:, d0:] for k in draw})
            if C > 1:
                a.draw_stride = draw[_mlp_call.MLP_PARAM_NAMES[0]].shape[1]
        a.out_loss, a.out_eval_loss, a.out_eval_sumsq = ptr(out_loss), ptr(ev_loss), ptr(ev_ss)
        ctx = _mlp_call.mlp_context(self.model)
        if C == 1:
            ctx.check(ctx.lib.hmcx_mlp_sgld_run(ctx.h, ctypes.byref(a)), "hmcx_mlp_sgld_run")
        else:
            ctx.check(ctx.lib.hmcx_mlp_sgld_chains_run(ctx.h, ctypes.byref(a)), "hmcx_mlp_sgld_chains_run")
        self.global_step += n_steps
        shape = (n_steps,) if C == 1 else (n_steps, C)
        self.loss_trace = out_loss.cpu().numpy().reshape(shape)          # waits for the call
        el, ss = ev_loss.cpu().numpy(), ev_ss.cpu().numpy()
        del noise_d, masks_d
        if want_draw is not None and C == 1:
            smp[2].append(draw)
        ll, nlp = np.full((n_steps, C), np.nan), np.full((n_steps, C), np.nan)
        e = 0
        for s in range(n_steps):
            if want[s] & 1:
                ll[s] = el[e]
                e += 1
            if want[s] & 2:
                nlp[s] = _mlp_call.nlp_from_eval(m, self.start, el[e], ss[e])
                e += 1
        ll, nlp = ll.reshape(shape), nlp.reshape(shape)
        if self.trace is not None:
            self.trace.extend({'L': 1.0, 'A': 1.0, 'accepted': True, 'eps': float(e_)} for e_ in eps)
        return RunResult(np.ones(n_steps), np.ones(n_steps, dtype=bool), ll, nlp=nlp if evals else None)

    def chain_diagnostics(self, vars=None):
        """{var: (split_rhat, ess)} of the kept draws (``device_draws``, [C, T, *shape]), each of the variable's
        shape, computed on the device one variable at a time (diagnostics.device_diagnostics)."""
        from dropout_hamiltonian_montecarlo_amd import diagnostics
        d = self.device_draws
        if d is None:
            raise HmcxError("chain_diagnostics: no draws (sample with keep_every)")
        return diagnostics.draws_diagnostics(
            {k: d[k] if self.chains > 1 else d[k][None] for k in (list(d.keys()) if vars is None else list(vars))},
            lambda T: "chain_diagnostics: needs at least 4 draws per chain, has %d" % T)

    def _step_mlp(self, state, momentum, rng, args):
        """sgld.step on the MLP: one hmcx_mlp_sgld_run of one step on the given minibatch, no evaluation."""
        m = self.model
        data = m._xy(args)
        st = {k: m._dev(state[k]).reshape(m.shapes[k]).contiguous().clone() for k in self.start}
        if self.variant == 'gpu':
            self._mom = {k: (m._dev(momentum[k]).reshape(m.shapes[k]).contiguous().clone() if momentum is not None
                             else torch.zeros_like(st[k])) for k in self.start}
        off = self._mlp_masks_off
        self._mlp_masks_off = _mlp_call.masks_off(args.get('masks', None))
        try:
            self._run_mlp(st, data, [0], [self.step_size], rng, data[0].shape[0], evals=False)
        finally:
            self._mlp_masks_off = off
        return st, (self._mom if self.variant == 'gpu' else None)
