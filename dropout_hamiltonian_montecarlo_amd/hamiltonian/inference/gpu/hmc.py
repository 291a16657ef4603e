"""Full-batch HMC — drop-in for hamiltonian/inference/{cpu,gpu}/hmc.py.

Reference: /root/reference/hamiltonian/inference/cpu/hmc.py:11-176.
step (hmc.py:39-64): per var  p −= ½ε·g;  q += ε·p;  g = ∇U(q);  p −= ε·g;  then p ← −p and
MH accept min(1, exp(E_cur − E_new)).  sample (hmc.py:90-119) draws one discarded momentum
first (hmc.py:93), runs burn-in, updates DualAveragingStepSize once and prints it (the value
is not used, hmc.py:101-102), then samples.

Device paths:

* MVN model (config 1): every step of a burn-in / sampling phase runs in ONE device launch
  (hmcx_hmc_mvn_run, one thread per chain);
* softmax (CPU prior) and logistic models: a burn-in / sampling phase is ONE hmcx_hmc_chains_run
  call — momentum, every kick/drift (fused into the gradient kernels' epilogues), the energies, the
  MH accept and the commit run on the device; the host only draws the schedule (path lengths, accept
  uniforms and, in noise='numpy' mode, the momenta) in the reference's order;
  Both are written for C chains (_schedule .. _chains_fused): sample runs them with C = 1,
  hmc_multicore.sample_multicore with C = ncores;
* the MLP: a step's whole leapfrog trajectory is ONE hmcx_mlp_hmc_leapfrog call (device gradients,
  kicks and drifts enqueued from C in the reference's order); the energies go out as device pieces
  read back once.  A model that overrides grad (or HMCX_HMC_HOST_LOOP=1) runs the reference's loop
  with device gradients (model.grad) and hmcx_axpy / hmcx_sumsq from the host instead.
"""
import os
import sys
from copy import deepcopy

import numpy as np
import torch

from dropout_hamiltonian_montecarlo_amd import _native as nat
from dropout_hamiltonian_montecarlo_amd._native import HmcxError, ptr

from .sghmc import _n_iter


def _host_loop():
    return os.environ.get("HMCX_HMC_HOST_LOOP", "0") == "1"


class hmc:
    NOISE_CHUNK = 1 << 24          # float64 momentum normals handed to one hmcx_hmc_chains_run call

    def __init__(self, model, start_p, path_length=1.0, step_size=0.1, verbose=True,
                 noise='numpy', seed=0, chain=0):
        self.start = start_p
        self.step_size = step_size
        self.path_length = path_length
        self.model = model
        self.verbose = verbose
        self.noise = noise
        self.seed, self.chain = int(seed), int(chain)
        self.global_step = 0
        self.trace = None
        self.out = sys.stdout
        if getattr(model, '_hmcx_model', None) is None:
            raise HmcxError("hmc needs a libhmcx model (hamiltonian.models.gpu.*)")

    def draw_momentum(self, rng):                                           # hmc.py:82-87
        return {var: rng.normal(0, 1, size=np.shape(self.start[var])) for var in self.start.keys()}

    def sample(self, niter=1e4, burnin=1e3, rng=None, **args):              # hmc.py:90-119
        if rng is None:
            rng = np.random.RandomState()
        niter, nburn = int(niter), int(burnin)
        if self.noise == 'numpy':
            self.draw_momentum(rng)                                          # hmc.py:93 consumes RNG
        mvn = self.model._hmcx_model == 'mvn_gaussian'
        if not mvn and not self._linear_fused():
            return self._sample_generic(niter, nburn, burnin, rng, DualAveragingStepSize(self.step_size), args)
        # one chain of the chain-batched code; burn-in losses are printed every burnin / 10 steps of the
        # caller's raw burnin (hmc.py:97)
        results, traces, _ = self._chains_fused(niter, nburn, 1, [rng], None if mvn else args, burnin / 10)
        if self.trace is not None:
            # this entry point records n_iter + 1, which differs from the drawn L only for L = 0
            self.trace.extend(dict(t, L=max(t['L'], 1.0)) for t in traces[0])
        return results[0]

    # ------------------------------------------------------------------ softmax / logistic fused path
    def _linear_fused(self):
        m = self.model
        return (m._hmcx_model in ('softmax', 'logistic') and getattr(m, 'prior', 'cpu') == 'cpu'
                and list(self.start.keys()) == ['weights', 'bias'])

    def _linear_data(self, args):
        m = self.model
        X, y = m._xy(args)
        return X.contiguous(), y.contiguous()

    def _linear_model_args(self, a, Xd, Yd, D, K, n_steps):
        """The model part of hmcx_hmc_chains_args."""
        m = self.model
        a.dtype, a.model = m.code, nat.MODEL_LOGISTIC if m._hmcx_model == 'logistic' else nat.MODEL_SOFTMAX
        a.B, a.D, a.K, a.n_steps = Xd.shape[0], D, K, n_steps
        a.alpha = m.alpha
        if m._hmcx_model == 'logistic':                                        # logistic.py:15-21
            for i, var in enumerate(('weights', 'bias')):
                dim = int(np.prod(np.shape(self.start[var])))
                a.lp_const[i] = dim * 0.5 * np.log(m.hyper['alpha'] / (2 * np.pi))
        else:
            a.log_prior = m.log_prior_const([np.shape(self.start[v]) for v in self.start])
        a.X, a.Y = ptr(Xd), ptr(Yd)

    # ------------------------------------------------------------------ fused routes: C chains per call
    # hmc.sample is one chain of this code (C = 1, rngs = [rng]); hmc_multicore.sample_multicore runs C.
    def _schedule(self, n_steps, C, P, rngs, step0, host_mom):
        """Steps step0.. of a phase: path iterations, accept uniforms and path lengths L, [n_steps, C]
        each, and the host momenta [n_steps, C, P] (None where the device draws them).
        noise='numpy': per step in the reference's draw order — hmc.py:41 the momentum of chains
        0..C−1, each from its rng (variables in start order), then :46 the path length and :61 the accept
        uniform from the global np.random, shared by the chains.  An rng that is the global stream itself
        therefore sees the reference's interleaving.  noise='philox': hmcx_philox_schedule, and with
        host_mom the host twin of the device's float64 momentum stream (the MVN route)."""
        if self.noise == 'numpy':
            n1 = np.empty(n_steps, dtype=np.int32)
            u1 = np.empty(n_steps, dtype=np.float64)
            L1 = np.empty(n_steps, dtype=np.float64)
            noise = np.empty((n_steps, C, P), dtype=np.float64)
            for s in range(n_steps):
                for c in range(C):
                    mom = self.draw_momentum(rngs[c])                                       # hmc.py:41
                    noise[s, c] = np.concatenate([np.reshape(mom[v], -1) for v in self.start])
                L1[s] = np.ceil(2 * np.random.rand() * self.path_length / self.step_size)   # hmc.py:46
                n1[s] = _n_iter(L1[s])
                u1[s] = np.random.rand()                                                    # hmc.py:61
            rep = lambda v: np.ascontiguousarray(np.repeat(v[:, None], C, axis=1))
            return rep(n1), rep(u1), rep(L1), noise
        g0 = self.global_step + step0
        eps = np.full(n_steps, self.step_size, dtype=np.float64)
        L, n_iter, u = nat.philox_schedule(self.seed, self.chain, C, g0, self.path_length, eps)
        noise = None
        if host_mom:
            noise = np.empty((n_steps, C, P), dtype=np.float64)
            for s in range(n_steps):
                for c in range(C):
                    noise[s, c] = nat.philox_normals(self.seed, self.chain + c, (g0 + s) & 0xFFFFFFFF, 0, 0, P,
                                                     dtype="f64")
        return n_iter, u, L, noise

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
        recording, the host trace and momenta [n_steps, C, P] and the device trace.  BUFFER-mode momenta
        (noise='numpy') of one call are capped at NOISE_CHUNK values; a longer phase is several calls
        over consecutive steps, which changes no result (the carried state of a call is recomputed by
        the same kernel on the same values)."""
        W, b, data, P = st
        dev, dt = self.model.device, self.model.dtype
        tr = torch.empty((n_steps, C, P), dtype=dt, device=dev) if record else None
        host_mom = self.noise == 'numpy'
        mo = torch.empty((n_steps, C, P), dtype=dt, device=dev) if (record and not host_mom) else None
        chunk = max(1, self.NOISE_CHUNK // (C * P)) if host_mom else n_steps
        outs, Ls, moms = [], [], []
        for s0 in range(0, n_steps, chunk):
            s1 = min(n_steps, s0 + chunk)
            n_iter, u, L, noise = self._schedule(s1 - s0, C, P, rngs, s0, False)
            Ls.append(L)
            if record and host_mom:
                moms.append(noise)
            outs.append(self._hmc_chains_call(W, b, data, n_iter, u,
                                              torch.from_numpy(noise.reshape(-1)).to(dev) if host_mom else None,
                                              self.global_step + s0, tr[s0:s1] if record else None,
                                              mo[s0:s1] if mo is not None else None))
        self.global_step += n_steps
        A, acc, nlp = (np.concatenate([o[i] for o in outs], axis=0) for i in range(3))
        trace = mom = None
        if record:
            trace = tr.cpu().numpy().astype(np.float64)
            mom = np.concatenate(moms, axis=0) if host_mom else mo.cpu().numpy().astype(np.float64)
        return A, acc, nlp, np.concatenate(Ls, axis=0), trace, mom, tr

    def _mvn_phase(self, st, n_steps, C, rngs, record):
        """The same for the MVN model: hmcx_hmc_mvn_run with C chains, x [C, dim]."""
        x, dim = st
        m = self.model
        # both modes hand the device the host-drawn momenta (philox: the f64 Philox stream's host twin),
        # so the returned momentums are exactly the ones used (dim = 2: nothing to save on the device)
        n_iter, u, L, noise = self._schedule(n_steps, C, dim, rngs, 0, True)
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
        return A, acc, nlp, L, out_tr.cpu().numpy() if record else None, noise, out_tr

    def _split(self, flat):
        D, K = np.shape(self.start['weights'])
        return {'weights': flat[:D * K].reshape(D, K).copy(), 'bias': flat[D * K:].reshape(np.shape(self.start['bias'])).copy()}

    def _chains_fused(self, niter, nburn, C, rngs, args, burn_print):
        """C chains in one device call per phase; per chain, in chain order, what hmc.sample prints and
        returns.  args None: the MVN model.  burn_print: a burn-in loss is printed every burn_print
        steps.  Returns the chains' (posterior, loss, positions, momentums), their per-step trace
        records (L as drawn) and the sampling phase's device trace [niter, C, P] (None if niter = 0)."""
        m = self.model
        mvn = args is None
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
        burn = phase(st, nburn, C, rngs, False) if nburn > 0 else None
        before = state()
        samp = phase(st, niter, C, rngs, True) if niter > 0 else None
        if not mvn:
            self.last_state = {'weights': st[0], 'bias': st[1]}
        shown = [i for i in range(nburn) if self.verbose is not None and (i % burn_print == 0)]
        A, acc, nlp, L, tr, mom = samp[:6] if samp is not None else (None,) * 6
        if mvn:
            posterior = lambda c: {'x': tr[:, c].copy()}
        else:
            posterior = lambda c: {'weights': tr[:, c, :D * K].reshape((niter,) + np.shape(self.start['weights'])),
                                   'bias': tr[:, c, D * K:].reshape((niter,) + np.shape(self.start['bias']))}
        results, traces = self._assemble_chains(
            C, nburn, niter, burn and (burn[0], burn[1], burn[3]), burn and burn[2][shown], samp and (A, acc, L, nlp),
            posterior, lambda c, i: split(before[c] if i == 0 else tr[i - 1, c]), lambda c, i: split(mom[i, c]))
        return results, traces, samp[6] if samp is not None else None

    def _assemble_chains(self, C, nburn, niter, burn, burn_losses, samp, posterior, position, momentum):
        """Per chain, in chain order, what hmc.sample prints and returns.  burn / samp: a phase's host A, accepted
        and L [n, C], samp also the draws' losses [niter, C]; None: no step.  burn_losses [n_printed, C] are
        printed.  posterior(c): chain c's {var: [niter, *shape]}; position(c, i): the state draw i started from;
        momentum(c, i): its momentum (momentum None: empty lists).  Returns the chains' (posterior, loss,
        positions, momentums) and their per-step trace records (L as drawn)."""
        def records(A, acc, L, n, c):
            return ({'L': float(L[i, c]), 'A': float(A[i, c]), 'accepted': bool(acc[i, c]), 'eps': self.step_size}
                    for i in range(n))
        traces, results = [[] for _ in range(C)], []
        for c in range(C):
            p_accept = None
            if burn is not None:
                for lo in burn_losses[:, c]:
                    print('loss: {0:.4f}'.format(lo), file=self.out)
                p_accept = burn[0][-1, c]
                traces[c].extend(records(*burn, nburn, c))
            _, avg_step_size = DualAveragingStepSize(self.step_size).update(p_accept)
            print('adapted step size : ', avg_step_size, file=self.out)
            if samp is None:
                results.append(({v: np.zeros((0,) + np.shape(self.start[v])) for v in self.start}, np.zeros(0), [], []))
                continue
            A, acc, L, loss = samp
            traces[c].extend(records(A, acc, L, niter, c))
            positions = [[position(c, i)] for i in range(niter)]
            momentums = [] if momentum is None else [[momentum(c, i)] for i in range(niter)]
            for i in range(niter):
                if self.verbose and (i % (niter / 10) == 0):
                    print('loss: {0:.4f}'.format(loss[i, c]), file=self.out)
            results.append((posterior(c), loss[:, c].copy(), positions, momentums))
        return results, traces

    # ------------------------------------------------------------------ generic path (device grads)
    def _K(self, p):                                                         # hmc.py:74-79
        """Σ_var ½·Σp²: one device reduction per variable into one buffer, one readback (the per-variable
        sums are added on the host in the reference's variable order)."""
        K = 0
        ctx = nat.context(self.model.device)
        ss = torch.empty(len(p), dtype=torch.float64, device=self.model.device)
        keep = []
        for i, var in enumerate(p.keys()):
            v = p[var].reshape(-1)
            keep.append(v)
            ctx.check(ctx.lib.hmcx_sumsq(ctx.h, self.model.code, ptr(v), v.numel(), ptr(ss[i:i + 1])), "hmcx_sumsq")
        for s2 in ss.cpu().numpy():
            K += 0.5 * float(s2)
        return K

    def _sumsq_into(self, p, out):
        """Σp² of each variable of p into out[i] (device, no readback)."""
        ctx = nat.context(self.model.device)
        keep = []
        for i, var in enumerate(p.keys()):
            v = p[var].reshape(-1)
            keep.append(v)
            ctx.check(ctx.lib.hmcx_sumsq(ctx.h, self.model.code, ptr(v), v.numel(), ptr(out[i:i + 1])), "hmcx_sumsq")
        return keep

    @staticmethod
    def _K_from(sums):                                                      # hmc.py:74-79
        K = 0
        for s2 in sums:
            K += 0.5 * float(s2)
        return K

    def _energies(self, q_new, p_new, q, p, args):
        """E_new, E_cur (hmc.py:57-58).  A model with energy_parts_device (the MLP) gets all four terms
        enqueued into one device buffer and read back once, in the reference's order of evaluation;
        otherwise through negative_log_posterior and _K."""
        m = self.model
        if not hasattr(m, "energy_parts_device"):
            E_new = m.negative_log_posterior(q_new, **args) + self._K(p_new)
            E_cur = m.negative_log_posterior(q, **args) + self._K(p)
            return E_new, E_cur
        nq, npv = len(q_new), len(p_new)
        buf = torch.empty(2 * (1 + nq + npv), dtype=torch.float64, device=m.device)
        o = [0, 1 + nq, 1 + nq + npv, 2 + 2 * nq + npv, 2 * (1 + nq + npv)]
        keep = [m.energy_parts_device(q_new, buf[o[0]:o[1]], **args), self._sumsq_into(p_new, buf[o[1]:o[2]]),
                m.energy_parts_device(q, buf[o[2]:o[3]], **args), self._sumsq_into(p, buf[o[3]:o[4]])]
        h = buf.cpu().numpy()
        del keep
        E_new = m.nlp_from_parts(h[o[0]:o[1]], q_new) + self._K_from(h[o[1]:o[2]])
        E_cur = m.nlp_from_parts(h[o[2]:o[3]], q) + self._K_from(h[o[3]:o[4]])
        return E_new, E_cur

    def _axpy(self, mode, a, x, y):
        """y −= a·x (mode 0) / y += a·x (mode 1) on the device (hmcx_axpy)."""
        ctx = nat.context(self.model.device)
        ctx.check(ctx.lib.hmcx_axpy(ctx.h, self.model.code, mode, y.numel(), float(a), ptr(x), ptr(y)), "hmcx_axpy")

    def step(self, state, momentum, rng, **args):                           # hmc.py:39-64
        m = self.model
        dev, dt = m.device, m.dtype
        q = {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).to(dev, dt).contiguous()
             for k, v in state.items()}
        p_host = self.draw_momentum(rng)
        p = {k: torch.as_tensor(v).to(dev, dt).contiguous() for k, v in p_host.items()}
        q_new = {k: v.clone() for k, v in q.items()}
        p_new = {k: v.clone() for k, v in p.items()}
        # the recorded momentum is the host draw in the model's dtype (what a device round trip returns)
        npdt = torch.empty(0, dtype=dt).numpy().dtype
        positions, momentums = [deepcopy(state)], [{k: np.asarray(v).astype(npdt) for k, v in p_host.items()}]
        epsilon = self.step_size
        path_length = np.ceil(2 * np.random.rand() * self.path_length / epsilon)
        if hasattr(m, "leapfrog_device") and m.leapfrog_device_ok() and not _host_loop():
            # the whole trajectory in one libhmcx call (hmcx_mlp_hmc_leapfrog): the same kernels in the
            # same order as the loop below, enqueued from C
            m.leapfrog_device(q_new, p_new, _n_iter(path_length), epsilon, list(self.start.keys()), **args)
        else:
            grad_q = m.grad(q, **args)
            for _ in range(_n_iter(path_length)):
                for var in self.start.keys():
                    self._axpy(0, 0.5 * epsilon, grad_q[var], p_new[var])      # hmc.py:50
                    self._axpy(1, epsilon, p_new[var], q_new[var])             # hmc.py:51
                    grad_q = m.grad(q_new, **args)
                    self._axpy(0, epsilon, grad_q[var], p_new[var])            # hmc.py:53
            for var in self.start.keys():
                self._axpy(0, 2.0, p_new[var], p_new[var])                     # hmc.py:55-56: p − 2p = −p
        E_new, E_cur = self._energies(q_new, p_new, q, p, args)
        acceptprob = min(1, np.exp(E_cur - E_new))
        accepted = bool(np.isfinite(acceptprob) and (np.random.rand() < acceptprob))
        if accepted:
            q, p = q_new, p_new
        if self.trace is not None:
            self.trace.append({'L': float(path_length), 'A': float(acceptprob), 'accepted': accepted,
                               'eps': float(epsilon)})
        return q, p, positions, momentums, acceptprob

    def _loss_and_state(self, q, args):
        """negative_log_posterior(q) (hmc.py:113) and q on the host.  With energy_parts_device and a
        device state: the loss pieces and the state (widened to float64, exactly) in one buffer, one
        readback."""
        m = self.model
        keys = list(self.start.keys())
        if not (hasattr(m, "energy_parts_device") and all(isinstance(q[v], torch.Tensor) for v in keys)):
            loss = m.negative_log_posterior(q, **args)
            return loss, {v: q[v].cpu().numpy() if isinstance(q[v], torch.Tensor) else q[v] for v in keys}
        nq = len(q)
        sizes = [q[v].numel() for v in keys]
        buf = torch.empty(1 + nq + sum(sizes), dtype=torch.float64, device=m.device)
        keep = m.energy_parts_device(q, buf[:1 + nq], **args)
        buf[1 + nq:].copy_(torch.cat([q[v].reshape(-1) for v in keys]))
        h = buf.cpu().numpy()
        del keep
        npdt = torch.empty(0, dtype=m.dtype).numpy().dtype
        qh, o = {}, 1 + nq
        for v, n in zip(keys, sizes):
            qh[v] = h[o:o + n].astype(npdt).reshape(tuple(q[v].shape))
            o += n
        return m.nlp_from_parts(h[:1 + nq], q), qh

    def _sample_generic(self, niter, nburn, burnin, rng, tuning, args):
        q, p = self.start, None
        p_accept = None
        for i in range(nburn):
            q, p, positions, momentums, p_accept = self.step(q, p, rng, **args)
            if self.verbose is not None and (i % (burnin / 10) == 0):
                print('loss: {0:.4f}'.format(self.model.negative_log_posterior(q, **args)), file=self.out)
        _, avg_step_size = tuning.update(p_accept)
        print('adapted step size : ', avg_step_size, file=self.out)
        loss = np.zeros(niter)
        sample_positions, sample_momentums = [], []
        posterior = {var: [] for var in self.start.keys()}
        for i in range(niter):
            q, p, positions, momentums, _ = self.step(q, p, rng, **args)
            sample_positions.append(positions)
            sample_momentums.append(momentums)
            loss[i], qh = self._loss_and_state(q, args)
            for var in self.start.keys():
                posterior[var].append(qh[var])
            if self.verbose and (i % (niter / 10) == 0):
                print('loss: {0:.4f}'.format(loss[i]), file=self.out)
        for var in self.start.keys():
            posterior[var] = np.array(posterior[var])
        return posterior, loss, sample_positions, sample_momentums

    def backend_mean(self, multi_backend, niter, ncores=None):               # hmc.py:132-138
        """Posterior mean from HDF5 backend files (h5trace: the image's HDF5 C library)."""
        from dropout_hamiltonian_montecarlo_amd import h5trace
        return h5trace.backend_mean(self.start, multi_backend, niter)


class DualAveragingStepSize:                                                # hmc.py:141-176
    def __init__(self, initial_step_size, target_accept=0.8, gamma=0.05, t0=10.0, kappa=0.75):
        self.mu = np.log(10 * initial_step_size)
        self.target_accept = target_accept
        self.gamma = gamma
        self.t = t0
        self.kappa = kappa
        self.error_sum = 0
        self.log_averaged_step = 0

    def update(self, p_accept):
        if p_accept is None:
            return np.nan, np.nan
        self.error_sum += self.target_accept - p_accept
        log_step = self.mu - self.error_sum / (np.sqrt(self.t) * self.gamma)
        eta = self.t ** -self.kappa
        self.log_averaged_step = eta * log_step + (1 - eta) * self.log_averaged_step
        self.t += 1
        return np.exp(log_step), np.exp(self.log_averaged_step)
