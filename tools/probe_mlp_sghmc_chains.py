#!/usr/bin/env python3
"""Multi-chain SGHMC on the config-3 MLP (784-256-256-10, B = 500, float32, N = 6000 synthetic device-resident rows,
Philox noise and masks, step size 0.001 and path length 0.01: L = ceil(2·U·10) in 1 .. 20 and longer as the step size
decays inside an epoch, E[L] about 10).  For every chain count C:
  (a) sghmc(mlp, chains=C).sample — one hmcx_mlp_sghmc_chains_run per epoch, the chains as the problems of batched
      unfused launches in groups of at most six (C = 1: the same entry with one chain, which sample() itself never
      takes — it keeps hmcx_mlp_sghmc_run for one chain);
  (b) C one-chain sghmc samplers (chain = c) run one after the other in the same process: hmcx_mlp_sghmc_run, the
      fused schedules.
Both draw their schedule from the same Philox streams, so chain c runs the same path lengths on either route.  Each
repetition times one window of `epochs` epochs of (a) and of (b), alternating, after one warm-up window of each; a
window is a host clock around work that ends in a device synchronise and is divided by its own count of leapfrog
iterations × chains.  Prints every window, the medians with min – max, their ratio and whether the windows overlap.
    python tools/probe_mlp_sghmc_chains.py [epochs per window, default 4] [repetitions, default 3] [C ...]
    python tools/probe_mlp_sghmc_chains.py --route-only C [epochs]     one window of (a) alone (for a kernel trace):
                                                                       also prints the steps and evaluations launched"""
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp  # noqa: E402
from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc  # noqa: E402

N, B, SHAPE, EPS, PATH = 6000, 500, (784, 256, 10), 0.001, 0.01


def main():
    route_only = len(sys.argv) > 1 and sys.argv[1] == "--route-only"
    argv = sys.argv[3:] if route_only else sys.argv[1:]
    epochs = int(argv[0]) if len(argv) > 0 else 4
    reps = int(argv[1]) if len(argv) > 1 else 3
    counts = [int(sys.argv[2])] if route_only else ([int(c) for c in argv[2:]] or [1, 2, 6, 12])
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    dev, dt = "cuda:0", torch.float32
    rs = np.random.RandomState(0)
    X = torch.as_tensor(rs.rand(N, SHAPE[0]), dtype=dt, device=dev)
    y = torch.as_tensor(rs.randint(0, SHAPE[2], N), dtype=torch.int32, device=dev)
    m = mlp({"alpha": 0.01}, *SHAPE, dtype=dt, device=dev)
    start = m.init_params(1)

    def sampler(chains, chain):
        s = sghmc(m, start, path_length=PATH, step_size=EPS, noise="philox", seed=3, chain=chain, chains=chains,
                  verbose=False)
        s.out, s.trace = io.StringIO(), []
        return s

    def iterations(s):
        return float(sum(np.sum(np.maximum(np.asarray(t['L']) - 1.0, 0.0)) for t in s.trace))

    def chains_route(C):
        s = sampler(C, 0)
        if C == 1:       # the chain entry with one chain: the state [*shape] is the stacked state [1, *shape]
            def one(state, data, rows, eps, rng, bs):
                res = s._run_mlp_chains(state, data, rows, eps, bs)
                res.ll, res.nlp = res.ll[:, 0], res.nlp[:, 0]
                return res
            s._run_mlp = one
        s.sample(epochs=epochs, burnin=0, batch_size=B, X_train=X, y_train=y)
        return [s]

    def sequential(C):
        out = []
        for c in range(C):
            s = sampler(1, c)
            s.sample(epochs=epochs, burnin=0, batch_size=B, X_train=X, y_train=y)
            out.append(s)
        return out

    def window(fn, C):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ss = fn(C)
        torch.cuda.synchronize()
        dt_ = time.perf_counter() - t0
        iters = sum(iterations(s) for s in ss)
        return iters / dt_, iters, ss

    if route_only:
        C = counts[0]
        window(chains_route, C)
        r, iters, ss = window(chains_route, C)
        L = np.array([np.atleast_1d(t['L']) for t in ss[0].trace])            # [steps, C]
        n = np.maximum(L - 1.0, 0.0)
        groups = [n[:, g:g + 6] for g in range(0, C, 6)]
        evals = int(sum(6 * g.max(axis=1).sum() for g in groups))
        print("route only, C=%d: %.1f leapfrog iterations x chains /s; per window %d steps x %d groups, %d evaluations "
              "launched (sum over steps and groups of 6 max_c n_c), %d leapfrog iterations x chains; two windows ran"
              % (C, r, L.shape[0], len(groups), evals, int(iters)), flush=True)
        return
    for C in counts:
        window(chains_route, C)
        window(sequential, C)
        ra, rb = [], []
        for _ in range(reps):
            (a, ia, _), (b, ib, _) = window(chains_route, C), window(sequential, C)
            ra.append(a)
            rb.append(b)
            print("C=%2d  (a) one call per epoch %9.1f (%d iterations)   (b) one-chain samplers in sequence %9.1f "
                  "(%d iterations) iterations x chains /s" % (C, a, ia, b, ib), flush=True)
        print("C=%2d  median (a) %.1f (min %.1f, max %.1f), (b) %.1f (min %.1f, max %.1f) leapfrog iterations x chains /s, "
              "ratio (a)/(b) %.2f, windows overlap: %s"
              % (C, float(np.median(ra)), min(ra), max(ra), float(np.median(rb)), min(rb), max(rb),
                 float(np.median(ra)) / float(np.median(rb)), not (min(ra) > max(rb) or min(rb) > max(ra))), flush=True)


if __name__ == "__main__":
    main()
