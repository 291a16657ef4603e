#!/usr/bin/env python3
"""Multi-chain full-batch HMC on the config-3 MLP (784-256-256-10, float32, N = 6000 synthetic device-resident rows,
step size 0.002 and path length 0.02: L = ceil(2·U·10) in 1 .. 20, E[L] = 10.5).  For every chain count C:
  (a) hmc_multicore(noise='philox').sample_multicore — one hmcx_mlp_hmc_chains_run per phase, the chains as the
      problems of batched launches in groups of at most six;
  (b) the per-chain fallback (_chains_sequential, what sample_multicore did before: hmc.sample once per chain, every
      step driven from the host).
(a) draws its path lengths from Philox, (b) from the global NumPy stream (hmc.step), so the windows hold different
leapfrog iterations with the same distribution; each window is divided by its own count.  Each
repetition times one window of `niter` sampling steps per chain of (a) and of (b), alternating, after one warm-up
window of each; a window ends in a device synchronise.  Prints leapfrog iterations × chains per second of every
window, the medians with min – max and their ratio.
Then the result check: one seed, masks='off', C = 12 chains, `check` steps per chain on either route (the routes then
differ only in who draws the momentum: the device's Philox stream or the host's RandomState(c)); per parameter the
z-score of the two ensemble means, z = (mean_a − mean_b) / sqrt(se_a² + se_b²) with se the chains' standard error,
reported as the share of |z| > 3 and the largest |z|.
    python tools/probe_mlp_hmc_chains.py [niter per chain, default 10] [repetitions, default 3] [check steps, default 40] [C ...]"""
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp  # noqa: E402
from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc_multicore import hmc_multicore  # noqa: E402

N, SHAPE, EPS, PATH = 6000, (784, 256, 10), 0.002, 0.02


def main():
    niter = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    check = int(sys.argv[3]) if len(sys.argv) > 3 else 40
    counts = [int(c) for c in sys.argv[4:]] or [1, 2, 6, 12]
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    dev, dt = "cuda:0", torch.float32
    rs = np.random.RandomState(0)
    X = torch.as_tensor(rs.rand(N, SHAPE[0]), dtype=dt, device=dev)
    y = torch.as_tensor(rs.randint(0, SHAPE[2], N), dtype=torch.int32, device=dev)
    m = mlp({"alpha": 0.01}, *SHAPE, dtype=dt, device=dev)
    start = m.init_params(1)

    def sampler(seed=3):
        s = hmc_multicore(m, start, path_length=PATH, step_size=EPS, noise="philox", seed=seed, verbose=None)
        s.out = io.StringIO()
        return s

    def fused(C, n, **kw):
        s = sampler()
        post = s.sample_multicore(n * C, 0, C, X_train=X, y_train=y, **kw)[0]
        return s, post

    def sequential(C, n, **kw):
        s = sampler()
        entry = np.random.get_state()
        res = s._chains_sequential(n, 0, C, entry, dict(X_train=X, y_train=y, **kw))
        np.random.set_state(entry)
        return s, {k: np.concatenate([r[0][k] for r in res], axis=0) for k in start}

    def window(fn, C):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s, _ = fn(C, niter)
        torch.cuda.synchronize()
        dt_ = time.perf_counter() - t0
        iters = sum(max(t['L'] - 1.0, 0.0) for tr in s.chain_traces for t in tr)
        return iters / dt_, iters

    for C in counts:
        window(fused, C)
        window(sequential, C)
        ra, rb = [], []
        for _ in range(reps):
            (a, ia), (b, ib) = window(fused, C), window(sequential, C)
            ra.append(a)
            rb.append(b)
            print("C=%2d  (a) one call per phase %9.1f (%d iterations)   (b) per chain %9.1f (%d iterations) iterations/s"
                  % (C, a, ia, b, ib), flush=True)
        print("C=%2d  median (a) %.1f (min %.1f, max %.1f), (b) %.1f (min %.1f, max %.1f) leapfrog iterations x chains /s, "
              "ratio %.2f, every (a) window above every (b) window: %s"
              % (C, float(np.median(ra)), min(ra), max(ra), float(np.median(rb)), min(rb), max(rb),
                 float(np.median(ra)) / float(np.median(rb)), min(ra) > max(rb)), flush=True)
    if check > 0:
        C = 12
        _, pa = fused(C, check, masks='off')
        _, pb = sequential(C, check, masks='off')
        zs = []
        for k in start:
            a = pa[k].reshape(C, check, -1).astype(np.float64).mean(axis=1)       # [C, P] chain means
            b = pb[k].reshape(C, check, -1).astype(np.float64).mean(axis=1)
            se = np.sqrt(a.var(axis=0, ddof=1) / C + b.var(axis=0, ddof=1) / C)
            zs.append((a.mean(axis=0) - b.mean(axis=0)) / np.where(se > 0, se, np.inf))
        z = np.abs(np.concatenate(zs))
        print("result check, masks off, C=%d, %d steps per chain: %d parameters, share of |z| > 3: %.5f, largest |z| %.2f "
              "(standard errors from %d chain means per route: about %d degrees of freedom)"
              % (C, check, z.size, float(np.mean(z > 3.0)), float(z.max()), C, 2 * C - 2), flush=True)


if __name__ == "__main__":
    main()
