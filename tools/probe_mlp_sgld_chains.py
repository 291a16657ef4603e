#!/usr/bin/env python3
"""Several SGLD chains on the config-3 MLP (784-256-256-10, B = 500, float32, Philox noise and masks), epochs over
N = 60,000 synthetic device-resident rows (120 steps each).  For every chain count C:
  (a) one sgld(chains=C).sample — one hmcx_mlp_sgld_chains_run per epoch (C = 1: hmcx_mlp_sgld_run, the one-chain
      path), the chains as the problems of batched launches in groups of at most six;
  (b) C one-chain sgld.sample runs back to back (chain = c), what a user does without it.
Each repetition times a window of `epochs` epochs of (a) and of (b), alternating, after one warm-up epoch of each;
a window ends in a device synchronise.  Prints chain-steps/s (steps × C per second) of every window, the medians
with min – max, their ratio, and whether every (a) window lies above every (b) window.  Then device time per step
and launch group between a call's first and last kernel (hmcx_get_timing) for (a).
    python tools/probe_mlp_sgld_chains.py [epochs per window, default 20] [repetitions, default 5] [C ...]"""
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp  # noqa: E402
from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sgld import sgld  # noqa: E402

N, B, SHAPE, EPS = 60000, 500, (784, 256, 10), 1e-3
GROUP = 6                                     # chains per launch group (MAXPROB of csrc/hmcx_mlp_kernels.h)


def main():
    epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    counts = [int(c) for c in sys.argv[3:]] or [1, 2, 4, 6, 8, 12]
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    dev, dt = "cuda:0", torch.float32
    rs = np.random.RandomState(0)
    X = torch.as_tensor(rs.rand(N, SHAPE[0]), dtype=dt, device=dev)
    y = torch.as_tensor(rs.randint(0, SHAPE[2], N), dtype=torch.int32, device=dev)
    m = mlp({"alpha": 0.01}, *SHAPE, dtype=dt, device=dev)
    start = m.init_params(1)
    nb = N // B

    def run(n, chains, chain=0):
        s = sgld(m, start, step_size=EPS, noise="philox", seed=3, chain=chain, chains=chains, verbose=False)
        s.out = io.StringIO()
        s.sample(epochs=n, burnin=0, batch_size=B, X_train=X, y_train=y)

    def one_call(C):
        return lambda n: run(n, C)

    def back_to_back(C):
        def fn(n):
            for c in range(C):
                run(n, 1, chain=c)
        return fn

    def window(fn, C):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(epochs)
        torch.cuda.synchronize()
        return C * epochs * nb / (time.perf_counter() - t0)

    for C in counts:
        fa, fb = one_call(C), back_to_back(C)
        fa(1)
        fb(1)
        ra, rb = [], []
        for _ in range(reps):
            ra.append(window(fa, C))
            rb.append(window(fb, C))
            print("C=%2d  (a) one call %10.1f   (b) back to back %10.1f chain-steps/s" % (C, ra[-1], rb[-1]), flush=True)
        per = []
        for _ in range(reps):
            m.ctx.set_timing(True)
            fa(epochs)
            torch.cuda.synchronize()
            ms, calls = m.ctx.get_timing()
            m.ctx.set_timing(False)
            per.append(1e3 * ms / (calls * nb * ((C + GROUP - 1) // GROUP)))
        print("C=%2d  median (a) %.1f (min %.1f, max %.1f), (b) %.1f (min %.1f, max %.1f) chain-steps/s, ratio %.2f, "
              "every (a) window above every (b) window: %s; device time per step and group %.1f us (min %.1f, "
              "max %.1f)" % (C, float(np.median(ra)), min(ra), max(ra), float(np.median(rb)), min(rb), max(rb),
                             float(np.median(ra)) / float(np.median(rb)), min(ra) > max(rb),
                             float(np.median(per)), min(per), max(per)), flush=True)


if __name__ == "__main__":
    main()
