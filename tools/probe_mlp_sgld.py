#!/usr/bin/env python3
"""SGLD on the config-3 MLP (784-256-256-10, B = 500, float32, Philox noise and masks), epochs over N = 60,000
synthetic rows (120 steps each), device-resident data:
  (a) sgld.sample — one hmcx_mlp_sgld_run call per epoch (12 log-line forwards and the epoch-end energy inside);
  (b) the host loop a user has to write without it: per minibatch mlp.grad (fresh Philox masks), one
      torch.randn_like per variable and the update statements (p = 2*eps*z - 0.5*eps*g; theta += p), a
      log_likelihood every tenth minibatch and negative_log_posterior at the epoch's end.
Each repetition times a window of `epochs` back-to-back epochs of (a) and of (b), alternating, after one warm-up
epoch of each; a window ends in a device synchronise.  Prints steps/s of every window, the medians and their
ratio.  Then device time per step between a call's first and last kernel (hmcx_get_timing; it counts timed
calls, not kernels — the launches per step are fixed by the host schedule: DESIGN.md §5.3) for
  (a) as above, (a1) the same with one log line per epoch (log_every = steps per epoch), and
  (c) hmcx_mlp_sgd_run (sgd.fit, one epoch per call): the same schedule up to its last launch, one evaluation.
    python tools/probe_mlp_sgld.py [epochs per window, default 5] [repetitions, default 5]"""
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp  # noqa: E402
from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sgd import sgd  # noqa: E402
from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sgld import sgld  # noqa: E402

N, B, SHAPE, EPS = 60000, 500, (784, 256, 10), 1e-3


def main():
    epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    dev, dt = "cuda:0", torch.float32
    rs = np.random.RandomState(0)
    X = torch.as_tensor(rs.rand(N, SHAPE[0]), dtype=dt, device=dev)
    y = torch.as_tensor(rs.randint(0, SHAPE[2], N), dtype=torch.int32, device=dev)
    m = mlp({"alpha": 0.01}, *SHAPE, dtype=dt, device=dev)
    start = m.init_params(1)
    nb = N // B

    def device_call(n, log_every=10):
        s = sgld(m, start, step_size=EPS, noise="philox", seed=3, verbose=False)
        s.out, s.log_every = io.StringIO(), log_every
        s.sample(epochs=n, burnin=0, batch_size=B, X_train=X, y_train=y)

    def host_loop(n):
        par = {k: m._dev(v).clone() for k, v in start.items()}
        for _ in range(n):
            for j in range(nb):
                kw = dict(X_train=X[j * B:(j + 1) * B], y_train=y[j * B:(j + 1) * B])
                g = m.grad(par, **kw)
                for k in par:
                    p = (2.0 * EPS) * torch.randn_like(par[k])
                    p += (-0.5 * EPS) * g[k]
                    par[k] += p
                if j % 10 == 0:
                    m.log_likelihood(par, **kw)
            m.negative_log_posterior(par, **kw)

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(epochs)
        torch.cuda.synchronize()
        return epochs * nb / (time.perf_counter() - t0)

    device_call(1)
    host_loop(1)
    rates = {"device call": [], "host loop": []}
    for _ in range(reps):
        for name, fn in (("device call", device_call), ("host loop", host_loop)):
            rates[name].append(window(fn))
            print("%-11s %d steps: %9.1f steps/s" % (name, epochs * nb, rates[name][-1]), flush=True)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    print("median: device call %.1f steps/s (min %.1f, max %.1f), host loop %.1f steps/s (min %.1f, max %.1f), "
          "ratio %.2f" % (med["device call"], min(rates["device call"]), max(rates["device call"]),
                          med["host loop"], min(rates["host loop"]), max(rates["host loop"]),
                          med["device call"] / med["host loop"]))

    def sgd_call(n):
        s = sgd(m, start, step_size=0.05, seed=3)
        for _ in range(n):
            s.fit(epochs=1, batch_size=B, gamma=0.9, X_train=X, y_train=y)

    # device time per step, alternating the three calls; the median over the repetitions
    per_step = {"sgld (a)": [], "sgld, one log line (a1)": [], "sgd (c)": []}
    for _ in range(reps):
        for name, fn in (("sgld (a)", device_call), ("sgld, one log line (a1)", lambda n: device_call(n, nb)),
                         ("sgd (c)", sgd_call)):
            m.ctx.set_timing(True)
            fn(epochs)
            torch.cuda.synchronize()
            ms, calls = m.ctx.get_timing()
            m.ctx.set_timing(False)
            per_step[name].append(1e3 * ms / (calls * nb))
    for name, v in per_step.items():
        print("%-24s %.1f us of device time per step (median of %d, min %.1f, max %.1f; %d steps per call)" % (
            name, float(np.median(v)), len(v), min(v), max(v), nb))


if __name__ == "__main__":
    main()
