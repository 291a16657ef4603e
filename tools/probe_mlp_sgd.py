#!/usr/bin/env python3
"""Momentum SGD on the config-3 MLP (784-256-256-10, B = 500, float32, Philox masks), one epoch over
N = 60,000 synthetic rows (120 steps):
  (a) sgd.fit — the whole epoch in one hmcx_mlp_sgd_run call;
  (b) the host loop it replaces: per minibatch mlp.grad (fresh Philox masks) and the twelve torch update
      statements (m = gamma*m - lr*g; theta += m for six variables).
Dataset, state and momentum are device tensors in both, so neither window holds an upload.  Each repetition
times a window of `epochs` back-to-back epochs of (a) and of (b), alternating, after one warm-up epoch of
each; a window ends in a device synchronise.  Prints steps/s of every window, the medians and their ratio,
and for (a) the device time per step between the call's first and last kernel (hmcx_get_timing; it counts
timed calls, not kernels — the launches per step are fixed by the host schedule: DESIGN.md §5.3).
    python tools/probe_mlp_sgd.py [epochs per window, default 5] [repetitions, default 5]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp  # noqa: E402
from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sgd import sgd  # noqa: E402

N, B, SHAPE, LR, GAMMA = 60000, 500, (784, 256, 10), 0.05, 0.9


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

    def device_call(n):
        s = sgd(m, start, step_size=LR, seed=3)
        for _ in range(n):
            s.fit(epochs=1, batch_size=B, gamma=GAMMA, X_train=X, y_train=y)

    def host_loop(n):
        par = {k: m._dev(v).clone() for k, v in start.items()}
        mom = {k: torch.zeros_like(v) for k, v in par.items()}
        for _ in range(n):
            for j in range(nb):
                g = m.grad(par, X_train=X[j * B:(j + 1) * B], y_train=y[j * B:(j + 1) * B])
                for k in par:
                    mom[k] = GAMMA * mom[k] - LR * g[k]
                    par[k] += mom[k]
            m.negative_log_posterior(par, X_train=X[(nb - 1) * B:nb * B], y_train=y[(nb - 1) * B:nb * B])

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
    m.ctx.set_timing(True)
    device_call(epochs)
    torch.cuda.synchronize()
    ms, calls = m.ctx.get_timing()
    m.ctx.set_timing(False)
    print("median: device call %.1f steps/s (min %.1f, max %.1f), host loop %.1f steps/s (min %.1f, max %.1f), "
          "ratio %.2f" % (med["device call"], min(rates["device call"]), max(rates["device call"]),
                          med["host loop"], min(rates["host loop"]), max(rates["host loop"]),
                          med["device call"] / med["host loop"]))
    print("device call: %.1f us of device time per step over %d timed calls of %d steps" % (
        1e3 * ms / (calls * nb), calls, nb))


if __name__ == "__main__":
    main()
