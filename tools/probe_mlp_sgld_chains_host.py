#!/usr/bin/env python3
"""Where sgld(mlp, chains=C).sample spends its time at config 3 (784-256-256-10, B = 500, float32, Philox noise and
masks, 60,000 device-resident rows, epochs of 120 steps): per epoch the time until the device call
(hmcx_mlp_sgld_chains_run; C = 1: hmcx_mlp_sgld_run) returns — the enqueue — against the time until the device has
finished, and the time sample() spends outside the calls (start upload, per-epoch read-back of the state into the
float64 posterior, the final stacking).  A call whose enqueue stays below its completion time is device-bound.
The calls are wrapped with a device synchronise before and after, so the figures are not those of a pipelined run.
    python tools/probe_mlp_sgld_chains_host.py [epochs, default 6] [repetitions, default 2] [C ...]"""
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


def main():
    epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    counts = [int(c) for c in sys.argv[3:]] or [1, 2, 4, 6, 12]
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    dev, dt = "cuda:0", torch.float32
    rs = np.random.RandomState(0)
    X = torch.as_tensor(rs.rand(N, SHAPE[0]), dtype=dt, device=dev)
    y = torch.as_tensor(rs.randint(0, SHAPE[2], N), dtype=torch.int32, device=dev)
    m = mlp({"alpha": 0.01}, *SHAPE, dtype=dt, device=dev)
    start = m.init_params(1)
    lib = m.ctx.lib
    rec = []

    def timed(orig):
        def f(*a):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = orig(*a)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            rec.append((t1 - t0, time.perf_counter() - t0))
            return rc
        return f

    for name in ("hmcx_mlp_sgld_chains_run", "hmcx_mlp_sgld_run"):
        setattr(lib, name, timed(getattr(lib, name)))
    for C in counts:
        for rep in range(reps):
            del rec[:]
            s = sgld(m, start, step_size=EPS, noise="philox", seed=3, chains=C, verbose=False)
            s.out = io.StringIO()
            t0 = time.perf_counter()
            s.sample(epochs=epochs, burnin=0, batch_size=B, X_train=X, y_train=y)
            wall = time.perf_counter() - t0
            enq, tot = np.median([r[0] for r in rec]), np.median([r[1] for r in rec])
            print("C=%2d rep %d: per epoch enqueue %.2f ms, until done %.2f ms (medians of %d calls); sample() %.1f ms "
                  "for %d epochs, of which outside the calls %.1f ms"
                  % (C, rep, 1e3 * enq, 1e3 * tot, len(rec), 1e3 * wall, epochs, 1e3 * (wall - sum(r[1] for r in rec))),
                  flush=True)


if __name__ == "__main__":
    main()
