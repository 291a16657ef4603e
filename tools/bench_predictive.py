#!/usr/bin/env python
"""Posterior predictive of the MLP: the one-call device paths against the loop the library offered before.

Default: shape 784-256-256-10, float32, N = 10 000 rows, S = 64 parameter sets, T = 1, Philox masks (the
options move along rows, sets, dtype and layer widths for the selection rule of path 0).  Three timings, each
the median of --runs runs after --warmup runs:

  path1     hmcx_mlp_predictive, general path (one forward per draw + reduce)
  path2     hmcx_mlp_predictive, fused row-block kernel
  baseline  64 × model.logits(par_s, X, masks=None), softmax and running mean on the device in torch

Device time of the two predictive paths comes from hmcx_set_timing / hmcx_get_timing (events around the
call's launches).  The baseline's launches are hmcx_mlp_masks + hmcx_mlp_loss + torch kernels, which that
pair does not bracket, so its device time is a torch event pair on the same stream around the whole loop.
Wall time is host time around the call including the final synchronisation.

Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_F32_TF = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--dropout", type=int, default=1)
    ap.add_argument("--dtype", choices=["float32", "float64"], default="float32")
    ap.add_argument("--n-in", type=int, default=784)
    ap.add_argument("--n-mid", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import MLP_PARAM_NAMES, mlp

    n_in, n_mid, n_out, N, S, T = a.n_in, a.n_mid, 10, a.rows, a.sets, a.dropout
    D = S * T
    dt, npdt = (torch.float32, np.float32) if a.dtype == "float32" else (torch.float64, np.float64)
    m = mlp({"alpha": 0.01}, n_in, n_mid, n_out, dtype=dt, device="cuda:0", seed=1)
    rs = np.random.RandomState(0)
    X = torch.as_tensor(rs.rand(N, n_in).astype(npdt)).to(m.device)
    sets = [m.init_params(s) for s in range(S)]
    post = {k: torch.as_tensor(np.stack([p[k] for p in sets]).astype(npdt)).to(m.device) for k in MLP_PARAM_NAMES}
    per_set = [{k: post[k][s] for k in MLP_PARAM_NAMES} for s in range(S)]
    ctx = m.ctx

    def predictive(path):
        def run():
            ctx.set_timing(True)
            t0 = time.perf_counter()
            r = m.posterior_predictive(post, X, n_dropout=T, path=path)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            ms, n = ctx.get_timing()
            ctx.set_timing(False)
            assert n == 1 and np.all(np.isfinite(r.mean))
            return ms, wall
        return run

    def baseline():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        mean = torch.zeros((N, n_out), dtype=torch.float64, device=m.device)
        for s in range(S):
            for _ in range(T):
                mean += torch.softmax(m.logits(per_set[s], X, masks=None).double(), dim=1)
        mean /= D
        e1.record()
        host = mean.cpu().numpy()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert np.all(np.isfinite(host))
        return e0.elapsed_time(e1), wall

    flops = 2.0 * N * D * (n_in * n_mid + n_mid * n_mid + n_mid * n_out)
    res = {"shape": [n_in, n_mid, n_mid, n_out], "dtype": a.dtype, "rows": N, "sets": S, "dropout_draws": T,
           "runs": a.runs, "warmup": a.warmup, "flops": flops}
    for name, fn in (("path1", predictive(1)), ("path2", predictive(2)), ("baseline", baseline)):
        for _ in range(a.warmup):
            fn()
        got = [fn() for _ in range(a.runs)]
        dev, wall = [g[0] for g in got], [g[1] for g in got]
        res[name] = {"device_ms": statistics.median(dev), "device_ms_min": min(dev), "device_ms_max": max(dev),
                     "wall_ms": statistics.median(wall),
                     "tflops": flops / (statistics.median(dev) * 1e-3) / 1e12}
        if a.dtype == "float32":
            res[name]["mfma_f32_fraction"] = res[name]["tflops"] / MFMA_F32_TF
    res["path2_over_path1"] = res["path2"]["device_ms"] / res["path1"]["device_ms"]
    res["path2_over_baseline"] = res["path2"]["device_ms"] / res["baseline"]["device_ms"]
    res["path1_over_baseline"] = res["path1"]["device_ms"] / res["baseline"]["device_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
