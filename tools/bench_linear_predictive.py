#!/usr/bin/env python
"""Posterior predictive of the softmax / logistic models: the one-call device paths against what the library
offered before.

Per point (model, N rows, D features, K classes, S parameter sets, T input-dropout masks per set, dtype), each
timing the median of --runs runs after --warmup runs:

  path1          hmcx_linear_predictive, general path (k_fwd in predict mode per chunk of draws + reduce)
  path2          hmcx_linear_predictive, fused row-block kernel (where the shape is eligible)
  device_only    T = 1, softmax: hmcx_softmax_predict of all S sets ([N][S·K] to HBM) and the mean over the
                 sets in torch on the device
  host_posterior T = 1, softmax: softmax.predict_posterior as it stands (the same launch, every probability
                 copied to the host and averaged in NumPy); wall time only
  loop           T > 1: S·T calls of predict_stochastic(prob=True), averaged on the host (what the library
                 offered for input dropout); wall time only

Device time of the two predictive paths comes from hmcx_set_timing / hmcx_get_timing (events around the
call's launches); device_only's is a torch event pair on the same stream.  Wall time is host time around the
call including the final synchronisation.  The parameters are on the device before the clock starts for every
variant except host_posterior, whose interface takes host arrays.

Without --point the suite of DESIGN.md §12 runs.  Prints one JSON line per point; --out appends them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MFMA_F32_TF = 157.3

# model, N, D, K, S, T, dtype
SUITE = [
    ("softmax", 10000, 784, 10, 64, 1, "float32"), ("softmax", 10000, 784, 10, 64, 1, "float64"),
    ("softmax", 10000, 784, 10, 1000, 1, "float32"), ("softmax", 10000, 784, 10, 1000, 1, "float64"),
    ("softmax", 10000, 784, 10, 64, 16, "float32"),
    ("softmax", 10000, 2048, 38, 64, 1, "float32"),
    ("softmax", 16, 784, 10, 1, 1, "float32"), ("softmax", 16, 784, 10, 2, 1, "float32"),
    ("softmax", 16, 784, 10, 64, 1, "float32"), ("softmax", 256, 784, 10, 1, 1, "float32"),
    ("softmax", 256, 784, 10, 8, 1, "float32"), ("softmax", 256, 784, 10, 64, 1, "float32"),
    ("softmax", 1000, 64, 3, 200, 1, "float64"), ("softmax", 256, 784, 10, 4, 8, "float32"),
    ("softmax", 1000, 784, 10, 64, 1, "float32"), ("softmax", 2500, 784, 10, 64, 1, "float32"),
    ("softmax", 5000, 784, 10, 64, 1, "float32"), ("softmax", 10000, 784, 10, 2, 1, "float32"),
    ("softmax", 10000, 784, 10, 8, 1, "float32"), ("softmax", 1000, 784, 10, 1000, 1, "float32"),
    ("logistic", 10000, 784, 1, 64, 1, "float32"), ("logistic", 10000, 784, 1, 256, 1, "float32"),
    ("logistic", 10000, 784, 1, 1000, 1, "float32"), ("logistic", 256, 32, 1, 1000, 1, "float64"),
]


def fused_eligible(D, K, elt):
    up = lambda n: (n + 15) // 16 * 16  # noqa: E731
    xp = (D + 15) // 16 * 16 + 16 // elt
    return 1 <= K <= 16 and up(16 * xp * elt) + up(4 * 16 * 65 * elt) + up(4 * 16 * 18 * 8) <= 160 * 1024


def point(kind, N, D, K, S, T, dtype, runs, warmup):
    import torch
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.logistic import logistic
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    from dropout_hamiltonian_montecarlo_amd._native import ptr
    dt, npdt, elt = (torch.float32, np.float32, 4) if dtype == "float32" else (torch.float64, np.float64, 8)
    m = (logistic if kind == "logistic" else softmax)({"alpha": 0.01}, dtype=dt, device="cuda:0")
    rs = np.random.RandomState(0)
    Xh = rs.rand(N, D).astype(npdt)
    Wh, bh = rs.normal(0, 0.05, (S, D, K)).astype(npdt), rs.normal(0, 0.3, (S, K)).astype(npdt)
    X = torch.as_tensor(Xh).to(m.device)
    post = {"weights": torch.as_tensor(Wh).to(m.device), "bias": torch.as_tensor(bh).to(m.device)}
    ctx = m.ctx

    def predictive(path):
        def run():
            ctx.set_timing(True)
            t0 = time.perf_counter()
            r = m.posterior_predictive(post, X, n_dropout=T if T > 1 else 0, seed=3, path=path)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            ms, n = ctx.get_timing()
            ctx.set_timing(False)
            assert n == 1 and np.all(np.isfinite(r.mean))
            return ms, wall
        return run

    Wc = post["weights"].permute(1, 0, 2).reshape(D, S * K).contiguous()     # [D][S·K], outside the clock
    bc = post["bias"].reshape(S * K).contiguous()

    def device_only():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        prob = torch.empty((N, S * K), dtype=dt, device=m.device)
        ctx.check(ctx.lib.hmcx_softmax_predict(ctx.h, m.code, ptr(X), N, D, K, S, ptr(Wc), ptr(bc), ptr(prob)),
                  "hmcx_softmax_predict")
        mean = prob.reshape(N, S, K).double().mean(dim=1)
        e1.record()
        host = mean.cpu().numpy()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert np.all(np.isfinite(host))
        return e0.elapsed_time(e1), wall

    def host_posterior():
        t0 = time.perf_counter()
        mean = m.predict_posterior({"weights": Wh, "bias": bh}, X, prob=True)
        wall = (time.perf_counter() - t0) * 1e3
        assert np.all(np.isfinite(mean))
        return float("nan"), wall

    per_set = [{"weights": post["weights"][s], "bias": post["bias"][s]} for s in range(S)]

    def loop():
        t0 = time.perf_counter()
        mean = np.zeros((N, K))
        for s in range(S):
            for _ in range(T):
                mean += m.predict_stochastic(per_set[s], X, prob=True, p=0.5)
        mean /= S * T
        wall = (time.perf_counter() - t0) * 1e3
        assert np.all(np.isfinite(mean))
        return float("nan"), wall

    flops = 2.0 * N * D * K * S * T
    res = {"model": kind, "rows": N, "D": D, "K": K, "sets": S, "dropout_draws": T, "dtype": dtype, "runs": runs,
           "warmup": warmup, "flops": flops}
    todo = [("path1", predictive(1))]
    if fused_eligible(D, K, elt):
        todo.append(("path2", predictive(2)))
    if kind == "softmax" and T == 1:
        todo += [("device_only", device_only), ("host_posterior", host_posterior)]
    if kind == "softmax" and T > 1:
        todo.append(("loop", loop))
    for name, fn in todo:
        slow = name in ("host_posterior", "loop")                # seconds per run at the large points
        w, n = (1, 3) if slow else (warmup, runs)
        for _ in range(w):
            fn()
        got = [fn() for _ in range(n)]
        dev, wall = [g[0] for g in got], [g[1] for g in got]
        res[name] = {"device_ms": statistics.median(dev), "device_ms_min": min(dev), "device_ms_max": max(dev),
                     "wall_ms": statistics.median(wall), "runs": n}
        if dev[0] == dev[0]:
            res[name]["tflops"] = flops / (statistics.median(dev) * 1e-3) / 1e12
            if dtype == "float32":
                res[name]["mfma_f32_fraction"] = res[name]["tflops"] / MFMA_F32_TF
    if "path2" in res:
        res["path2_over_path1"] = res["path2"]["device_ms"] / res["path1"]["device_ms"]
        if "device_only" in res:
            res["path2_over_device_only"] = res["path2"]["device_ms"] / res["device_only"]["device_ms"]
    if "device_only" in res:
        res["path1_over_device_only"] = res["path1"]["device_ms"] / res["device_only"]["device_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", default=None, help="model,N,D,K,S,T,dtype (default: the suite)")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pts = SUITE
    if a.point:
        f = a.point.split(",")
        pts = [(f[0],) + tuple(int(v) for v in f[1:6]) + (f[6],)]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for pt in pts:
        line = json.dumps(point(*pt, runs=a.runs, warmup=a.warmup))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
