"""Device ms per call: hmcx_hmc_chains_run at C = 1, 6, 48 vs C sequential hmcx_hmc_run calls.
MNIST-shaped f64, N=60000, D=784, K=10, eps=1e-3, 10 steps, n_iter = 5 for all chains.
Uses hmcx_set_timing / hmcx_get_timing: a warm-up, then the median of three calls.  HMCX_LIB names the
library under dropout_hamiltonian_montecarlo_amd/lib/ to load (default libhmcx.so); with a build of an older
commit that lacks hmcx_hmc_chains_run only the sequential hmcx_hmc_run figures are printed — the baseline
of DESIGN §5.7.  Last, at the launch-bound N = 200: host wall ms of one hmcx_hmc_run call plus synchronize,
median and quartiles of 21 calls.  --one-chain stops after the hmcx_hmc_run, C = 1 line.  One JSON line per figure (profiles/hmc_chains_measure.jsonl)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dropout_hamiltonian_montecarlo_amd import _native as nat  # noqa: E402
from dropout_hamiltonian_montecarlo_amd._native import ptr  # noqa: E402

N, D, K, S, NIT, EPS = 60000, 784, 10, 10, 5, 1e-3
N_SMALL = 200
P = D * K + K
dev = torch.device("cuda:0")
lib_name = os.environ.get("HMCX_LIB", "libhmcx.so")
ctx = nat.context(dev)
has_chains = hasattr(ctx.lib, "hmcx_hmc_chains_run")
rs = np.random.RandomState(0)


def problem(n):
    X = torch.as_tensor(rs.rand(n, D)).to(dev)
    Yh = np.zeros((n, K))
    Yh[np.arange(n), rs.randint(0, K, n)] = 1.0
    return X, torch.as_tensor(Yh).to(dev)


X, Y = problem(N)
log_prior = -1.234


def common(a, C):
    a.dtype, a.model = nat.HMCX_F64, nat.MODEL_SOFTMAX
    a.B, a.D, a.K, a.n_steps = X.shape[0], D, K, S
    a.alpha, a.log_prior = 0.01, log_prior
    a.X, a.Y = ptr(X), ptr(Y)
    a.noise_mode = nat.NOISE_PHILOX
    a.seed, a.step_base = 7, 0


def run_single(chain, keep):
    eps = np.full(S, EPS)
    n_iter = np.full(S, NIT, dtype=np.int32)
    u = np.full(S, 0.5)
    W = torch.zeros((D, K), dtype=torch.float64, device=dev)
    b = torch.zeros(K, dtype=torch.float64, device=dev)
    out_f = torch.empty(4 * S, dtype=torch.float64, device=dev)
    out_acc = torch.empty(S, dtype=torch.int32, device=dev)
    a = nat.HmcArgs()
    common(a, 1)
    a.eps, a.n_iter, a.u_accept = eps.ctypes.data_as(nat.c_dblp), n_iter.ctypes.data_as(nat.c_i32p), u.ctypes.data_as(nat.c_dblp)
    a.chain = chain
    a.W, a.b = ptr(W), ptr(b)
    a.out_A, a.out_nlp, a.out_E, a.out_accepted = ptr(out_f[:S]), ptr(out_f[S:2 * S]), ptr(out_f[2 * S:]), ptr(out_acc)
    ctx.check(ctx.lib.hmcx_hmc_run(ctx.h, a), "hmcx_hmc_run")
    keep.append((W, b, out_f, out_acc, eps, n_iter, u))
    return W, out_f


def run_chains(C):
    eps = np.full(S, EPS)
    n_iter = np.full(S * C, NIT, dtype=np.int32)
    u = np.full(S * C, 0.5)
    W = torch.zeros((D, C * K), dtype=torch.float64, device=dev)
    b = torch.zeros(C * K, dtype=torch.float64, device=dev)
    nsc = S * C
    out_f = torch.empty(4 * nsc, dtype=torch.float64, device=dev)
    out_acc = torch.empty(nsc, dtype=torch.int32, device=dev)
    a = nat.HmcChainsArgs()
    common(a, C)
    a.C, a.chain0 = C, 0
    a.eps, a.n_iter, a.u_accept = eps.ctypes.data_as(nat.c_dblp), n_iter.ctypes.data_as(nat.c_i32p), u.ctypes.data_as(nat.c_dblp)
    a.W, a.b = ptr(W), ptr(b)
    a.out_A, a.out_nlp, a.out_E, a.out_accepted = ptr(out_f[:nsc]), ptr(out_f[nsc:2 * nsc]), ptr(out_f[2 * nsc:]), ptr(out_acc)
    ctx.check(ctx.lib.hmcx_hmc_chains_run(ctx.h, a), "hmcx_hmc_chains_run")
    torch.cuda.synchronize()
    return W, out_f


def timed(fn):
    ctx.set_timing(True)
    r = fn()
    torch.cuda.synchronize()
    ms, n = ctx.get_timing()
    ctx.set_timing(False)
    return ms, n, r


def emit(**kw):
    kw.update(lib=lib_name, N=X.shape[0], D=D, K=K, steps=S, n_iter=NIT, dtype="f64")
    print(json.dumps(kw), flush=True)


def seq(C):
    keep = []
    for c in range(C):
        run_single(c, keep)
    torch.cuda.synchronize()
    return keep


# warm-up, then the single-chain call
timed(lambda: seq(1))
one = sorted(timed(lambda: seq(1))[0] for _ in range(3))
emit(what="hmcx_hmc_run", C=1, ms=one[1], all_ms=one)
W1 = seq(1)[0][0].cpu().numpy()
if "--one-chain" in sys.argv:      # only the C = 1 line: for A/B runs that alternate two libraries
    sys.exit(0)
for C in (6, 48):
    reps = 3 if one[1] * C * 3 < 90e3 else 1
    t = sorted(timed(lambda: seq(C))[0] for _ in range(reps))
    emit(what="sequential hmcx_hmc_run", C=C, ms=t[len(t) // 2], all_ms=t, reps=reps)
if has_chains:
    for C in (1, 6, 48):
        timed(lambda: run_chains(C))
        res = [timed(lambda: run_chains(C)) for _ in range(3)]
        t = sorted(r[0] for r in res)
        emit(what="hmcx_hmc_chains_run", C=C, ms=t[1], all_ms=t)
        Wc = res[0][2][0].cpu().numpy()
        # chain 0 of the batched call against the single-chain call on the same stream
        emit(what="chain0 max rel diff vs hmcx_hmc_run", C=C,
             value=float(np.max(np.abs(Wc[:, :K] - W1) / (np.abs(W1) + 1e-300))))

# launch-bound shape: host wall time of one hmcx_hmc_run call plus synchronize (where per-call uploads
# and launch overhead show), median of 21 calls after a warm-up
X, Y = problem(N_SMALL)


def wall():
    t0 = time.perf_counter()
    seq(1)
    return (time.perf_counter() - t0) * 1e3


wall()
w = sorted(wall() for _ in range(21))
emit(what="hmcx_hmc_run wall", C=1, ms=w[10], q1_ms=w[5], q3_ms=w[15], all_ms=w)
