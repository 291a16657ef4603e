"""Device time of hmcx_mh_run (random-walk Metropolis, linear models) per step, and where it goes.
MNIST-shaped softmax, full batch N = 10000, D = 784, K = 10, f64 and f32, C = 1, 6, 48 chains, 20 steps per
call with the trace on (a sampling phase), Philox noise, multipliers 0.002 and u = 0.5 (a mix of accepts
and rejects).

    python tools/mh_measure.py [--out FILE]
        per (dtype, C): a warm-up call, then three timed calls (hmcx_set_timing / hmcx_get_timing); one
        JSON line with the median device ms per step.
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/mh_measure.py [--out FILE]
    python tools/mh_measure.py --summarize DIR [--out FILE]
        the same run under the profiler, then per (dtype, C) one JSON line with the per-kernel device µs per
        step (median over the three timed calls of the summed kernel durations of a call ÷ steps; a call's
        S + 1 forward passes include the one at the starting states) and the share outside k_fwd.  Calls are
        told apart in the kernel trace by their closing k_mh_commit launch, in the order this script makes them.

Lines are printed and appended to FILE (default profiles/mh_measure.jsonl)."""
import csv
import glob
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, K, S = 10000, 784, 10, 20
CONFIGS = [(dt, C) for dt in ("f64", "f32") for C in (1, 6, 48)]
CALLS = 4                                    # per configuration: one warm-up, three timed
KERNELS = ("k_fwd", "k_mh_propose", "k_mh_accept", "k_mh_commit")

out_path = os.path.join(REPO, "profiles", "mh_measure.jsonl")
if "--out" in sys.argv:
    out_path = sys.argv[sys.argv.index("--out") + 1]


def emit(**kw):
    kw.update(N=N, D=D, K=K, steps=S)
    line = json.dumps(kw)
    print(line, flush=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def summarize(folder):
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under " + folder)
    rows = []
    for fn in files:
        with open(fn, newline="") as f:
            for r in csv.DictReader(f):
                r = {k.lower(): v for k, v in r.items()}
                rows.append((int(r["start_timestamp"]), int(r["end_timestamp"]), r["kernel_name"]))
    rows.sort()
    calls, cur = [], dict.fromkeys(KERNELS + ("other",), 0.0)
    for t0, t1, name in rows:
        kind = next((k for k in KERNELS if k in name), "other")
        if kind == "other" and not any(cur[k] for k in KERNELS):
            continue                             # torch fills / copies between two calls
        cur[kind] += (t1 - t0) / 1e3             # µs
        if kind == "k_mh_commit":
            calls.append(cur)
            cur = dict.fromkeys(KERNELS + ("other",), 0.0)
    if len(calls) != len(CONFIGS) * CALLS:
        raise SystemExit("expected %d hmcx_mh_run calls in the trace, found %d" % (len(CONFIGS) * CALLS, len(calls)))
    for i, (dt, C) in enumerate(CONFIGS):
        timed = calls[i * CALLS + 1:(i + 1) * CALLS]
        med = {k: sorted(c[k] for c in timed)[1] / S for k in timed[0]}
        tot = sum(med.values())
        emit(what="hmcx_mh_run kernels", dtype=dt, C=C, us_per_step={k: round(v, 3) for k, v in med.items()},
             us_per_step_total=round(tot, 3), share_outside_k_fwd=round(1.0 - med["k_fwd"] / tot, 4),
             source="rocprofv3 --kernel-trace --stats")


if "--summarize" in sys.argv:
    summarize(sys.argv[sys.argv.index("--summarize") + 1])
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, REPO)
from dropout_hamiltonian_montecarlo_amd import _native as nat  # noqa: E402
from dropout_hamiltonian_montecarlo_amd._native import ptr  # noqa: E402

dev = torch.device("cuda:0")
ctx = nat.context(dev)
rs = np.random.RandomState(0)
P = D * K + K
X64 = rs.rand(N, D)
Y64 = np.zeros((N, K))
Y64[np.arange(N), rs.randint(0, K, N)] = 1.0


def run(dt, C, X, Y):
    tdt = torch.float64 if dt == "f64" else torch.float32
    nsc = S * C
    mult = np.full(nsc * 2, 0.002)
    site = np.full(nsc * 2, -1, dtype=np.int32)
    u = np.full(nsc, 0.5)
    W = torch.zeros((D, C * K), dtype=tdt, device=dev)
    b = torch.zeros(C * K, dtype=tdt, device=dev)
    out_f = torch.empty(2 * nsc, dtype=torch.float64, device=dev)
    out_acc = torch.empty(nsc, dtype=torch.int32, device=dev)
    tr = torch.empty((S, C, P), dtype=tdt, device=dev)
    a = nat.MhArgs()
    a.dtype, a.model = (nat.HMCX_F64 if dt == "f64" else nat.HMCX_F32), nat.MODEL_SOFTMAX
    a.B, a.D, a.K, a.C, a.n_steps = N, D, K, C, S
    a.alpha, a.log_prior = 0.01, -1.234
    a.X, a.Y = ptr(X), ptr(Y)
    a.mult, a.site = mult.ctypes.data_as(nat.c_dblp), site.ctypes.data_as(nat.c_i32p)
    a.u_accept = u.ctypes.data_as(nat.c_dblp)
    a.noise_mode, a.seed, a.chain0, a.step_base = nat.NOISE_PHILOX, 7, 0, 0
    a.W, a.b = ptr(W), ptr(b)
    a.out_A, a.out_logp, a.out_accepted, a.out_trace = ptr(out_f[:nsc]), ptr(out_f[nsc:]), ptr(out_acc), ptr(tr)
    ctx.set_timing(True)
    ctx.check(ctx.lib.hmcx_mh_run(ctx.h, a), "hmcx_mh_run")
    torch.cuda.synchronize()
    ms, n = ctx.get_timing()
    ctx.set_timing(False)
    assert n == 1
    return ms, float(out_acc.float().mean().item())


for dt, C in CONFIGS:
    tdt = torch.float64 if dt == "f64" else torch.float32
    X, Y = torch.as_tensor(X64).to(dev, tdt), torch.as_tensor(Y64).to(dev, tdt)
    res = [run(dt, C, X, Y) for _ in range(CALLS)]
    t = sorted(r[0] for r in res[1:])
    emit(what="hmcx_mh_run", dtype=dt, C=C, ms_per_step=t[1] / S, all_ms_per_call=t, accept_rate=res[1][1],
         source="hmcx_get_timing")
