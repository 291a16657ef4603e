"""Heterogeneous, host-scripted SGHMC schedules for the chain-compaction tests (test infrastructure;
tests/test_gpu_chain_compaction.py drives the device with them, tests/test_sghmc_batch_plan.py checks
their preconditions on the CPU).

A case has C device chains and P prototypes.  Chain c follows prototype c mod P at every step: its path
length at step s is table[(c mod P + 5·s) mod P], and the chains of one prototype read one noise region
(noise_off), so the float64 reference (tests/_sghmc_ref.py) runs P chains while every one of the C
device chains is compared.  The accept uniforms differ per chain — spread over [0.3, 0.7] by chain
index — and the tables hold only path lengths whose acceptance probability is >= 0.9 or <= 0.1, so the
chains of a prototype take the same decisions and no decision is within reach of rounding.
With C >= 512, P >= 48: no two chains within three 16-chain tiles share a prototype.
"""
import functools

import numpy as np

from oracle import inputs as gi

from _sghmc_ref import flip_features, sghmc_step

N_STEPS = 3
ALPHA = 0.01


def _table(counts):
    """{n_iter: prototypes holding it} -> table, values interleaved so that neighbouring prototypes
    (neighbouring chains) differ in path length."""
    vals = [v for v, n in sorted(counts.items()) for _ in range(n)]
    P = len(vals)
    stride = next(k for k in (7, 5, 3, 1) if np.gcd(k, P) == 1)
    return [vals[(i * stride) % P] for i in range(P)]


# name -> shape, step size and path-length table ({n_iter: number of prototypes}); see the shapes table
# in tests/test_gpu_chain_compaction.py for what each reaches
CASES = {
    "S1": dict(C=40, B=50, D=50, K=10, eps=5e-2, seed=201, counts={0: 1, 1: 1, 2: 2, 4: 1, 9: 1, 10: 1, 12: 1}),
    "S2": dict(C=528, B=70, D=64, K=10, eps=5e-2, seed=202, counts={0: 3, 1: 14, 2: 14, 9: 8, 10: 5, 11: 4}),
    "S3": dict(C=528, B=460, D=976, K=10, eps=5e-3, seed=203, counts={0: 1, 1: 1, 2: 12, 6: 20, 7: 14}),
    "S4a": dict(C=5, B=50, D=50, K=10, eps=5e-2, seed=204, counts={0: 1, 1: 2, 9: 1, 11: 1}),
    "S4b": dict(C=20, B=50, D=50, K=7, eps=5e-2, seed=205, counts={0: 1, 1: 2, 2: 2, 4: 1, 9: 2, 10: 1, 12: 1}),
    "S4c": dict(C=16, B=50, D=33, K=10, eps=5e-2, seed=206, counts={0: 1, 1: 1, 2: 2, 3: 1, 10: 2, 12: 1}),
}


@functools.lru_cache(maxsize=None)
def schedule(name):
    """The designed schedule of a case: dict with the arrays _schedule returns (n_iter, u, noise_off
    [N_STEPS, C]; noise 1-D float64), the prototype of every chain, the per-prototype path lengths
    ni_p [N_STEPS, P] and noise offsets off_p [N_STEPS, P], and the data (X, Y, rows)."""
    c = CASES[name]
    C, B, D, K = c["C"], c["B"], c["D"], c["K"]
    table = _table(c["counts"])
    P = len(table)
    assert C % P == 0 and (C < 512 or P >= 48)
    Ppar = D * K + K
    proto = np.arange(C) % P
    ni_p = np.array([[table[(p + 5 * s) % P] for p in range(P)] for s in range(N_STEPS)], dtype=np.int32)
    sizes = Ppar * (1 + ni_p.astype(np.int64))
    off_p = (np.cumsum(sizes.reshape(-1)) - sizes.reshape(-1)).reshape(N_STEPS, P)
    noise = np.random.RandomState(c["seed"]).standard_normal(int(sizes.sum()))
    u = np.tile(0.3 + 0.4 * np.arange(C) / max(C - 1, 1), (N_STEPS, 1))
    X, Y = gi.dataset(c["seed"] + 1000, N_STEPS * B, D, K)
    for a in (noise, X, Y):
        a.setflags(write=False)
    return dict(n_iter=ni_p[:, proto].copy(), u=u, noise=noise, noise_off=off_p[:, proto].copy(), proto=proto,
                P=P, ni_p=ni_p, off_p=off_p, X=X, Y=Y, rows=[s * B for s in range(N_STEPS)])


@functools.lru_cache(maxsize=None)
def reference(name, dtype="float64", flip=False):
    """The P prototype chains of a case through tests/_sghmc_ref.py from the zero start, computed once
    per session and shared (arrays read-only).  Returns dict of [N_STEPS, P, ...] arrays: states
    (flat, weights then bias, in the unflipped feature order), A, E [.., 2], accepted, ll.  The accept
    uniform is 0.5: by the precondition on A (check_conditions) any u in [0.3, 0.7] decides alike."""
    c = CASES[name]
    sc = schedule(name)
    B, D, K, P = c["B"], c["D"], c["K"], sc["P"]
    Ppar = D * K + K
    dt = np.dtype(dtype).type
    out = dict(states=np.zeros((N_STEPS, P, Ppar)), A=np.zeros((N_STEPS, P)), E=np.zeros((N_STEPS, P, 2)),
               accepted=np.zeros((N_STEPS, P), dtype=bool), ll=np.zeros((N_STEPS, P)))
    for p in range(P):
        q = {"weights": np.zeros((D, K)), "bias": np.zeros(K)}
        for s in range(N_STEPS):
            r, ni, off = sc["rows"][s], int(sc["ni_p"][s, p]), int(sc["off_p"][s, p])
            Xb, Yb, z = sc["X"][r:r + B], sc["Y"][r:r + B], sc["noise"][off:off + Ppar * (1 + ni)]
            if flip:
                _, Xb, z = flip_features(q, Xb, z)         # q is kept in the flipped order already
            q, A, E, acc, ll = sghmc_step(q, Xb, Yb, c["eps"], ALPHA, ni, z, 0.5, dtype=dt)
            w = q["weights"][::-1] if flip else q["weights"]
            out["states"][s, p] = np.concatenate([np.asarray(w, dtype=np.float64).reshape(-1), q["bias"]])
            out["A"][s, p], out["E"][s, p], out["accepted"][s, p], out["ll"][s, p] = A, E, acc, ll
    for a in out.values():
        a.setflags(write=False)
    return out


def check_conditions(name):
    """The preconditions of a case, on the reference alone: every moving (step, prototype) pair has
    A >= 0.9 or A <= 0.1, the float32 reference and the flipped float64 reference take the same
    decisions, and accept and reject each cover at least 20 % of the moving (step, chain) pairs.
    If one fails after a change of the data or the shapes, change the case's table, not this."""
    sc, ref = schedule(name), reference(name)
    moving = sc["ni_p"] > 0
    A = ref["A"][moving]
    assert np.all((A >= 0.9) | (A <= 0.1)), "%s: undecided A %s" % (name, A[(A < 0.9) & (A > 0.1)])
    assert np.all(ref["accepted"][~moving])
    np.testing.assert_array_equal(reference(name, flip=True)["accepted"], ref["accepted"])
    if name in ("S1", "S2"):
        r32 = reference(name, "float32")
        np.testing.assert_array_equal(r32["accepted"], ref["accepted"])
        A32 = r32["A"][moving]
        assert np.all((A32 >= 0.9) | (A32 <= 0.1))
    mv = sc["n_iter"] > 0                                   # per (step, chain)
    acc = ref["accepted"][np.arange(N_STEPS)[:, None], sc["proto"][None, :]]
    share = np.sum(acc & mv) / np.sum(mv)
    assert 0.2 <= share <= 0.8, "%s: accepted share of the moving pairs %.3f" % (name, share)
    assert np.any(~moving) and len(set(sc["ni_p"][0])) < sc["P"]          # zeros and ties
    return share


def reject_delta(name):
    """δ of a case: the largest relative difference of the rejected trajectories' E_new between the
    float64 reference and the same reference with the feature axis reversed (another summation
    order, the same mathematics) — how far summation order alone moves those hot energies."""
    sc, ref, rf = schedule(name), reference(name), reference(name, flip=True)
    rej = (sc["ni_p"] > 0) & ~ref["accepted"]
    e, ef = ref["E"][..., 1][rej], rf["E"][..., 1][rej]
    return float(np.max(np.abs(e - ef) / np.abs(e)))


def f32_distance(name):
    """Per step: the largest |float32 reference − float64 reference| over the prototypes' kept states,
    and the scale (largest |state|) of the float64 reference."""
    ref, r32 = reference(name), reference(name, "float32")
    d = np.abs(r32["states"] - ref["states"]).reshape(N_STEPS, -1).max(axis=1)
    return d, np.abs(ref["states"]).reshape(N_STEPS, -1).max(axis=1)


def c_act(name):
    """[N_STEPS][it] chains still moving at leapfrog iteration it (the launcher's c_act)."""
    ni = schedule(name)["n_iter"]
    return [[int(np.sum(ni[s] > it)) for it in range(int(ni[s].max()))] for s in range(N_STEPS)]
