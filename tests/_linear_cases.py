"""Case tables, references and tolerances of the linear-model kernel tests (test infrastructure):
tests/test_gpu_linear_kernels.py and test_sgld_f32_paths_vs_oracle (tests/test_gpu_samplers.py) drive the
device with them, tests/test_linear_cases_cpu.py checks their preconditions on the CPU.

Primitive matrix.  Every softmax case (B, D, K, C) and logistic case (B, D, C) is the smallest shape that
reaches one instantiation of k_fwd<T, NBLK, VEC, NW> / k_grad<T, NBLK, NW> (csrc/hmcx_softmax.hip) through
the C ABI; ``fwd_instance`` / ``grad_instance`` mirror the host code that picks the instantiation, and the
table states which one every case is meant to reach, so a retuned threshold fails the CPU test instead of
hollowing the GPU ones out.  Inputs come from oracle/inputs.py; chain 0 holds its weights, the further
chains (parameter sets) independent draws of the same scale.

References are oracle/models.py in float64, per chain.  ``dtype='float32'`` rounds the inputs to float32
first and widens them again, so the float64 reference sees what the float32 kernel sees and input rounding
is not counted as kernel error.  The yardstick of the float32 tolerances is the same NumPy code run in
float32 (dtype-preserving clip bounds): d = the largest |float32 run − float64 run| of an output of a case.

SGLD.  ``sgld_reference`` runs oracle/samplers.py::sgld on the float32-rounded data in float64 (the
reference) or in float32 throughout (the yardstick: float32 data, start and noise).
"""
import functools
import io

import numpy as np

from oracle import inputs as gi
from oracle import models as om
from oracle import samplers as osm

from _sghmc_ref import _softmax

SOFTMAX_ALPHA = 0.01
LOGISTIC_ALPHA = 0.25            # tests/test_gpu_logistic_sgd.py
F32_GRAD = 2e-5                  # of the |X|ᵀ|ŷ − y| + α|θ| scale, + 1 (tests/test_gpu_softmax.py)
F32_FLOOR = 1e-5                 # of the output's scale (tests/test_gpu_chain_compaction.py)
F32_FACTOR = 16                  # × d (same)


# ---------------------------------------------------------------------------------- tiling mirror
def make_tiling(B, D, K, C):
    """make_tiling (csrc/hmcx_softmax.hip, after launch_fwd_split): CB chains per tile, NBLK 16-column
    MFMA tiles per chain tile, and the grid extents."""
    CB = 1 if K >= 64 else min(64 // K, C)
    CB = max(CB, 1)
    NT = (CB * K + 15) // 16 * 16
    return dict(CB=CB, NBLK=NT // 16, nCT=-(-C // CB), nRB=-(-B // 16), nDB=-(-D // 16))


def fwd_instance(B, D, K, C):
    """(NBLK, VEC, NW) of the k_fwd that launch_fwd (csrc/hmcx_softmax.hip) runs for a direct call
    (hmcx_softmax_grad / _loglik / _predict: slab_mode 0, one D slice): ``vec = D % 4 == 0``;
    ``deep = nRB·nCT·nz <= 512 && D / nz >= 1024``; the switch gives NBLK 1 and 2 eight waves and
    NBLK 3 and 4 (the default branch) eight when deep, else four."""
    t = make_tiling(B, D, K, C)
    deep = t["nRB"] * t["nCT"] <= 512 and D >= 1024
    nblk = t["NBLK"] if t["NBLK"] <= 3 else 4
    return nblk, D % 4 == 0, 8 if (nblk <= 2 or deep) else 4


def grad_instance(B, D, K, C):
    """(NBLK, NW) of the k_grad that launch_grad runs: ``deep = nDB·nCT <= 512``, same switch."""
    t = make_tiling(B, D, K, C)
    deep = t["nDB"] * t["nCT"] <= 512
    nblk = t["NBLK"] if t["NBLK"] <= 3 else 4
    return nblk, 8 if (nblk <= 2 or deep) else 4


ALL_FWD = {(n, v, 8) for n in (1, 2) for v in (False, True)} | \
          {(n, v, w) for n in (3, 4) for v in (False, True) for w in (4, 8)}
ALL_GRAD = {(1, 8), (2, 8), (3, 8), (3, 4), (4, 8), (4, 4)}


# ---------------------------------------------------------------------------------- case tables
def _sm(B, D, K, C, fwd, grad, seed=11, wscale=0.3):
    return dict(B=B, D=D, K=K, C=C, fwd=fwd, grad=grad, seed=seed, wscale=wscale)


# shape, the forward (NBLK, vector X loads, waves) and gradient (NBLK, waves) it is meant to reach
SOFTMAX_CASES = [
    _sm(1, 1, 2, 1, (1, False, 8), (1, 8)),            # one row, one feature
    _sm(33, 68, 16, 1, (1, True, 8), (1, 8)),          # 1-row last block; a wave owning 4 features
    _sm(16, 64, 16, 1, (1, True, 8), (1, 8)),          # exact tiles
    _sm(20, 37, 17, 1, (2, False, 8), (2, 8)),         # K one past a class tile
    _sm(40, 100, 10, 3, (2, True, 8), (2, 8)),         # three chains in one tile
    _sm(35, 100, 38, 1, (3, True, 4), (3, 8)),
    _sm(35, 101, 38, 1, (3, False, 4), (3, 8)),
    _sm(20, 1028, 38, 1, (3, True, 8), (3, 8), seed=12),    # deep forward (seed 11: the last class column moves ll by 0.1 tol)
    _sm(20, 1027, 38, 1, (3, False, 8), (3, 8)),
    _sm(20, 160, 38, 52, (3, True, 4), (3, 4)),        # nDB·nCT = 520 > 512
    _sm(21, 30, 49, 1, (4, False, 4), (4, 8)),
    _sm(18, 1028, 64, 1, (4, True, 8), (4, 8), seed=12),    # largest K (seed 11: the last class column moves gb by 1.5 tol)
    _sm(18, 1030, 64, 1, (4, False, 8), (4, 8)),
    _sm(20, 784, 10, 61, (4, True, 4), (4, 4)),        # 11 chain tiles, the last with one chain
    _sm(19, 70, 10, 13, (4, False, 4), (4, 8)),        # last tile with one chain
]


def _lg(B, D, C, nblk, seed=11, wscale=0.3, saturated=False):
    return dict(B=B, D=D, C=C, nblk=nblk, seed=seed, wscale=wscale, saturated=saturated)


# (B, D, C) and the NBLK it reaches; the last two are the shapes and weight scales of
# oracle.inputs.LOGISTIC_CASES[3] and [4]: logits far past ±17, where a float32 sigmoid is exactly 0 or 1.
# Their seeds are the first from which the last row is misclassified (with the inputs' own seeds 3 and 4
# it is saturated on the right side, y − ŷ = 0, and leaving it out moves no gradient) and both labels
# occur among the rows with z > 17 (tests/test_linear_cases_cpu.py)
LOGISTIC_CASES = [
    _lg(1, 1, 1, 1),
    _lg(77, 33, 1, 1),
    _lg(30, 12, 20, 2),
    _lg(25, 1028, 40, 3),                               # deep
    _lg(50, 8, 70, 4),                                  # tiles of 64 + 6 parameter sets
    _lg(gi.LOGISTIC_CASES[3][1], gi.LOGISTIC_CASES[3][2], 1, 1, seed=10, wscale=gi.LOGISTIC_CASES[3][3],
        saturated=True),
    _lg(gi.LOGISTIC_CASES[4][1], gi.LOGISTIC_CASES[4][2], 1, 1, seed=5, wscale=gi.LOGISTIC_CASES[4][3],
        saturated=True),
]


def case_id(c):
    return "-".join(str(c[k]) for k in ("B", "D", "K", "C") if k in c) + ("-sat" if c.get("saturated") else "")


def _round32(a):
    return a.astype(np.float32).astype(np.float64)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def softmax_problem(i, dtype="float64"):
    """X [B, D], Y [B, K], Ws [C, D, K], bs [C, K] of SOFTMAX_CASES[i] in float64 (read-only, shared);
    dtype 'float32': every value rounded to float32."""
    c = SOFTMAX_CASES[i]
    X, Y, W, b = gi.softmax_inputs(c["seed"], c["B"], D=c["D"], K=c["K"], wscale=c["wscale"])
    rs = np.random.RandomState(c["seed"] + 7000)
    Ws = np.concatenate([W[None], rs.normal(0, c["wscale"], (c["C"] - 1, c["D"], c["K"]))])
    bs = np.concatenate([b[None], rs.normal(0, c["wscale"], (c["C"] - 1, c["K"]))])
    if dtype == "float32":
        X, Ws, bs = _round32(X), _round32(Ws), _round32(bs)
    return _freeze(X, Y, Ws, bs)


@functools.lru_cache(maxsize=None)
def logistic_problem(i, dtype="float64"):
    """X [B, D], y [B], Ws [C, D, 1], bs [C, 1] of LOGISTIC_CASES[i]."""
    c = LOGISTIC_CASES[i]
    X, y, W, b = gi.logistic_inputs(c["seed"], c["B"], c["D"], wscale=c["wscale"])
    rs = np.random.RandomState(c["seed"] + 7000)
    Ws = np.concatenate([W[None], rs.normal(0, c["wscale"], (c["C"] - 1, c["D"], 1))])
    bs = np.concatenate([b[None], rs.normal(0, c["wscale"], (c["C"] - 1, 1))])
    if dtype == "float32":
        X, Ws, bs = _round32(X), _round32(Ws), _round32(bs)
    return _freeze(X, y, Ws, bs)


# ---------------------------------------------------------------------------------- references
class _logistic(om.logistic):
    """oracle logistic whose clip bounds take the dtype of the logits and whose prior weight is a plain
    float (a no-op in float64; keeps a float32 run in float32)."""

    def __init__(self, hyper):
        self.hyper = dict(hyper)

    def net(self, par, **args):
        y_linear = np.dot(np.asarray(args["X_train"]), par["weights"]) + par["bias"]
        y_linear = np.minimum(y_linear, y_linear.dtype.type(om.CLIP_HI))
        y_linear = np.maximum(y_linear, y_linear.dtype.type(om.CLIP_LO))
        return self.sigmoid(y_linear)


def softmax_outputs(X, Y, Ws, bs):
    """gW [C, D, K], gb [C, K], ll [C], prob [C, B, K] of C parameter sets on one minibatch, in the dtype of
    the arrays (ll as float64 scalars), and the gradient scales sW, sb = |X|ᵀ|ŷ − y| + α|θ|."""
    m = _softmax({"alpha": SOFTMAX_ALPHA})
    out = dict(gW=[], gb=[], ll=[], prob=[], sW=[], sb=[])
    for W, b in zip(Ws, bs):
        par = {"weights": W, "bias": b}
        g = m.grad(par, X_train=X, y_train=Y)
        p = m.net(par, X)
        R = np.abs(p - Y)
        out["gW"].append(g["weights"])
        out["gb"].append(g["bias"])
        out["ll"].append(float(m.log_likelihood(par, X_train=X, y_train=Y)))
        out["prob"].append(p)
        out["sW"].append(np.abs(X).T @ R + SOFTMAX_ALPHA * np.abs(W))
        out["sb"].append(R.sum(0) + SOFTMAX_ALPHA * np.abs(b))
    return {k: np.array(v) for k, v in out.items()}


def logistic_outputs(X, y, Ws, bs):
    """The same for the logistic model: gW [C, D, 1], gb [C, 1], ll [C], prob [C, B, 1]; ``lls`` [C] is the
    absolute-value scale of the log-likelihood, Σ_i (1 + Σ_d |x_id||w_d| + |b|)."""
    m = _logistic({"alpha": LOGISTIC_ALPHA})
    out = dict(gW=[], gb=[], ll=[], prob=[], sW=[], sb=[], lls=[])
    for W, b in zip(Ws, bs):
        par = {"weights": W, "bias": b}
        with np.errstate(all="ignore"):                 # a float32 run overflows exp(−z) and takes log(0)
            g = m.grad(par, X_train=X, y_train=y)
            p = m.net(par, X_train=X)
            ll = float(m.log_likelihood(par, X_train=X, y_train=y))
        R = np.abs(y.reshape(-1, 1) - p)
        out["gW"].append(g["weights"])
        out["gb"].append(g["bias"])
        out["ll"].append(ll)
        out["prob"].append(p)
        out["sW"].append(np.abs(X).T @ R + LOGISTIC_ALPHA * np.abs(W))
        out["sb"].append(R.sum(0) + LOGISTIC_ALPHA * np.abs(b))
        out["lls"].append(float(np.sum(1.0 + np.abs(X) @ np.abs(W)[:, 0] + np.abs(b[0]))))
    return {k: np.array(v) for k, v in out.items()}


def _problem(model, i, dtype):
    return softmax_problem(i, dtype) if model == "softmax" else logistic_problem(i, dtype)


def _outputs(model, X, Y, Ws, bs):
    return softmax_outputs(X, Y, Ws, bs) if model == "softmax" else logistic_outputs(X, Y, Ws, bs)


@functools.lru_cache(maxsize=None)
def reference(model, i, dtype="float64"):
    """float64 reference outputs of case i of ``model`` ('softmax' / 'logistic') on the inputs of ``dtype``,
    computed once per session and shared (read-only)."""
    out = _outputs(model, *_problem(model, i, dtype))
    _freeze(*out.values())
    return out


@functools.lru_cache(maxsize=None)
def f32_distance(model, i):
    """d per output: the largest |NumPy float32 run − float64 reference| of case i.  The logistic
    log-likelihood has none: the float32 run is not finite on the saturated cases."""
    X, Y, Ws, bs = (a.astype(np.float32) for a in _problem(model, i, "float32"))
    lo, ref = _outputs(model, X, Y, Ws, bs), reference(model, i, "float32")
    assert lo["prob"].dtype == np.float32 and lo["gW"].dtype == np.float32
    d = {"prob": float(np.max(np.abs(lo["prob"].astype(np.float64) - ref["prob"])))}
    if model == "softmax":
        d["ll"] = float(np.max(np.abs(lo["ll"] - ref["ll"])))
    return d


def f32_tolerances(model, i, ref=None, d=None):
    """Allowed |device float32 − float64 reference| per output of case i (arrays shaped like the output, or
    scalars).  ``ref`` / ``d`` default to the case's own."""
    ref = reference(model, i, "float32") if ref is None else ref
    d = f32_distance(model, i) if d is None else d
    tol = {"gW": F32_GRAD * (ref["sW"] + 1), "gb": F32_GRAD * (ref["sb"] + 1),
           "prob": max(F32_FACTOR * d["prob"], F32_FLOOR)}
    if model == "softmax":
        tol["ll"] = np.maximum(F32_FACTOR * d["ll"], F32_FLOOR * np.maximum(1.0, np.abs(ref["ll"])))
    else:
        tol["ll"] = F32_GRAD * ref["lls"]
    return tol


def f64_tolerances(model, i):
    """The project's float64 bounds (tests/test_gpu_softmax.py, tests/test_gpu_logistic_sgd.py); the
    probabilities are compared with rtol 1e-11."""
    ref = reference(model, i, "float64")
    B = _problem(model, i, "float64")[0].shape[0]
    return {"gW": 1e-12 * ref["sW"] + 1e-300, "gb": 1e-12 * ref["sb"] + 1e-300,
            "ll": 1e-12 * np.maximum(1.0, np.abs(ref["ll"])) * np.sqrt(B), "prob": 1e-11 * np.abs(ref["prob"]) + 1e-300}


MUTATIONS = ("row", "feature", "wcol")


def mutated(model, i, mutation):
    """The float64 reference outputs of case i (float32-rounded inputs) with one defect a kernel could have:
    'row'     the last minibatch row left out of the gradient and the log-likelihood; for the probabilities
              the last row's output replaced by row 0's — with one row there is no other, so by the output
              of an all-zero row (what a kernel that never loaded the row would give);
    'feature' the last feature column of X zeroed;
    'wcol'    the last class / parameter-set column of W (the last column of [D][C·K]) zeroed."""
    X, Y, Ws, bs = _problem(model, i, "float32")
    if mutation == "row":
        out = dict(_outputs(model, X[:-1], Y[:-1], Ws, bs))
        prob = reference(model, i, "float32")["prob"].copy()
        if X.shape[0] > 1:
            prob[:, -1] = prob[:, 0]
        else:
            prob[:, -1] = _outputs(model, np.zeros_like(X), Y, Ws, bs)["prob"][:, -1]
        out["prob"] = prob
        return out
    if mutation == "feature":
        Xm = X.copy()
        Xm[:, -1] = 0.0
        return _outputs(model, Xm, Y, Ws, bs)
    assert mutation == "wcol"
    Wm = Ws.copy()
    Wm[-1, :, -1] = 0.0
    return _outputs(model, X, Y, Wm, bs)


def old_logistic_loglik_f32(X, y, W, b):
    """The sigmoid-link log-likelihood as the float32 kernel computed it before the fix, in NumPy float32:
    y·log(ŷ) + (1 − y)·log(1 − ŷ) with ŷ = 1/(1 + exp(−z)) rounded to float32 (logistic.py:71)."""
    f = np.float32
    z = np.dot(X.astype(f), W.astype(f)) + b.astype(f)
    z = np.maximum(np.minimum(z, f(om.CLIP_HI)), f(om.CLIP_LO))[:, 0]
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        yh = f(1) / (f(1) + np.exp(-z))
        return float(np.sum(y.astype(f) * np.log(yh) + (f(1) - y.astype(f)) * np.log(f(1) - yh)))


# ---------------------------------------------------------------------------------- SGLD trajectories
SGLD_SHAPES = [(2, 1, 1), (3, 7, 13), (17, 8, 5), (10, 131, 77), (64, 300, 40), (10, 785, 65), (38, 2000, 130)]   # K, D, B
SGLD_PATHS = [("0", None), ("1", "1"), ("1", "0")]          # HMCX_SGLD_WIDE, HMCX_WIDE_FUSE


def sgld_config(K, D, B):
    return dict(kind="sgld", N=2 * B, B=B, D=D, K=K, alpha=0.01, step_size=1e-2, path_length=1.0,
                burnin=1, epochs=2, data_seed=41, np_seed=2, rng_seed=3)


class _rng32:
    """The sampler's RandomState with float32 draws (the float64 draw rounded)."""

    def __init__(self, seed):
        self.rs = np.random.RandomState(seed)

    def normal(self, *a, **kw):
        return self.rs.normal(*a, **kw).astype(np.float32)


class _softmax_drop_row(_softmax):
    """A gradient that leaves the last minibatch row out."""

    def grad(self, par, **args):
        return super().grad(par, X_train=args["X_train"][:-1], y_train=args["y_train"][:-1])


@functools.lru_cache(maxsize=None)
def sgld_reference(K, D, B, dtype="float64", mutation=None):
    """oracle.samplers.sgld from the zero start on the float32-rounded dataset of sgld_config(K, D, B):
    (states [epochs, D·K + K] — weights then bias —, logp [epochs]).  dtype 'float32': data, start and
    noise in float32, so the run stays in float32.  mutation 'row': the last row of every minibatch left
    out of the gradient; 'feature': the last feature of the dataset zeroed."""
    c = sgld_config(K, D, B)
    X, Y = gi.dataset(c["data_seed"], c["N"], D, K)
    dt = np.dtype(dtype).type
    X, Y = X.astype(np.float32).astype(dt), Y.astype(dt)
    if mutation == "feature":
        X[:, -1] = 0
    model = (_softmax_drop_row if mutation == "row" else _softmax)({"alpha": c["alpha"]})
    s = osm.sgld(model, {"weights": np.zeros((D, K), dtype=dt), "bias": np.zeros(K, dtype=dt)},
                 path_length=c["path_length"], step_size=c["step_size"], verbose=True)
    s.out = io.StringIO()
    np.random.seed(c["np_seed"])
    rng = np.random.RandomState(c["rng_seed"]) if dtype == "float64" else _rng32(c["rng_seed"])
    post, logp = s.sample(epochs=c["epochs"], burnin=c["burnin"], batch_size=B, rng=rng, X_train=X, y_train=Y)
    assert post["weights"].dtype == dt and post["bias"].dtype == dt
    states = np.concatenate([post["weights"].reshape(c["epochs"], -1), post["bias"]], axis=1).astype(np.float64)
    return _freeze(states, np.asarray(logp, dtype=np.float64))


def sgld_loglik(K, D, B, logp):
    """The log-likelihood inside logp = −(ll + log_prior) / B (sgmcmc.py:79).  log_prior is a constant of
    the shape (softmax.py:22-30) that dwarfs ll at small B — |logp| is 1550 at (64, 300, 40), of which ll / B
    is 4 — so the same error is measured against ll as well."""
    lp = om.softmax({"alpha": SOFTMAX_ALPHA}).log_prior({"weights": np.zeros((D, K)), "bias": np.zeros(K)})
    return -(B * np.asarray(logp, dtype=np.float64) + lp)


def sgld_tolerances(K, D, B):
    """({output: allowed |device float32 − reference|}, {output: d}) of 'states', 'logp' and 'll' (the
    log-likelihood inside logp, sgld_loglik): max(16·d, 1e-5·s), s the largest |state|, the largest |logp|,
    max(1, largest |ll|)."""
    s64, l64 = sgld_reference(K, D, B)
    s32, l32 = sgld_reference(K, D, B, "float32")
    ll64, ll32 = sgld_loglik(K, D, B, l64), sgld_loglik(K, D, B, l32)
    d = {"states": float(np.max(np.abs(s32 - s64))), "logp": float(np.max(np.abs(l32 - l64))),
         "ll": float(np.max(np.abs(ll32 - ll64)))}
    s = {"states": float(np.max(np.abs(s64))), "logp": float(np.max(np.abs(l64))),
         "ll": max(1.0, float(np.max(np.abs(ll64))))}
    return {o: max(F32_FACTOR * d[o], F32_FLOOR * s[o]) for o in d}, d
