"""Float64 reference of the MLP posterior predictive (hmcx_mlp_predictive / mlp.posterior_predictive):
oracle.models.mlp._forward per draw plus NumPy, all eight quantities, and the small problems the CPU and
GPU tests share.  Draw d = s·T + t is parameter set s under mask block d.

The seeds below are the ones for which the oracle meets the "gap" preconditions of the exact comparisons
(argmax outputs are only comparable when no reference decision hangs on rounding);
tests/test_mlp_predictive_cpu.py asserts them on the oracle alone and is the authority: a seed that stops
meeting a condition is searched again, the condition stays."""
import functools
from collections import namedtuple

import numpy as np

from oracle import models as om

Ref = namedtuple("Ref", "mean pred entropy expected_entropy mutual_information lppd draw_nll draw_correct "
                        "draw_accuracy mean_gap logit_gap")


def _top2_gap(a):
    """Smallest difference between the largest and second largest entry of a row (inf for one column)."""
    if a.shape[-1] < 2:
        return np.inf
    s = np.sort(a, axis=-1)
    return float((s[..., -1] - s[..., -2]).min())


def _entropy(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log(p), 0.0)
    return -t.sum(axis=-1)


def predictive_ref(par_sets, X, y=None, masks=None, T=1):
    """par_sets: S parameter dicts; masks: None (no dropout, T must be 1) or [S·T, 3, N, n_mid]."""
    X = np.asarray(X, dtype=np.float64)
    S, N = len(par_sets), X.shape[0]
    D = S * T
    assert masks is not None or T == 1
    shp = par_sets[0]['/l1/W'].shape
    net = om.mlp({"alpha": 0.0}, shp[1], shp[0], par_sets[0]['/l3/W'].shape[0])
    zs, ps = [], []
    for d in range(D):
        par = {k: np.asarray(v, dtype=np.float64) for k, v in par_sets[d // T].items()}
        z, _ = net._forward(par, X, None if masks is None else list(np.asarray(masks[d], dtype=np.float64)))
        e = np.exp(z - z.max(axis=1, keepdims=True))
        zs.append(z)
        ps.append(e / e.sum(axis=1, keepdims=True))
    z, p = np.stack(zs), np.stack(ps)                              # [D, N, K]
    mean = p.mean(axis=0)
    ent, eent = _entropy(mean), _entropy(p).mean(axis=0)
    lppd = nll = corr = acc = None
    if y is not None:
        t = np.asarray(y).astype(int)
        py = p[:, np.arange(N), t]                                 # [D, N]
        lppd = np.log(py.mean(axis=0))
        nll = np.array([net._ce(z[d], t)[0] for d in range(D)])
        corr = (z.argmax(axis=2) == t[None, :]).sum(axis=1).astype(np.int32)
        acc = corr / float(N)
    return Ref(mean, mean.argmax(axis=1), ent, eent, ent - eent, lppd, nll, corr, acc, _top2_gap(mean), _top2_gap(z))


# ----------------------------------------------------------------------------- shared problems
# (N, n_in, n_mid, n_out, S, T), whether the fused kernel serves the shape, seed (float64 gaps > 1e-6 and
# float32-rounded gaps > 1e-3 on every row, with and without dropout)
Case = namedtuple("Case", "shape fused seed")
CASES = [
    Case((19, 50, 37, 7, 3, 2), False, 1),      # general path, nothing aligned
    Case((1, 3, 1, 2, 1, 1), False, 1),         # smallest shape
    Case((70, 33, 64, 40, 2, 1), False, 4),     # n_out beyond the fused limit
    Case((20, 16, 32, 5, 4, 3), True, 1),       # fused path, row blocks 16 + 4
    Case((36, 40, 96, 16, 5, 2), True, 6),      # fused path, three column waves, n_out at the limit
    Case((4, 8, 256, 2, 2, 2), True, 1),        # fused path, full width, a single short row block
    # fused path, just past two row blocks (16 + 16 + 3); 40 draws: more than the 32 draw groups a launch
    # takes, so a workgroup loops over several draws
    Case((35, 24, 64, 3, 2, 20), True, 3),
]
MULTIBLOCK = CASES[6]
GAP64, GAP32 = 1e-6, 1e-3


def fused_eligible(n_in, n_mid, n_out, elt):
    """Python twin of hmcx_mlp_pred.hip::pred_fused_shape_ok (16 rows of X, h1 and d3 within 160 KiB)."""
    if n_mid % 32 or n_mid > 256 or n_out > 16 or n_in % 8:
        return False
    up = lambda b: (b + 15) // 16 * 16
    pad = 16 // elt
    xp, hp = (n_in + 15) // 16 * 16 + pad, n_mid + pad
    total = up(16 * xp * elt) + 2 * up(16 * hp * elt) + up(8 * 16 * 17 * elt) + up(3 * 132 * 4) + up(128) + up(64)
    return total <= 160 * 1024


def f32r(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


Problem = namedtuple("Problem", "par_sets X y masks")


@functools.lru_cache(maxsize=None)
def problem(shape, seed, rounded=False):
    """S parameter sets, X, labels and D mask blocks of a case (read-only: shared between tests).
    rounded: every input rounded through float32 (what a float32 model sees)."""
    N, n_in, n_mid, n_out, S, T = shape
    rs = np.random.RandomState(seed)
    sets = [{k: rs.normal(0, 0.3, s) for k, s in om.mlp_param_shapes(n_in, n_mid, n_out).items()} for _ in range(S)]
    X = rs.rand(N, n_in)
    y = rs.randint(0, n_out, N)
    masks = np.stack([np.stack(om.dropout_masks(rs, N, n_mid, dtype=np.float64)) for _ in range(S * T)])
    if rounded:
        sets = [{k: f32r(v) for k, v in p.items()} for p in sets]
        X, masks = f32r(X), f32r(masks)
    return Problem(sets, X, y, masks)


def stack(par_sets):
    """{name: [S, *shape]} as sample() returns it."""
    return {k: np.stack([p[k] for p in par_sets]) for k in om.MLP_PARAM_NAMES}


@functools.lru_cache(maxsize=None)
def case_ref(shape, seed, dropout=True, rounded=False):
    """The reference of a case: with its D mask blocks, or (dropout False) of the S sets without dropout."""
    pb = problem(shape, seed, rounded)
    if dropout:
        return predictive_ref(pb.par_sets, pb.X, pb.y, pb.masks, shape[5])
    return predictive_ref(pb.par_sets, pb.X, pb.y, None, 1)
