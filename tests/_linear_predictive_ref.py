"""Float64 reference of the linear models' posterior predictive (hmcx_linear_predictive /
softmax.posterior_predictive, logistic.posterior_predictive): oracle.models.softmax.net and
oracle.models.logistic.net per draw plus NumPy, all eight quantities and the top-two gaps, and the small
problems the CPU and GPU tests share.  Draw d = s·T + t is parameter set s under input-dropout mask block d
(X ⊙ Z_d, the reference's predict_stochastic).

The seeds below are the ones for which the oracle meets the "gap" preconditions of the exact comparisons
(pred and draw_correct are only comparable when no reference decision hangs on rounding);
tests/test_linear_predictive_cpu.py asserts them on the oracle alone and is the authority: a seed that stops
meeting a condition is searched again, the condition stays."""
import functools
from collections import namedtuple

import numpy as np

from oracle import models as om

from _predictive_ref import GAP32, GAP64, f32r  # noqa: F401  (the same preconditions as the MLP's)

# mean_gap: smallest top-two gap of a row of `mean` (logistic: smallest |mean − 0.5|); draw_gap: the same for
# every draw's decision (softmax: the clipped logits; logistic: |p_d − 0.5|)
Ref = namedtuple("Ref", "mean pred entropy expected_entropy mutual_information lppd draw_nll draw_correct "
                        "draw_accuracy mean_gap draw_gap")


def _top2_gap(a):
    s = np.sort(a, axis=-1)
    return float((s[..., -1] - s[..., -2]).min())


def _entropy(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log(p), 0.0)
    return -t.sum(axis=-1)


def predictive_ref(model, W, b, X, y=None, masks=None, T=1):
    """model: 'softmax' or 'logistic'; W [S, D, K], b [S, K]; masks: None (no dropout, T must be 1) or
    [S·T, N, D]."""
    X = np.asarray(X, dtype=np.float64)
    W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
    S, N, K = W.shape[0], X.shape[0], W.shape[2]
    D = S * T
    assert masks is not None or T == 1
    logistic = model == 'logistic'
    net = om.logistic({"alpha": 1.0}) if logistic else om.softmax({"alpha": 1.0})
    t = None if y is None else np.asarray(y).astype(int)
    ps, gaps, nll, corr = [], [], [], []
    for d in range(D):
        par = {'weights': W[d // T], 'bias': b[d // T]}
        Xd = X if masks is None else np.multiply(X, np.asarray(masks[d], dtype=np.float64))
        if logistic:
            p1 = net.net(par, X_train=Xd)                              # [N, 1]
            ps.append(np.concatenate([1.0 - p1, p1], axis=1))
            gaps.append(float(np.abs(p1 - 0.5).min()))
            if t is not None:
                nll.append(-net.log_likelihood(par, X_train=Xd, y_train=t) / N)
                corr.append(int(((p1 > 0.5).astype(int).flatten() == t).sum()))
        else:
            z = net.logits(par, Xd)
            ps.append(net.net(par, Xd))
            gaps.append(_top2_gap(z))
            if t is not None:
                nll.append(-net.log_likelihood(par, X_train=Xd, y_train=om.one_hot(t, K)) / N)
                corr.append(int((z.argmax(axis=1) == t).sum()))
    p = np.stack(ps)                                                   # [D, N, classes]
    pm = p.mean(axis=0)
    ent, eent = _entropy(pm), _entropy(p).mean(axis=0)
    if logistic:
        mean, pred = pm[:, 1:], (pm[:, 1] > 0.5).astype(int)
        mean_gap = float(np.abs(pm[:, 1] - 0.5).min())
    else:
        mean, pred, mean_gap = pm, pm.argmax(axis=1), _top2_gap(pm)
    lppd = dn = dc = acc = None
    if t is not None:
        lppd = np.log(p[:, np.arange(N), t].mean(axis=0))
        dn, dc = np.array(nll), np.array(corr, dtype=np.int32)
        acc = dc / float(N)
    return Ref(mean, pred, ent, eent, ent - eent, lppd, dn, dc, acc, mean_gap, min(gaps))


# ----------------------------------------------------------------------------- eligibility and path choice
def fused_eligible(D, K, elt):
    """Python twin of hmcx_lin_pred.hip::lpred_fused_shape_ok: K within one MFMA tile, and 16 rows of X, four
    waves' 16 × 65 logit tiles and their 16 × 18 float64 row partials within 160 KiB of LDS."""
    if K < 1 or K > 16 or D < 1:
        return False
    up = lambda n: (n + 15) // 16 * 16  # noqa: E731
    xp = (D + 15) // 16 * 16 + 16 // elt
    return up(16 * xp * elt) + up(4 * 16 * 65 * elt) + up(4 * 16 * 18 * 8) <= 160 * 1024


def path0_is_fused(N, D, K, elt, S, T, dropout):
    """Python twin of hmcx_lin_pred.hip::lin_pred_path0_fused: with input dropout from 32 draws;
    without, from 4 units (of ⌊64 / K⌋ parameter sets) and either 1536 row-block × unit pairs or 200 sets."""
    if not fused_eligible(D, K, elt):
        return False
    if dropout:
        return S * T >= 32
    spu = 64 // K
    nunits, nrb = (S + spu - 1) // spu, (N + 15) // 16
    return nunits >= 4 and (nrb * nunits >= 1536 or S >= 200)


def first_ineligible_D(K, elt):
    D = 1
    while fused_eligible(D, K, elt):
        D += 1
    return D


# ----------------------------------------------------------------------------- shared problems
# model, (N, D, K, S, T), seed: float64 gaps > 1e-6 and float32-rounded gaps > 1e-3 for every decision, with
# and without dropout
Case = namedtuple("Case", "model shape seed")
CASES = [
    Case('softmax', (1, 1, 2, 1, 1), 0),         # smallest shape
    Case('softmax', (19, 50, 7, 3, 2), 0),       # nothing aligned
    Case('softmax', (35, 24, 3, 2, 20), 8),      # row blocks 16 + 16 + 3; more draws than draw groups
    Case('softmax', (20, 16, 10, 40, 1), 1856),     # many sets per column tile; K does not divide 16
    Case('softmax', (17, 40, 16, 5, 2), 32),      # K at the fused limit
    Case('softmax', (33, 24, 38, 2, 2), 33),      # K beyond the fused limit: general path only
    Case('logistic', (1, 1, 1, 1, 1), 0),        # smallest shape
    Case('logistic', (21, 13, 1, 6, 3), 14),      # dropout, more than one row block
    Case('logistic', (36, 32, 1, 33, 1), 49560),     # many sets, no dropout
]
MULTIBLOCK = {'softmax': CASES[2], 'logistic': CASES[7]}
# N = 5, S = 2 at the smallest D the float64 rule rejects: path 2 must refuse it, path 0 must serve it
LDS_EDGE = Case('softmax', (5, first_ineligible_D(3, 8), 3, 2, 1), 0)


def case_id(c):
    return c.model + "-" + "x".join(map(str, c.shape))


def eligible(c, elt=8):
    return fused_eligible(c.shape[1], c.shape[2], elt)


Problem = namedtuple("Problem", "W b X y masks")


@functools.lru_cache(maxsize=None)
def problem(c, rounded=False):
    """S parameter sets, X, labels and S·T mask blocks of a case (read-only: shared between tests).
    rounded: every input rounded through float32 (what a float32 model sees)."""
    N, D, K, S, T = c.shape
    rs = np.random.RandomState(c.seed)
    W, b = rs.normal(0, 0.3, (S, D, K)), rs.normal(0, 0.3, (S, K))
    X = rs.rand(N, D)
    y = rs.randint(0, 2 if c.model == 'logistic' else K, N)
    masks = rs.binomial(1, 0.5, (S * T, N, D)).astype(np.uint8)
    if rounded:
        W, b, X = f32r(W), f32r(b), f32r(X)
    return Problem(W, b, X, y, masks)


def posterior(pb):
    """{'weights': [S, D, K], 'bias': [S, K]} as sample() returns it."""
    return {'weights': pb.W, 'bias': pb.b}


@functools.lru_cache(maxsize=None)
def case_ref(c, dropout=True, rounded=False):
    """The reference of a case: with its S·T mask blocks, or (dropout False) of the S sets without dropout."""
    pb = problem(c, rounded)
    if dropout:
        return predictive_ref(c.model, pb.W, pb.b, pb.X, pb.y, pb.masks, c.shape[4])
    return predictive_ref(c.model, pb.W, pb.b, pb.X, pb.y, None, 1)
