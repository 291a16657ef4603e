"""GPU: every instantiation of k_fwd<T, NBLK, VEC, NW> and k_grad<T, NBLK, NW> (csrc/hmcx_softmax.hip) in both
dtypes, through the C ABI (hmcx_softmax_grad / _loglik / _predict with W [D][C·K]; hmcx_logistic_* with
W [D][C]), against oracle/models.py in float64, chain by chain.  The cases, the instantiation each reaches,
the references and the tolerances are tests/_linear_cases.py; tests/test_linear_cases_cpu.py checks on the
CPU that the table covers all 12 forward and 6 gradient instantiations and that a dropped row, feature or
class column moves every output compared here by at least 8 tolerances.

Tolerances.  float64: gradient within 1e-12 of the |X|ᵀ|ŷ − y| + α|θ| scale, log-likelihood within
1e-12·max(1, |ll|)·√B, probabilities rtol 1e-11.  float32 (reference on the float32-rounded inputs):
gradient within 2e-5·(scale + 1); softmax log-likelihood and all probabilities within max(16·d, 1e-5·s),
d the largest |NumPy float32 − float64| of that output of the case, s = max(1, |ll|) resp. 1; logistic
log-likelihood within 2e-5·Σ_i (1 + Σ_d |x_id||w_d| + |b|) — the NumPy float32 yardstick is itself NaN
where the sigmoid saturates, which is what the two saturated cases are about: before the float32
instantiation took log ŷ and log(1 − ŷ) from the clipped logit, they returned NaN / −inf.

Measured on MI355X, float32, largest over the cases (err = |device − float64 reference|; every float32 case
prints its own err, d and err/d):
  softmax log-likelihood   err/d 5.7  at (1, 1, 2, 1): err 5.1e-8, d 8.9e-9 — one row, d is a single rounding;
                           0.19 at (20, 784, 10, 61), the largest d (6.6e-5); err/tolerance at most 0.012
  softmax probabilities    err/d 3.3  at (18, 1028, 64, 1): err 6.6e-7, d 2.0e-7; err/tolerance at most 0.066
  logistic probabilities   err/d 1.01 at (50, 8, 70): err 1.0e-7, d 9.9e-8; err/tolerance at most 0.054
  gradients                err/tolerance at most 0.029 (softmax), 0.072 (logistic, (25, 1028, 40))
  logistic log-likelihood  err/tolerance 0.87 at (25, 1028, 40), err 0.166 — and that is the float64 reference's
                           own error, not the device's: for a y = 0 row with z between 30 and the clip bound,
                           1 − ŷ is a few float64 ulps of 1 and log(1 − ŷ) is off by up to 0.4.  NumPy float64
                           with min(−z, 0) − log1p(exp(−|z|)) in its place differs from the reference by the
                           same 0.869 tolerances there (0.068 and 0 on the two saturated cases, where the
                           device measures 0.068 and 2e-5): the float32 kernel, which takes log(1 − ŷ) from the
                           logit, is the more accurate of the two.
No output needed more than 16·d; the 1e-5 floor governs everywhere except the one-row case.
float64: err/tolerance at most 0.022 (gradients), 0.0011 (log-likelihood), 0.0085 (probabilities).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _linear_cases as lc  # noqa: E402
from dropout_hamiltonian_montecarlo_amd import _native as nat  # noqa: E402

DTYPES = {"float64": (torch.float64, nat.HMCX_F64), "float32": (torch.float32, nat.HMCX_F32)}


def _device_outputs(model, X, Y, Ws, bs, dtype):
    """gW [C, D, K], gb [C, K], ll [C], prob [C, B, K] from the three C-ABI calls (K = 1 for the logistic
    model), as float64 host arrays.  The output buffers start as NaN: an element no kernel writes fails."""
    tdt, code = DTYPES[dtype]
    dev = torch.device("cuda:0")
    C, D, K = Ws.shape
    B = X.shape[0]
    # copies: the shared inputs are read-only
    Xd = torch.from_numpy(np.array(X, order="C")).to(dev, tdt)
    Yd = torch.from_numpy(np.array(Y, order="C")).to(dev, tdt)
    Wd = torch.from_numpy(np.array(Ws.transpose(1, 0, 2), order="C").reshape(D, C * K)).to(dev, tdt)
    bd = torch.from_numpy(np.array(bs, order="C").reshape(C * K)).to(dev, tdt)
    gW, gb = torch.full_like(Wd, float("nan")), torch.full_like(bd, float("nan"))
    ll = torch.full((C,), float("nan"), dtype=torch.float64, device=dev)
    prob = torch.full((B, C * K), float("nan"), dtype=tdt, device=dev)
    ctx = nat.context(0)
    p = nat.ptr
    if model == "softmax":
        ctx.check(ctx.lib.hmcx_softmax_grad(ctx.h, code, p(Xd), p(Yd), B, D, K, C, p(Wd), p(bd), lc.SOFTMAX_ALPHA,
                                            p(gW), p(gb)), "grad")
        ctx.check(ctx.lib.hmcx_softmax_loglik(ctx.h, code, p(Xd), p(Yd), B, D, K, C, p(Wd), p(bd), p(ll)), "loglik")
        ctx.check(ctx.lib.hmcx_softmax_predict(ctx.h, code, p(Xd), B, D, K, C, p(Wd), p(bd), p(prob)), "predict")
    else:
        ctx.check(ctx.lib.hmcx_logistic_grad(ctx.h, code, p(Xd), p(Yd), B, D, C, p(Wd), p(bd), lc.LOGISTIC_ALPHA,
                                             p(gW), p(gb)), "grad")
        ctx.check(ctx.lib.hmcx_logistic_loglik(ctx.h, code, p(Xd), p(Yd), B, D, C, p(Wd), p(bd), p(ll)), "loglik")
        ctx.check(ctx.lib.hmcx_logistic_predict(ctx.h, code, p(Xd), B, D, C, p(Wd), p(bd), p(prob)), "predict")
    h = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
    return {"gW": h(gW).reshape(D, C, K).transpose(1, 0, 2), "gb": h(gb).reshape(C, K), "ll": h(ll),
            "prob": h(prob).reshape(B, C, K).transpose(1, 0, 2)}


def _check(model, i, dtype):
    X, Y, Ws, bs = lc.softmax_problem(i, dtype) if model == "softmax" else lc.logistic_problem(i, dtype)
    ref = lc.reference(model, i, dtype)
    tol = lc.f32_tolerances(model, i) if dtype == "float32" else lc.f64_tolerances(model, i)
    d = lc.f32_distance(model, i) if dtype == "float32" else {}
    out = _device_outputs(model, X, Y, Ws, bs, dtype)
    name = "%s %s %s" % (model, lc.case_id((lc.SOFTMAX_CASES if model == "softmax" else lc.LOGISTIC_CASES)[i]), dtype)
    bad = []
    for o in ("gW", "gb", "ll", "prob"):
        assert out[o].shape == ref[o].shape
        err = np.abs(out[o] - ref[o])
        ratio = np.where(np.isfinite(err), err / tol[o], np.inf)
        line = "%s %s: max err %.3e, err/tol %.3g" % (name, o, float(np.max(err)), float(np.max(ratio)))
        if o in d:
            line += ", d %.3e, err/d %.3g" % (d[o], float(np.max(err)) / d[o] if d[o] > 0 else float("inf"))
        print(line)
        if not np.all(ratio <= 1.0):
            bad.append(line)
    assert not bad, bad


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("i", range(len(lc.SOFTMAX_CASES)), ids=lambda i: lc.case_id(lc.SOFTMAX_CASES[i]))
def test_softmax_link_vs_oracle(i, dtype):
    _check("softmax", i, dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("i", range(len(lc.LOGISTIC_CASES)), ids=lambda i: lc.case_id(lc.LOGISTIC_CASES[i]))
def test_sigmoid_link_vs_oracle(i, dtype):
    _check("logistic", i, dtype)
