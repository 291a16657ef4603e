"""GPU: the k_mm launches of the dropout MLP (csrc/hmcx_mlp.hip) at every launch branch a one-off call can
take, in both dtypes, through the C ABI — hmcx_mlp_grad (six gradients and the loss) and hmcx_mlp_loss (loss
and logits) — against oracle/models.py::mlp in float64.  The cases, the launch signature each reaches, the
references, the error bounds and the tolerances are tests/_mlp_cases.py; tests/test_mlp_cases_cpu.py checks
on the CPU that the table covers the branch inventory and that each of eight kernel defects (a lost row,
feature, hidden unit or class, swapped masks, a misplaced gradient tile, zeroed logit rows) moves a compared
output by at least 8 tolerances.

Tolerances.  float64: gradients within 1e-9 of the largest entry, the loss within 1e-11 relative, logits
within the float64 forward-error bound.  float32 (reference on the float32-rounded inputs): per element within
4 x r x bound, bound = the absolute-value run x summed contraction length x 2^-24 and r the worst err / bound
of the case measured on an MI355X (_mlp_cases.F32_RATIO, the table below; 4 x: summation order differs
between machines), and never looser than 2e-4 of the output's largest entry.

Measured on MI355X, float32, worst err / bound per case over the eight outputs (every case prints its own per
output).  In every case the worst output is the b3 gradient — a column sum of the cross-entropy gradient, whose
error is the few ulps of exp and log, not a contraction's — and the largest error of any output is 3.3e-7 of
its largest entry, 600 times inside the 2e-4 the float32 gradients were compared at before:

    case                   worst r     |err| there   largest err / largest entry over the outputs
    100-100-128-5          2.638e-3    1.77e-8       1.6e-7
    8-520-256-3            6.00e-4     2.63e-8       2.2e-7
    40-24-256-32           4.828e-3    8.20e-9       2.5e-7
    33-20-1024-4           3.59e-4     2.41e-8       2.0e-7
    12-16-600-33           2.476e-3    1.09e-8       3.3e-7
    130-260-128-33         3.186e-3    1.14e-8       2.0e-7
    300-400-100-9          1.455e-3    2.01e-8       1.8e-7
    36-776-64-10           1.453e-3    2.34e-8       2.1e-7
    21-30-38-3             6.458e-3    2.99e-8       3.3e-7
    19-50-37-7             8.623e-3    4.04e-8       2.4e-7
    1-3-1-2                1.106e-1    4.14e-8       1.7e-7
    70-33-64-40            1.871e-2    1.11e-8       3.0e-7
    40-64-768-6            3.30e-4     1.67e-8       2.1e-7
    33-24-64-12-off1       1.102e-2    1.99e-8       1.8e-7
    100-100-128-5-nomask   2.191e-3    3.42e-8       1.7e-7
    19-50-37-7-nomask      1.119e-2    1.99e-8       2.0e-7

With r set by the b3 gradient, 4 x r x bound passes the 2e-4 cap for the loss or the logits of four cases
(8-520-256-3, 33-20-1024-4, 12-16-600-33, 40-64-768-6: by up to 2.5 times), where the cap governs; everywhere
else the bound does, down to 0.02 of the cap.  float64: every output within 1.7e-15 of its largest entry and
within 0.028 of its own float64 bound.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _mlp_cases as mc  # noqa: E402
from oracle import models as om  # noqa: E402
from dropout_hamiltonian_montecarlo_amd import _native as nat  # noqa: E402

DTYPES = {"float64": (torch.float64, nat.HMCX_F64), "float32": (torch.float32, nat.HMCX_F32)}


def _device_outputs(i, dtype):
    """The outputs of the two C-ABI calls as float64 host arrays ('loss' from hmcx_mlp_grad, 'loss2' from
    hmcx_mlp_loss).  The output buffers start as NaN: an element no kernel writes fails."""
    c = mc.CASES[i]
    p = mc.problem(i, dtype)
    tdt, code = DTYPES[dtype]
    dev = torch.device("cuda:0")
    B, n_in, n_mid, n_out = c["B"], c["n_in"], c["n_mid"], c["n_out"]
    up = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev, tdt)  # noqa: E731  (copies: inputs are read-only)
    X = up(p["X"])
    y = torch.from_numpy(np.array(p["y"])).to(dev, torch.int32)
    par = [up(p[k]) for k in om.MLP_PARAM_NAMES]
    grads = [torch.full_like(t, float("nan")) for t in par]
    mp, gp = nat.MlpParams(), nat.MlpParams()
    for j in range(6):
        mp.p[j], gp.p[j] = par[j].data_ptr(), grads[j].data_ptr()
    masks = None
    if p["masks"] is not None:
        n3 = 3 * B * n_mid
        off = 0 if c["aligned"] else 1                      # one element past a 16-byte boundary
        buf = torch.zeros(n3 + 4, dtype=tdt, device=dev)
        masks = buf[off:off + n3]
        masks.copy_(up(p["masks"]).reshape(-1))
        assert (masks.data_ptr() % 16 == 0) == c["aligned"]
    loss = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    logits = torch.full((B, n_out), float("nan"), dtype=tdt, device=dev)
    ctx = nat.context(0)
    ptr = nat.ptr
    ctx.check(ctx.lib.hmcx_mlp_grad(ctx.h, code, ptr(X), ptr(y), B, n_in, n_mid, n_out, ctypes.byref(mp), ptr(masks),
                                    mc.ALPHA, ctypes.byref(gp), ptr(loss[0:1])), "hmcx_mlp_grad")
    ctx.check(ctx.lib.hmcx_mlp_loss(ctx.h, code, ptr(X), ptr(y), B, n_in, n_mid, n_out, ctypes.byref(mp), ptr(masks),
                                    ptr(loss[1:2]), ptr(logits)), "hmcx_mlp_loss")
    h = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
    out = {o: h(g) for o, g in zip(("gW1", "gb1", "gW2", "gb2", "gW3", "gb3"), grads)}
    lo = h(loss)
    out.update(loss=lo[0], loss2=lo[1], logits=h(logits))
    return out


def _cases():
    return [pytest.param(i, d, id="%s-%s" % (mc.case_id(c), d)) for i, c in enumerate(mc.CASES) for d in c["dtypes"]]


@pytest.mark.parametrize("i,dtype", _cases())
def test_mlp_grad_and_loss_vs_oracle(i, dtype):
    ref, tol, bound = mc.reference(i, dtype), mc.tolerances(i, dtype), mc.bounds(i, dtype)
    out = _device_outputs(i, dtype)
    name = "mlp %s %s" % (mc.case_id(mc.CASES[i]), dtype)
    bad, worst = [], 0.0
    for o in mc.OUTPUTS + ("loss2",):
        k = "loss" if o == "loss2" else o
        r = np.asarray(ref[k])
        assert np.shape(out[o]) == r.shape
        err = np.abs(out[o] - r)
        ratio = np.where(np.isfinite(err), err / tol[k], np.inf)
        eb = float(np.max(np.where(np.isfinite(err), err / bound[k], np.inf)))
        worst = max(worst, eb)
        line = "%s %s: max err %.3e, err/tol %.3g, err/bound %.3g, err/largest %.3g" % (
            name, o, float(np.max(err)), float(np.max(ratio)), eb, float(np.max(err)) / max(float(np.max(np.abs(r))), 1e-300))
        print(line)
        if not np.all(ratio <= 1.0):
            bad.append(line)
    print("%s WORST err/bound %.4g" % (name, worst))
    assert not bad, bad
