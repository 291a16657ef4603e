"""Scripted-schedule SGHMC reference (test infrastructure): one step of oracle/samplers.py::sghmc
(step + accept) on oracle/models.py::softmax, with every draw passed in instead of taken from a
random stream, so a test can script path lengths, noise and accept uniforms per chain.

The draws are laid out as the device reads them in buffer-noise mode (include/hmcx.h noise_off):
z[slot·P + e] with P = D·K + K, slot 0 the momentum, slot it + 1 the noise of leapfrog iteration it
(standard normals; the step scales them by 2·eps), e = d·K + k for the weights and D·K + k for the
bias.  That is also the order in which the oracle draws them from its RandomState (weights, then bias,
per iteration), so fed the oracle's own draws the step is the oracle's, bit for bit
(tests/test_sghmc_ref_cpu.py).

``dtype=np.float32`` runs the same operations in float32 (states, momenta, noise, X and Y cast once):
the distance between that run and the float64 one is the yardstick of the float32 device tests.
"""
import numpy as np

from oracle import models as om


class _softmax(om.softmax):
    """oracle softmax whose clip bounds take the dtype of the logits (a no-op in float64; keeps a
    float32 run in float32)."""

    def logits(self, par, X):
        y_linear = np.dot(X, par['weights']) + par['bias']
        y_linear = np.minimum(y_linear, y_linear.dtype.type(om.CLIP_HI))
        y_linear = np.maximum(y_linear, y_linear.dtype.type(om.CLIP_LO))
        return y_linear


def _kinetic(p):                                      # oracle sghmc.potential_energy (hmc.py:74-79)
    K = 0
    for var in p.keys():
        K += 0.5 * (np.sum(np.square(p[var])))
    return K


def sghmc_step(q, X_batch, Y_batch, eps, alpha, n_iter, z, u, dtype=np.float64):
    """One SGHMC step from state q = {'weights': [D, K], 'bias': [K]} with explicit draws.

    n_iter leapfrog iterations (the oracle's ``len(np.arange(path_length - 1))``), z the 1-D array
    of (1 + n_iter)·P standard normals described in the module docstring, u the accept uniform.
    Returns (state, A, (E_current, E_new), accepted, ll): the state the step keeps, the acceptance
    probability, both energies of the accept test, the flag, and the log-likelihood of the kept state
    on this minibatch (what the sampler reports per step).

    n_iter == 0 follows the device's convention (k_fix_acc): the chain does not move, the step is
    reported as accepted with A = 1 and E_new = E_current — which is also what the oracle computes
    (q_new is q, p_new is p, A = min(1, exp(0)), u < 1).
    """
    model = _softmax({'alpha': alpha})
    args = {'X_train': np.asarray(X_batch, dtype=dtype), 'y_train': np.asarray(Y_batch, dtype=dtype)}
    q = {var: np.array(q[var], dtype=dtype) for var in ('weights', 'bias')}
    D, K = q['weights'].shape
    P = D * K + K
    n_iter = int(n_iter)
    z = np.asarray(z)
    assert z.shape == ((1 + n_iter) * P,), (z.shape, n_iter, P)
    zt = z.astype(dtype)

    def draws(slot):
        s = zt[slot * P:(slot + 1) * P]
        return {'weights': s[:D * K].reshape(D, K), 'bias': s[D * K:]}

    p = {var: np.array(v) for var, v in draws(0).items()}
    E_current = float(model.negative_log_posterior(q, **args) + _kinetic(p))
    if n_iter == 0:
        return q, 1.0, (E_current, E_current), bool(u < 1.0), float(model.log_likelihood(q, **args))
    q_new = {var: q[var].copy() for var in q}
    p_new = {var: p[var].copy() for var in p}
    scale = 2 * eps
    for it in range(n_iter):
        noise = draws(it + 1)
        for var in ('weights', 'bias'):                                   # sghmc.py:29-34
            rvar = dtype(scale) * noise[var]
            q_new[var] += eps * p_new[var]
            grad_q = model.grad(q_new, **args)
            p_new[var] = (1 - eps) * p_new[var] + eps * grad_q[var] + rvar
    E_new = float(model.negative_log_posterior(q_new, **args) + _kinetic(p_new))
    A = min(1, np.exp(E_current - E_new))                                 # hmc.py:67-71 (NaN -> 1)
    accepted = bool(np.isfinite(A) and (u < A))
    kept = q_new if accepted else q
    return kept, float(A), (E_current, E_new), accepted, float(model.log_likelihood(kept, **args))


def flip_features(q, X_batch, z):
    """The same problem with the feature axis of X and W reversed (z permuted to match): identical
    mathematics, another summation order in every product over features.  Returns (q, X_batch, z)."""
    D, K = q['weights'].shape
    P = D * K + K
    zz = np.asarray(z).reshape(-1, P).copy()
    zz[:, :D * K] = zz[:, :D * K].reshape(-1, D, K)[:, ::-1, :].reshape(-1, D * K)
    qf = {'weights': np.ascontiguousarray(q['weights'][::-1]), 'bias': q['bias'].copy()}
    return qf, np.ascontiguousarray(np.asarray(X_batch)[:, ::-1]), zz.reshape(-1)
