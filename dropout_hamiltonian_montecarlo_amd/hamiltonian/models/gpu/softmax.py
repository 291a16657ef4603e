"""HIP-backed softmax regression — drop-in for the reference's softmax model.

Reference: /root/reference/hamiltonian/models/cpu/softmax.py:12-100 (NumPy, the parity
target) and models/gpu/softmax.py:12-121 (CuPy; the slot this class fills).
Every compute call goes through libhmcx (k_fwd / k_grad MFMA kernels); arrays may be
NumPy or torch, results are torch tensors on the model's HIP device.

Semantics follow the CPU file (the NumPy oracle): ``log_prior`` is the constant of
softmax.py:22-30.  ``prior='gpu'`` selects the CuPy file's −½α·Σθ²/dim (gpu/softmax.py:29-39).
"""
import ctypes

import numpy as np
import torch

from dropout_hamiltonian_montecarlo_amd._native import (HmcxError, LinearPredictiveArgs, MLP_MASKS_FIXED, MLP_MASKS_NONE,
                                                        MLP_MASKS_PHILOX, MODEL_LOGISTIC, MODEL_SOFTMAX, context,
                                                        dtype_code, ptr)


def as_device(a, dtype, device):
    if isinstance(a, torch.Tensor):
        t = a.to(device=device, dtype=dtype)
    else:
        t = torch.as_tensor(np.asarray(a), dtype=dtype).to(device)
    return t.contiguous()


def _batch(args):
    X = y = None
    for k, v in args.items():
        if k == 'X_train':
            X = v
        elif k == 'y_train':
            y = v
    return X, y



def _log0(x):
    """np.log without the divide-by-zero RuntimeWarning at α = 0 (−inf, as the reference computes it:
    its model files silence warnings, models/cpu/softmax.py:1-2)."""
    with np.errstate(divide="ignore"):
        return np.log(x)

def input_masks(device, N, D, p, seed, step, chain=0):
    """One Philox input-dropout mask [N, D] (uint8 on the device, hmcx_input_masks): what draw ``step`` of
    posterior_predictive(n_dropout=T, p=p, seed=seed) uses, and sgd.fit_dropout's mask for that (seed, step)."""
    ctx = context(device)
    out = torch.empty((N, D), dtype=torch.uint8, device=ctx.device)
    ctx.check(ctx.lib.hmcx_input_masks(ctx.h, N, D, float(p), int(seed), int(chain), int(step), ptr(out)),
              "hmcx_input_masks")
    return out


def linear_posterior_predictive(model, posterior, X, y=None, n_dropout=0, p=0.5, Z=None, seed=0, path=0):
    """posterior_predictive of the softmax and logistic models (one hmcx_linear_predictive call)."""
    from .mlp import Predictive
    logistic = model._hmcx_model == 'logistic'
    Xd = model._dev(X)
    if Xd.dim() != 2:
        raise HmcxError("posterior_predictive: X must be [N, D]")
    N, D = Xd.shape
    W, b = posterior['weights'], posterior['bias']
    W = W if isinstance(W, torch.Tensor) else np.asarray(W)
    b = b if isinstance(b, torch.Tensor) else np.asarray(b)
    if W.ndim < 2 or W.shape[-2] != D:
        raise HmcxError("posterior_predictive: weights must be [..., %d, K]" % D)
    K = int(W.shape[-1])
    if logistic and K != 1:
        raise HmcxError("logistic: weights must be [..., D, 1]")
    W = model._dev(W).reshape(-1, D, K).contiguous()           # leading dimensions flatten row-major
    S = W.shape[0]
    b = model._dev(b).reshape(-1)
    if b.numel() != S * K:
        raise HmcxError("posterior_predictive: bias must be [..., %d] with the leading dimensions of weights" % K)
    b = b.reshape(S, K).contiguous()
    T = int(n_dropout)
    if T < 0:
        raise ValueError("n_dropout must be >= 0")
    a = LinearPredictiveArgs()
    a.dtype, a.model = model.code, MODEL_LOGISTIC if logistic else MODEL_SOFTMAX
    a.N, a.D, a.K, a.S, a.T, a.path = N, D, K, S, max(T, 1), int(path)
    a.X, a.W, a.b = Xd.data_ptr(), W.data_ptr(), b.data_ptr()
    Zd = None
    if T == 0:
        if Z is not None:
            raise ValueError("n_dropout=0 means no input dropout: Z must be None")
        a.mask_mode = MLP_MASKS_NONE
    elif Z is None:
        a.mask_mode, a.keep_p, a.seed, a.chain, a.step0 = MLP_MASKS_PHILOX, float(p), int(seed), 0, 0
    else:
        Zd = Z if isinstance(Z, torch.Tensor) else torch.as_tensor(np.asarray(Z))
        if tuple(Zd.shape) != (S * T, N, D):
            raise HmcxError("posterior_predictive: Z must be [%d, %d, %d]" % (S * T, N, D))
        Zd = (Zd.to(model.device) != 0).to(torch.uint8).contiguous()
        a.mask_mode, a.masks = MLP_MASKS_FIXED, Zd.data_ptr()
    DR = S * max(T, 1)
    yt = None
    if y is not None:
        yt = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))
        if yt.dim() == 2 and logistic and yt.shape[1] == 1:
            yt = yt.reshape(-1)
        elif yt.dim() == 2 and not logistic and yt.shape[1] == K:
            yt = yt.argmax(dim=1)                               # one-hot
        if yt.dim() != 1 or yt.shape[0] != N:
            raise HmcxError("posterior_predictive: y must be integer labels [N] (or one-hot [N, K])")
        yt = yt.to(model.device, torch.int32).contiguous()
        a.y = yt.data_ptr()
    f64 = dict(dtype=torch.float64, device=model.device)
    i32 = dict(dtype=torch.int32, device=model.device)
    mean, pred = torch.empty((N, K), **f64), torch.empty(N, **i32)
    ent, eent = torch.empty(N, **f64), torch.empty(N, **f64)
    a.out_mean, a.out_pred = mean.data_ptr(), pred.data_ptr()
    a.out_entropy, a.out_exp_entropy = ent.data_ptr(), eent.data_ptr()
    lppd = nll = corr = None
    if yt is not None:
        lppd, nll, corr = torch.empty(N, **f64), torch.empty(DR, **f64), torch.empty(DR, **i32)
        a.out_lppd, a.out_draw_nll, a.out_draw_correct = lppd.data_ptr(), nll.data_ptr(), corr.data_ptr()
    ctx = context(model.device)
    ctx.check(ctx.lib.hmcx_linear_predictive(ctx.h, ctypes.byref(a)), "hmcx_linear_predictive")
    host = [None if t is None else t.cpu().numpy() for t in (mean, pred, ent, eent, lppd, nll, corr)]
    del W, b, Zd, yt, Xd                                  # read by the launches the copies above waited for
    mean, pred, ent, eent, lppd, nll, corr = host
    return Predictive(mean, pred, ent, eent, ent - eent, lppd, nll, None if corr is None else corr / float(N))


_PP_DOC = """Model averaging on the device in one libhmcx call (hmcx_linear_predictive): over the S parameter
        sets of ``posterior`` ({'weights': [..., D, K], 'bias': [..., K]}: what ``sample`` returns, a
        [chains, epochs, …] trace, or a single set; leading dimensions flatten row-major) and, with
        ``n_dropout = T >= 1``, T Bernoulli(p) input-dropout masks per set (the reference's predict_stochastic,
        X ⊙ Z), S·T draws in all (draw d = s·T + t); n_dropout = 0 is no input dropout.  The masks are Philox
        draws of ``seed`` (draw d is input_masks(device, N, D, p, seed, d)) unless ``Z`` [S·T, N, D] injects them.
        Returns mlp's ``Predictive`` of host arrays: mean [N, K] (logistic: [N, 1], the mean of P(y = 1)),
        pred [N], entropy [N] of the mean, expected_entropy [N], mutual_information [N] and, with labels ``y``
        ([N] class indices, or one-hot [N, K]), lppd [N], draw_nll [S·T] (−log-likelihood / N of each draw) and
        draw_accuracy [S·T]; those three are None without y.  path: 0 by shape, 1 general, 2 fused
        (include/hmcx.h)."""


class softmax:
    _hmcx_model = 'softmax'

    def __init__(self, _hyper, dtype=torch.float64, device=None, prior='cpu'):
        self.hyper = _hyper
        self.alpha = float(np.asarray(_hyper['alpha']))
        self.dtype = dtype
        self.code = dtype_code(dtype)
        self.ctx = context(device)
        self.device = self.ctx.device
        if prior not in ('cpu', 'gpu'):
            raise ValueError("prior must be 'cpu' or 'gpu'")
        self.prior = prior

    # -------------------------------------------------------------- helpers
    def _dev(self, a):
        return as_device(a, self.dtype, self.device)

    def _par(self, par):
        W = self._dev(par['weights'])
        b = self._dev(par['bias'])
        if W.dim() != 2 or b.dim() != 1 or W.shape[1] != b.shape[0]:
            raise HmcxError("softmax: weights must be [D,K] and bias [K]")
        return W, b

    def _xy(self, args):
        X, y = _batch(args)
        X = self._dev(X)
        Y = self._dev(y)
        if X.dim() != 2 or Y.dim() != 2 or X.shape[0] != Y.shape[0]:
            raise HmcxError("softmax: X_train [B,D] and one-hot y_train [B,K] expected")
        return X, Y

    # -------------------------------------------------------------- model surface
    def grad(self, par, **args):                                          # softmax.py:45-61
        X, Y = self._xy(args)
        W, b = self._par(par)
        B, D = X.shape
        K = W.shape[1]
        if W.shape[0] != D or Y.shape[1] != K:
            raise HmcxError("softmax.grad: shape mismatch")
        gW = torch.empty_like(W)
        gb = torch.empty_like(b)
        ctx = context(self.device)
        ctx.check(ctx.lib.hmcx_softmax_grad(ctx.h, self.code, ptr(X), ptr(Y), B, D, K, 1, ptr(W), ptr(b),
                                            self.alpha, ptr(gW), ptr(gb)), "hmcx_softmax_grad")
        return {'weights': gW, 'bias': gb}

    def log_likelihood_device(self, par, **args):
        X, Y = self._xy(args)
        W, b = self._par(par)
        B, D = X.shape
        K = W.shape[1]
        ll = torch.empty(1, dtype=torch.float64, device=self.device)
        ctx = context(self.device)
        ctx.check(ctx.lib.hmcx_softmax_loglik(ctx.h, self.code, ptr(X), ptr(Y), B, D, K, 1, ptr(W), ptr(b),
                                              ptr(ll)), "hmcx_softmax_loglik")
        return ll

    def log_likelihood(self, par, **args):                                # softmax.py:63-72
        return np.float64(self.log_likelihood_device(par, **args).item())

    def log_prior(self, par, **args):                                     # softmax.py:22-30
        K = 0
        if self.prior == 'cpu':
            for var in par.keys():
                dim = int(np.prod(tuple(par[var].shape)))
                K -= 0.5 * dim * np.log(2 * np.pi) - 0.5 * dim * _log0(self.hyper['alpha'])
            return K
        ctx = context(self.device)
        for var in par.keys():                                            # gpu/softmax.py:29-39
            v = self._dev(par[var]).reshape(-1)
            ss = torch.empty(1, dtype=torch.float64, device=self.device)   # Σθ² on the device (hmcx_sumsq)
            ctx.check(ctx.lib.hmcx_sumsq(ctx.h, self.code, ptr(v), v.numel(), ptr(ss)), "hmcx_sumsq")
            K -= 0.5 * self.alpha * ss.item() / v.numel()
        return K

    def log_prior_const(self, shapes):
        """Constant CPU-semantics log prior for parameter shapes (used by the fused samplers)."""
        if self.prior != 'cpu':
            raise HmcxError("fused samplers implement the CPU (constant) log prior only")
        K = 0
        for shp in shapes:
            dim = int(np.prod(shp))
            K -= 0.5 * dim * np.log(2 * np.pi) - 0.5 * dim * _log0(self.hyper['alpha'])
        return K

    def negative_log_posterior(self, par, **args):                        # softmax.py:74-79
        n_data = args['X_train'].shape[0]
        return (-1.0 / n_data) * (self.log_likelihood(par, **args) + self.log_prior(par, **args))

    def loss(self, par, **args):
        """North-star surface name: the sampler energy U = negative_log_posterior."""
        return self.negative_log_posterior(par, **args)

    def net(self, par, X):                                                # softmax.py:38-43
        return self._net_device(par, X)

    def _net_device(self, par, X):
        X = self._dev(X)
        W, b = self._par(par)
        B, D = X.shape
        K = W.shape[1]
        prob = torch.empty((B, K), dtype=self.dtype, device=self.device)
        ctx = context(self.device)
        ctx.check(ctx.lib.hmcx_softmax_predict(ctx.h, self.code, ptr(X), B, D, K, 1, ptr(W), ptr(b), ptr(prob)),
                  "hmcx_softmax_predict")
        return prob

    def predict(self, par, X, prob=False, batchsize=None):                # softmax.py:82-89
        """CPU semantics (cpu/softmax.py:82-89) by default; with ``batchsize`` the GPU file's
        batching (gpu/softmax.py:90-102): whole batches only, and prob=True returns the
        probabilities flattened to 1-D (its ``results.reshape(-1,)``)."""
        if batchsize:
            n = (X.shape[0] // batchsize) * batchsize
            yhat = self._net_device(par, X[:n])
            out = yhat if prob else yhat.argmax(dim=1)
            return out.cpu().numpy().reshape(-1)
        yhat = self._net_device(par, X)
        out = yhat if prob else yhat.argmax(dim=1)
        return out.cpu().numpy()

    def predict_stochastic(self, par, X, prob=False, p=0.5, Z=None, batchsize=None):   # softmax.py:91-100
        """Input dropout X ⊙ Z, Z ~ Bernoulli(p) (``Z`` may be given).  With ``batchsize`` the GPU
        file's batching (gpu/softmax.py:105-121): whole batches, output reshaped to
        (-1, last dimension) as there."""
        X = self._dev(X)
        if batchsize:
            n = (X.shape[0] // batchsize) * batchsize
            X = X[:n]
            Z = Z[:n] if Z is not None else None
        if Z is None:
            Z = torch.bernoulli(torch.full_like(X, p))
        else:
            Z = self._dev(Z)
        yhat = self._net_device(par, X * Z)
        out = (yhat if prob else yhat.argmax(dim=1)).cpu().numpy()
        if batchsize:
            out = out.reshape(-1, out.shape[-1]) if prob else out.reshape(-1, batchsize)
        return out

    def predict_posterior(self, posterior, X, prob=False):
        """Posterior predictive over S samples (extension): mean over s of softmax(X·W_s + b_s), all
        S parameter sets in ONE launch (the chain-interleaved layout W[D][S][K] of hmcx_softmax_predict).
        ``posterior``: {'weights': [S, D, K], 'bias': [S, K]} as returned by ``sample``."""
        Ws = np.asarray(posterior['weights'])
        bs = np.asarray(posterior['bias'])
        S, D, K = Ws.shape
        Xd = self._dev(X)
        B = Xd.shape[0]
        W = self._dev(np.ascontiguousarray(Ws.transpose(1, 0, 2)).reshape(D, S * K))
        b = self._dev(bs.reshape(S * K))
        prob_all = torch.empty((B, S * K), dtype=self.dtype, device=self.device)
        ctx = context(self.device)
        ctx.check(ctx.lib.hmcx_softmax_predict(ctx.h, self.code, ptr(Xd), B, D, K, S, ptr(W), ptr(b),
                                               ptr(prob_all)), "hmcx_softmax_predict")
        mean = prob_all.cpu().numpy().reshape(B, S, K).mean(axis=1)
        return mean if prob else mean.argmax(axis=1)

    def posterior_predictive(self, posterior, X, y=None, n_dropout=0, p=0.5, Z=None, seed=0, path=0):
        return linear_posterior_predictive(self, posterior, X, y, n_dropout, p, Z, seed, path)

    posterior_predictive.__doc__ = _PP_DOC
