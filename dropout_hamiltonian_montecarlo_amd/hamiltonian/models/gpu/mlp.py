"""HIP-backed dropout MLP — drop-in for the reference's Chainer MLP (config 3).

Reference: /root/reference/hamiltonian/models/gpu/mlp.py:19-96.  ``MyNetwork`` (:19-31) is
l1 (n_in→n_mid) → dropout(.1) → relu → l2 (n_mid→n_mid) → dropout → relu → dropout → l3
(n_mid→n_out); ``grad`` (:47-64) returns ∇ mean softmax-CE + ½α·θ per parameter,
``log_likelihood`` (:66-78) returns the mean CE *loss*, ``log_prior`` (:40-45) is
−Σ_var ½α·Σθ²/dim and ``negative_log_posterior`` (:80-82) is loss + log_prior.

Parameters use Chainer's ``namedparams`` names and [out, in] weight layout ('/l1/W' [n_mid, n_in],
'/l1/b', '/l2/W', '/l2/b', '/l3/W' [n_out, n_mid], '/l3/b').  Labels are integers (mlp.py:52).
Every compute call goes through libhmcx (k_mm MFMA GEMMs with fused bias/dropout/relu/gradient
epilogues, hmcx_mlp.hip).

Dropout.  Chainer draws fresh masks on every forward (train mode).  Here ``masks=None`` draws them
on the device from Philox (hmcx_mlp_masks, keyed by the model's seed and a call counter);
``masks='off'`` disables dropout; an explicit ``masks=[m1, m2, m3]`` (each [B, n_mid]) injects
them — the parity mode against oracle/models.py::mlp.

The dropout ratio is the model's: ``mlp(..., dropout=r)`` (default 0.1, the reference's ``F.dropout(ratio=.1)``)
drops an element with probability r and gives a kept one the value 1/(1 − r) in every Philox mask drawn for this
model — grad, the samplers' device calls, predict, predict_stochastic and posterior_predictive alike.  Injected
masks (``masks=[...]``, ``mask_provider``) are used as given: with a ratio other than the default they should carry
1/(1 − dropout) where they keep.  The contexts of a device are shared by its models, so every call first makes the
context's ratio the calling model's (``mlp_context``).
"""
import collections
import ctypes

import numpy as np
import torch

from dropout_hamiltonian_montecarlo_amd._native import (HmcxError, MlpLeapfrogArgs, MlpParams, MlpPredictiveArgs,
                                                        MLP_MASK_SLOT0, MLP_MASKS_FIXED, MLP_MASKS_NONE,
                                                        MLP_MASKS_PHILOX, MLP_DROPOUT_DEFAULT, context, dtype_code,
                                                        mlp_dropout_threshold, ptr)

from .softmax import _batch, as_device

MLP_PARAM_NAMES = ('/l1/W', '/l1/b', '/l2/W', '/l2/b', '/l3/W', '/l3/b')

# posterior_predictive's result (host NumPy arrays; the last three are None without labels)
Predictive = collections.namedtuple('Predictive', ('mean', 'pred', 'entropy', 'expected_entropy', 'mutual_information',
                                                   'lppd', 'draw_nll', 'draw_accuracy'))


def mlp_param_shapes(n_in, n_mid, n_out):
    return {'/l1/W': (n_mid, n_in), '/l1/b': (n_mid,), '/l2/W': (n_mid, n_mid), '/l2/b': (n_mid,),
            '/l3/W': (n_out, n_mid), '/l3/b': (n_out,)}


def init_params(shape, seed=0):
    """Chainer L.Linear defaults for MyNetwork(n_in, n_mid, n_out): W ~ LeCunNormal (N(0, 1/fan_in)),
    b = 0 (host numpy, float64).  Needs no device."""
    shapes = mlp_param_shapes(*shape)
    rs = np.random.RandomState(seed)
    out = {}
    for k in MLP_PARAM_NAMES:
        shp = shapes[k]
        out[k] = rs.normal(0, 1.0 / np.sqrt(shp[1]), shp) if len(shp) == 2 else np.zeros(shp)
    return out


def mlp_context(model):
    """The context of the model's device with the model's dropout ratio set: what every call that reaches an
    hmcx_mlp_* entry on behalf of ``model`` uses (here and, through inference/gpu/_mlp_call.py, in the samplers).
    A model without the attribute (a stand-in) runs at the default."""
    ctx = context(model.device)
    ctx.set_mlp_dropout(getattr(model, 'dropout', MLP_DROPOUT_DEFAULT))
    return ctx


class mlp:
    _hmcx_model = 'mlp'

    def __init__(self, _hyper, n_in, n_mid_units, n_out, dtype=torch.float32, device=None, seed=0,
                 dropout=MLP_DROPOUT_DEFAULT):
        mlp_dropout_threshold(dropout)                 # ValueError for an invalid ratio, before any device is touched
        self.dropout = float(dropout)
        self.hyper = _hyper
        self.alpha = float(np.asarray(_hyper['alpha']))
        self.n_in, self.n_mid, self.n_out = int(n_in), int(n_mid_units), int(n_out)
        self.dtype = dtype
        self.code = dtype_code(dtype)
        self.ctx = context(device)
        self.device = self.ctx.device
        self.seed = int(seed)
        self._mask_calls = 0
        self.shapes = mlp_param_shapes(self.n_in, self.n_mid, self.n_out)

    # -------------------------------------------------------------- helpers
    def init_params(self, seed=0):
        """Chainer L.Linear defaults: W ~ LeCunNormal (N(0, 1/fan_in)), b = 0 (host numpy, float64)."""
        return init_params((self.n_in, self.n_mid, self.n_out), seed)

    def _dev(self, a):
        return as_device(a, self.dtype, self.device)

    def _params(self, par):
        ts = []
        for k in MLP_PARAM_NAMES:
            if k not in par:
                raise HmcxError("mlp: missing parameter %r (expected %s)" % (k, MLP_PARAM_NAMES))
            t = self._dev(par[k])
            if tuple(t.shape) != self.shapes[k]:
                raise HmcxError("mlp: %s has shape %s, expected %s" % (k, tuple(t.shape), self.shapes[k]))
            ts.append(t)
        mp = MlpParams()
        for i, t in enumerate(ts):
            mp.p[i] = t.data_ptr()
        return ts, mp

    def _xy(self, args, need_y=True):
        X, y = _batch(args)
        X = self._dev(X)
        if X.dim() != 2 or X.shape[1] != self.n_in:
            raise HmcxError("mlp: X_train must be [B, %d]" % self.n_in)
        if not need_y:
            return X, None
        yt = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))
        yt = yt.to(self.device, torch.int32).contiguous()
        if yt.dim() != 1 or yt.shape[0] != X.shape[0]:
            raise HmcxError("mlp: y_train must be integer labels [B] (mlp.py:52)")
        return X, yt

    def draw_masks(self, B):
        """Fresh Philox dropout masks [3, B, n_mid] on the device (one forward's worth)."""
        out = torch.empty((3, B, self.n_mid), dtype=self.dtype, device=self.device)
        slot = (MLP_MASK_SLOT0 + self._mask_calls) & 0xFFFFFFFF
        self._mask_calls += 1
        ctx = mlp_context(self)
        ctx.check(ctx.lib.hmcx_mlp_masks(ctx.h, self.code, B, self.n_mid, self.seed, 0, 0xFFFFFFFF, slot, ptr(out)),
                  "hmcx_mlp_masks")
        return out

    def _masks(self, masks, B):
        if masks is None:
            return self.draw_masks(B)
        if isinstance(masks, str):
            if masks != 'off':
                raise ValueError("masks must be None, 'off' or [m1, m2, m3]")
            return None
        m = torch.stack([self._dev(x) for x in masks]) if isinstance(masks, (list, tuple)) else self._dev(masks)
        if tuple(m.shape) != (3, B, self.n_mid):
            raise HmcxError("mlp: masks must be 3 x [B, n_mid]")
        return m.contiguous()

    # -------------------------------------------------------------- model surface
    def grad(self, par, masks=None, **args):                              # mlp.py:47-64
        X, y = self._xy(args)
        B = X.shape[0]
        ts, mp = self._params(par)
        m = self._masks(masks, B)
        gs = [torch.empty_like(t) for t in ts]
        gp = MlpParams()
        for i, g in enumerate(gs):
            gp.p[i] = g.data_ptr()
        ctx = mlp_context(self)
        ctx.check(ctx.lib.hmcx_mlp_grad(ctx.h, self.code, ptr(X), ptr(y), B, self.n_in, self.n_mid, self.n_out, mp,
                                        ptr(m), self.alpha, gp, None), "hmcx_mlp_grad")
        return {k: g for k, g in zip(MLP_PARAM_NAMES, gs)}

    def leapfrog_device_ok(self):
        """hmc.step may hand the whole trajectory to leapfrog_device only when grad is this class's own
        (a subclass that overrides grad, e.g. to inject masks per call, keeps the host loop)."""
        return type(self).grad is mlp.grad

    def leapfrog_device(self, q, p, n_iter, eps, keys, masks=None, **args):
        """hmc.py:46-56 for the MLP in one libhmcx call (hmcx_mlp_hmc_leapfrog): q and p (dicts of device
        tensors of the model's dtype, keyed in the sampler's start order `keys`) are advanced in place
        and p is negated at the end.  The 1 + 6·n_iter gradient calls take their masks as grad() would:
        masks=None draws fresh Philox masks per call (the same slots as that many grad() calls),
        'off' disables dropout, explicit masks are used by every call.  Returns the gradient at the
        final position."""
        X, y = self._xy(args)
        B = X.shape[0]
        order = [MLP_PARAM_NAMES.index(k) for k in keys]
        if sorted(order) != list(range(6)):
            raise HmcxError("mlp: leapfrog keys must be the six parameters, got %s" % (list(keys),))
        a = MlpLeapfrogArgs()
        a.dtype, a.B, a.n_in, a.n_mid, a.n_out, a.n_iter = self.code, B, self.n_in, self.n_mid, self.n_out, int(n_iter)
        for i, v in enumerate(order):
            a.order[i] = v
        a.eps, a.alpha = float(eps), self.alpha
        a.X, a.y = X.data_ptr(), y.data_ptr()
        gs = {}
        for k in MLP_PARAM_NAMES:
            for t in (q[k], p[k]):
                if not (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == self.dtype
                        and t.is_contiguous() and tuple(t.shape) == self.shapes[k]):
                    raise HmcxError("mlp: leapfrog state %s must be a contiguous %s device tensor of shape %s"
                                    % (k, self.dtype, self.shapes[k]))
            i = MLP_PARAM_NAMES.index(k)
            gs[k] = torch.empty_like(q[k])
            a.q.p[i], a.p.p[i], a.g.p[i] = q[k].data_ptr(), p[k].data_ptr(), gs[k].data_ptr()
        keep = None
        if masks is None:
            keep = torch.empty((3, B, self.n_mid), dtype=self.dtype, device=self.device)
            a.mask_mode, a.masks = MLP_MASKS_PHILOX, keep.data_ptr()
            a.seed, a.chain, a.step = self.seed, 0, 0xFFFFFFFF
            a.slot0 = (MLP_MASK_SLOT0 + self._mask_calls) & 0xFFFFFFFF
            self._mask_calls += 1 + 6 * int(n_iter)
        else:
            keep = self._masks(masks, B)
            a.mask_mode = MLP_MASKS_NONE if keep is None else MLP_MASKS_FIXED
            a.masks = None if keep is None else keep.data_ptr()
        ctx = mlp_context(self)
        ctx.check(ctx.lib.hmcx_mlp_hmc_leapfrog(ctx.h, ctypes.byref(a)), "hmcx_mlp_hmc_leapfrog")
        del keep                                        # stream-ordered: the allocator reuses it after the launches
        return gs

    def loss_device(self, par, masks=None, **args):
        X, y = self._xy(args)
        B = X.shape[0]
        _, mp = self._params(par)
        m = self._masks(masks, B)
        out = torch.empty(1, dtype=torch.float64, device=self.device)
        ctx = mlp_context(self)
        ctx.check(ctx.lib.hmcx_mlp_loss(ctx.h, self.code, ptr(X), ptr(y), B, self.n_in, self.n_mid, self.n_out, mp,
                                        ptr(m), ptr(out), None), "hmcx_mlp_loss")
        return out

    def log_likelihood(self, par, masks=None, **args):                    # mlp.py:66-78 (returns the loss)
        return np.float64(self.loss_device(par, masks=masks, **args).item())

    def log_prior(self, par, **args):                                     # mlp.py:40-45
        """−Σ_var ½·alpha·Σθ²/dim, with Σθ² a float64 device reduction (hmcx_sumsq)."""
        ctx = mlp_context(self)
        ss = torch.empty(len(par), dtype=torch.float64, device=self.device)
        keep = []
        for i, var in enumerate(par.keys()):
            v = self._dev(par[var]).contiguous()
            keep.append(v)
            ctx.check(ctx.lib.hmcx_sumsq(ctx.h, self.code, ptr(v), v.numel(), ptr(ss[i:i + 1])), "hmcx_sumsq")
        sums = ss.cpu().numpy()
        K = 0.0
        for v, s2 in zip(keep, sums):
            K -= 0.5 * self.alpha * float(s2) / v.numel()
        return K

    def negative_log_posterior(self, par, masks=None, **args):           # mlp.py:80-82
        return self.log_likelihood(par, masks=masks, **args) + self.log_prior(par, **args)

    def energy_parts_device(self, par, out, masks=None, **args):
        """The device pieces of negative_log_posterior without a readback: out[0] = the loss
        (log_likelihood), out[1 + i] = Σθ² of the i-th variable of par.  nlp_from_parts adds them up on
        the host exactly as negative_log_posterior does, so a sampler can enqueue several energies and
        read them back once.  Returns the device tensors the launches read (keep them until then)."""
        X, y = self._xy(args)
        B = X.shape[0]
        _, mp = self._params(par)
        m = self._masks(masks, B)
        ctx = mlp_context(self)
        ctx.check(ctx.lib.hmcx_mlp_loss(ctx.h, self.code, ptr(X), ptr(y), B, self.n_in, self.n_mid, self.n_out, mp,
                                        ptr(m), ptr(out[0:1]), None), "hmcx_mlp_loss")
        keep = [m]
        for i, var in enumerate(par.keys()):
            v = self._dev(par[var]).contiguous()
            keep.append(v)
            ctx.check(ctx.lib.hmcx_sumsq(ctx.h, self.code, ptr(v), v.numel(), ptr(out[1 + i:2 + i])), "hmcx_sumsq")
        return keep

    def nlp_from_parts(self, parts, par):
        """negative_log_posterior from energy_parts_device's values (same float64 operations, same order)."""
        ll = np.float64(parts[0])
        K = 0.0
        for i, var in enumerate(par.keys()):
            K -= 0.5 * self.alpha * float(parts[1 + i]) / int(np.prod(np.shape(par[var])))
        return ll + K

    def loss(self, par, masks=None, **args):
        """North-star surface name: the sampler energy U = negative_log_posterior."""
        return self.negative_log_posterior(par, masks=masks, **args)

    def logits(self, par, X, masks='off'):
        X = self._dev(X)
        B = X.shape[0]
        _, mp = self._params(par)
        m = self._masks(masks, B)
        z = torch.empty((B, self.n_out), dtype=self.dtype, device=self.device)
        ctx = mlp_context(self)
        ctx.check(ctx.lib.hmcx_mlp_loss(ctx.h, self.code, ptr(X), None, B, self.n_in, self.n_mid, self.n_out, mp,
                                        ptr(m), None, ptr(z)), "hmcx_mlp_loss")
        return z

    def predict(self, par, X_test, prob=False, masks=None):              # mlp.py:84-96
        """Chainer runs the net in train mode here too, so dropout is on by default (masks=None);
        pass masks='off' for the deterministic network."""
        z = self.logits(par, X_test, masks=masks).cpu().numpy()
        if prob:                                                          # F.softmax on the host (:92)
            e = np.exp(z - z.max(axis=1, keepdims=True))
            return e / e.sum(axis=1, keepdims=True)
        return z.argmax(axis=1)

    # -------------------------------------------------------------- posterior predictive (extension)
    def _stacked(self, posterior):
        """{name: [..., *shape]} → six contiguous device tensors [S, *shape] (leading dimensions flattened
        row-major) and their MlpParams; names and shapes checked as _params does."""
        ts, S = [], None
        for k in MLP_PARAM_NAMES:
            if k not in posterior:
                raise HmcxError("mlp: missing parameter %r (expected %s)" % (k, MLP_PARAM_NAMES))
            t = self._dev(posterior[k])
            shp = self.shapes[k]
            nl = t.dim() - len(shp)
            if nl < 0 or tuple(t.shape[nl:]) != shp:
                raise HmcxError("mlp: %s has shape %s, expected [..., %s]" % (k, tuple(t.shape), shp))
            t = t.reshape((-1,) + shp).contiguous()
            if S is None:
                S = t.shape[0]
            elif t.shape[0] != S:
                raise HmcxError("mlp: %s holds %d parameter sets, the others %d" % (k, t.shape[0], S))
            ts.append(t)
        if S < 1:
            raise HmcxError("mlp: the posterior holds no parameter set")
        mp = MlpParams()
        for i, t in enumerate(ts):
            mp.p[i] = t.data_ptr()
        return ts, mp, S

    def posterior_predictive(self, posterior, X_test, y=None, masks=None, n_dropout=1, path=0):
        """Model averaging on the device in one libhmcx call (hmcx_mlp_predictive): over the S parameter
        sets of ``posterior`` ({name: [..., *shape]}, e.g. what ``sample`` returns, or [chains, epochs, …])
        and ``n_dropout`` dropout draws per set, D = S·n_dropout draws in all (draw d = s·n_dropout + t).
        Returns ``Predictive`` of host arrays: mean [N, n_out] class probabilities, pred [N] (their argmax),
        entropy [N] of the mean, expected_entropy [N] (mean entropy of the draws), mutual_information [N]
        = entropy − expected_entropy and, with labels ``y``, lppd [N] = log mean_d p_d[n, y_n],
        draw_nll [D] (each draw's mean cross-entropy) and draw_accuracy [D]; those three are None without y.
        masks: None draws Philox masks (the model's seed and call counter, as ``predict`` does: the next
        draw_masks / predict continues after these D slots); 'off' disables dropout (n_dropout must be 1);
        an array [D, 3, N, n_mid] injects them.  path: 0 by shape, 1 general, 2 fused (include/hmcx.h)."""
        X = self._dev(X_test)
        if X.dim() != 2 or X.shape[1] != self.n_in:
            raise HmcxError("mlp: X_test must be [N, %d]" % self.n_in)
        N, T = X.shape[0], int(n_dropout)
        if T < 1:
            raise ValueError("n_dropout must be >= 1")
        ts, mp, S = self._stacked(posterior)
        D = S * T
        a = MlpPredictiveArgs()
        a.dtype, a.N, a.n_in, a.n_mid, a.n_out, a.S, a.T = self.code, N, self.n_in, self.n_mid, self.n_out, S, T
        a.path = int(path)
        a.X, a.par = X.data_ptr(), mp
        m = None
        if masks is None:
            a.mask_mode = MLP_MASKS_PHILOX
            a.seed, a.chain, a.step = self.seed, 0, 0xFFFFFFFF
            a.slot0 = (MLP_MASK_SLOT0 + self._mask_calls) & 0xFFFFFFFF
            self._mask_calls += D
        elif isinstance(masks, str):
            if masks != 'off':
                raise ValueError("masks must be None, 'off' or an array [D, 3, N, n_mid]")
            if T != 1:
                raise ValueError("masks='off' makes every draw of a parameter set the same: n_dropout must be 1")
            a.mask_mode = MLP_MASKS_NONE
        else:
            m = self._dev(masks)
            if tuple(m.shape) != (D, 3, N, self.n_mid):
                raise HmcxError("mlp: masks must be [%d, 3, %d, %d]" % (D, N, self.n_mid))
            a.mask_mode, a.masks = MLP_MASKS_FIXED, m.data_ptr()
        yt = None
        if y is not None:
            yt = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))
            yt = yt.to(self.device, torch.int32).contiguous()
            if yt.dim() != 1 or yt.shape[0] != N:
                raise HmcxError("mlp: y must be integer labels [N]")
            a.y = yt.data_ptr()
        f64 = dict(dtype=torch.float64, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        mean, pred = torch.empty((N, self.n_out), **f64), torch.empty(N, **i32)
        ent, eent = torch.empty(N, **f64), torch.empty(N, **f64)
        a.out_mean, a.out_pred = mean.data_ptr(), pred.data_ptr()
        a.out_entropy, a.out_exp_entropy = ent.data_ptr(), eent.data_ptr()
        lppd = nll = corr = None
        if yt is not None:
            lppd, nll, corr = torch.empty(N, **f64), torch.empty(D, **f64), torch.empty(D, **i32)
            a.out_lppd, a.out_draw_nll, a.out_draw_correct = lppd.data_ptr(), nll.data_ptr(), corr.data_ptr()
        ctx = mlp_context(self)
        ctx.check(ctx.lib.hmcx_mlp_predictive(ctx.h, ctypes.byref(a)), "hmcx_mlp_predictive")
        host = [None if t is None else t.cpu().numpy() for t in (mean, pred, ent, eent, lppd, nll, corr)]
        del ts, m, yt, X                                  # read by the launches the copies above waited for
        mean, pred, ent, eent, lppd, nll, corr = host
        return Predictive(mean, pred, ent, eent, ent - eent, lppd, nll,
                          None if corr is None else corr / float(N))

    def predict_posterior(self, posterior, X_test, prob=False, **kw):
        """Posterior predictive over the parameter sets of ``posterior`` (softmax.predict_posterior's
        contract): the mean class probabilities (prob=True) or their argmax.  Keywords go to
        posterior_predictive (masks, n_dropout, path)."""
        r = self.posterior_predictive(posterior, X_test, **kw)
        return r.mean if prob else r.pred

    def predict_stochastic(self, par, X_test, prob=False, n_dropout=10, **kw):
        """MC dropout of one parameter set: the reference's predict (train mode, mlp.py:84-96) averaged
        over n_dropout mask draws on the device."""
        r = self.posterior_predictive(par, X_test, n_dropout=n_dropout, **kw)
        return r.mean if prob else r.pred
