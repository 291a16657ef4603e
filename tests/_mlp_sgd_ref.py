"""Momentum-SGD reference for the dropout MLP: oracle.samplers.sgd over oracle.models.mlp with the dropout masks
injected in the fit's call order.

The gradient of global step k takes the masks of (k, forward 0); the epoch-end negative_log_posterior
(cpu/sgd.py:42) those of (k of the epoch's last step, forward 1).  Masks come from a function
``mask_fn(k, f) -> [m1, m2, m3]`` (or None: no dropout); ``stream_masks`` builds it from
tests/_mlp_fixtures.mask_stream.  The wrapper also records what the oracle sampler does not return: the
mean CE of every gradient forward (at the state before the update) and the momentum, restated with the
sampler's own expression (samplers.py sgd.fit: m = gamma·m − step_size·g).
"""
import functools
import io
from collections import namedtuple

import numpy as np

from oracle import models as om
from oracle import samplers as osm

import _mlp_fixtures as fx

ALPHA, STEP_SIZE, GAMMA, EPOCHS = 0.01, 0.05, 0.9, 3
TAIL = 3                      # rows appended to the 6·B of the recipe: the fit drops them (sgd.py:21)


def problem(n_in, n_mid, n_out, B):
    """_mlp_fixtures.problem with TAIL more rows (float32-rounded like the rest): N = 6·B + 3."""
    X, y, start = fx.problem(n_in, n_mid, n_out, B)
    rs = np.random.RandomState(41)
    X = np.concatenate([X, fx._f32(rs.rand(TAIL, n_in))])
    y = np.concatenate([y, rs.randint(0, n_out, TAIL)])
    return X, y, start


def stream_masks(B, n_mid, f32=False):
    """(provider, mask_fn) over mask_stream: provider is the samplers' ``mask_provider`` (get), mask_fn the
    oracle's view of the same values (rounded through float32 when the device holds them in float32)."""
    get, _ = fx.mask_stream(B, n_mid)

    def mask_fn(k, f):
        m = get(k, f + 1)[f]
        return list(fx._f32(m) if f32 else m)
    return get, mask_fn


class MaskedSgdMLP:
    """oracle mlp whose grad / epoch-end energy take injected masks in sgd.fit's call order."""

    def __init__(self, inner, mask_fn, step_size, gamma):
        self.inner, self.mask_fn = inner, mask_fn
        self.step_size, self.gamma = step_size, gamma
        self.k = 0
        self.loss_trace, self.momentum = [], None

    def grad(self, par, **args):
        m = self.mask_fn(self.k, 0) if self.mask_fn else None
        self.k += 1
        self.loss_trace.append(float(self.inner.log_likelihood(par, masks=m, **args)))
        g = self.inner.grad(par, masks=m, **args)
        if self.momentum is None:
            self.momentum = {v: np.zeros_like(par[v]) for v in par}
        for v in par:
            self.momentum[v] = self.gamma * self.momentum[v] - self.step_size * g[v]
        return g

    def negative_log_posterior(self, par, **args):
        m = self.mask_fn(self.k - 1, 1) if self.mask_fn else None
        return self.inner.negative_log_posterior(par, masks=m, **args)


SgdRun = namedtuple("SgdRun", "par loss_val loss_trace momentum")


def oracle_fit(shape, B, mask_fn, order=None, epochs=EPOCHS):
    """The float64 oracle fit of problem(*shape, B) under mask_fn, start_p in ``order`` (default canonical)."""
    X, y, start = problem(*shape, B)
    if order is not None:
        start = {k: start[k] for k in order}
    model = MaskedSgdMLP(om.mlp({"alpha": ALPHA}, *shape), mask_fn, STEP_SIZE, GAMMA)
    o = osm.sgd(model, start, step_size=STEP_SIZE)
    o.out = io.StringIO()
    par, loss_val = o.fit(epochs=epochs, batch_size=B, gamma=GAMMA, X_train=X, y_train=y)
    return SgdRun(par, loss_val, np.asarray(model.loss_trace), model.momentum)


@functools.lru_cache(maxsize=None)
def _fixture_fit(name, order, kind):
    f = fx.BY_NAME[name]
    mask_fn = None if kind == "off" else stream_masks(f.B, f.n_mid, f32=(kind == "f32"))[1]
    return oracle_fit((f.n_in, f.n_mid, f.n_out), f.B, mask_fn, order=list(order) if order else None)


def fixture_fit(f, order=None, kind="f64"):
    """The oracle fit of a fixture (computed once per process and shared: treat it as read-only).
    kind: 'f64' stream masks, 'f32' the same rounded through float32, 'off' no dropout."""
    return _fixture_fit(f.name, tuple(order) if order is not None else None, kind)
