"""SGLD reference for the dropout MLP: oracle.samplers.sgld / sgld_gpu_variant over oracle.models.mlp with the
dropout masks and the noise injected in the sampler's call order.

Masks.  The forwards of global step k are numbered in call order: 0 the gradient forward, then the outer loop's
log line (log_likelihood, every 10th minibatch) if the step has one, then the epoch-end negative_log_posterior if
the step is an epoch's last.  ``mask_fn(k, f) -> [m1, m2, m3]`` (or None: no dropout); ``stream_masks`` builds it
from tests/_mlp_fixtures.mask_stream.

Noise.  draw_momentum calls ``rng.normal(0, 2ε, shape)`` per variable in start order; ``StreamRng`` answers with
``2ε·z``, z the next values of a given stream of standard normals (``source(n)``), which is what NumPy's own
RandomState.normal returns for the same z (loc 0).  The same object also answers ``standard_normal(n)`` from the
same stream, the call the device sampler makes.

The wrapper records what the oracle sampler does not return: the mean CE of every gradient forward (at the state
before the update), every log line's value and the last step's momentum.
"""
import functools
import io
import re
from collections import namedtuple

import numpy as np

from oracle import models as om
from oracle import samplers as osm

import _mlp_fixtures as fx
import _mlp_sgd_ref as sgd_ref

ALPHA, STEP_SIZE, BURNIN, EPOCHS = 0.01, 0.05, 1, 2       # (1 + 2) epochs of 6 minibatches: 18 steps
NOISE_SEED = 8
problem = sgd_ref.problem                                   # N = 6·B + 3, the tail is dropped
stream_masks = sgd_ref.stream_masks


class StreamRng:
    """rng whose normal(0, scale, size) is scale·z and whose standard_normal(n) is z, z = source(count)."""

    def __init__(self, source):
        self.source = source

    def normal(self, loc, scale, size=None):
        assert loc == 0
        shape = (size,) if np.isscalar(size) else tuple(size)
        return scale * np.asarray(self.source(int(np.prod(shape))), dtype=np.float64).reshape(shape)

    def standard_normal(self, n):
        return np.asarray(self.source(int(n)), dtype=np.float64)


def numpy_source(seed=NOISE_SEED, f32=False):
    rs = np.random.RandomState(seed)
    return (lambda n: fx._f32(rs.standard_normal(n))) if f32 else rs.standard_normal


def zero_source(n):
    return np.zeros(n)


def array_source(z):
    """The values of z, in order."""
    pos = [0]

    def source(n):
        out = z[pos[0]:pos[0] + n]
        assert out.size == n, "noise stream exhausted"
        pos[0] += n
        return out
    return source


class MaskedSgldMLP:
    """oracle mlp whose grad, log line and epoch-end energy take injected masks in sgmcmc.sample's call order."""

    def __init__(self, inner, mask_fn):
        self.inner, self.mask_fn = inner, mask_fn
        self.k, self.f = -1, 0
        self.loss_trace, self.log_trace = [], []

    def _next(self):
        m = self.mask_fn(self.k, self.f) if self.mask_fn else None
        self.f += 1
        return m

    def grad(self, par, **args):
        self.k, self.f = self.k + 1, 0
        m = self._next()
        self.loss_trace.append(float(self.inner.log_likelihood(par, masks=m, **args)))
        return self.inner.grad(par, masks=m, **args)

    def log_likelihood(self, par, **args):
        v = self.inner.log_likelihood(par, masks=self._next(), **args)
        self.log_trace.append(float(v))
        return v

    def negative_log_posterior(self, par, **args):
        return self.inner.negative_log_posterior(par, masks=self._next(), **args)


def sampler_class(variant):
    base = osm.sgld_gpu_variant if variant == "gpu" else osm.sgld

    class Recording(base):
        def step(self, state, momentum, rng, **args):
            out = super().step(state, momentum, rng, **args)
            self.last_q, self.last_p = out[0], out[1]
            return out
    return Recording


_LINE = re.compile(r"^(?:(burnin|epoch) (\d+), )?loss: (-?[0-9.]+|nan|-?inf)(?:, mini-batch update : (\d+))?$")


def parse_lines(text):
    """The printed loss lines as (kind, epoch, minibatch, value): kind 'burnin' / 'epoch' for the log lines,
    None for the epoch-end 'loss:' line (epoch and minibatch None there)."""
    out = []
    for line in text.splitlines():
        mt = _LINE.match(line.strip())
        if mt:
            out.append((mt.group(1), None if mt.group(2) is None else int(mt.group(2)),
                        None if mt.group(4) is None else int(mt.group(4)), float(mt.group(3))))
    return out


SgldRun = namedtuple("SgldRun", "post logp loss_trace log_trace lines q p")


def oracle_run(shape, B, mask_fn, variant, source, order=None, epochs=EPOCHS, burnin=BURNIN, data=None):
    """The float64 oracle run of problem(*shape, B) (or ``data`` = (X, y, start)) under mask_fn and the noise
    stream ``source``, start_p in ``order`` (default canonical)."""
    X, y, start = data if data is not None else problem(*shape, B)
    if order is not None:
        start = {k: start[k] for k in order}
    model = MaskedSgldMLP(om.mlp({"alpha": ALPHA}, *shape), mask_fn)
    o = sampler_class(variant)(model, start, step_size=STEP_SIZE)
    o.out = io.StringIO()
    post, logp = o.sample(epochs=epochs, burnin=burnin, batch_size=B, rng=StreamRng(source), X_train=X, y_train=y)
    return SgldRun(post, logp, np.asarray(model.loss_trace), np.asarray(model.log_trace),
                   parse_lines(o.out.getvalue()), o.last_q, o.last_p)


@functools.lru_cache(maxsize=None)
def _fixture_run(name, variant, order, kind):
    f = fx.BY_NAME[name]
    f32 = kind == "f32"
    mask_fn = None if kind == "off" else stream_masks(f.B, f.n_mid, f32=f32)[1]
    source = zero_source if kind == "zero" else numpy_source(f32=f32)
    return oracle_run((f.n_in, f.n_mid, f.n_out), f.B, mask_fn, variant, source, order=list(order) if order else None)


def fixture_run(f, variant="cpu", order=None, kind="f64"):
    """The oracle run of a fixture (computed once per process and shared: treat it as read-only).
    kind: 'f64' stream masks and RandomState(NOISE_SEED) noise, 'f32' both rounded through float32, 'off' no
    dropout, 'zero' the noise replaced by zeros."""
    return _fixture_run(f.name, variant, tuple(order) if order is not None else None, kind)


def state_distance(a, b):
    """max |a − b| over every entry of two states, relative to the largest entry of a."""
    return max(np.abs(a[k] - b[k]).max() for k in a) / max(np.abs(a[k]).max() for k in a)
