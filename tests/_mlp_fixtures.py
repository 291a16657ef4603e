"""Shared MLP SGHMC test fixtures: the masked oracle wrappers and a table of small problems whose
oracle trajectories take real accept / reject decisions.

The oracle is oracle.samplers.sghmc over oracle.models.mlp with dropout masks injected in the
sampler's call order.  With the reference's prior weight alpha = 0.01 every small trajectory is
accepted (friction removes about 2·eps·KE per iteration while the loss is a mean, O(1)); a large alpha
makes the ``+eps·grad`` momentum update grow the prior term, and about a third of the multi-iteration
steps reject with |dE| of 10 - 300.  tests/test_mlp_fixtures_cpu.py asserts, on the oracle alone, that
every fixture below has the mix of decisions the GPU parity tests rely on; it is the authority for the
seeds (a seed that stops meeting a condition is searched again, the condition stays).
"""
import functools
import io
from collections import namedtuple

import numpy as np

from oracle import models as om
from oracle import samplers as osm


# ----------------------------------------------------------------------------- masked oracle
def mask_stream(B, n_mid):
    """Masks of forward f of global step k: sequential draws of RandomState(1000 + k)."""
    cache = {}

    def get(k, n):
        rs = np.random.RandomState(1000 + k)
        return np.stack([np.stack(om.dropout_masks(rs, B, n_mid, dtype=np.float64)) for _ in range(n)])

    def one(k, f):
        if k not in cache or cache[k].shape[0] <= f:
            cache[k] = get(k, max(f + 1, 2 * (f + 1)))
        return cache[k][f]
    return get, one


class MaskedOracleMLP:
    """oracle mlp whose grad / accept energies take injected masks in the sampler's call order.
    ``nlp_log`` collects the negative_log_posterior values of the accept calls, in call order
    (hmc.py:67-71: the proposal's first, then the current state's)."""

    def __init__(self, inner, one):
        self.inner, self.one = inner, one
        self.k, self.f, self.in_step = 0, 0, False
        self.nlp_log = []

    def grad(self, par, **args):
        m = self.one(self.k, self.f)
        self.f += 1
        return self.inner.grad(par, masks=list(m), **args)

    def negative_log_posterior(self, par, **args):
        if not self.in_step:
            return self.inner.negative_log_posterior(par, masks=None, **args)
        m = self.one(self.k, self.f)
        self.f += 1
        v = self.inner.negative_log_posterior(par, masks=list(m), **args)
        self.nlp_log.append(float(v))
        return v

    def log_likelihood(self, par, **args):
        return self.inner.log_likelihood(par, masks=None, **args)


class OracleSghmc(osm.sghmc):
    def step(self, state, momentum, rng, **args):
        self.model.in_step, self.model.f = True, 0
        out = super().step(state, momentum, rng, **args)
        self.model.in_step = False
        self.model.k += 1
        return out


class RecordingOracleSghmc(OracleSghmc):
    """Also records, per step, the accept uniform (the step's last global np.random.rand draw: sghmc.py:25
    draws the path length first, :36 the uniform) and the two nlp values of the accept call."""

    def step(self, state, momentum, rng, **args):
        draws, n0 = [], len(self.model.nlp_log)
        real = np.random.rand

        def rand(*a):
            v = real(*a)
            draws.append(v)
            return v
        np.random.rand = rand
        try:
            out = super().step(state, momentum, rng, **args)
        finally:
            np.random.rand = real
        nlp = self.model.nlp_log[n0:]
        assert len(draws) == 2 and len(nlp) == 2
        self.trace[-1]['u'] = float(draws[1])
        self.trace[-1]['nlp'] = (nlp[0], nlp[1])          # (proposal, current)
        return out


# ----------------------------------------------------------------------------- fixtures
Fixture = namedtuple("Fixture", "name n_in n_mid n_out B alpha s1 fwdr")

STEPS_PER_CALL = 6          # N = 6·B: one libhmcx call (epoch) is six steps
EPOCHS = 3
KW = dict(path_length=0.01, step_size=0.005, verbose=True)

FIXTURES = [
    # one column wave of k_fwdr; row blocks 16 + 4
    Fixture("w32_b20", 16, 32, 5, 20, 100.0, 51, True),
    # three column waves; n_out at k_fwdr's limit; row blocks 16 + 16 + 4.  (Seeds 14 and 53 meet every
    # per-fixture condition as well, but no seed of theirs or the other rows' draws an L = 5.)
    Fixture("w96_b36", 40, 96, 16, 36, 100.0, 1925, True),
    # full width; a single 4-row block; n_out = 2
    Fixture("w256_b4", 8, 256, 2, 4, 100.0, 56, True),
    # n_mid % 32 != 0: the k_mm forwards (the shape of test_sghmc_mlp_matches_oracle)
    Fixture("w20_b30", 24, 20, 5, 30, 150.0, 59, False),
]
BY_NAME = {f.name: f for f in FIXTURES}

# One condition of hmcx_mlp.hip::fwdr_ok missed at a time, from the eligible 16-32-5 / B = 20 shape:
# n_out > 16, n_in % 8, B % 4, n_mid % 32.  One call of three steps each (alpha as the reference's).
NEAR_MISS = [(16, 32, 17, 20), (12, 32, 5, 20), (16, 32, 5, 18), (16, 48, 5, 20)]
NEAR_MISS_ALPHA, NEAR_MISS_SEED = 0.01, 51

# The fused layer-2/3 launch (k_mm, MM_L23) past 16 classes, where its 32 × n_out logit items outnumber the
# workgroup's 512 threads (n_in, n_mid, n_out, B): one, two and three column slices; full and partial row
# blocks; 30, 21 and 16 rows of a block inside the first 512 items.  Recipe as for NEAR_MISS.
WIDE_CLASS = [(16, 32, 17, 32), (16, 64, 24, 36), (24, 96, 32, 70), (16, 32, 32, 33)]
WIDE_CLASS_ALPHA, WIDE_CLASS_SEED = 0.01, 51

PERMUTED = ['/l3/b', '/l1/W', '/l2/b', '/l3/W', '/l1/b', '/l2/W']


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def problem(n_in, n_mid, n_out, B, n_batches=STEPS_PER_CALL):
    """X, y and start weights of the recipe, rounded through float32 (both dtypes see the same inputs)."""
    rs = np.random.RandomState(4)
    N = n_batches * B
    X = _f32(rs.rand(N, n_in))
    y = rs.randint(0, n_out, N)
    start = {k: _f32(rs.normal(0, 0.2, s)) for k, s in om.mlp_param_shapes(n_in, n_mid, n_out).items()}
    return X, y, start


OracleRun = namedtuple("OracleRun", "trace post logp")


def oracle_run(n_in, n_mid, n_out, B, alpha, s1, order=None, n_batches=STEPS_PER_CALL, epochs=EPOCHS):
    X, y, start = problem(n_in, n_mid, n_out, B, n_batches)
    if order is not None:
        start = {k: start[k] for k in order}
    _, one = mask_stream(B, n_mid)
    o = RecordingOracleSghmc(MaskedOracleMLP(om.mlp({"alpha": alpha}, n_in, n_mid, n_out), one), start, **KW)
    o.trace, o.out = [], io.StringIO()
    np.random.seed(s1)
    post, logp = o.sample(epochs=epochs, burnin=0, batch_size=B, rng=np.random.RandomState(8), X_train=X, y_train=y)
    return OracleRun(o.trace, post, logp)


@functools.lru_cache(maxsize=None)
def _fixture_oracle(name, order):
    f = BY_NAME[name]
    return oracle_run(f.n_in, f.n_mid, f.n_out, f.B, f.alpha, f.s1, order=list(order) if order else None)


def fixture_oracle(fx, order=None):
    """The oracle run of a fixture (computed once per process and shared: treat it as read-only)."""
    return _fixture_oracle(fx.name, tuple(order) if order is not None else None)


@functools.lru_cache(maxsize=None)
def wide_class_oracle(shape):
    """The oracle run of a WIDE_CLASS shape: one call of three steps (computed once, read-only)."""
    return oracle_run(*shape, WIDE_CLASS_ALPHA, WIDE_CLASS_SEED, n_batches=3, epochs=1)


def margins(trace):
    """|dE - ln u| of every step, dE = E_current - E_new: the distance of each accept decision from
    flipping (the step accepts iff ln u < dE)."""
    return [abs((t["E"][0] - t["E"][1]) - np.log(t["u"])) for t in trace]
