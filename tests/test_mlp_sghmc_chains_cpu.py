"""CPU-side checks of multi-chain SGHMC on the dropout MLP (hmcx_mlp_sghmc_chains_run, sghmc(mlp, chains=C)): the
NumPy restatement of the call agrees with the oracle's sghmc.sample on every shape and chain of the recipe
(tests/_mlp_sghmc_chains_ref.py), the recipe's chains take the decisions the GPU tests rely on (asserted on the oracle
alone: this file is the authority for the seeds — a seed that stops meeting a condition is searched again, the
condition stays), the ctypes mirror matches the header, and the Python route refuses what it cannot serve without a
device."""
import ctypes
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import _mlp_fixtures as fx
import _mlp_sghmc_chains_ref as ref
from oracle import models as om

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-3                 # every accept decision at least this far from flipping: min |dE − ln u|


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    _native.load_library()
    return _native


def _agrees(name, c, order=None):
    o, r = ref.oracle_run(name, c, order), ref.restate_chain(name, c, order)
    f = fx.BY_NAME[name]
    assert len(o.trace) == ref.NSTEPS == len(r)
    assert [s.accepted for s in r] == [t['accepted'] for t in o.trace]
    np.testing.assert_allclose([s.A for s in r], [t['A'] for t in o.trace], rtol=1e-10)
    np.testing.assert_allclose([s.E for s in r], [t['E'] for t in o.trace], rtol=1e-10)
    # the oracle's accept call: nlp of the proposal first, then of the current state; the kept one is the call's out_nlp
    for s, t in zip(r, o.trace):
        np.testing.assert_allclose(s.nlp, t['nlp'][0] if s.accepted else t['nlp'][1], rtol=1e-10)
    # posterior: the state at every epoch's end; logp: its negative_log_posterior on the last minibatch, no dropout
    X, y, _ = ref.chain_start(name, c, order)
    m = om.mlp({"alpha": f.alpha}, f.n_in, f.n_mid, f.n_out)
    n = fx.STEPS_PER_CALL
    for e in range(fx.EPOCHS):
        q = r[e * n + n - 1].q
        for k in q:
            np.testing.assert_allclose(q[k], o.post[k][e], rtol=1e-10, atol=0, err_msg=k)
        last = ref.rows(name)[n - 1]
        logp = m.negative_log_posterior(q, masks=None, X_train=X[last:last + f.B], y_train=y[last:last + f.B])
        np.testing.assert_allclose(logp, o.logp[e], rtol=1e-10)


@pytest.mark.parametrize("c", [0, 1, 2])
@pytest.mark.parametrize("name", ref.SHAPES)
def test_restatement_agrees_with_the_oracle(name, c):
    _agrees(name, c)


def test_restatement_agrees_with_the_oracle_in_permuted_order():
    _agrees("w32_b20", 0, fx.PERMUTED)
    o = ref.oracle_run("w32_b20", 0, fx.PERMUTED)
    assert list(o.post.keys()) == fx.PERMUTED
    assert min(fx.margins(o.trace)) >= MARGIN


def test_chain_zero_is_the_committed_fixture_run():
    for name in ref.SHAPES:
        a, b = ref.oracle_run(name, 0).trace, fx.fixture_oracle(fx.BY_NAME[name]).trace
        assert [(t['L'], t['accepted'], t['A']) for t in a] == [(t['L'], t['accepted'], t['A']) for t in b]


def _conditions(name, steps_of, u_of):
    """Over the three chains: an accept and a reject of a multi-iteration step (n >= 2), an n = 0 and an n >= 3 step, ragged
    path lengths, every decision at least MARGIN from flipping."""
    n_all, got = [], dict(acc=False, rej=False)
    for c in range(3):
        o = ref.oracle_run(name, c)
        steps, u = steps_of(c), u_of(c)
        mg = min(ref.margins(steps, u))
        print("%s chain %d: n_iter %s accepts %d of %d, smallest |dE - ln u| %.3g"
              % (name, c, o.n_iter.tolist(), sum(s.accepted for s in steps), len(steps), mg))
        assert mg >= MARGIN, (name, c, mg)
        got['acc'] |= any(s.accepted and n >= 2 for s, n in zip(steps, o.n_iter))
        got['rej'] |= any(not s.accepted and n >= 2 for s, n in zip(steps, o.n_iter))
        n_all.append(o.n_iter)
    n_all = np.stack(n_all, axis=1)                              # [steps, chains]
    assert got['acc'] and got['rej'], name
    assert (n_all == 0).any() and (n_all >= 3).any(), name
    assert (n_all.min(axis=1) != n_all.max(axis=1)).sum() >= ref.NSTEPS // 2, name     # the steps are ragged


@pytest.mark.parametrize("name", ref.SHAPES)
def test_recipe_conditions_on_the_oracle(name):
    for c in range(3):
        o = ref.oracle_run(name, c)
        for t in o.trace:                                         # the recorded quantities are consistent
            dE = t["E"][0] - t["E"][1]
            assert t["accepted"] == bool(np.log(t["u"]) < dE)
        assert min(fx.margins(o.trace)) >= MARGIN
    _conditions(name, lambda c: ref.restate_chain(name, c), lambda c: ref.oracle_run(name, c).u)
    # the chains are different runs
    a, b = ref.oracle_run(name, 0), ref.oracle_run(name, 1)
    assert not np.array_equal(a.n_iter, b.n_iter) and not np.array_equal(a.post['/l1/W'], b.post['/l1/W'])


@pytest.mark.parametrize("name", ref.SHAPES)
def test_recipe_conditions_hold_with_float32_rounded_inputs(name):
    """Momenta, noise and mask values rounded through float32 (what the float32 GPU test feeds both sides): no
    decision flips and every one keeps its margin."""
    rounded = {c: ref.restate_chain(name, c, rnd=_f32) for c in range(3)}
    for c in range(3):
        assert [s.accepted for s in rounded[c]] == [t['accepted'] for t in ref.oracle_run(name, c).trace], (name, c)
    _conditions(name, lambda c: rounded[c], lambda c: ref.oracle_run(name, c).u)


def test_null_arguments_rejected_without_device(nat):
    lib = nat.load_library()
    assert lib.hmcx_mlp_sghmc_chains_run(None, None) == -1
    assert lib.hmcx_last_error(None) == b"null context"
    assert "hmcx_mlp_sghmc_chains_run" in nat.EXPORTS


def test_struct_layout_matches_header(nat, tmp_path):
    """Size and every field offset of MlpSghmcChainsArgs equal what gcc computes from include/hmcx.h."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    py, c = "MlpSghmcChainsArgs", "hmcx_mlp_sghmc_chains_args"
    st = getattr(nat, py)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hmcx.h"', "int main(void) {",
             'printf("sizeof %%zu\\n", sizeof(%s));' % c]
    for f in st._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (f[0], c, f[0]))
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict((ln.split()[0], int(ln.split()[1]))
               for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines() if ln)
    assert ctypes.sizeof(st) == got["sizeof"] and len(got) == len(st._fields_) + 1
    for f in st._fields_:
        assert getattr(st, f[0]).offset == got[f[0]], f[0]


def test_refused_combinations_raise_without_device():
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp_param_shapes

    shapes = mlp_param_shapes(4, 8, 3)
    start = {k: np.zeros(s) for k, s in shapes.items()}
    model = types.SimpleNamespace(_hmcx_model="mlp", shapes=shapes)
    s = sghmc(model, start, chains=3, noise='philox', keep_every=2)
    assert s.chains == 3 and s.keep_every == 2 and s._mlp_start['/l1/W'].shape == (3,) + shapes['/l1/W']
    per_chain = {k: np.zeros((3,) + s_) for k, s_ in shapes.items()}
    assert sghmc(model, per_chain, chains=3, noise='philox').start['/l2/W'].shape == shapes['/l2/W']
    with pytest.raises(HmcxError, match="noise='philox'"):
        sghmc(model, start, chains=3)                                      # the default noise='numpy'
    with pytest.raises(HmcxError, match="at most 64 chains"):
        sghmc(model, start, chains=65, noise='philox')
    with pytest.raises(HmcxError, match="keep_every"):
        sghmc(model, start, chains=1, noise='philox', keep_every=2)
    with pytest.raises(HmcxError, match="expected"):
        sghmc(model, {k: np.zeros((2,) + s_) for k, s_ in shapes.items()}, chains=3, noise='philox')
    with pytest.raises(HmcxError, match="single-chain"):
        s.step(start, None, None, X_train=np.zeros((2, 4)), y_train=np.zeros(2))
    s.mask_provider = lambda k, n: None
    with pytest.raises(HmcxError, match="mask_provider"):
        s.sample(epochs=1, burnin=0, batch_size=2, X_train=np.zeros((2, 4)), y_train=np.zeros(2))
    with pytest.raises(HmcxError, match="no draws"):
        sghmc(model, start, chains=3, noise='philox').chain_diagnostics()
