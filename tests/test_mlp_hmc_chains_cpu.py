"""CPU-side checks of multi-chain HMC on the dropout MLP (hmcx_mlp_hmc_chains_run, hmc_multicore on the GPU mlp):
the NumPy restatement of the call agrees with the oracle's hmc.step, the fixtures take the decisions the GPU tests
rely on (asserted on the oracle alone: this file is the authority for the seeds — a seed that stops meeting a
condition is searched again, the condition stays), the ctypes mirror matches the header, and the Python route is
chosen without a device."""
import ctypes
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import _mlp_hmc_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-3                 # every accept decision at least this far from flipping: min |A − u|


@pytest.fixture(scope="module")
def nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    _native.load_library()
    return _native


@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_fixture_conditions_on_the_oracle(shape):
    o = ref.oracle_run(shape)
    acc = [t['accepted'] for t in o.trace]
    L = [t['L'] for t in o.trace]
    margin = min(abs(t['A'] - t['u']) for t in o.trace)
    print("L %s accepted %s min |A - u| %.3e" % (L, [int(a) for a in acc], margin))
    assert len(o.trace) == ref.NSTEPS
    assert any(acc) and not all(acc)
    assert o.n_iter.min() == 0 and o.n_iter.max() >= 3
    assert margin >= MARGIN


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_other_chains_keep_the_margin(shape, c):
    """Chains 1 and 2 of the three-chain GPU test (their own start, momenta, masks and global stream): their
    decisions are as far from flipping, and their final states differ from chain 0's."""
    o, o0 = ref.oracle_run(shape, c), ref.oracle_run(shape, 0)
    margin = min(abs(t['A'] - t['u']) for t in o.trace)
    print("chain %d: n_iter %s accepted %s min |A - u| %.3e"
          % (c, o.n_iter.tolist(), [int(t['accepted']) for t in o.trace], margin))
    assert margin >= MARGIN
    for k in ref.NAMES:
        assert np.abs(o.trace[-1]['q'][k] - o0.trace[-1]['q'][k]).max() > 1e-3 * np.abs(o0.trace[-1]['q'][k]).max(), k


@pytest.mark.parametrize("c", [0, 1, 2])
@pytest.mark.parametrize("shape", ref.SHAPES, ids=ref.IDS)
def test_restatement_agrees_with_oracle_step(shape, c):
    o, r = ref.oracle_run(shape, c), ref.restate_chain(shape, c)
    assert [s.accepted for s in r] == [t['accepted'] for t in o.trace]
    np.testing.assert_array_equal(o.n_iter, [max(0, int(t['L']) - 1) for t in o.trace])
    np.testing.assert_allclose([s.A for s in r], [t['A'] for t in o.trace], rtol=1e-12)
    np.testing.assert_allclose([s.E for s in r], [t['E'] for t in o.trace], rtol=1e-12)
    for s, t in zip(r, o.trace):
        for k in ref.NAMES:
            np.testing.assert_allclose(s.q[k], t['q'][k], rtol=1e-12, atol=0)


def test_null_arguments_rejected_without_device(nat):
    lib = nat.load_library()
    assert lib.hmcx_mlp_hmc_chains_run(None, None) == -1
    assert lib.hmcx_last_error(None) == b"null context"
    assert "hmcx_mlp_hmc_chains_run" in nat.EXPORTS


def test_struct_layout_matches_header(nat, tmp_path):
    """Size and every field offset of MlpHmcChainsArgs equal what gcc computes from include/hmcx.h."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    py, c = "MlpHmcChainsArgs", "hmcx_mlp_hmc_chains_args"
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


def test_route_is_chosen_without_device():
    """The device route needs the GPU mlp with its own grad, noise='philox' and Philox or no masks; everything else
    keeps the per-chain path."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.hmc_multicore import hmc_multicore
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp, mlp_param_shapes

    shapes = mlp_param_shapes(4, 8, 3)
    start = {k: np.zeros(s) for k, s in shapes.items()}
    own = types.SimpleNamespace(_hmcx_model="mlp", shapes=shapes, leapfrog_device_ok=lambda: True)
    overridden = types.SimpleNamespace(_hmcx_model="mlp", shapes=shapes, leapfrog_device_ok=lambda: False)
    masks = [np.ones((5, 8))] * 3
    s = hmc_multicore(own, start, noise='philox')
    assert s._mlp_fused({}) and s._mlp_fused({'masks': None}) and s._mlp_fused({'masks': 'off'})
    assert not s._mlp_fused({'masks': masks})
    assert not hmc_multicore(own, start)._mlp_fused({})                       # the default noise='numpy'
    assert not hmc_multicore(overridden, start, noise='philox')._mlp_fused({})
    assert not hmc_multicore(types.SimpleNamespace(_hmcx_model="softmax"), start, noise='philox')._mlp_fused({})
    assert hmc_multicore(own, start, noise='philox', keep_momentum=False).keep_momentum is False

    class injected(mlp):                                                        # a subclass that overrides grad
        def grad(self, par, **args):
            return mlp.grad(self, par, **args)
    assert mlp.leapfrog_device_ok(object.__new__(mlp)) and not mlp.leapfrog_device_ok(object.__new__(injected))
