"""CPU-side checks of the random-walk Metropolis sampler: the NumPy restatement tests/_mh_ref.py against
the golden files the reference's own MH produced (tools/gen_golden_mh.py); the library class's host loop
(callable logp) against the same files; hmcx_mh_run / hmcx_mh_mvn_run exported, validating a null context
without touching a device, their ctypes mirrors laid out as the header's structs; the reference's import
path; the Philox host schedule; and the law criterion of tests/test_gpu_mh.py shown satisfiable by two
restatement ensembles with disjoint seeds."""
import ctypes
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import inputs as gi
from oracle import models as om

import _mh_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MVN_HYPER = {"mu": np.zeros(2), "cov": np.array([[1.0, 0.8], [0.8, 1.0]])}


def configs():
    """name -> (fixture file, group, oracle model, X, y, start, scale, update_sequential, burnin, niter)."""
    X, Y = gi.dataset(3, 60, 24, 10)
    s_start = {"weights": np.zeros((24, 10)), "bias": np.zeros(10)}
    Xl, yl, _, _ = gi.logistic_inputs(3, 77, 33)
    l_start = {"weights": np.zeros((33, 1)), "bias": np.zeros(1)}
    return {
        "softmax_seq": ("mh_softmax.npz", "seq", om.softmax({"alpha": 0.01}), X, Y, s_start, 0.1, True, 8, 12),
        "softmax_site": ("mh_softmax.npz", "site", om.softmax({"alpha": 0.01}), X, Y, s_start, 0.5, False, 8, 12),
        "logistic": ("mh_logistic.npz", "seq", om.logistic({"alpha": 0.25}), Xl, yl, l_start, 0.05, True, 8, 12),
        "mvn_near": ("mh_mvn.npz", "near", om.mvn_gaussian(MVN_HYPER), None, None, {"x": np.zeros(2)}, 1.0, True,
                     50, 200),
        "mvn_far": ("mh_mvn.npz", "far", om.mvn_gaussian(MVN_HYPER), None, None, {"x": np.array([60.0, -60.0])},
                    30.0, True, 0, 40),
    }


@pytest.fixture(scope="module")
def nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    _native.load_library()
    return _native


def _golden(golden_dir, fname, group):
    z = np.load(os.path.join(golden_dir, fname))
    return {k[len(group) + 1:]: z[k] for k in z.files if k.startswith(group + "_")}


@pytest.mark.parametrize("name", ["softmax_seq", "softmax_site", "logistic", "mvn_near", "mvn_far"])
def test_restatement_vs_golden(golden_dir, name):
    """Flags, tuned scale and printed lines equal; draws bit-equal (same NumPy operations)."""
    fname, group, model, X, y, start, scale, seq, burnin, niter = configs()[name]
    g = _golden(golden_dir, fname, group)
    r = _mh_ref.MH(X, y, model, start, model.hyper, scale=scale, update_sequential=seq)
    np.random.seed(0)
    post = r.sample(niter, burnin, np.random.RandomState(0))
    rec = r.records[0]
    assert np.array_equal(np.array(rec.accepted), g["accepted"])
    assert np.array_equal(np.array(rec.u), g["u"])
    assert np.array_equal(np.array(rec.A), g["A"])                   # inf entries included
    assert rec.scale == float(g["scale"])
    assert rec.lines == [str(s) for s in g["lines"]]
    np.testing.assert_allclose(np.array(rec.logp), g["logp"], rtol=0, atol=0)
    for v in start:
        assert post[v].shape == (niter, np.asarray(start[v]).size)
        assert np.array_equal(post[v], g["post_" + v])
    if name == "mvn_far":
        bad = ~np.isfinite(g["A"])
        assert 11 <= bad.sum() <= 23 and np.all(np.isposinf(g["A"][bad])) and not g["accepted"][bad].any()


@pytest.mark.parametrize("name", ["softmax_site", "logistic", "mvn_far"])
def test_library_host_loop_vs_golden(golden_dir, name):
    """MH with a callable logp runs the reference's loop on the host (no device): the golden draws,
    tuned scale and printed lines."""
    from hamiltonian.inference.cpu.metropolis import MH
    fname, group, model, X, y, start, scale, seq, burnin, niter = configs()[name]
    g = _golden(golden_dir, fname, group)
    mh = MH(X, y, _mh_ref.logp_of(model), start, model.hyper, scale=scale, update_sequential=seq)
    mh.out = io.StringIO()
    np.random.seed(0)
    post = mh.sample(niter, burnin, np.random.RandomState(0))
    for v in start:
        assert np.array_equal(post[v], g["post_" + v])
    assert mh.scale == float(g["scale"]) and mh._scale == mh.scale
    assert mh.out.getvalue().splitlines() == [str(s) for s in g["lines"]]
    assert np.array_equal(mh.accepted[:, 0], g["accepted"][burnin:])


def test_null_context(nat):
    lib = nat.load_library()
    assert lib.hmcx_mh_run(None, None) == -1
    assert lib.hmcx_mh_run(None, ctypes.byref(nat.MhArgs())) == -1
    assert lib.hmcx_mh_mvn_run(None, None) == -1
    assert lib.hmcx_mh_mvn_run(None, ctypes.byref(nat.MhMvnArgs())) == -1


@pytest.mark.parametrize("py,c", [("MhArgs", "hmcx_mh_args"), ("MhMvnArgs", "hmcx_mh_mvn_args")])
def test_args_layout_matches_header(nat, tmp_path, py, c):
    """Field offsets and size of the ctypes mirrors equal what gcc computes from include/hmcx.h."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
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
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {line.split()[0]: int(line.split()[1]) for line in out if line}
    assert ctypes.sizeof(st) == got["sizeof"]
    for f in st._fields_:
        assert getattr(st, f[0]).offset == got[f[0]], f[0]
    hdr = open(os.path.join(REPO, "include", "hmcx.h")).read()
    body = hdr[hdr.index("typedef struct %s {" % c):hdr.index("} %s;" % c)]
    assert all(f[0] in body for f in st._fields_)
    last = st._fields_[-1]
    assert getattr(st, last[0]).offset + ctypes.sizeof(last[1]) == ctypes.sizeof(st)   # no field of the header missing


def test_cpu_import_path_is_the_gpu_class():
    import hamiltonian.inference.cpu.metropolis as cpu_mod
    import hamiltonian.inference.gpu.metropolis as gpu_mod
    assert cpu_mod.MH is gpu_mod.MH
    for name in ("sample", "multicore_sample", "chain_diagnostics", "random_walk", "accept", "tune"):
        assert callable(getattr(cpu_mod.MH, name))


@pytest.mark.parametrize("seq", [True, False])
def test_philox_host_schedule(nat, seq):
    """Deterministic, element by element the documented Philox draws, and in range."""
    from hamiltonian.inference.gpu.metropolis import MH
    start = {"weights": np.zeros((24, 10)), "bias": np.zeros(10)}
    mh = MH(None, None, lambda *a: 0.0, start, None, update_sequential=seq, noise="philox", seed=11, chain=5)
    mh.global_step = 7
    scales = [1.0, 0.5, 2.0]
    mult, site, u, z = mh._schedule(6, 3, None, scales, 2, False)
    mult2, site2, u2, _ = mh._schedule(6, 3, None, scales, 2, False)
    assert z is None
    assert np.array_equal(mult, mult2) and np.array_equal(site, site2) and np.array_equal(u, u2)
    assert mult.shape == (6, 3, 2) and site.shape == (6, 3, 2) and u.shape == (6, 3)
    dims = (240, 10)
    for s in range(6):
        for c in range(3):
            pu = nat.philox_uniforms(11, 5 + c, 7 + 2 + s, nat.SLOT_PATH, 4)
            for k in range(2):
                assert mult[s, c, k] == np.exp(-1.5 + 3.0 * pu[k]) * scales[c]
                assert site[s, c, k] == (-1 if seq else int(np.floor(pu[2 + k] * dims[k])))
            assert u[s, c] == nat.philox_uniforms(11, 5 + c, 7 + 2 + s, nat.SLOT_ACCEPT, 1)[0]
    factors = mult / np.array(scales)[None, :, None]
    assert np.all(factors >= np.exp(-1.5) * (1 - 1e-15)) and np.all(factors <= np.exp(1.5) * (1 + 1e-15))
    assert np.all((u >= 0) & (u < 1))
    if not seq:
        assert np.all(site >= 0) and np.all(site[:, :, 0] < 240) and np.all(site[:, :, 1] < 10)


def test_law_criterion_is_satisfiable():
    """Two restatement ensembles (C = 64, 100 + 400 steps, MVN, disjoint Philox seeds) pass the moment
    criterion tests/test_gpu_mh.py applies to the device ensemble."""
    import _stats
    a = _mh_ref.mvn_ensemble(seed=101, C=64, burnin=100, niter=400)
    b = _mh_ref.mvn_ensemble(seed=202, C=64, burnin=100, niter=400)
    assert a.shape == (64, 400, 2)
    _stats.assert_same_moments(_stats.compare(a, b))
