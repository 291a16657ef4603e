"""CPU-side checks of hmcx_mlp_sgld_run (SGLD on the dropout MLP): the entry validates without a device, its
ctypes mirror matches the header, and the oracle runs the GPU parity tests compare against
(tests/_mlp_sgld_ref.py) meet the conditions those tests rely on: finite, every variable moved far beyond the
tolerances, and a noise contribution to the final state of at least ten times the float32 bound — so a kernel
that drops or misplaces the noise cannot hide inside any tolerance."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _mlp_fixtures as fx
import _mlp_sgld_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_FLOOR = 2e-4            # 10 × the float32 state bound (2e-5 of the largest entry)


@pytest.fixture(scope="module")
def nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    _native.load_library()
    return _native


def test_null_arguments_rejected_without_device(nat):
    lib = nat.load_library()
    assert lib.hmcx_mlp_sgld_run(None, None) == -1
    assert lib.hmcx_last_error(None) == b"null context"


_MIRRORS = [("MlpSgldArgs", "hmcx_mlp_sgld_args")]


def test_sgld_struct_layout_matches_header(nat, tmp_path):
    """Size and every field offset of MlpSgldArgs equal what gcc computes from include/hmcx.h (the method of
    test_mlp_sgd_cpu.test_sgd_struct_layout_matches_header)."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hmcx.h"', "int main(void) {"]
    for py, c in _MIRRORS:
        st = getattr(nat, py)
        lines.append('printf("%s sizeof %%zu\\n", sizeof(%s));' % (py, c))
        for f in st._fields_:
            lines.append('printf("%s %s %%zu\\n", offsetof(%s, %s));' % (py, f[0], c, f[0]))
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {}
    for line in out:
        if line:
            py, name, val = line.split()
            got[(py, name)] = int(val)
    for py, _ in _MIRRORS:
        st = getattr(nat, py)
        assert ctypes.sizeof(st) == got[(py, "sizeof")], py
        assert len(got) == len(st._fields_) + 1
        for f in st._fields_:
            assert getattr(st, f[0]).offset == got[(py, f[0])], (py, f[0])


@pytest.mark.parametrize("variant", ["cpu", "gpu"])
@pytest.mark.parametrize("f", fx.FIXTURES, ids=[f.name for f in fx.FIXTURES])
def test_oracle_runs_meet_the_parity_conditions(f, variant):
    r = ref.fixture_run(f, variant)
    _, _, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    assert len(r.loss_trace) == (ref.BURNIN + ref.EPOCHS) * fx.STEPS_PER_CALL == 18
    assert len(r.log_trace) == ref.BURNIN + ref.EPOCHS and r.logp.shape == (ref.EPOCHS,)
    assert np.all(np.isfinite(r.loss_trace)) and np.all(np.isfinite(r.log_trace)) and np.all(np.isfinite(r.logp))
    for k in start:
        assert np.all(np.isfinite(r.q[k])) and np.all(np.isfinite(r.p[k])), k
        assert r.post[k].shape == (ref.EPOCHS,) + start[k].shape
        np.testing.assert_array_equal(r.post[k][-1], r.q[k])
        moved = np.abs(r.q[k] - start[k]).max()
        assert moved > 1e-3 * np.abs(start[k]).max(), (k, moved)
    # the noise's share of the final state: the same run with the noise replaced by zeros
    noise = ref.state_distance(r.q, ref.fixture_run(f, variant, kind="zero").q)
    print("%s %s: zeroing the noise moves the final state by %.3e of its largest entry" % (f.name, variant, noise))
    assert noise >= NOISE_FLOOR, noise
    # and the two update rules are told apart by more than that
    other = ref.fixture_run(f, "gpu" if variant == "cpu" else "cpu")
    assert ref.state_distance(r.q, other.q) > NOISE_FLOOR


def test_stream_rng_is_numpys_normal():
    """StreamRng over RandomState(s).standard_normal returns what RandomState(s).normal(0, scale, shape)
    returns, bit for bit, in any chunking — the device sampler's one standard_normal call per epoch replays the
    oracle's per-variable draws."""
    a, b = ref.StreamRng(ref.numpy_source(3)), np.random.RandomState(3)
    for shape in [(5, 3), (7,), (2, 2)]:
        np.testing.assert_array_equal(a.normal(0, 0.1, shape), b.normal(0, 0.1, size=shape))
    c = ref.StreamRng(ref.numpy_source(3))
    z = c.standard_normal(15 + 7 + 4)
    np.testing.assert_array_equal(0.1 * z[:15].reshape(5, 3), np.random.RandomState(3).normal(0, 0.1, size=(5, 3)))
