"""CPU-side checks of hmcx_mlp_sgd_run (momentum SGD on the dropout MLP): the entry validates without a
device, its ctypes mirror matches the header, and the oracle fits the GPU parity tests compare against
(tests/_mlp_sgd_ref.py) are finite and move every variable far beyond the tests' tolerances."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _mlp_fixtures as fx
import _mlp_sgd_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    _native.load_library()
    return _native


def test_null_arguments_rejected_without_device(nat):
    lib = nat.load_library()
    assert lib.hmcx_mlp_sgd_run(None, None) == -1
    assert lib.hmcx_last_error(None) == b"null context"


_MIRRORS = [("MlpSgdArgs", "hmcx_mlp_sgd_args")]


def test_sgd_struct_layout_matches_header(nat, tmp_path):
    """Size and every field offset of MlpSgdArgs equal what gcc computes from include/hmcx.h (the method of
    test_capi.test_struct_layout_matches_header)."""
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


@pytest.mark.parametrize("f", fx.FIXTURES, ids=[f.name for f in fx.FIXTURES])
def test_oracle_fits_are_finite_and_move(f):
    """Every fixture's oracle fit stays finite and moves each variable by more than 1e-3 of its largest
    entry (the parity bounds are 1e-8 and 2e-5 of it: a wrong update cannot hide inside them); the loss
    trace has one entry per step and the momentum is the last update."""
    r = ref.fixture_fit(f)
    _, _, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    assert len(r.loss_trace) == ref.EPOCHS * fx.STEPS_PER_CALL == 18
    assert np.all(np.isfinite(r.loss_trace)) and np.all(np.isfinite(r.loss_val))
    for k in start:
        assert np.all(np.isfinite(r.par[k])), k
        moved = np.abs(r.par[k] - start[k]).max()
        assert moved > 1e-3 * np.abs(start[k]).max(), (k, moved)
        assert np.abs(r.momentum[k]).max() > 0, k
