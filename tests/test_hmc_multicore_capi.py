"""CPU-side checks of the multi-chain full-batch HMC surface: hmcx_hmc_chains_run is exported and
validates a null context without touching a device, its ctypes mirror has the header's layout, and
the reference's import path hamiltonian.inference.cpu.hmc_multicore resolves to the libhmcx class."""
import ctypes
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    _native.load_library()
    return _native


def test_chains_run_null_context(nat):
    lib = nat.load_library()
    assert lib.hmcx_hmc_chains_run(None, None) == -1
    a = nat.HmcChainsArgs()
    assert lib.hmcx_hmc_chains_run(None, ctypes.byref(a)) == -1


def test_chains_args_layout_matches_header(nat, tmp_path):
    """Field offsets and size of HmcChainsArgs equal what gcc computes from include/hmcx.h."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    st, c = nat.HmcChainsArgs, "hmcx_hmc_chains_args"
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
    # every field of the header's struct is mirrored (C, chain0 and the rest), in the header's order
    assert [f[0] for f in st._fields_] == [
        "dtype", "model", "B", "D", "K", "C", "n_steps", "alpha", "log_prior", "lp_const", "X", "Y", "eps",
        "n_iter", "u_accept", "noise_mode", "noise", "noise_off", "seed", "chain0", "step_base", "W", "b",
        "out_A", "out_accepted", "out_nlp", "out_E", "out_trace", "out_mom"]


def test_cpu_import_path_is_the_gpu_class():
    import hamiltonian.inference.cpu.hmc_multicore as cpu_mod
    import hamiltonian.inference.gpu.hmc_multicore as gpu_mod
    from hamiltonian.inference.gpu.hmc import hmc
    assert cpu_mod.hmc_multicore is gpu_mod.hmc_multicore
    assert issubclass(cpu_mod.hmc_multicore, hmc)
    assert callable(cpu_mod.hmc_multicore.sample_multicore) and callable(cpu_mod.hmc_multicore.chain_diagnostics)
