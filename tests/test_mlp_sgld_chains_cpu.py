"""CPU-side checks of multi-chain SGLD on the dropout MLP (hmcx_mlp_sgld_chains_run, sgld(mlp, chains=C)): the
ctypes mirror matches the header, the sampler's start_p / chains checks need no device, and the two starts of the
GPU replicas test (tests/test_gpu_mlp_sgld_chains.py: the fixture start and its negation, same masks and noise)
lead the oracle to final states far enough apart that a kernel that mixes up chains cannot pass it."""
import ctypes
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import _mlp_fixtures as fx
import _mlp_sgld_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_FLOOR = 2e-4            # 10 × the float32 state bound (2e-5 of the largest entry)


@pytest.fixture(scope="module")
def nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    _native.load_library()
    return _native


def second_start(start):
    """The second chain's start of the replicas test: every entry of the fixture start negated."""
    return {k: -v for k, v in start.items()}


def replica_oracle(f, variant, start, f32=False):
    """The oracle run of fixture f from `start` under the stream masks and the RandomState(NOISE_SEED) noise."""
    X, y, _ = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    return ref.oracle_run((f.n_in, f.n_mid, f.n_out), f.B, ref.stream_masks(f.B, f.n_mid, f32=f32)[1], variant,
                          ref.numpy_source(f32=f32), data=(X, y, start))


@pytest.mark.parametrize("variant", ["cpu", "gpu"])
@pytest.mark.parametrize("name", ["w32_b20", "w20_b30"])
def test_the_two_starts_of_the_replicas_test_stay_apart(name, variant):
    f = fx.BY_NAME[name]
    _, _, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    a, b = replica_oracle(f, variant, start), replica_oracle(f, variant, second_start(start))
    d = min(ref.state_distance(a.q, b.q), ref.state_distance(b.q, a.q))
    print("%s %s: the two starts end %.3e of the largest entry apart" % (name, variant, d))
    assert d >= CHAIN_FLOOR, d
    for k in a.q:                                              # variable by variable, too
        assert np.abs(a.q[k] - b.q[k]).max() / np.abs(a.q[k]).max() >= CHAIN_FLOOR, k
    assert not np.allclose(a.loss_trace, b.loss_trace, rtol=1e-4)


def _stub_model(f):
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp_param_shapes
    return types.SimpleNamespace(_hmcx_model="mlp", shapes=mlp_param_shapes(f.n_in, f.n_mid, f.n_out))


def test_start_and_chain_count_are_checked_without_device():
    from dropout_hamiltonian_montecarlo_amd._native import HmcxError
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sgld import sgld
    f = fx.BY_NAME["w32_b20"]
    m = _stub_model(f)
    _, _, start = ref.problem(f.n_in, f.n_mid, f.n_out, f.B)
    C = 3
    stack = lambda n: {k: np.stack([v] * n) for k, v in start.items()}  # noqa: E731
    with pytest.raises(HmcxError):
        sgld(m, stack(C + 1), chains=C)
    with pytest.raises(HmcxError):
        sgld(m, stack(2), chains=1)                            # one chain takes the variable's own shape only
    with pytest.raises(ValueError):
        sgld(m, start, chains=0)
    with pytest.raises(HmcxError):
        sgld(m, start, chains=65)
    mixed = stack(C)
    mixed["/l2/b"] = start["/l2/b"]                            # a replicated variable next to stacked ones
    for sp in (start, stack(C), mixed):
        s = sgld(m, sp, chains=C, noise="philox")
        assert list(s.start.keys()) == list(start.keys())
        for k in start:
            assert s.start[k].shape == start[k].shape and s._mlp_start[k].shape == (C,) + start[k].shape
            np.testing.assert_array_equal(s._mlp_start[k][C - 1], start[k])
    # noise='numpy' replays one host stream in every chain (replicas): it takes per-chain starts only
    with pytest.raises(HmcxError):
        sgld(m, start, chains=C, noise="numpy")
    assert sgld(m, stack(C), chains=C, noise="numpy")._mlp_start["/l1/W"].shape[0] == C
    assert sgld(m, mixed, chains=C, noise="numpy").chains == C
    with pytest.raises(HmcxError):
        sgld(m, start, chains=C, noise="philox").step(start, None, None)   # step() is the single-chain API


def test_null_arguments_rejected_without_device(nat):
    lib = nat.load_library()
    assert lib.hmcx_mlp_sgld_chains_run(None, None) == -1
    assert lib.hmcx_last_error(None) == b"null context"
    assert "hmcx_mlp_sgld_chains_run" in nat.EXPORTS


def test_chains_struct_layout_matches_header(nat, tmp_path):
    """Size and every field offset of MlpSgldChainsArgs equal what gcc computes from include/hmcx.h, and the
    one-chain struct is the same fields without C and draw_stride (chain0 in the place of chain)."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    py, c = "MlpSgldChainsArgs", "hmcx_mlp_sgld_chains_args"
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
    one = [f[0] for f in nat.MlpSgldArgs._fields_]
    assert [f[0] for f in st._fields_ if f[0] not in ("C", "draw_stride")] == ["chain0" if n == "chain" else n for n in one]
