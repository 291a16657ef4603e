"""CPU-side checks of the MLP posterior predictive (no GPU): the C ABI of hmcx_mlp_predictive, the
float64 reference helper tests/_predictive_ref.py, and — on the oracle alone — the gap preconditions the
exact comparisons of tests/test_gpu_mlp_predictive.py rely on (the pattern of test_mlp_fixtures_cpu.py)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _predictive_ref as pr
from oracle import models as om

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    from dropout_hamiltonian_montecarlo_amd import _native
    _native.load_library()
    return _native


def test_predictive_struct_layout_matches_header(nat, tmp_path):
    """Field offsets and size of the ctypes mirror equal what gcc computes from include/hmcx.h (the method
    of test_capi.py::test_struct_layout_matches_header)."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    st, c = nat.MlpPredictiveArgs, "hmcx_mlp_predictive_args"
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
    # every field of the header's struct is mirrored (a missing trailing field would pass the offsets)
    hdr = open(os.path.join(REPO, "include", "hmcx.h")).read()
    body = hdr[hdr.index("typedef struct hmcx_mlp_predictive_args {"):hdr.index("} hmcx_mlp_predictive_args;")]
    n_decl = sum(len(line.split(";")[0].split(",")) for line in body.split("\n")[1:] if ";" in line)
    assert n_decl == len(st._fields_)


def test_predictive_null_context_and_exports(nat):
    lib = nat.load_library()
    assert "hmcx_mlp_predictive" in nat.EXPORTS
    assert lib.hmcx_mlp_predictive(None, None) == -1          # no device touched
    assert lib.hmcx_version() == 10000


def test_helper_single_draw_is_oracle_predict():
    c = pr.CASES[0]
    pb = pr.problem(c.shape, c.seed)
    N, n_in, n_mid, n_out, _, _ = c.shape
    ref = om.mlp({"alpha": 0.01}, n_in, n_mid, n_out)
    for masks in (None, pb.masks[:1]):
        r = pr.predictive_ref(pb.par_sets[:1], pb.X, pb.y, masks, 1)
        mk = None if masks is None else list(masks[0])
        np.testing.assert_array_equal(r.mean, ref.predict(pb.par_sets[0], pb.X, prob=True, masks=mk))
        np.testing.assert_array_equal(r.pred, ref.predict(pb.par_sets[0], pb.X, masks=mk))
        assert r.draw_nll[0] == ref.log_likelihood(pb.par_sets[0], masks=mk, X_train=pb.X, y_train=pb.y)
        # one draw: the mean is the draw, so nothing is gained by knowing which draw it was
        np.testing.assert_allclose(r.mutual_information, 0.0, atol=1e-15)
        np.testing.assert_allclose(r.lppd, np.log(r.mean[np.arange(N), pb.y]), rtol=1e-15)
        assert r.draw_accuracy[0] == np.mean(r.pred == pb.y)


@pytest.mark.parametrize("c", pr.CASES, ids=lambda c: "x".join(map(str, c.shape)))
def test_helper_mutual_information_identities(c):
    for dropout in (True, False):
        r = pr.case_ref(c.shape, c.seed, dropout)
        assert r.mutual_information.min() >= -1e-12             # Jensen: H[mean] >= mean H
        np.testing.assert_allclose(r.mean.sum(axis=1), 1.0, rtol=1e-14)
        assert r.entropy.max() <= np.log(c.shape[3]) + 1e-12
    # all draws equal: the same parameter set S times, no dropout
    pb = pr.problem(c.shape, c.seed)
    r = pr.predictive_ref([pb.par_sets[0]] * 3, pb.X, pb.y, None, 1)
    np.testing.assert_allclose(r.mutual_information, 0.0, atol=1e-14)
    one = pr.predictive_ref(pb.par_sets[:1], pb.X, pb.y, None, 1)
    np.testing.assert_allclose(r.mean, one.mean, rtol=1e-15)


@pytest.mark.parametrize("c", pr.CASES, ids=lambda c: "x".join(map(str, c.shape)))
def test_case_gap_preconditions(c):
    """No reference argmax (of the mean: pred; of a draw's logits: draw_correct) hangs on rounding:
    every top-two gap exceeds 1e-6 in float64 and 1e-3 at float32-rounded inputs, on every row."""
    for rounded, gap in ((False, pr.GAP64), (True, pr.GAP32)):
        for dropout in (True, False):
            r = pr.case_ref(c.shape, c.seed, dropout, rounded)
            assert r.mean_gap > gap and r.logit_gap > gap, (rounded, dropout, r.mean_gap, r.logit_gap)


def test_case_table_sides_of_the_fused_predicate():
    for c in pr.CASES:
        _, n_in, n_mid, n_out, _, _ = c.shape
        assert pr.fused_eligible(n_in, n_mid, n_out, 8) == c.fused, c.shape
        assert pr.fused_eligible(n_in, n_mid, n_out, 4) == c.fused, c.shape
    # the benchmark shape: float32 fits 16 rows of X, h1 and d3 in 160 KiB, float64 does not
    assert pr.fused_eligible(784, 256, 10, 4) and not pr.fused_eligible(784, 256, 10, 8)
    # several row blocks, the last one short
    assert pr.MULTIBLOCK.shape[0] > 32 and pr.MULTIBLOCK.shape[0] % 16
