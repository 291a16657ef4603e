"""Every poll-pass variant of the persistent single-chain SGHMC kernel (csrc/hmcx_p2x.h: poll_nb, polln_nb,
the spread gathers) at the smallest shapes that reach it, against the NumPy oracle.

A pass of those helpers loads its whole batch, tests ONE miss word and either takes every value from
that pass or re-reads everything; entries a thread does not want alias one it does.  What can go wrong
is a sum in another order (state off by rounding), a value taken from an aliased entry (state plainly
wrong) or a pass that never completes (4 s timeout, then a re-run on the kernel-per-phase path that
hides it behind a correct result) — so every case checks the trajectory AND that no hand-off timed out.

All cases: float64 unless said, path 2 (persistent only), N = 3·B, one epoch, no burn-in, ε = 1e-3,
path length 5e-3.  Plans are plan_p2's (csrc/hmcx_persist2.hip; HMCX_P2_DEBUG=1 prints them)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_samplers import _run_gpu, _run_oracle  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(B, D, K):
    return dict(kind="sghmc", N=3 * B, B=B, D=D, K=K, alpha=0.01, step_size=1e-3, path_length=5e-3, burnin=0,
                epochs=1, data_seed=23, np_seed=2, rng_seed=9)


_ORACLE = {}


def _oracle(B, D, K):
    """The oracle's run of a shape, computed once and shared (the f32 case reuses the first shape's)."""
    if (B, D, K) not in _ORACLE:
        _ORACLE[(B, D, K)] = _run_oracle(_config(B, D, K))
    return _ORACLE[(B, D, K)]


def _check(B, D, K, capfd):
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    post_r, _, tr_r, _ = _oracle(B, D, K)
    before = dict(nat.recoveries_all())
    post_g, _, tr_g, _ = _run_gpu(_config(B, D, K), path=2)
    assert [t["L"] for t in tr_g] == [t["L"] for t in tr_r]
    assert [t["accepted"] for t in tr_g] == [t["accepted"] for t in tr_r]
    for v in ("weights", "bias"):
        np.testing.assert_allclose(post_g[v], post_r[v], rtol=1e-9, atol=1e-11)
    assert "timed out" not in capfd.readouterr().err
    assert dict(nat.recoveries_all()) == before


def test_16x16_sixteen_producer_batches(capfd):
    """B=300, D=1500, K=10: plan 16x16 (Br 32, Bf 94, Ro 2, Fo 6), KC 10, spread off (16·(60 + 11) pairs
    exceed the staging area), B all-reduce.  Reaches poll_nb<2> with 16 producers in A-RS (SUM) and in
    A-AG (SUM headers, stores of the diff rows), and polln_nb<2, 2> (64 loads per pass) over two item
    passes (951 items > 512), the second with absent second items."""
    _check(300, 1500, 10, capfd)


def test_4x8_reduce_scatter_and_all_gather(capfd):
    """B=100, D=400, K=12: plan 4x8 (Br 32, Bf 50, Ro 4, Fo 13), KC 16, no room for the noise threads, so
    `bar` is off: B-RS by poll_nb<1, SUM> with 4 producers, B-AG by poll_nb<1, stores> with pskip = own
    row and a per-thread producer count, A-AG by the 3-granule spread gather (8·81 pairs)."""
    _check(100, 400, 12, capfd)


def test_8x16_generic_kernel_without_spread(capfd):
    """B=500, D=784, K=3: config 2's plan 8x16 (Br 64, Bf 49, Ro 4, Fo 7) on the generic kernel (KC 16),
    spread off (16·(17 + 64) pairs exceed the staging area): A-AG by poll<true> (headers) and
    poll<false> (diff rows) with 16 producers, B all-reduce by polln_nb<2, 1> in two item passes."""
    _check(500, 784, 3, capfd)


def test_8x8_one_granule_gather(capfd):
    """B=120, D=700, K=10: plan 8x8 (Br 16, Bf 88, Ro 2, Fo 11), KC 10, spread on: A-AG by the
    1-granule spread gather (8·31 = 248 pairs, threads 248-255 want nothing), B all-reduce by
    polln_nb<2, 1> in two item passes (891 items).  (D = 784 gives the same plan with Fo 13, whose
    8·(130 + 11) pairs switch every spread gather off; D = 700 keeps the coverage.)"""
    _check(120, 700, 10, capfd)


def test_2x4_ragged_rows_and_features(capfd):
    """B=33, D=17, K=2: plan 2x4 (Br 32, Bf 5, Ro 8, Fo 3), KC 16: row team 1 holds one row, so three of
    its members own no softmax rows (they want nothing in A-RS), feature team 3 holds 2 of its 5
    features; 3-granule gather whose last granule is absent for most threads (580 pairs), B all-reduce
    in one item pass with absent second items."""
    _check(33, 17, 2, capfd)


def test_1x1_teams_of_one(capfd):
    """B=16, D=8, K=10: plan 1x1, `bar` off: every round has one producer — B-AG skips it (pskip = 0 of
    np = 1: nothing wanted, no load issued), the accept round polls one workgroup."""
    _check(16, 8, 10, capfd)


def test_16x16_f32(capfd):
    """The first shape in float32 (same plan): the granules carry the float's double; tolerances of
    test_gpu_samplers.test_trajectory_f32."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    B, D, K = 300, 1500, 10
    post_r, logp_r, tr_r, _ = _oracle(B, D, K)
    before = dict(nat.recoveries_all())
    post_g, logp_g, tr_g, _ = _run_gpu(_config(B, D, K), dtype=torch.float32, path=2)
    assert [t["L"] for t in tr_g] == [t["L"] for t in tr_r]
    scale = np.abs(post_r["weights"]).max() + 1e-3
    assert np.abs(post_g["weights"] - post_r["weights"]).max() <= 1e-3 * scale
    np.testing.assert_allclose(logp_g, logp_r, rtol=1e-4)
    assert "timed out" not in capfd.readouterr().err
    assert dict(nat.recoveries_all()) == before


_CHILD = r"""
import io, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from oracle import inputs as gi
from dropout_hamiltonian_montecarlo_amd import _native as nat
from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
X, Y = gi.dataset(23, 1500, 784, 10)
m = softmax({"alpha": 0.01}, dtype=torch.float64, device="cuda:0")
m.ctx.set_sghmc_path(2)
s = sghmc(m, {"weights": np.zeros((784, 10)), "bias": np.zeros(10)}, path_length=5e-3, step_size=1e-3, verbose=True)
s.trace = []
s.out = io.StringIO()
np.random.seed(2)
post, logp = s.sample(epochs=1, burnin=0, batch_size=500, rng=np.random.RandomState(9), X_train=X, y_train=Y)
assert not any(nat.recoveries_all().values()), nat.recoveries_all()
np.savez(sys.argv[2], weights=post["weights"], bias=post["bias"], E=np.array([t["E"] for t in s.trace], dtype=np.float64),
         L=np.array([t["L"] for t in s.trace]))
"""


def test_folded_kernel_equals_generic_kernel_bit_for_bit(tmp_path):
    """Config 2's shape (B=500, D=784, K=10, N=1500, one epoch): the folded instantiation
    k_sghmc_p2<double, 10, 1> (region offsets compiled in, cold arguments read where they are used) and
    the generic kernel (HMCX_P2_SPEC=0) return bit-equal weights, bias and energies.  The variable is
    read once per process, so each run is a fresh child."""
    got = []
    for spec in (None, "0"):
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "HMCX_P2_SPEC")}
        if spec is not None:
            env["HMCX_P2_SPEC"] = spec
        out = tmp_path / ("spec_%s.npz" % spec)
        r = subprocess.run([sys.executable, "-c", _CHILD, REPO, str(out)], cwd=REPO, env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "timed out" not in r.stderr
        got.append(np.load(out))
    a, b = got
    assert a["L"].sum() > len(a["L"])                          # leapfrogs were run
    for name in ("weights", "bias", "E", "L"):
        assert np.array_equal(a[name], b[name]), name
