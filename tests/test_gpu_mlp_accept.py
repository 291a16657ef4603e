"""GPU parity of the dropout-MLP SGHMC sampler (hmcx_mlp.hip::hmcx_mlp_sghmc_run) on the fixtures of
tests/_mlp_fixtures.py, whose oracle trajectories accept AND reject multi-iteration proposals
(test_mlp_fixtures_cpu.py checks that on the oracle alone).  What the config-3 tests cannot see, because
every one of their steps is accepted, is pinned here on every path of the sampler:

* the reject path: k_mlp_commit after a call's last step, the commit folded into the next step's start
  launch (init_block's ``take``), the state a step starts from after a reject;
* both energies of every accept test (E_current, E_new), not only A = min(1, exp(dE)), which hides
  them whenever E_new < E_current;
* ``logp``: the nlp of the accept test's own forward of the state the epoch's last step kept;
* k_fwdr at small shapes (waves without columns, partial row blocks, n_out from 2 to 16);
* which host schedule every step took (k_fwdr, quad, chunked, one at a time): the host-side forward
  counters (hmcx_get_mlp_forward_counts) must equal, exactly, what that schedule launches for the
  trace's path lengths (_expected_counts).

Float32 energy figures (measured on an MI355X, against the float64 oracle at the float32-rounded
inputs; worst of HMCX_MLP_FWDR=1 / 0; asserted at 4x: summation order differs between boxes):

    fixture    max |dE_gpu - dE_oracle|   max |A_gpu - A_oracle|   decision margin
    w32_b20    1.235e-4                   4.41e-6                  0.930
    w96_b36    1.280e-3                   1.27e-18                 2.659
    w256_b4    4.626e-3                   6.02e-83                 4.701
    w20_b30    7.992e-5                   3.59e-6                  0.285

(k_fwdr and the k_mm forwards agree to three digits on every fixture; on w96_b36 and w256_b4 every
unsaturated A belongs to a reject with dE below -30, so its absolute error is A times the dE error.)
"""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _mlp_fixtures as fx  # noqa: E402

# measured float32 errors per fixture (see the table above): (max |dE err|, max |A err|)
F32_MEASURED = {
    "w32_b20": (1.235e-4, 4.41e-6),
    "w96_b36": (1.280e-3, 1.27e-18),
    "w256_b4": (4.626e-3, 6.02e-83),
    "w20_b30": (7.992e-5, 3.59e-6),
}


def _classes():
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.mlp import mlp
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
    return mlp, sghmc


class _Run:
    pass


def _gpu_run(n_in, n_mid, n_out, B, alpha, s1, dtype, order=None, n_batches=fx.STEPS_PER_CALL, epochs=fx.EPOCHS,
             philox_seed=None):
    """sample() on the recipe's problem: injected masks and NumPy streams (the oracle's), or with
    ``philox_seed`` device noise and masks.  Returns trace, posterior, logp and the forward launches
    counted during the run."""
    mlp, sghmc = _classes()
    X, y, start = fx.problem(n_in, n_mid, n_out, B, n_batches)
    if order is not None:
        start = {k: start[k] for k in order}
    m = mlp({"alpha": alpha}, n_in, n_mid, n_out, dtype=dtype, device="cuda:0")
    c0 = m.ctx.mlp_forward_counts()
    if philox_seed is None:
        s = sghmc(m, start, noise='numpy', **fx.KW)
        s.mask_provider = fx.mask_stream(B, n_mid)[0]
    else:
        s = sghmc(m, start, noise='philox', seed=philox_seed, chain=1, **fx.KW)
    s.trace, s.out = [], io.StringIO()
    np.random.seed(s1)
    r = _Run()
    r.post, r.logp = s.sample(epochs=epochs, burnin=0, batch_size=B, rng=np.random.RandomState(8), X_train=X, y_train=y)
    r.trace = s.trace
    c1 = m.ctx.mlp_forward_counts()
    r.counts = {k: c1[k] - c0[k] for k in c1}
    return r


def _fixture_run(f, dtype, order=None):
    return _gpu_run(f.n_in, f.n_mid, f.n_out, f.B, f.alpha, f.s1, dtype, order=order)


def _close(a, b, rel):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b).max()
    assert err <= rel * scale, "max abs err %.3e > %.1e x %.3e" % (err, rel, scale)


def _expected_logp(tr):
    """sample()'s logp of epoch i: the nlp the accept test of the epoch's last step computed (its own
    masked forward) for the state that step kept — the proposal's when accepted, else the current one's."""
    n = fx.STEPS_PER_CALL
    last = [tr[i * n + n - 1] for i in range(len(tr) // n)]
    return [t["nlp"][0] if t["accepted"] else t["nlp"][1] for t in last]


def _expected_counts(tr, schedule):
    """The forward launches (hmcx_get_mlp_forward_counts) of a run whose every step with iterations took
    the host schedule ``schedule`` (DESIGN 5.3 "Host schedules"), from the trace's path lengths, n = L - 1
    leapfrog iterations per step.  A step without iterations runs its two energy forwards one at a time on
    every schedule.

    * ``fwdr``: one k_fwdr launch per iteration, the energy forwards riding in the first and the last;
    * ``quad``: two batched fused launches per iteration; both energy forwards ride along unless n = 1
      (E_current then has no room in the only iteration's second launch and runs after it);
    * ``chunked`` with all six fused grids co-resident (l23_fit = 6, as on the fixtures' few workgroups):
      one batched launch per iteration and one for the two energy forwards;
    * ``single``: six forwards per iteration and the two energy forwards, one launch each.

    The formulas are derived from the host code; the library from before the host call was split into
    per-schedule functions meets every one of them on these tests (27 of 27), so none needed correcting."""
    ns = [int(t["L"]) - 1 for t in tr]
    idle = 2 * sum(1 for n in ns if n == 0)
    real = [n for n in ns if n >= 1]
    if schedule == "fwdr":
        return {"fwdr": sum(ns), "batched": 0, "single": idle}
    if schedule == "quad":
        return {"fwdr": 0, "batched": sum(2 * n + (n == 1) for n in real), "single": idle}
    if schedule == "chunked":
        return {"fwdr": 0, "batched": sum(n + 1 for n in real), "single": idle}
    assert schedule == "single"
    return {"fwdr": 0, "batched": 0, "single": sum(6 * n + 2 for n in ns)}


# ----------------------------------------------------------------------------- float64
@pytest.mark.parametrize("variant", ["batched", "batch0", "permuted"])
@pytest.mark.parametrize("f", fx.FIXTURES, ids=lambda f: f.name)
def test_f64_accept_reject_parity(f, variant, monkeypatch):
    """float64 through the batched iterations (default), one sub-step at a time (HMCX_MLP_BATCH=0) and
    a permuted variable order (unbatched: W1 is not first): path lengths and accept flags equal, both
    energies of every step and A within rel 1e-8 (the project's float64 MLP state tolerance; the
    energies are functions of that state), states within rel 1e-8, logp within rel 1e-9 of the accept
    test's own nlp of the kept state."""
    order = fx.PERMUTED if variant == "permuted" else None
    if variant == "batch0":
        monkeypatch.setenv("HMCX_MLP_BATCH", "0")
    ref = fx.fixture_oracle(f, order)
    g = _fixture_run(f, torch.float64, order)
    assert len(g.trace) == len(ref.trace) == fx.STEPS_PER_CALL * fx.EPOCHS
    assert [t["L"] for t in g.trace] == [t["L"] for t in ref.trace]
    assert [t["accepted"] for t in g.trace] == [t["accepted"] for t in ref.trace]
    np.testing.assert_allclose([t["E"] for t in g.trace], [t["E"] for t in ref.trace], rtol=1e-8, atol=0)
    np.testing.assert_allclose([t["A"] for t in g.trace], [t["A"] for t in ref.trace], rtol=1e-8, atol=0)
    for k in ref.post:
        np.testing.assert_allclose(g.post[k], ref.post[k], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(g.logp, _expected_logp(ref.trace), rtol=1e-9, atol=0)
    # every step ran the schedule the variant names, and no other: float64 batched is the chunked schedule
    # (k_fwdr and quad are float32 only); HMCX_MLP_BATCH=0 and an order without W1 first run one at a time
    print("f64 %s %s: %s" % (f.name, variant, g.counts))
    assert g.counts == _expected_counts(ref.trace, "chunked" if variant == "batched" else "single")


# ----------------------------------------------------------------------------- float32
def _f32_cases():
    out = []
    for f in fx.FIXTURES:
        for fwdr in (("1", "0") if f.fwdr else ("1",)):
            out.append(pytest.param(f, fwdr, id="%s-fwdr%s" % (f.name, fwdr)))
    return out


@pytest.mark.parametrize("f,fwdr", _f32_cases())
def test_f32_accept_reject_parity(f, fwdr, monkeypatch):
    """float32 through k_fwdr (HMCX_MLP_FWDR=1, default: one launch per leapfrog iteration on the
    eligible shapes, none on w20_b30 whose n_mid is no multiple of 32) and through the k_mm forwards
    (=0), against the float64 oracle at the float32-rounded inputs: path lengths and flags equal,
    states within 2e-5 of the largest entry (the project's float32 trajectory tolerance), dE and A
    within 4x the errors measured on an MI355X (module docstring), and that bound no more than a
    quarter of the fixture's decision margin."""
    monkeypatch.setenv("HMCX_MLP_FWDR", fwdr)
    ref = fx.fixture_oracle(f)
    g = _fixture_run(f, torch.float32)
    assert [t["L"] for t in g.trace] == [t["L"] for t in ref.trace]
    assert [t["accepted"] for t in g.trace] == [t["accepted"] for t in ref.trace]
    # k_fwdr on every iteration and nothing else; without it (switched off, or the shape not eligible)
    # every step on the quad schedule
    print("f32 %s fwdr=%s: %s" % (f.name, fwdr, g.counts))
    assert g.counts == _expected_counts(ref.trace, "fwdr" if f.fwdr and fwdr == "1" else "quad")
    for k in ref.post:
        _close(g.post[k], ref.post[k], 2e-5)
    dE_g = np.array([t["E"][0] - t["E"][1] for t in g.trace])
    dE_r = np.array([t["E"][0] - t["E"][1] for t in ref.trace])
    err_dE = float(np.abs(dE_g - dE_r).max())
    err_A = float(np.abs(np.array([t["A"] for t in g.trace]) - np.array([t["A"] for t in ref.trace])).max())
    margin = min(fx.margins(ref.trace))
    print("f32 %s fwdr=%s: max|dE err| = %.3e  max|A err| = %.3e  margin = %.3f" % (f.name, fwdr, err_dE, err_A, margin))
    m_dE, m_A = F32_MEASURED[f.name]
    assert err_dE <= 4 * m_dE
    assert err_A <= 4 * m_A
    assert 4 * m_dE <= margin / 4


# ----------------------------------------------------------------------------- the fallback boundary of fwdr_ok
# the schedule each near miss lands on: all four still pass quad_ok (n_mid and n_in multiples of 4, aligned
# masks, four fused grids co-resident)
NEAR_MISS_SCHEDULE = {shape: "quad" for shape in fx.NEAR_MISS}


@pytest.mark.parametrize("n_in,n_mid,n_out,B", fx.NEAR_MISS,
                         ids=["n_out17", "n_in12", "B18", "n_mid48"])
def test_f32_near_miss_shapes_fall_back(n_in, n_mid, n_out, B):
    """One condition of fwdr_ok missed at a time, from the eligible 16-32-5 / B = 20 shape (n_out > 16,
    n_in % 8, B % 4, n_mid % 32): one call of three steps, no k_fwdr launch but exactly the launches of
    the schedule the shape lands on (NEAR_MISS_SCHEDULE), the state within 2e-5 of the oracle's."""
    ref = fx.oracle_run(n_in, n_mid, n_out, B, fx.NEAR_MISS_ALPHA, fx.NEAR_MISS_SEED, n_batches=3, epochs=1)
    assert min(t["L"] for t in ref.trace) >= 2                    # three real trajectories
    g = _gpu_run(n_in, n_mid, n_out, B, fx.NEAR_MISS_ALPHA, fx.NEAR_MISS_SEED, torch.float32, n_batches=3, epochs=1)
    assert [t["L"] for t in g.trace] == [t["L"] for t in ref.trace]
    print("f32 near miss %s: %s" % ((n_in, n_mid, n_out, B), g.counts))
    assert g.counts == _expected_counts(ref.trace, NEAR_MISS_SCHEDULE[(n_in, n_mid, n_out, B)])
    for k in ref.post:
        _close(g.post[k], ref.post[k], 2e-5)


# ----------------------------------------------------------------------------- Philox mode
PHILOX_ALPHA = 150.0
PHILOX_SEED = {"w96_b36": 1, "w20_b30": 1}     # both flag values among real steps, in both dtypes


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["w96_b36", "w20_b30"])
def test_philox_batched_equals_one_at_a_time_with_rejects(name, dtype, monkeypatch):
    """Device noise and masks (the oracle cannot follow them draw for draw): the batched iterations and
    the one-sub-step-at-a-time order (HMCX_MLP_BATCH=0), both on the k_mm forwards (HMCX_MLP_FWDR=0),
    give bit-identical path lengths, flags, energies, states and logp — as
    test_batched_iterations_equal_one_at_a_time asserts at config 3, but on trajectories that reject
    real proposals as well as accept them."""
    f = fx.BY_NAME[name]
    monkeypatch.setenv("HMCX_MLP_FWDR", "0")
    runs = []
    for batch in ("1", "0"):
        monkeypatch.setenv("HMCX_MLP_BATCH", batch)
        runs.append(_gpu_run(f.n_in, f.n_mid, f.n_out, f.B, PHILOX_ALPHA, 0, dtype, philox_seed=PHILOX_SEED[name]))
    a, b = runs
    assert [t["L"] for t in a.trace] == [t["L"] for t in b.trace]
    # the schedules the two runs name (their own path lengths: no oracle follows device noise): without
    # k_fwdr the batched float32 run is quad, the float64 run chunked
    print("philox %s: batched %s, one at a time %s" % (name, a.counts, b.counts))
    assert a.counts == _expected_counts(a.trace, "quad" if dtype == torch.float32 else "chunked")
    assert b.counts == _expected_counts(b.trace, "single")
    assert [t["accepted"] for t in a.trace] == [t["accepted"] for t in b.trace]
    real = [t["accepted"] for t in a.trace if t["L"] >= 2]
    assert True in real and False in real
    np.testing.assert_array_equal([t["E"] for t in a.trace], [t["E"] for t in b.trace])
    for k in a.post:
        np.testing.assert_array_equal(a.post[k], b.post[k])
    np.testing.assert_array_equal(a.logp, b.logp)
