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
* the fused layer-2/3 launch at 17 to 32 classes (fx.WIDE_CLASS), where the logit items of a row block
  outnumber the workgroup's threads: float64 on both orders, float32 on the quad schedule, fused against
  unfused;
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


# ----------------------------------------------------------------------------- fused forwards at 17-32 classes
# The fused layer-2/3 launch (MM_L23) serves n_out <= 32 and k_fwdr stops at 16 classes (fwdr_ok), so float32
# takes exactly these launches there.  The schedule each shape lands on: fwdr_ok fails on n_out > 16; quad_ok
# holds — float32, buffer masks, n_mid and n_in multiples of 4 (so xw, W2, ga2 rows and the [3, B, n_mid] mask
# blocks are 16-byte aligned), and the at most 3 x 3 workgroups of a fused grid fit four times over.
WIDE_CLASS_SCHEDULE = {shape: "quad" for shape in fx.WIDE_CLASS}
# float32 max |E_gpu - E_oracle| over both energies of the three steps, measured on an MI355X (asserted at 4x;
# |E| is 1.1e3 to 7.5e3, so these are 3e-8 of it).  The library whose publish / poll stopped at 512 items
# measured 3.4e-2, 2.4e-1, 2.5e-1 and 9.6e-2 here, and passed the state bound.
WIDE_CLASS_F32_E = {(16, 32, 17, 32): 3.330e-5, (16, 64, 24, 36): 1.035e-4, (24, 96, 32, 70): 2.256e-4,
                    (16, 32, 32, 33): 4.105e-5}
WIDE_IDS = ["%d-%d-%d-B%d" % s for s in fx.WIDE_CLASS]


def _wide_run(shape, dtype):
    return _gpu_run(*shape, fx.WIDE_CLASS_ALPHA, fx.WIDE_CLASS_SEED, dtype, n_batches=3, epochs=1)


@pytest.mark.parametrize("variant", ["batched", "batch0"])
@pytest.mark.parametrize("shape", fx.WIDE_CLASS, ids=WIDE_IDS)
def test_f64_wide_class_parity(shape, variant, monkeypatch):
    """float64 with 17 to 32 classes through the batched iterations and one sub-step at a time
    (HMCX_MLP_BATCH=0), both on the fused launch, whose 32·n_out logit items per row block outnumber its 512
    threads: path lengths and flags equal, states and both energies of every step within rel 1e-8.
    (Before the publish / poll of the logit partials looped over the items, rows 512 // n_out and up of every
    32-row block took their logits from the K reduction's leftovers in LDS.)"""
    if variant == "batch0":
        monkeypatch.setenv("HMCX_MLP_BATCH", "0")
    ref = fx.wide_class_oracle(shape)
    g = _wide_run(shape, torch.float64)
    assert [t["L"] for t in g.trace] == [t["L"] for t in ref.trace]
    assert [t["accepted"] for t in g.trace] == [t["accepted"] for t in ref.trace]
    print("f64 wide class %s %s: %s" % (shape, variant, g.counts))
    assert g.counts == _expected_counts(ref.trace, "chunked" if variant == "batched" else "single")
    np.testing.assert_allclose([t["E"] for t in g.trace], [t["E"] for t in ref.trace], rtol=1e-8, atol=0)
    for k in ref.post:
        np.testing.assert_allclose(g.post[k], ref.post[k], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("shape", fx.WIDE_CLASS, ids=WIDE_IDS)
def test_f32_wide_class_parity(shape):
    """float32 with the default switches: no k_fwdr launch but exactly the launches of the schedule the shape
    lands on (WIDE_CLASS_SCHEDULE), path lengths equal, the state within 2e-5 of the oracle's largest entry."""
    ref = fx.wide_class_oracle(shape)
    g = _wide_run(shape, torch.float32)
    assert [t["L"] for t in g.trace] == [t["L"] for t in ref.trace]
    print("f32 wide class %s: %s" % (shape, g.counts))
    assert g.counts == _expected_counts(ref.trace, WIDE_CLASS_SCHEDULE[shape])
    for k in ref.post:
        _close(g.post[k], ref.post[k], 2e-5)
    # three steps at eps = 0.005 move the state too little for the state bound to see a wrong gradient (the
    # library with the half-covered publish / poll passes it); both energies of every step do see it
    err_E = float(np.abs(np.array([t["E"] for t in g.trace]) - np.array([t["E"] for t in ref.trace])).max())
    print("f32 wide class %s: max |E err| = %.3e (largest |E| %.3e)" % (
        shape, err_E, float(np.abs([t["E"] for t in ref.trace]).max())))
    assert err_E <= 4 * WIDE_CLASS_F32_E[shape]


@pytest.mark.parametrize("shape", fx.WIDE_CLASS, ids=WIDE_IDS)
def test_f64_wide_class_fused_equals_unfused(shape):
    """The same streams with the fused launch switched off for the context (layer 2, then layer 3 in launches
    of their own): equal path lengths and accept flags, states within rel 1e-10 — the two differ only in the
    summation order of the logits (the bound of test_mlp_fused_timeout_is_recovered_in_process)."""
    from dropout_hamiltonian_montecarlo_amd import _native as nat
    fused = _wide_run(shape, torch.float64)
    ctx = nat.context(0)
    ctx.set_mlp_fuse(False)
    try:
        plain = _wide_run(shape, torch.float64)
    finally:
        ctx.set_mlp_fuse(True)
    assert [t["L"] for t in fused.trace] == [t["L"] for t in plain.trace]
    assert [t["accepted"] for t in fused.trace] == [t["accepted"] for t in plain.trace]
    for k in plain.post:
        np.testing.assert_allclose(fused.post[k], plain.post[k], rtol=1e-10, atol=1e-13)


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
