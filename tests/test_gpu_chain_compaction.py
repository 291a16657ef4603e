"""GPU: active-chain compaction of the chain-batched SGHMC path (csrc/hmcx_batch.h, sghmc_batch_t in
csrc/hmcx_softmax.hip) against a per-chain float64 reference, under host-scripted heterogeneous path
lengths (tests/_sghmc_cases.py): the perm gather, partially active chain tiles, the kernel switches
inside one trajectory (64-row -> tail forward, k_bgradw -> k_bgrad), the partial buffers they share,
and real accept and reject decisions — every chain, every step.

Shapes (3 steps each, K = 10, alpha = 0.01, zero start, oracle.inputs.dataset inputs unless stated):

  S1   C = 40,  B = 50,  D = 50,  eps 5e-2   k_bfwd<T,1,.>, k_bgrad; C % 16 = 8, D % 32 = 18, B % 32 = 18;
                                             c_act 35 -> 30 -> 20 -> 15 -> 10 -> 5 crosses 32 and 16
  S2   C = 528, B = 70,  D = 64,  eps 5e-2   big: E_current on k_bfwd<T,2,0>, every iteration on the tail
                                             forward (32-row tiles, or the 8-wave 64-row kernel under
                                             HMCX_BTAIL32=0); ceil(70/32) = 3 blocks against nRB = 4: the
                                             zero-filled partial block is summed by the accept kernel
  S3   C = 528, B = 460, D = 976, eps 5e-3   big: c_act 517 (full forward, k_bgradw) -> 506 (tail forward,
                                             k_bgradw) -> 374 (k_bgrad) -> 154; D % 64 = 16: tail_last;
                                             ceil(460/32) = 15 is odd; path lengths 1 and 2 end under
                                             k_bgradw, 6 and 7 under k_bgrad
  S4   C = 5 / C = 20, K = 7 / C = 16, D = 33   the kernel-per-phase path under the same kind of schedule

The S3 path-length table is {0: 1, 1: 1, 2: 12, 6: 20, 7: 14} prototypes of 48 (11 chains each): from the
states the accepted steps reach, path lengths 3 to 5 give acceptance probabilities anywhere between 0 and
1 (E_current - E_new from -790 to +120 over the prototypes), so they cannot carry a decision that must
hold for every chain of a prototype; 1-2 (>= +43) and 6-7 (<= -75) can.  The launch plan of every
iteration is read from hmcx_sghmc_batch_plan_query with the device's CU count and asserted, so a retuned
threshold fails these tests instead of hollowing them out.

Tolerances.  float64: flags bit-exact; states, A rtol 1e-9 atol 1e-12; log-likelihood rtol 1e-10;
E_current, and E_new of accepted trajectories, rtol 1e-10 atol 1e-9 (those of tests/test_gpu_chains.py).
E_new of rejected (hot) trajectories: max(that, 16·δ·|E_new|), δ the largest relative change of those
energies when the float64 reference is re-run with the feature axis of X and W reversed (same
mathematics, another summation order; 16 because the device's tiled order differs from both).
Measured δ: S1 2.1e-16, S2 4.0e-16, S3 2.6e-16, S4a 2.5e-16, S4b 2.1e-16, S4c 2.1e-16 — the hot
energies are no more sensitive to the order than the others, so the project tolerance governs.
float32 (S1, S2): flags bit-exact; states within max(16·d, 1e-5·scale) of the float64 reference, d the
largest distance between the reference run in float32 and in float64 at that step, scale the largest
|state|.  Measured d per step: S1 2.9e-8, 2.9e-8, 3.4e-8 (scale 0.29, 0.30, 0.39); S2 3.8e-8, 5.0e-8,
5.2e-8 (scale 0.37, 0.45, 0.53) — the 1e-5 floor governs.
"""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _sghmc_cases as cases  # noqa: E402
from oracle import inputs as gi  # noqa: E402
from dropout_hamiltonian_montecarlo_amd import _native as nat  # noqa: E402


def _dirty_workspace():
    """One short Philox-mode step of 528 chains at D = 2048: its working copies of W and of the momentum
    (non-zero everywhere, 173 MB) span the context's workspace past the footprint of every case here, so
    a partial block that a case's kernels fail to write or zero-fill holds garbage when the accept kernel
    sums it — whatever ran before in the process, and in whatever order the tests run."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
    X, Y = gi.dataset(7, 32, 2048, 10)
    g = sghmc(softmax({"alpha": cases.ALPHA}, dtype=torch.float64, device="cuda:0"),
              {"weights": np.full((2048, 10), 0.01), "bias": np.zeros(10)}, path_length=1e-3, step_size=1e-3,
              noise="philox", seed=1, chains=528)
    g.out = io.StringIO()
    g._run(g._init_state(), g._upload_data(X, Y), [0], [1e-3], None, 32)


def _run_device(name, dtype):
    """The case's C chains on the device through the scripted schedule; returns the RunResult (states
    after every step recorded) and the final state [C, P]."""
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.models.gpu.softmax import softmax
    from dropout_hamiltonian_montecarlo_amd.hamiltonian.inference.gpu.sghmc import sghmc
    c, sc = cases.CASES[name], cases.schedule(name)
    _dirty_workspace()

    class scripted(sghmc):
        def _schedule(self, n_steps, eps, rng, P):
            assert n_steps == cases.N_STEPS and P == c["D"] * c["K"] + c["K"]
            return sc["n_iter"].copy(), sc["u"].copy(), sc["noise"].copy(), sc["noise_off"].copy()

    start = {"weights": np.zeros((c["D"], c["K"])), "bias": np.zeros(c["K"])}
    g = scripted(softmax({"alpha": cases.ALPHA}, dtype=dtype, device="cuda:0"), start, path_length=1.0,
                 step_size=c["eps"], noise="numpy", chains=c["C"])
    g.out = io.StringIO()
    g.record_steps = True
    data = g._upload_data(sc["X"].copy(), sc["Y"].copy())         # the shared arrays are read-only
    st = g._init_state()
    res = g._run(st, data, sc["rows"], [c["eps"]] * cases.N_STEPS, None, c["B"])
    fin = g._state_to_host(st)
    final = np.concatenate([fin["weights"].reshape(c["C"], -1), fin["bias"].reshape(c["C"], -1)], axis=1)
    return res, final


def _plans(name, **knobs):
    """Launch plan of every (step, iteration) of the case on this device."""
    c = cases.CASES[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return [[nat.sghmc_batch_plan(c["B"], c["D"], c["K"], c["C"], ca, cus, **knobs) for ca in step]
            for step in cases.c_act(name)]


def _check_f64(name, res, final):
    c, sc, ref = cases.CASES[name], cases.schedule(name), cases.reference(name)
    pr, ni = sc["proto"], sc["n_iter"]
    delta = cases.reject_delta(name)
    steps = res.steps.astype(np.float64)
    prev = np.zeros_like(steps[0])
    for s in range(cases.N_STEPS):
        acc_r = ref["accepted"][s, pr]
        np.testing.assert_array_equal(res.accepted[s], acc_r, err_msg="%s step %d flags" % (name, s))
        still = ni[s] == 0
        assert np.all(res.accepted[s][still])
        np.testing.assert_array_equal(steps[s][still], prev[still])
        np.testing.assert_array_equal(steps[s][~acc_r], prev[~acc_r])          # a rejected chain keeps its bits
        np.testing.assert_allclose(steps[s], ref["states"][s, pr], rtol=1e-9, atol=1e-12,
                                   err_msg="%s step %d states" % (name, s))
        np.testing.assert_allclose(res.A[s], ref["A"][s, pr], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(res.ll[s], ref["ll"][s, pr], rtol=1e-10)
        E_r = ref["E"][s, pr]
        np.testing.assert_allclose(res.E[s, :, 0], E_r[:, 0], rtol=1e-10, atol=1e-9)
        np.testing.assert_allclose(res.E[s, acc_r, 1], E_r[acc_r, 1], rtol=1e-10, atol=1e-9)
        rej = ~acc_r
        tol = np.maximum(1e-9 + 1e-10 * np.abs(E_r[rej, 1]), 16 * delta * np.abs(E_r[rej, 1]))
        err = np.abs(res.E[s, rej, 1] - E_r[rej, 1])
        w = int(np.argmax(err / tol)) if err.size else 0
        assert np.all(err <= tol), "%s step %d E_new of rejected trajectories: |err| %.3e, allowed %.3e" % (
            name, s, err[w], tol[w])
        prev = steps[s]
    np.testing.assert_array_equal(final, steps[-1])                              # the closing commit


def _check_f32(name, res):
    sc, ref = cases.schedule(name), cases.reference(name)
    d, scale = cases.f32_distance(name)
    pr = sc["proto"]
    for s in range(cases.N_STEPS):
        np.testing.assert_array_equal(res.accepted[s], ref["accepted"][s, pr])
        tol = max(16 * d[s], 1e-5 * scale[s])
        err = float(np.max(np.abs(res.steps[s].astype(np.float64) - ref["states"][s, pr])))
        print("%s float32 step %d: max |dev - ref64| %.3e, allowed %.3e (16 d = %.3e)" % (name, s, err, tol, 16 * d[s]))
        assert err <= tol, (name, s, err, tol)


def test_s1_partial_tiles_small_kernels_f64():
    cases.check_conditions("S1")
    pl = _plans("S1")
    assert all(p["batched"] and not p["big"] and p["fwd_rows"] == 32 and not p["wide"] for st in pl for p in st)
    assert {p["nCT"] for p in pl[0]} == {3, 2, 1}
    _check_f64("S1", *_run_device("S1", torch.float64))


def test_s1_partial_tiles_small_kernels_f32():
    cases.check_conditions("S1")
    _check_f32("S1", _run_device("S1", torch.float32)[0])


def _assert_s2_plan(pl, tail32):
    for st in pl:
        for p in st:
            assert p["batched"] and p["big"] and p["fwd_tail"] and not p["wide"]
            assert p["nRB"] == 4                               # 2 x 64-row tiles; 32-row tiles fill 3
            if tail32:
                assert (p["fwd_rows"], p["fwd_waves"], p["fwd_nX"]) == (32, 4, 3)
            else:
                assert (p["fwd_rows"], p["fwd_waves"], p["fwd_nX"]) == (64, 8, 2)
    assert any(p["nCT"] * 16 != ca for p, ca in zip(pl[0], cases.c_act("S2")[0]))       # partial chain tiles


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_s2_tail_forward_32_row_tiles(dtype, monkeypatch):
    monkeypatch.delenv("HMCX_BTAIL32", raising=False)
    cases.check_conditions("S2")
    _assert_s2_plan(_plans("S2"), True)
    res, final = _run_device("S2", getattr(torch, dtype))
    if dtype == "float64":
        _check_f64("S2", res, final)
    else:
        _check_f32("S2", res)


def test_s2_tail_forward_8_wave_kernel(monkeypatch):
    """HMCX_BTAIL32=0 (read per call): the tail forwards run k_bfwd<T,2,1,8>."""
    monkeypatch.setenv("HMCX_BTAIL32", "0")
    cases.check_conditions("S2")
    _assert_s2_plan(_plans("S2", tail32=0), False)
    _check_f64("S2", *_run_device("S2", torch.float64))


def test_s3_kernel_switches_inside_one_trajectory(monkeypatch):
    monkeypatch.delenv("HMCX_BTAIL32", raising=False)
    cases.check_conditions("S3")
    ni = cases.schedule("S3")["n_iter"]
    for st, plans in enumerate(_plans("S3")):
        assert all(p["batched"] and p["big"] and p["nRB"] == 16 and p["nDB"] == 31 for p in plans)
        full = [it for it, p in enumerate(plans) if (p["fwd_rows"], p["fwd_waves"], p["fwd_tail"]) == (64, 4, 0)]
        tail = [it for it, p in enumerate(plans) if (p["fwd_rows"], p["fwd_tail"], p["fwd_nX"]) == (32, 1, 15)]
        wide = [it for it, p in enumerate(plans) if p["wide"] and p["tail_last"] and p["grad_nX"] == 16]
        narrow = [it for it, p in enumerate(plans) if not p["wide"] and p["grad_nX"] == 31]
        assert full and tail and wide and narrow and len(full) + len(tail) == len(plans) == len(wide) + len(narrow)
        # the longest trajectories pass through every kernel; a tail forward feeds a k_bgradw launch
        assert max(full) < min(tail) and max(wide) < min(narrow) and set(tail) & set(wide)
        # chains end their trajectories (kin_part, ll_part written) under both gradient kernels
        assert any(np.any(ni[st] == it + 1) for it in wide) and any(np.any(ni[st] == it + 1) for it in narrow)
    _check_f64("S3", *_run_device("S3", torch.float64))


@pytest.mark.parametrize("name", ["S4a", "S4b", "S4c"])
def test_s4_kernel_per_phase_path_same_schedule(name):
    """C < 16, K != 10 and odd D fall out of the batched path: one k_fwd + one k_grad per iteration."""
    cases.check_conditions(name)
    c = cases.CASES[name]
    assert not nat.sghmc_batch_plan(c["B"], c["D"], c["K"], c["C"], c["C"], 256)["batched"]
    _check_f64(name, *_run_device(name, torch.float64))
