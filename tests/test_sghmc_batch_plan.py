"""Host side of the chain-batched SGHMC launcher (csrc/hmcx_batch.h plan_batch_iter through
hmcx_sghmc_batch_plan_query — host arithmetic only, no device), pinned at the shapes of the compaction
tests (tests/_sghmc_cases.py, tests/test_gpu_chain_compaction.py) for a 256-CU device; and the
preconditions of those tests' schedules, which need only the CPU reference."""
import pytest

import _sghmc_cases as cases
from dropout_hamiltonian_montecarlo_amd import _native as nat


def _plan(name, c_act, num_cus=256, **knobs):
    c = cases.CASES[name]
    return nat.sghmc_batch_plan(c["B"], c["D"], c["K"], c["C"], c_act, num_cus, **knobs)


def _launch(p):
    return (p["fwd_rows"], p["fwd_waves"], p["fwd_tail"], p["fwd_nX"], p["nCT"], p["wide"], p["tail_last"], p["grad_nX"])


def test_s1_small_kernels_and_partial_chain_tiles():
    assert cases.c_act("S1")[0] == [35, 30, 20, 20, 15, 15, 15, 15, 15, 10, 5, 5]
    for ca, nct in ((35, 3), (30, 2), (20, 2), (15, 1), (5, 1)):
        p = _plan("S1", ca)
        assert (p["batched"], p["big"], p["nRB"], p["nDB"]) == (1, 0, 2, 2)
        assert _launch(p) == (32, 4, 0, 2, nct, 0, 0, 2)


def test_s2_every_iteration_on_the_tail_forward():
    assert cases.c_act("S2")[0] == [495, 341] + [187] * 7 + [99, 44]
    for ca in (495, 341, 187, 99, 44):
        nct = (ca + 15) // 16
        p = _plan("S2", ca)
        # nRB = 4 (two 64-row tiles) while the 32-row tail tiles fill 3: block 3 is zero-filled
        assert (p["batched"], p["big"], p["nRB"], p["nDB"]) == (1, 1, 4, 2)
        assert _launch(p) == (32, 4, 1, 3, nct, 0, 0, 2)
        assert _launch(_plan("S2", ca, tail32=0)) == (64, 8, 1, 2, nct, 0, 0, 2)
        assert _launch(_plan("S2", ca, tail32=0, bfwd8=0)) == (64, 4, 1, 2, nct, 0, 0, 2)


def test_s3_switches_kernels_inside_one_trajectory():
    assert cases.c_act("S3")[0] == [517, 506, 374, 374, 374, 374, 154]
    for ca in (517, 506, 374, 154):
        p = _plan("S3", ca)
        assert (p["batched"], p["big"], p["nRB"], p["nDB"]) == (1, 1, 16, 31)
    assert _launch(_plan("S3", 517)) == (64, 4, 0, 8, 33, 1, 1, 16)      # full forward, k_bgradw tail_last
    assert _launch(_plan("S3", 506)) == (32, 4, 1, 15, 32, 1, 1, 16)     # tail forward, still k_bgradw
    assert _launch(_plan("S3", 374)) == (32, 4, 1, 15, 24, 0, 0, 31)     # k_bgrad
    assert _launch(_plan("S3", 154)) == (32, 4, 1, 15, 10, 0, 0, 31)
    assert _launch(_plan("S3", 506, bgw_tail=0))[5:7] == (1, 0)


def test_thresholds_follow_the_cu_count_and_the_knobs():
    # tail forward: nX64 · nCT <= num_cus; k_bgradw: nDB2 · nCT >= 2 · num_cus
    assert _plan("S3", 528, num_cus=264)["fwd_tail"] == 1 and _plan("S3", 528, num_cus=263)["fwd_tail"] == 0
    assert _plan("S3", 512, num_cus=256)["wide"] == 1 and _plan("S3", 496, num_cus=256)["wide"] == 0
    assert _plan("S3", 496, num_cus=248)["wide"] == 1
    assert _plan("S3", 517, tail_wg=264)["fwd_tail"] == 1 and _plan("S3", 374, bgw_min=384)["wide"] == 1
    # D a multiple of 64, or a last tile more than half full: no tail_last
    assert nat.sghmc_batch_plan(460, 960, 10, 528, 528, 256)["tail_last"] == 0
    assert nat.sghmc_batch_plan(460, 1000, 10, 528, 528, 256)["tail_last"] == 0
    assert nat.sghmc_batch_plan(460, 784, 10, 1024, 1024, 256)["tail_last"] == 1


def test_shapes_outside_the_batched_path_and_bad_arguments():
    for name in ("S4a", "S4b", "S4c"):                                    # C < 16, K != 10, odd D
        c = cases.CASES[name]
        assert _plan(name, c["C"]) == dict.fromkeys(nat.BATCH_PLAN_FIELDS, 0)
    assert _plan("S1", 40)["batched"] == 1
    for bad in (0, 41):
        with pytest.raises(nat.HmcxError):
            _plan("S1", bad)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_schedule_preconditions(name):
    """Every moving (step, prototype) pair is decided (A >= 0.9 or <= 0.1), alike in float64, float32
    and the feature-reversed float64 reference; accept and reject each cover >= 20 % of the moving
    (step, chain) pairs; the tables hold zeros and ties."""
    share = cases.check_conditions(name)
    assert 0.2 <= share <= 0.8
    sc = cases.schedule(name)
    assert sc["n_iter"].shape == sc["u"].shape == sc["noise_off"].shape == (cases.N_STEPS, cases.CASES[name]["C"])
    assert 0.3 <= sc["u"].min() and sc["u"].max() <= 0.7
    assert cases.reject_delta(name) < 1e-13          # the docstring's claim: the project tolerance governs
