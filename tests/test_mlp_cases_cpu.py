"""The dropout-MLP kernel cases of tests/_mlp_cases.py, checked on the CPU (no GPU): the table reaches every
launch branch of the inventory (REQUIRED) in every dtype the branch exists in, the restated backward pass is
the oracle's, and each defect a kernel could have (MUTATIONS) moves at least one compared output of every case
it applies to by at least 8 tolerances, in both dtypes' tolerances — the figure the linear cases use.  A seed
that stops meeting the condition is searched again; the condition stays."""
import numpy as np
import pytest

import _mlp_cases as mc

IDS = [mc.case_id(c) for c in mc.CASES]


def test_case_table_reaches_every_launch_branch():
    hit = mc.coverage()
    missing = ["%s (%s)" % k for k, v in hit.items() if not v]
    for (label, d), v in hit.items():
        print("%-60s %-8s %s" % (label, d, ", ".join(v)))
    assert not missing, "no case reaches: " + "; ".join(missing)


def test_mirror_on_known_launches():
    """The mirror against facts stated in csrc/hmcx_mlp.hip (xcd_choose), csrc/hmcx_mlp_kernels.h (l3_backward)
    and DESIGN 5.3 for config 3 (784-256-256-10, B = 500, float32): the W1 gradient's 8 x 25 tile plane takes
    the y-major chunks, 6880 = the largest n_out·n_mid with W3 staged in LDS, float64 never leaves the dispatch
    order."""
    g = {s["name"]: s for s in mc.launches(500, 784, 256, 10, "float32")}
    assert g["gW1"]["tiles"] == (8, 25) and g["gW1"]["xmap"] == 1
    assert g["layer1"]["Kq"] == 112 and g["layer2"]["Kq"] == 32 and g["gW2"]["Kq"] == 64
    assert all(s["xmap"] == 0 for s in mc.launches(500, 784, 256, 10, "float64"))
    assert mc.layer3("float32", 32, 215, 32, True)["wl"] and not mc.layer3("float32", 32, 216, 32, True)["wl"]
    assert mc.layer3("float32", 32, 256, 33, True)["kind"] == "wide"
    assert mc.l3_rows(512, 600) == (1, 16, 2) and mc.l3_rows(512, 37) == (13, 2, 1)


def test_cases_state_what_they_reach():
    """Every case's own reason, spot-checked against the mirror (the coverage test is the authority)."""
    by = {mc.case_id(c): c for c in mc.CASES}
    s = {x["name"]: x for x in mc.case_launches(by["100-100-128-5"], "float32")}
    assert all(s[k]["xmap"] == 2 for k in ("layer1", "gW1", "gW2")) and s["layer1"]["ragged_m"] and s["gW1"]["ragged_n"]
    s = {x["name"]: x for x in mc.case_launches(by["8-520-256-3"], "float32")}
    assert s["gW1"]["xmap"] == 1 and s["gW1"]["ragged_n"] and s["layer1"]["Kq"] == 80
    s = {x["name"]: x for x in mc.case_launches(by["33-24-64-12-off1"], "float32")}
    assert not s["layer2"]["av"] and s["layer2"]["bv"] and s["layer1"]["av"]
    s = {x["name"]: x for x in mc.case_launches(by["21-30-38-3"], "float64")}
    assert not s["layer2"]["av"] and s["layer2"]["bv"]


@pytest.mark.parametrize("i", range(len(mc.CASES)), ids=IDS)
def test_restated_backward_is_the_oracles(i):
    """``outputs`` with an identity edit (its own backward pass) against oracle.models.mlp.grad."""
    ref = mc.reference(i, "float32")
    own = mc.outputs(mc.problem(i, "float32"), z_edit=lambda z: z)
    for o in mc.OUTPUTS:
        np.testing.assert_allclose(own[o], ref[o], rtol=1e-13, atol=1e-16)
    assert all(np.all(np.asarray(b) > 0) for b in mc.bounds(i, "float32").values())


@pytest.mark.parametrize("i,mutation", [pytest.param(i, m, id="%s-%s" % (IDS[i], m)) for i in range(len(mc.CASES))
                                        for m in mc.MUTATIONS if mc.applies(i, m)])
def test_every_defect_moves_an_output_by_8_tolerances(i, mutation):
    ref = mc.reference(i, "float32")
    mu = mc.mutated(i, mutation)
    for dtype in mc.CASES[i]["dtypes"]:
        tol = mc.tolerances(i, dtype, ref)
        moved = {o: float(np.max(np.abs(np.asarray(mu[o]) - np.asarray(ref[o])) / tol[o])) for o in mc.OUTPUTS}
        print("%s %s %s: %s" % (IDS[i], dtype, mutation, {o: "%.3g" % v for o, v in moved.items()}))
        assert max(moved.values()) >= 8, (dtype, moved)
        if mutation.startswith("tile"):                     # the exchanged tiles themselves
            assert moved["g" + mutation[4:]] >= 8, (dtype, moved)


def test_every_mutation_applies_somewhere():
    for m in mc.MUTATIONS:
        assert any(mc.applies(i, m) for i in range(len(mc.CASES))), m


def test_float32_tolerance_never_looser_than_the_projects():
    for i, c in enumerate(mc.CASES):
        if "float32" not in c["dtypes"]:
            continue
        ref, tol = mc.reference(i, "float32"), mc.tolerances(i, "float32")
        for o in mc.OUTPUTS:
            assert np.all(tol[o] <= mc.F32_CAP * np.max(np.abs(ref[o])) * (1 + 1e-12)), (IDS[i], o)
