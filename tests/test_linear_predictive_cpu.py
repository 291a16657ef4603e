"""CPU checks of the linear models' posterior-predictive reference (tests/_linear_predictive_ref.py): the gap
preconditions the GPU tests' exact comparisons rest on, asserted on the oracle alone (this file is the
authority for the cases' seeds), the reference's internal identities, and the Python twins of the fused
kernel's eligibility rule and of the path-0 selection rule at their bounds.  Then the launch plans: the twins of
the host launch logic at their bounds, that LAUNCH_CASES reach every branch of the inventory whatever the device's
size, and that each branch's emulated defect moves an output of the covering case by 8 tolerances.  Last the
saturated problems: band populations, gaps and the conditioning of the reference itself."""
import numpy as np
import pytest

import _linear_predictive_ref as lr
from oracle import models as om

ALL = lr.CASES + [lr.LDS_EDGE]


@pytest.mark.parametrize("c", ALL, ids=lr.case_id)
@pytest.mark.parametrize("dropout", [True, False], ids=["fixed", "off"])
def test_reference_gaps(c, dropout):
    """No decision of the reference hangs on rounding: every argmax of `mean` and of a draw's logits (logistic:
    every mean and every draw's probability against 0.5) is decided by more than GAP64 in float64 and by more
    than GAP32 at float32-rounded inputs."""
    r64, r32 = lr.case_ref(c, dropout), lr.case_ref(c, dropout, True)
    assert r64.mean_gap > lr.GAP64 and r64.draw_gap > lr.GAP64, (r64.mean_gap, r64.draw_gap)
    assert r32.mean_gap > lr.GAP32 and r32.draw_gap > lr.GAP32, (r32.mean_gap, r32.draw_gap)
    np.testing.assert_array_equal(r64.pred, r32.pred)
    np.testing.assert_array_equal(r64.draw_correct, r32.draw_correct)


@pytest.mark.parametrize("c", ALL, ids=lr.case_id)
def test_reference_identities(c):
    N, D, K, S, T = c.shape
    r = lr.case_ref(c)
    classes = 2 if c.model == 'logistic' else K
    assert r.mean.shape == (N, K) and r.pred.shape == (N,)
    assert r.draw_nll.shape == (S * T,) and r.draw_correct.shape == (S * T,)
    if c.model == 'softmax':
        np.testing.assert_allclose(r.mean.sum(axis=1), 1.0, rtol=1e-12)
    else:
        assert np.all((r.mean > 0) & (r.mean < 1))
    assert r.mutual_information.min() >= -1e-12
    assert r.entropy.max() <= np.log(classes) + 1e-12 and r.expected_entropy.min() >= 0
    assert np.all(r.lppd <= 0) and np.all(r.draw_nll >= 0)
    assert np.all((0 <= r.draw_correct) & (r.draw_correct <= N))


@pytest.mark.parametrize("c", [c for c in lr.CASES if c.shape[0] >= 2], ids=lr.case_id)
def test_single_draw_is_predict(c):
    """S = T = 1 without masks is the oracle's predict(prob=True) (logistic: its net, every row)."""
    pb = lr.problem(c)
    N = c.shape[0]
    r = lr.predictive_ref(c.model, pb.W[:1], pb.b[:1], pb.X, pb.y)
    par = {'weights': pb.W[0], 'bias': pb.b[0]}
    if c.model == 'logistic':
        want = om.logistic({"alpha": 1.0}).predict(par, pb.X, prob=True, batchsize=N)
        np.testing.assert_array_equal(r.mean.reshape(-1), want)
        np.testing.assert_array_equal(r.pred, om.logistic({"alpha": 1.0}).predict(par, pb.X, batchsize=N))
    else:
        np.testing.assert_array_equal(r.mean, om.softmax({"alpha": 1.0}).predict(par, pb.X, prob=True))
        np.testing.assert_array_equal(r.pred, om.softmax({"alpha": 1.0}).predict(par, pb.X))
    assert np.abs(r.mutual_information).max() <= 1e-12         # one draw: the mean is the draw


def test_fused_eligibility_bounds():
    # K: one MFMA tile
    assert lr.fused_eligible(24, 16, 8) and not lr.fused_eligible(24, 17, 8)
    assert lr.fused_eligible(1, 1, 4) and not lr.fused_eligible(24, 0, 4)
    # LDS: 16 rows of X (D rounded up to 16, one 16-byte pad per row) + 4 logit tiles + row partials <= 160 KiB
    for elt, last in ((8, 944), (4, 2144)):
        assert lr.fused_eligible(last, 10, elt) and not lr.fused_eligible(last + 1, 10, elt)
        assert lr.first_ineligible_D(3, elt) == last + 1
    assert lr.LDS_EDGE.shape == (5, 945, 3, 2, 1)
    assert lr.fused_eligible(784, 10, 8) and lr.fused_eligible(2048, 16, 4) and not lr.fused_eligible(2048, 16, 8)
    flags = [lr.eligible(c) for c in lr.CASES]
    assert flags == [True, True, True, True, True, False, True, True, True]


def test_path0_rule_twin():
    # the headline shapes: N = 10 000, D = 784, K = 10 (6 sets per unit)
    assert lr.path0_is_fused(10000, 784, 10, 4, 64, 1, False) and lr.path0_is_fused(10000, 784, 10, 8, 1000, 1, False)
    assert not lr.path0_is_fused(10000, 784, 10, 4, 8, 1, False)          # 2 units
    assert not lr.path0_is_fused(1000, 784, 10, 4, 64, 1, False)          # 63 x 11 pairs
    assert lr.path0_is_fused(2500, 784, 10, 4, 64, 1, False) and lr.path0_is_fused(1000, 784, 10, 4, 1000, 1, False)
    # the bounds: 4 units and 1536 pairs; K = 16 has 4 sets per unit
    assert lr.path0_is_fused(6144, 8, 16, 4, 16, 1, False)
    assert not lr.path0_is_fused(6128, 8, 16, 4, 16, 1, False) and not lr.path0_is_fused(8192, 8, 16, 4, 12, 1, False)
    # ... or 200 parameter sets (still 4 units: K = 1 packs 64 sets per unit)
    assert lr.path0_is_fused(32, 8, 16, 4, 200, 1, False) and not lr.path0_is_fused(32, 8, 16, 4, 199, 1, False)
    assert lr.path0_is_fused(256, 32, 1, 8, 1000, 1, False) and not lr.path0_is_fused(256, 32, 1, 8, 192, 1, False)
    # input dropout: 32 draws
    assert lr.path0_is_fused(16, 784, 10, 4, 2, 16, True) and not lr.path0_is_fused(16, 784, 10, 4, 1, 31, True)
    # never on an ineligible shape
    assert not lr.path0_is_fused(10000, 24, 38, 8, 1000, 1, False) and not lr.path0_is_fused(10000, 945, 3, 8, 1000, 1, False)
    assert not lr.path0_is_fused(10000, 24, 38, 8, 64, 16, True)


# ----------------------------------------------------------------------------- launch plans and their cases
LIDS = [lr.case_id(c) for c in lr.LAUNCH_CASES]


def test_fused_plan_twin():
    """fused_plan against lin_predictive_t's fused arm and lpred_groups, read side by side."""
    P = lr.FusedPlan
    # one unit, one group; upg <= 4 is not rounded: 3 units on 3 groups of 1
    assert lr.fused_plan(1, 1, 2, 1, 1, False, 256) == P(1, 32, 1, 1, 1, 1, 1, 1, 3)
    assert lr.fused_plan(20, 16, 10, 14, 1, False, 256)[3:7] == (3, 3, 1, 1)
    # 128 units are 32 groups of 4 and one round; the 129th makes upg = 5 -> 8, 17 groups, two rounds
    assert lr.fused_plan(20, 16, 16, 512, 1, False, 256)[3:] == (128, 32, 4, 1, 4, 0)
    assert lr.fused_plan(20, 16, 16, 513, 1, False, 256)[3:] == (129, 17, 8, 2, 1, 4)
    # the shapes DESIGN §12 quotes: 133, 134, 172 and 136 units
    assert lr.fused_plan(20, 16, 16, 530, 1, False, 1024)[3:] == (133, 17, 8, 2, 5, 3)
    assert lr.fused_plan(20, 16, 10, 800, 1, False, 1024)[1:] == (6, 1, 134, 17, 8, 2, 6, 2)
    assert lr.fused_plan(19, 13, 1, 43, 14, True, 1024)[2:] == (4, 172, 22, 8, 2, 4, 4)
    assert lr.fused_plan(35, 24, 3, 34, 15, True, 1024)[2:] == (4, 136, 17, 8, 2, 8, 0)
    # lpred_groups: the fewest groups that fill 90 % of the rounds they occupy, else the best filling
    assert lr.lpred_groups(231, 40, 256) == 1 and lr.lpred_groups(230, 40, 256) == 10     # 230 / 256 < 0.9
    assert lr.lpred_groups(625, 167, 1024) == 3 and lr.lpred_groups(2, 5, 256) == 5 and lr.lpred_groups(2, 99, 256) == 32
    # units in order: (group, round, draws)
    u = lr.fused_unit_draws(19, 13, 1, 43, 14, True, 256)
    assert u[3] == (0, 0, [12, 13]) and u[4] == (0, 1, [14, 15, 16, 17]) and u[8] == (1, 0, [28, 29, 30, 31])
    u = lr.fused_unit_draws(3, 16, 16, 530, 1, False, 256)
    assert u[-1] == (16, 1, [528, 529]) and u[-2] == (16, 0, [524, 525, 526, 527]) and len(u) == 133


def test_general_plan_twin():
    P = lr.GeneralPlan
    assert lr.general_plan(270, 1, 71, 1, False, 4) == P(5, 64, 2, 7, 2, 1)
    assert lr.general_plan(64, 3, 64, 1, False, 8) == P(1, 64, 1, 64, 1, 1)
    assert lr.general_plan(65, 3, 128, 1, False, 8) == P(2, 64, 2, 64, 1, 1)
    assert lr.general_plan(35, 3, 34, 15, True, 8) == P(1, 1, 510, 1, 1, 2)           # dropout: a chunk is a draw
    assert lr.general_plan(256, 3, 3, 1, False, 8) == P(4, 3, 1, 3, 1, 1)             # no more than S
    # the chunk buffer [N][CH·K] stays within 64 MiB: CH drops below 64 once N·K·elt passes 1 MiB
    assert lr.general_plan(262144, 1, 100, 1, False, 4).CH == 64 and lr.general_plan(262145, 1, 100, 1, False, 4).CH == 63
    assert lr.general_plan(131072, 1, 100, 1, False, 8).CH == 64 and lr.general_plan(131073, 1, 100, 1, False, 8).CH == 63
    assert lr.general_plan(1 << 20, 16, 100, 1, False, 8).CH == 1 and lr.general_plan(1 << 21, 64, 9, 1, False, 8).CH == 1


def test_launch_cases_reach_every_branch():
    hit = {item: [i for i, c in zip(LIDS, lr.LAUNCH_CASES) if item in lr.reaches(c)] for item in lr.INVENTORY}
    for item, v in hit.items():
        print("%-85s %s" % (item, ", ".join(v)))
    assert all(hit.values()), "no case reaches: " + "; ".join(k for k, v in hit.items() if not v)
    assert all(lr.reaches(c) for c in lr.LAUNCH_CASES)                 # no case without a reason
    assert set(lr.INVENTORY.values()) == set(lr.DEFECTS)


@pytest.mark.parametrize("c", lr.LAUNCH_CASES, ids=LIDS)
def test_launch_plan_does_not_depend_on_the_device(c):
    """Resident workgroups (compute units x occupancy) are known only on the device: the case's fused plan, and so
    what it reaches, is the same for every count from 256 to 2048."""
    N, D, K, S, _ = c.shape
    assert lr.eligible(c, 8) and lr.eligible(c, 4)                     # every launch case runs on both paths
    plans = {lr.fused_plan(N, D, K, S, lr.launch_T(c), c.dropout, s) for s in lr.SLOTS}
    assert len(plans) == 1
    p = plans.pop()
    # few row blocks: the 90 % rule cannot fire and the best filling is the largest count
    assert p.nrb * min(p.nunits, lr.LF_MAXG) < 0.9 * min(lr.SLOTS)
    assert all(lr.lpred_groups(p.nrb, p.nunits, s) == min(p.nunits, lr.LF_MAXG) for s in lr.SLOTS)
    assert len({frozenset(lr.reaches(c, s)) for s in lr.SLOTS}) == 1


@pytest.mark.parametrize("c", lr.LAUNCH_CASES, ids=LIDS)
def test_launch_case_reference_gaps(c):
    """test_reference_gaps for a launch case, in the mode it is run in."""
    r64, r32 = lr.case_ref(c, c.dropout), lr.case_ref(c, c.dropout, True)
    assert r64.mean_gap > lr.GAP64 and r64.draw_gap > lr.GAP64, (r64.mean_gap, r64.draw_gap)
    assert r32.mean_gap > lr.GAP32 and r32.draw_gap > lr.GAP32, (r32.mean_gap, r32.draw_gap)
    np.testing.assert_array_equal(r64.pred, r32.pred)
    np.testing.assert_array_equal(r64.draw_correct, r32.draw_correct)
    assert len(set(r64.draw_correct.tolist())) > 1                     # draw_accuracy is not one constant


@pytest.mark.parametrize("c", lr.LAUNCH_CASES, ids=LIDS)
def test_emulation_without_defect_is_the_reference(c):
    ref, own = lr.case_ref(c, c.dropout), lr.emulated(c)
    for name in lr.ROW_OUTPUTS + lr.DRAW_OUTPUTS:
        np.testing.assert_allclose(own[name], getattr(ref, name), rtol=1e-12, atol=1e-14, err_msg=name)


@pytest.mark.parametrize("c,item", [pytest.param(c, item, id="%s-%s" % (i, lr.INVENTORY[item]))
                                    for i, c in zip(LIDS, lr.LAUNCH_CASES) for item in lr.INVENTORY
                                    if item in lr.reaches(c)])
def test_every_defect_moves_an_output_by_8_tolerances(c, item):
    """A case covers a branch only if it would see the branch's defect: at least one of the outputs the defect
    touches moves by 8 times the GPU test's float32 bound (its loosest; the float64 bounds are far inside it)."""
    defect = lr.INVENTORY[item]
    ref, mu = lr.case_ref(c, c.dropout, True), lr.emulated(c, defect)
    base = lr.emulated(c)
    moved = {o: float(np.abs(mu[o] - base[o]).max() / lr.tol32(ref, o)) for o in lr.DEFECTS[defect]}
    print("%s %s: %s" % (lr.case_id(c), defect, {o: "%.3g" % v for o, v in moved.items()}))
    assert max(moved.values()) >= 8, moved


# ----------------------------------------------------------------------------- saturated logits
SAT = [(c, d) for c in lr.SAT_CASES for d in (True, False)]
SAT_IDS = ["%s-%s" % (lr.sat_id(c), "fixed" if d else "off") for c, d in SAT]


def _spread(mask):
    """(distinct rows, row blocks, draws) of the True entries of mask [draws, N]."""
    d, n = np.nonzero(mask)
    return len(set(n)), len(set(n // 16)), len(set(d))


@pytest.mark.parametrize("c,dropout", SAT, ids=SAT_IDS)
def test_saturated_band_populations(c, dropout):
    """Every required band x label combination holds at least 4 rows, in more than one row block and more than
    one draw; every logit is in a stated band, the logistic ones never in 26 < |z| < 37 (float64 problems: never
    in 12 < |z| < 37), and at float32-rounded inputs each logit is in the same band."""
    N, _, K, S, T = c.shape
    assert N >= 33 and S * (T if dropout else 1) >= 6
    pb = lr.sat_problem(c)
    z, zr = lr.sat_logits(c, dropout), lr.sat_logits(c, dropout, True)
    y = pb.y[None, :]
    hi, lo, mid = z >= lr.BAND_C, z <= -lr.BAND_C, np.abs(z) <= lr.BAND_O
    f = (z >= lr.BAND_F[0]) & (z <= lr.BAND_F[1])
    fneg = (z <= -lr.BAND_F[0]) & (z >= -lr.BAND_F[1])                 # the driven-down side of an F row: harmless
    for a, b in ((hi, zr >= lr.BAND_C), (lo, zr <= -lr.BAND_C), (mid, np.abs(zr) <= lr.BAND_O)):
        np.testing.assert_array_equal(a, b)
    if c.bandF:
        assert np.all(hi | lo | mid | f | fneg)
    else:
        assert np.all(hi | lo | mid)
    assert z.max() < 60 and z.min() > -60
    if c.model == 'logistic':
        assert not np.any((np.abs(z) > 26) & (np.abs(z) < lr.BAND_C))
        z1 = z[..., 0]
        combos = {"C+ y=1": (z1 >= lr.BAND_C) & (y == 1), "C+ y=0": (z1 >= lr.BAND_C) & (y == 0),
                  "C- y=1": (z1 <= -lr.BAND_C) & (y == 1), "C- y=0": (z1 <= -lr.BAND_C) & (y == 0),
                  "O y=1": (np.abs(z1) <= lr.BAND_O) & (y == 1), "O y=0": (np.abs(z1) <= lr.BAND_O) & (y == 0)}
        if c.bandF:
            combos["F y=1"], combos["F y=0"] = f[..., 0] & (y == 1), f[..., 0] & (y == 0)
    else:
        assert (z >= lr.BAND_C).sum(axis=-1).max() == 1                # never two classes at the upper clip
        zy = np.take_along_axis(z, np.broadcast_to(y, z.shape[:2])[..., None], axis=-1)[..., 0]
        top = z.max(axis=-1)
        combos = {"C+ label": zy >= lr.BAND_C, "C+ other": (top >= lr.BAND_C) & (zy < lr.BAND_C),
                  "C- label": zy <= -lr.BAND_C, "C- other": (z.min(axis=-1) <= -lr.BAND_C) & (zy > -lr.BAND_C),
                  "O": np.abs(z).max(axis=-1) <= lr.BAND_O}
        if c.bandF:
            combos["F label"] = (zy >= lr.BAND_F[0]) & (zy <= lr.BAND_F[1])
            combos["F other"] = (top >= lr.BAND_F[0]) & (top <= lr.BAND_F[1]) & (zy < lr.BAND_F[0])
        # the float32 general path takes −log of a float32 probability: the logit spread stays inside exp's
        # float32 range (e^−87.3 is the smallest normal float32)
        assert (np.minimum(z, om.CLIP_HI).max(axis=-1) - z.min(axis=-1)).max() < 86
    for name, m in combos.items():
        rows, blocks, draws = _spread(m)
        print("%-10s rows %2d blocks %d draws %2d" % (name, rows, blocks, draws))
        assert rows >= 4 and blocks >= 2 and draws >= 2, (name, rows, blocks, draws)
    ref = lr.sat_ref(c, dropout)
    if c.model == 'logistic':                                          # the reference prices the rows as stated
        assert ref.draw_nll.max() * N > om.CLIP_HI


@pytest.mark.parametrize("c,dropout", SAT, ids=SAT_IDS)
def test_saturated_reference_gaps(c, dropout):
    r64, r32 = lr.sat_ref(c, dropout), lr.sat_ref(c, dropout, True)
    assert r64.mean_gap > lr.GAP64 and r64.draw_gap > lr.GAP64, (r64.mean_gap, r64.draw_gap)
    assert r32.mean_gap > lr.GAP32 and r32.draw_gap > lr.GAP32, (r32.mean_gap, r32.draw_gap)
    np.testing.assert_array_equal(r64.pred, r32.pred)
    np.testing.assert_array_equal(r64.draw_correct, r32.draw_correct)
    for r in (r64, r32):
        assert all(np.all(np.isfinite(getattr(r, k))) for k in ("mean", "entropy", "expected_entropy", "lppd", "draw_nll"))


@pytest.mark.parametrize("c,dropout", [(c, d) for c, d in SAT if c.model == 'logistic'],
                         ids=[i for i, (c, d) in zip(SAT_IDS, SAT) if c.model == 'logistic'])
def test_saturated_logistic_reference_is_well_conditioned(c, dropout):
    """The reference's log(1 − p) moves by 2⁻⁵³·p / (1 − p) = 2⁻⁵³·e^z when p moves by one ulp.  Summed into every
    compared quantity over the unclipped entries (a clipped logit has the same bits on both sides, so p and
    1 − p = 2⁻⁵² are exact), that stays below a tenth of the tolerance the GPU test applies: the float64
    tolerances for the O + C problems, 2e-4 of the largest entry for the float32 ones."""
    N = c.shape[0]
    pb, ref = lr.sat_problem(c, c.bandF), lr.sat_ref(c, dropout, c.bandF)
    z = lr.sat_logits(c, dropout, c.bandF)[..., 0]                      # [draws, N]
    DR = z.shape[0]
    free = z < om.CLIP_HI
    p = 1.0 / (1.0 + np.exp(-np.minimum(z, om.CLIP_HI)))
    u = 2.0 ** -53
    dq = np.where(free, u * p, 0.0)                                    # |Δ(1 − p)| = |Δp|
    dlogq = dq / (1.0 - p)
    y0 = (pb.y == 0)[None, :]
    amp = {
        "draw_nll": (np.where(y0, dlogq, u)).sum(axis=1) / N,
        "lppd": (np.where(y0, dq, u * p)).sum(axis=0) / DR / np.exp(ref.lppd),
        "expected_entropy": (dq * (np.abs(np.log(1.0 - p)) + np.abs(np.log(p)) + 2.0)).sum(axis=0) / DR,
        "mean": dq.sum(axis=0) / DR + u,
    }
    pm = ref.mean[:, 0]
    amp["entropy"] = amp["mean"] * (np.abs(np.log(pm)) + np.abs(np.log(1.0 - pm)) + 2.0)
    for name, a in amp.items():
        want = np.asarray(getattr(ref, name)).reshape(a.shape)
        if c.bandF:
            tol = np.full(a.shape, 2e-4 * np.abs(want).max())
        else:
            rtol, atol = (1e-11, 1e-14) if name in ("mean", "draw_nll") else (1e-10, 1e-12)
            tol = rtol * np.abs(want) + atol
        worst = float((a / tol).max())
        print("%-17s amplification / tolerance %.3g" % (name, worst))
        assert worst < 0.1, (name, worst)
