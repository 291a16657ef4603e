"""Float64 reference of the linear models' posterior predictive (hmcx_linear_predictive /
softmax.posterior_predictive, logistic.posterior_predictive): oracle.models.softmax.net and
oracle.models.logistic.net per draw plus NumPy, all eight quantities and the top-two gaps, and the small
problems the CPU and GPU tests share.  Draw d = s·T + t is parameter set s under input-dropout mask block d
(X ⊙ Z_d, the reference's predict_stochastic).

The seeds below are the ones for which the oracle meets the "gap" preconditions of the exact comparisons
(pred and draw_correct are only comparable when no reference decision hangs on rounding);
tests/test_linear_predictive_cpu.py asserts them on the oracle alone and is the authority: a seed that stops
meeting a condition is searched again, the condition stays.

Further down: Python twins of the host launch logic (fused_plan, general_plan), the inventory of launch branches
with the cases that reach it (LAUNCH_CASES) and the CPU emulation of each branch's defect, and the constructed
problems with saturated logits (SAT_CASES)."""
import functools
from collections import namedtuple

import numpy as np

from oracle import models as om

from _predictive_ref import GAP32, GAP64, f32r  # noqa: F401  (the same preconditions as the MLP's)

# mean_gap: smallest top-two gap of a row of `mean` (logistic: smallest |mean − 0.5|); draw_gap: the same for
# every draw's decision (softmax: the clipped logits; logistic: |p_d − 0.5|)
Ref = namedtuple("Ref", "mean pred entropy expected_entropy mutual_information lppd draw_nll draw_correct "
                        "draw_accuracy mean_gap draw_gap")


def _top2_gap(a):
    s = np.sort(a, axis=-1)
    return float((s[..., -1] - s[..., -2]).min())


def _entropy(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log(p), 0.0)
    return -t.sum(axis=-1)


def predictive_ref(model, W, b, X, y=None, masks=None, T=1):
    """model: 'softmax' or 'logistic'; W [S, D, K], b [S, K]; masks: None (no dropout, T must be 1) or
    [S·T, N, D]."""
    X = np.asarray(X, dtype=np.float64)
    W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64)
    S, N, K = W.shape[0], X.shape[0], W.shape[2]
    D = S * T
    assert masks is not None or T == 1
    logistic = model == 'logistic'
    net = om.logistic({"alpha": 1.0}) if logistic else om.softmax({"alpha": 1.0})
    t = None if y is None else np.asarray(y).astype(int)
    ps, gaps, nll, corr = [], [], [], []
    for d in range(D):
        par = {'weights': W[d // T], 'bias': b[d // T]}
        Xd = X if masks is None else np.multiply(X, np.asarray(masks[d], dtype=np.float64))
        if logistic:
            p1 = net.net(par, X_train=Xd)                              # [N, 1]
            ps.append(np.concatenate([1.0 - p1, p1], axis=1))
            gaps.append(float(np.abs(p1 - 0.5).min()))
            if t is not None:
                nll.append(-net.log_likelihood(par, X_train=Xd, y_train=t) / N)
                corr.append(int(((p1 > 0.5).astype(int).flatten() == t).sum()))
        else:
            z = net.logits(par, Xd)
            ps.append(net.net(par, Xd))
            gaps.append(_top2_gap(z))
            if t is not None:
                nll.append(-net.log_likelihood(par, X_train=Xd, y_train=om.one_hot(t, K)) / N)
                corr.append(int((z.argmax(axis=1) == t).sum()))
    p = np.stack(ps)                                                   # [D, N, classes]
    pm = p.mean(axis=0)
    ent, eent = _entropy(pm), _entropy(p).mean(axis=0)
    if logistic:
        mean, pred = pm[:, 1:], (pm[:, 1] > 0.5).astype(int)
        mean_gap = float(np.abs(pm[:, 1] - 0.5).min())
    else:
        mean, pred, mean_gap = pm, pm.argmax(axis=1), _top2_gap(pm)
    lppd = dn = dc = acc = None
    if t is not None:
        lppd = np.log(p[:, np.arange(N), t].mean(axis=0))
        dn, dc = np.array(nll), np.array(corr, dtype=np.int32)
        acc = dc / float(N)
    return Ref(mean, pred, ent, eent, ent - eent, lppd, dn, dc, acc, mean_gap, min(gaps))


# ----------------------------------------------------------------------------- eligibility and path choice
def fused_eligible(D, K, elt):
    """Python twin of hmcx_lin_pred.hip::lpred_fused_shape_ok: K within one MFMA tile, and 16 rows of X, four
    waves' 16 × 65 logit tiles and their 16 × 18 float64 row partials within 160 KiB of LDS."""
    if K < 1 or K > 16 or D < 1:
        return False
    up = lambda n: (n + 15) // 16 * 16  # noqa: E731
    xp = (D + 15) // 16 * 16 + 16 // elt
    return up(16 * xp * elt) + up(4 * 16 * 65 * elt) + up(4 * 16 * 18 * 8) <= 160 * 1024


def path0_is_fused(N, D, K, elt, S, T, dropout):
    """Python twin of hmcx_lin_pred.hip::lin_pred_path0_fused: with input dropout from 32 draws;
    without, from 4 units (of ⌊64 / K⌋ parameter sets) and either 1536 row-block × unit pairs or 200 sets."""
    if not fused_eligible(D, K, elt):
        return False
    if dropout:
        return S * T >= 32
    spu = 64 // K
    nunits, nrb = (S + spu - 1) // spu, (N + 15) // 16
    return nunits >= 4 and (nrb * nunits >= 1536 or S >= 200)


def first_ineligible_D(K, elt):
    D = 1
    while fused_eligible(D, K, elt):
        D += 1
    return D


# ----------------------------------------------------------------------------- shared problems
# model, (N, D, K, S, T), seed: float64 gaps > 1e-6 and float32-rounded gaps > 1e-3 for every decision, with
# and without dropout
Case = namedtuple("Case", "model shape seed")
CASES = [
    Case('softmax', (1, 1, 2, 1, 1), 0),         # smallest shape
    Case('softmax', (19, 50, 7, 3, 2), 0),       # nothing aligned
    Case('softmax', (35, 24, 3, 2, 20), 8),      # row blocks 16 + 16 + 3; more draws than draw groups
    Case('softmax', (20, 16, 10, 40, 1), 1856),     # many sets per column tile; K does not divide 16
    Case('softmax', (17, 40, 16, 5, 2), 32),      # K at the fused limit
    Case('softmax', (33, 24, 38, 2, 2), 33),      # K beyond the fused limit: general path only
    Case('logistic', (1, 1, 1, 1, 1), 0),        # smallest shape
    Case('logistic', (21, 13, 1, 6, 3), 14),      # dropout, more than one row block
    Case('logistic', (36, 32, 1, 33, 1), 49560),     # many sets, no dropout
]
MULTIBLOCK = {'softmax': CASES[2], 'logistic': CASES[7]}
# N = 5, S = 2 at the smallest D the float64 rule rejects: path 2 must refuse it, path 0 must serve it
LDS_EDGE = Case('softmax', (5, first_ineligible_D(3, 8), 3, 2, 1), 0)


def case_id(c):
    return c.model + "-" + "x".join(map(str, c.shape))


def eligible(c, elt=8):
    return fused_eligible(c.shape[1], c.shape[2], elt)


Problem = namedtuple("Problem", "W b X y masks")


@functools.lru_cache(maxsize=None)
def problem(c, rounded=False):
    """S parameter sets, X, labels and S·T mask blocks of a case (read-only: shared between tests).
    rounded: every input rounded through float32 (what a float32 model sees)."""
    N, D, K, S, T = c.shape
    rs = np.random.RandomState(c.seed)
    W, b = rs.normal(0, 0.3, (S, D, K)), rs.normal(0, 0.3, (S, K))
    X = rs.rand(N, D)
    y = rs.randint(0, 2 if c.model == 'logistic' else K, N)
    masks = rs.binomial(1, 0.5, (S * T, N, D)).astype(np.uint8)
    boost = getattr(c, 'boost', 0.0)                                   # launch cases (LCase) only
    if boost and c.model == 'logistic':
        b = b + boost * rs.choice([-1.0, 1.0], (S, 1))
    elif boost:
        b[np.arange(S), rs.randint(0, K, S)] += boost
    if rounded:
        W, b, X = f32r(W), f32r(b), f32r(X)
    return Problem(W, b, X, y, masks)


def posterior(pb):
    """{'weights': [S, D, K], 'bias': [S, K]} as sample() returns it."""
    return {'weights': pb.W, 'bias': pb.b}


@functools.lru_cache(maxsize=None)
def case_ref(c, dropout=True, rounded=False):
    """The reference of a case: with its S·T mask blocks, or (dropout False) of the S sets without dropout."""
    pb = problem(c, rounded)
    if dropout:
        return predictive_ref(c.model, pb.W, pb.b, pb.X, pb.y, pb.masks, c.shape[4])
    return predictive_ref(c.model, pb.W, pb.b, pb.X, pb.y, None, 1)


# ----------------------------------------------------------------------------- launch plans
# Python twins of the host code of hmcx_lin_pred.hip::lin_predictive_t.  `slots` (resident workgroups: compute
# units × occupancy) is known only on the device; every LAUNCH_CASE has few enough row blocks that its plan is
# the same for each of SLOTS (the 90 % rule of lpred_groups cannot fire, so G = min(nunits, 32)).
LF_ROWS, LF_NW, LF_NACC, LF_COLS, LF_MAXG = 16, 4, 4, 64, 32
LG_NT, LG_CHUNK, LG_CHUNK_BYTES = 64, 64, 64 << 20
SLOTS = tuple(range(256, 2049, 256))


def lpred_groups(nrb, nunits, slots):
    """hmcx_lin_pred.hip::lpred_groups."""
    best, beff = 1, 0.0
    for G in range(1, min(nunits, LF_MAXG) + 1):
        wg = nrb * G
        rounds = (wg + slots - 1) // slots
        eff = wg / float(rounds * slots)
        if eff >= 0.9:
            return G
        if eff > beff:
            beff, best = eff, G
    return best


# last_units: units of the last group; idle_last: waves without a unit in that group's last round
FusedPlan = namedtuple("FusedPlan", "nrb spu tu nunits G upg nit last_units idle_last")


def fused_plan(N, D, K, S, T, dropout, slots):
    """The fused arm of lin_predictive_t: a unit is ⌊64 / K⌋ sets (no dropout) or up to 4 masks of a set."""
    assert 1 <= K <= 16 and D >= 1
    nrb = (N + LF_ROWS - 1) // LF_ROWS
    spu, tu = LF_COLS // K, (T + LF_NACC - 1) // LF_NACC
    nunits = S * tu if dropout else (S + spu - 1) // spu
    G = lpred_groups(nrb, nunits, slots)
    upg = (nunits + G - 1) // G
    if upg > LF_NW:
        upg = (upg + LF_NW - 1) // LF_NW * LF_NW
    G = (nunits + upg - 1) // upg
    nit = (upg + LF_NW - 1) // LF_NW
    last_units = nunits - (G - 1) * upg
    idle_last = LF_NW - min(LF_NW, max(0, last_units - (nit - 1) * LF_NW))
    return FusedPlan(nrb, spu, tu, nunits, G, upg, nit, last_units, idle_last)


def fused_unit_draws(N, D, K, S, T, dropout, slots):
    """[(group, round, draws)] of every unit of the fused launch, in unit order."""
    p = fused_plan(N, D, K, S, T, dropout, slots)
    out = []
    for u in range(p.nunits):
        if dropout:
            s, t0 = u // p.tu, (u % p.tu) * LF_NACC
            draws = [s * T + t for t in range(t0, min(T, t0 + LF_NACC))]
        else:
            draws = list(range(u * p.spu, min(S, (u + 1) * p.spu)))
        out.append((u // p.upg, (u % p.upg) // LF_NW, draws))
    return out


# CH: draws per chunk; last: draws of the last chunk; finish_blocks / draws_blocks: workgroups of k_lpred_finish
# and k_lpred_draws (those two are the same on the fused path)
GeneralPlan = namedtuple("GeneralPlan", "nb CH chunks last finish_blocks draws_blocks")


def general_plan(N, K, S, T, dropout, elt):
    """The general arm of lin_predictive_t."""
    DR = S * T
    CH = 1 if dropout else max(1, min(LG_CHUNK, LG_CHUNK_BYTES // (N * K * elt), S))
    chunks = (DR + CH - 1) // CH
    return GeneralPlan((N + LG_NT - 1) // LG_NT, CH, chunks, DR - (chunks - 1) * CH, (N + 255) // 256,
                       (DR + 255) // 256)


# The launch branches the cases below must reach between them (tests/test_linear_predictive_cpu.py asserts it),
# each with the defect that branch would have: DEFECTS names the emulation and the outputs it has to move.
INVENTORY = {
    "fused: nit >= 2 without dropout, idle waves in the last round, last group shorter than upg": "rounds-dropped",
    "fused: the same with K not dividing 64": "last-group-dropped",
    "fused: nit >= 2 with dropout and T % 4 != 0": "rounds-dropped",
    "fused: S % spu != 0 (ragged last unit)": "last-unit-dropped",
    "fused: D < 16 on more than one row block (TAIL body only)": "pad-columns-live",
    "fused: D % 16 == 0 (no TAIL body)": "last-chunk-dropped",
    "general: several no-dropout chunks, the last partial": "chunk-overwrites",
    "general: N > 64, N % 64 != 0 (several k_lpred_reduce workgroups)": "rows-past-64-unsummed",
    "k_lpred_finish: N > 256": "rows-past-256-unfinished",
    "k_lpred_draws: S*T > 256": "draws-past-256-unsummed",
}
ROW_OUTPUTS = ("mean", "entropy", "expected_entropy", "lppd")
DRAW_OUTPUTS = ("draw_nll",)
# defect → the outputs of which at least one has to move by 8 tolerances
DEFECTS = {
    "rounds-dropped": ROW_OUTPUTS, "last-group-dropped": ROW_OUTPUTS, "last-unit-dropped": ROW_OUTPUTS,
    "pad-columns-live": ROW_OUTPUTS, "last-chunk-dropped": ROW_OUTPUTS, "chunk-overwrites": ROW_OUTPUTS,
    "rows-past-64-unsummed": DRAW_OUTPUTS, "rows-past-256-unfinished": ROW_OUTPUTS,
    "draws-past-256-unsummed": DRAW_OUTPUTS,
}

# dropout: the mode the case is run in; boost: added to one bias entry of every set (softmax: a class drawn per
# set; logistic: with a sign drawn per set), which keeps thousands of per-draw decisions away from a tie
LCase = namedtuple("LCase", "model shape seed dropout boost")
LAUNCH_CASES = [
    LCase('softmax', (3, 16, 16, 530, 1), 0, False, 3.0),     # 133 units: 17 groups of 8, the last of 5; D = 16
    LCase('softmax', (4, 21, 15, 530, 1), 0, False, 3.0),     # the same at K = 15 (4 idle columns per unit)
    LCase('logistic', (19, 13, 1, 43, 14), 1, True, 2.0),     # 172 units of 4 + 4 + 4 + 2 masks; D = 13, two row blocks
    LCase('softmax', (35, 24, 3, 34, 15), 2, True, 3.0),      # 136 units of 4 + 4 + 4 + 3 masks; three row blocks
    LCase('logistic', (270, 12, 1, 71, 1), 1, False, 2.0),    # chunks of 64 + 7 sets; row workgroups 4 x 64 + 14
]


def reaches(c, slots=SLOTS[0]):
    """The INVENTORY items a launch case reaches, on the paths it is run on (path 1, path 2 where eligible)."""
    N, D, K, S, T = c.shape
    if not c.dropout:
        T = 1
    got = set()
    names = list(INVENTORY)
    gp = general_plan(N, K, S, T, c.dropout, 8)
    if not c.dropout and gp.chunks > 1 and gp.last < gp.CH:
        got.add(names[6])
    if N > LG_NT and N % LG_NT:
        got.add(names[7])
    if gp.finish_blocks > 1:
        got.add(names[8])
    if gp.draws_blocks > 1:
        got.add(names[9])
    if eligible(c):
        fp = fused_plan(N, D, K, S, T, c.dropout, slots)
        rounds = fp.nit >= 2
        if not c.dropout and rounds and fp.idle_last > 0 and fp.last_units < fp.upg:
            got.add(names[0])
            if LF_COLS % K:
                got.add(names[1])
        if c.dropout and rounds and T % LF_NACC:
            got.add(names[2])
        if not c.dropout and S % fp.spu:
            got.add(names[3])
        if D < 16 and N > LF_ROWS:
            got.add(names[4])
        if D % 16 == 0:
            got.add(names[5])
    return got


def launch_T(c):
    return c.shape[4] if c.dropout else 1


# ----------------------------------------------------------------------------- defect emulation
def _per_draw(model, pb, T, dropout, zextra=None, W=None):
    """Per-draw class probabilities [DR, N, classes] and per-row −log-likelihood and hit [DR, N], restated in
    plain NumPy (the emulations need per-row terms; test_linear_predictive_cpu.py holds it to the oracle)."""
    W = pb.W if W is None else W
    S, N = W.shape[0], pb.X.shape[0]
    ps, nl, hit = [], [], []
    for d in range(S * T):
        s = d // T
        Xd = pb.X * pb.masks[d] if dropout else pb.X
        z = Xd @ W[s] + pb.b[s]
        if zextra is not None:
            z = z + zextra[d]
        z = np.maximum(np.minimum(z, om.CLIP_HI), om.CLIP_LO)
        if model == 'logistic':
            p1 = 1.0 / (1.0 + np.exp(-z[:, 0]))
            p = np.stack([1.0 - p1, p1], axis=1)
            hit.append((p1 > 0.5).astype(int) == pb.y)
        else:
            e = np.exp(z - z.max(axis=1, keepdims=True))
            p = e / e.sum(axis=1, keepdims=True)
            hit.append(z.argmax(axis=1) == pb.y)
        ps.append(p)
        nl.append(-np.log(p[np.arange(N), pb.y]))
    return np.stack(ps), np.stack(nl), np.stack(hit)


def _assemble(model, p, nl, y, row_draws=None, draw_rows=None, rows_done=None, draws_done=None):
    """The compared outputs from per-draw terms.  row_draws: the draws that reach the per-row sums (which are
    still divided by all S·T); draw_rows: the rows that reach the per-draw sums; rows_done / draws_done: the
    entries the finishing launches write (the others stay 0)."""
    DR, N = nl.shape
    rd = np.ones(DR, bool) if row_draws is None else row_draws
    dr = np.ones(N, bool) if draw_rows is None else draw_rows
    pm = p[rd].sum(axis=0) / DR
    out = {"mean": pm[:, 1:] if model == 'logistic' else pm, "entropy": _entropy(pm),
           "expected_entropy": _entropy(p)[rd].sum(axis=0) / DR,
           "lppd": np.log(p[:, np.arange(N), y][rd].sum(axis=0) / DR), "draw_nll": nl[:, dr].sum(axis=1) / N}
    if rows_done is not None:
        for k in ROW_OUTPUTS:
            out[k] = np.where(rows_done.reshape((-1,) + (1,) * (out[k].ndim - 1)), out[k], 0.0)
    if draws_done is not None:
        out["draw_nll"] = np.where(draws_done, out["draw_nll"], 0.0)
    return out


def emulated(c, defect=None):
    """The compared outputs of a launch case if its launch had `defect` (None: none; then it is case_ref)."""
    N, D, K, S, _ = c.shape
    T = launch_T(c)
    DR = S * T
    pb = problem(c)
    kw, zextra, W = {}, None, None
    if defect in ("rounds-dropped", "last-group-dropped", "last-unit-dropped"):
        units = fused_unit_draws(N, D, K, S, T, c.dropout, SLOTS[0])
        last_group = units[-1][0]
        keep = np.zeros(DR, bool)
        for i, (g, rnd, draws) in enumerate(units):
            if defect == "rounds-dropped":
                ok = rnd == 0
            elif defect == "last-group-dropped":
                ok = g != last_group
            else:
                ok = i != len(units) - 1
            if ok:
                keep[draws] = True
        kw = dict(row_draws=keep, draws_done=keep)
    elif defect == "pad-columns-live":
        # the X tile's columns D … Dp − 1 hold what follows the row in memory, against W's row D − 1
        Dp = (D + 15) // 16 * 16
        flat = np.concatenate([pb.X.reshape(-1), np.zeros(Dp)])
        zextra = []
        for d in range(DR):
            x = np.array([flat[n * D + D:n * D + Dp].sum() for n in range(N)])
            zextra.append(x[:, None] * pb.W[d // T, D - 1][None, :])
    elif defect == "last-chunk-dropped":
        W = pb.W.copy()
        W[:, D - 16:, :] = 0.0
    elif defect == "chunk-overwrites":
        gp = general_plan(N, K, S, T, c.dropout, 8)
        kw = dict(row_draws=np.arange(DR) >= (gp.chunks - 1) * gp.CH)
    elif defect == "rows-past-64-unsummed":
        kw = dict(draw_rows=np.arange(N) < LG_NT)
    elif defect == "rows-past-256-unfinished":
        kw = dict(rows_done=np.arange(N) < 256)
    elif defect == "draws-past-256-unsummed":
        kw = dict(draws_done=np.arange(DR) < 256)
    else:
        assert defect is None, defect
    p, nl, _ = _per_draw(c.model, pb, T, c.dropout, zextra, W)
    return _assemble(c.model, p, nl, pb.y, **kw)


def tol32(ref, name):
    """The float32 bound of the GPU test (the loosest it applies): 2e-4 of the largest reference entry."""
    return 2e-4 * float(np.abs(getattr(ref, name)).max())


# ----------------------------------------------------------------------------- saturated logits
# Constructed problems whose pre-clip logit (X ⊙ Z)·W + b lands in stated bands.  Column 0 of X drives: it holds a
# row's scale (0 … 1, ±SAT_C or SAT_F) against a weight of ±1 per set; the other columns add less than 4 in all.
# With dropout a row whose driver is masked falls back to band O, so every band mixes over rows and draws.
#   O: |z| <= 12.   C: z >= 37 or z <= −37 (the upper clip is 36.0437: both dtypes clip the same entries).
#   F: 17.5 <= z <= 26 (a float32 sigmoid rounds to 1), in the float32 problems only.
# Logistic: no logit in 26 < |z| < 37, where the reference's own log(1 − p) moves by 2⁻⁵³·e^z per ulp of p.
BAND_O, BAND_C, BAND_F = 12.0, 37.0, (17.5, 26.0)
SAT_C, SAT_F, SAT_LOW = 45.0, 21.5, -40.0
SatCase = namedtuple("SatCase", "model shape seed bandF")
SAT_CASES = [
    SatCase('logistic', (40, 8, 1, 6, 2), 0, False), SatCase('logistic', (40, 8, 1, 6, 2), 0, True),
    SatCase('softmax', (40, 8, 3, 6, 2), 1, False), SatCase('softmax', (40, 8, 3, 6, 2), 1, True),
]


def sat_id(c):
    return "%s-%s" % (c.model, "OCF" if c.bandF else "OC")


def sat_case(model, dtype_is_f32):
    return [c for c in SAT_CASES if c.model == model and c.bandF == dtype_is_f32][0]


@functools.lru_cache(maxsize=None)
def sat_problem(c, rounded=False):
    N, D, K, S, T = c.shape
    rs = np.random.RandomState(c.seed)
    W, b = rs.uniform(-0.5, 0.5, (S, D, K)), rs.uniform(-0.5, 0.5, (S, K))
    X = rs.rand(N, D)
    y = rs.randint(0, 2 if c.model == 'logistic' else K, N)
    masks = rs.binomial(1, 0.5, (S * T, N, D)).astype(np.uint8)
    scale = [None, SAT_C, -SAT_C, SAT_F if c.bandF else None]          # by row: n % 4
    for n in range(N):
        if scale[n % 4] is not None:
            X[n, 0] = scale[n % 4]
    for s in range(S):
        if c.model == 'logistic':
            W[s, 0, 0] = -1.0 if s % 3 == 2 else 1.0                   # four sets up, two down: no mean at 0.5
        else:                                                          # one class up, another down (to SAT_LOW)
            up = rs.randint(0, K)
            dn = (up + 1 + rs.randint(0, K - 1)) % K
            W[s, 0, :] = 0.0
            W[s, 0, up], W[s, 0, dn] = 1.0, SAT_LOW / SAT_C
    if rounded:
        W, b, X = f32r(W), f32r(b), f32r(X)
    return Problem(W, b, X, y, masks)


@functools.lru_cache(maxsize=None)
def sat_ref(c, dropout=True, rounded=False):
    pb = sat_problem(c, rounded)
    if dropout:
        return predictive_ref(c.model, pb.W, pb.b, pb.X, pb.y, pb.masks, c.shape[4])
    return predictive_ref(c.model, pb.W, pb.b, pb.X, pb.y, None, 1)


def sat_logits(c, dropout, rounded=False):
    """The pre-clip logits [draws, N, K] of a saturated problem."""
    pb = sat_problem(c, rounded)
    T = c.shape[4] if dropout else 1
    return np.stack([(pb.X * pb.masks[d] if dropout else pb.X) @ pb.W[d // T] + pb.b[d // T]
                     for d in range(c.shape[3] * T)])
