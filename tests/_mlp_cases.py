"""Case table, launch mirror, references and tolerances of the dropout-MLP kernel tests (test infrastructure):
tests/test_gpu_mlp_kernels.py drives hmcx_mlp_grad / hmcx_mlp_loss with them, tests/test_mlp_cases_cpu.py checks
their preconditions on the CPU.  Needs neither a GPU nor torch.

Launch mirror.  ``launches`` restates the host code of csrc/hmcx_mlp.hip (kernel side: csrc/hmcx_mlp_kernels.h,
cited by function name) that decides what a one-off call
(mlp_grad_t / mlp_loss_t: the unfused launches) runs for a shape, dtype, mask kind and mask alignment: per
k_mm launch the epilogue, the operand vector paths (AV, BV), the XCD placement, the K range each of the eight
waves takes, and for layer 3 the narrow (MM_L3CE) / wide (k_l3_wide) kernel with its column slices, the ``wl``
test and the row groups of l3_backward.  The cases are the smallest shapes that reach every value in REQUIRED;
a retuned threshold fails the CPU test instead of hollowing the GPU ones out.

References are oracle/models.py::mlp in float64; ``dtype='float32'`` rounds the inputs to float32 first, so
input rounding is not counted as kernel error.  ``bounds`` is the forward-error yardstick of the float32
tolerances: the same forward and backward with every operand replaced by its absolute value (and every
subtraction by an addition), times the summed length of the contractions the array has passed through, times
the unit roundoff of the dtype.
"""
import functools

import numpy as np

from oracle import models as om

ALPHA = 0.01
MM_NW, MM_NT = 8, 512                     # hmcx_mlp_kernels.h
UNIT = {"float32": 2.0 ** -24, "float64": 2.0 ** -53}
F32_CAP = 2e-4                            # of the largest entry (tests/test_gpu_mlp.py): never looser than this
F32_MARGIN = 4                            # × the measured worst err / bound (tests/test_gpu_mlp_accept.py)
F64_GRAD, F64_LOSS = 1e-9, 1e-11          # of the largest entry; relative (tests/test_gpu_mlp.py)
GRADS = ("gW1", "gb1", "gW2", "gb2", "gW3", "gb3")
OUTPUTS = GRADS + ("loss", "logits")


# ---------------------------------------------------------------------------------- launch mirror
def xcd_choose(dtype, GX, GY, gx, gy):
    """xcd_choose (hmcx_mlp.hip): (xmap, xbx, xby) of a gx × gy tile plane in a GX × GY grid."""
    if dtype != "float32" or gx * gy < 16 or (GX * GY) % 8:
        return 0, 0, 0
    per = GX * GY // 8
    best = (gx + 7) // 8 + gy if GX % 8 == 0 else gx + gy
    xmap, xb = 0, (0, 0)
    P = gx * gy
    q = P // 8 + (1 if P % 8 else 0)
    if q <= per:
        c = min(gx, q) + (q + gx - 1) // gx + 1
        if c < best:
            best, xmap = c, 1
    for bx in range(1, gx + 1):
        if gx % bx:
            continue
        for by in range(1, gy + 1):
            if gy % by or (gx // bx) * (gy // by) != 8 or bx * by > per:
                continue
            if bx + by < best:
                best, xmap, xb = bx + by, 2, (bx, by)
    return (xmap,) + (xb if xmap == 2 else (0, 0))


def k_split(K):
    """mm_body's K split (hmcx_mlp_kernels.h): Kq = the k range per wave (a multiple of 16); ``chunks`` the number of
    16-wide chunks of each of the eight waves — 1 to 3 fill the register ring, 4, 5 and 6 reload slot 0, 1
    and 2 (at +48 / +64 / +80), 7 and 8 go round again — and 0 for a wave with no K at all."""
    Kq = (K + 16 * MM_NW - 1) // (16 * MM_NW) * 16
    chunks = []
    for w in range(MM_NW):
        kb = w * Kq
        ke = min(K, kb + Kq)
        chunks.append(max(0, -(-(ke - kb) // 16)))
    return Kq, tuple(chunks)


def mm(name, epi, dtype, M, N, K, TA, TB, h1_a=False, vec_masks=True, placed=False, mk="none"):
    """mm() (hmcx_mlp.hip) for operands whose base pointers are 16-byte aligned (device
    allocations and workspace blocks are): the launch signature of one k_mm."""
    V = 4 if dtype == "float32" else 2
    lda, ldb = (M if TA else K), (K if TB else N)
    kvec = K % V == 0
    av = (not TA) and (not h1_a or vec_masks) and kvec and lda % V == 0          # mm(): h1ok, kvec, aal
    bv = bool(TB) and kvec and ldb % V == 0                                       # mm(): bv
    gx, gy = (M + 31) // 32, (N + 31) // 32                                       # mm(): grid
    xmap = xcd_choose(dtype, gx, gy, gx, gy) if placed else (0, 0, 0)             # mm(): MM_STORE / MM_UPD
    Kq, chunks = k_split(K)
    return dict(name=name, epi=epi, av=av, bv=bv, xmap=xmap[0], block=xmap[1:], Kq=Kq, chunks=chunks,
                empty_wave=0 in chunks, ragged_m=M % 32 != 0, ragged_n=N % 32 != 0, ragged_k=K % 16 != 0,
                tiles=(gx, gy), K=K, mk=mk)


def l3_rows(nt, nj):
    """l3_backward (hmcx_mlp_kernels.h) for a slice of nj columns: R row groups, RB rows per pass and the
    number of ``jb`` passes over the slice."""
    R = max(1, nt // nj)
    cols = nt // R
    RB = 16 if R <= 2 else 8 if R <= 4 else 4 if R <= 8 else 2
    return R, RB, -(-nj // cols)


def layer3(dtype, B, n_mid, n_out, backward):
    """mlp_forward's narrow / wide choice (hmcx_mlp.hip), the MM_L3CE slice count (mm()'s grid.y; mm_body's column
    slices, hmcx_mlp_kernels.h) and the ``wl`` test (l3_backward; scratch of the narrow kernel (MM_NW − 1)·32·33
    values, mm_body's MM_L3CE epilogue; of the wide one MM_NT, k_l3_wide)."""
    if n_out <= 32:
        gy = max(1, min(8, n_mid // 32))
        cw = -(-n_mid // gy)
        widths = tuple(min(n_mid, min(n_mid, s * cw) + cw) - min(n_mid, s * cw) for s in range(gy))
        scr_n, kind = (MM_NW - 1) * 32 * 33, "narrow"
    else:
        widths, scr_n, kind = (n_mid,), MM_NT, "wide"
    sig = dict(kind=kind, slices=len(widths), widths=widths)
    if backward:
        rows = [l3_rows(MM_NT, nj) for nj in widths if nj > 0]
        sig.update(wl=n_out * n_mid + MM_NT <= scr_n, R=tuple(sorted({r[0] for r in rows})),
                   RB=tuple(sorted({r[1] for r in rows})), jb=max(r[2] for r in rows))
    return sig


def launches(B, n_in, n_mid, n_out, dtype, masks="vals", aligned=True):
    """The launches of hmcx_mlp_grad (mlp_grad_t → mlp_grad_launch, hmcx_mlp.hip) followed by those hmcx_mlp_loss adds
    when it returns logits (mlp_loss_t): a list of mm() signatures, the layer-3 one under 'l3'.
    masks 'vals' (a [3][B][n_mid] buffer; ``aligned``: on a 16-byte boundary) or 'none' (NULL)."""
    mk = masks
    vec_masks = n_mid % 4 == 0 and (aligned or masks == "none")                   # net_init, oneoff_net
    out = [mm("layer1", "STORE", dtype, B, n_mid, n_in, 0, 1, placed=True),      # mlp_forward: xw
           mm("layer2", "L2", dtype, B, n_mid, n_mid, 0, 1, h1_a=True, vec_masks=vec_masks, mk=mk)]   # mlp_forward: h2, d3
    l3 = layer3(dtype, B, n_mid, n_out, True)
    if l3["kind"] == "narrow":
        g = mm("layer3", "L3CE", dtype, B, n_out, n_mid, 0, 1, mk=mk)            # mlp_forward: n_out ≤ 32
    else:
        g = mm("layer3", "STORE", dtype, B, n_out, n_mid, 0, 1, placed=True)     # mlp_forward: d3·W3ᵀ, then k_l3_wide
    g["l3"] = l3
    out.append(g)
    out.append(mm("ga1", "GA1", dtype, B, n_mid, n_mid, 0, 0, mk=mk))            # mlp_ga1
    out.append(mm("gW1", "UPD", dtype, n_mid, n_in, B, 1, 0, placed=True))       # wgrad_build, v = 0
    out.append(mm("gW2", "UPD", dtype, n_mid, n_mid, B, 1, 0, placed=True, mk=mk))   # v = 2 (B operand OP_H1)
    out.append(mm("logits", "STORE", dtype, B, n_out, n_mid, 0, 1, placed=True))     # mlp_forward: logits
    return out


# ---------------------------------------------------------------------------------- case table
def _c(B, n_in, n_mid, n_out, masks="vals", aligned=True, dtypes=("float64", "float32"), seed=5, why=""):
    return dict(B=B, n_in=n_in, n_mid=n_mid, n_out=n_out, masks=masks, aligned=aligned, dtypes=dtypes, seed=seed,
                why=why)


CASES = [
    _c(100, 100, 128, 5, why="xmap 2 on all three plain GEMMs, ragged M and N edges under it"),
    _c(8, 520, 256, 3, why="xmap 1 with a ragged N edge (W1 gradient); Kq 80"),
    _c(40, 24, 256, 32, why="narrow layer 3 with W3 not staged in LDS (wl false)"),
    _c(33, 20, 1024, 4, why="R = 4 (RB 8) in the narrow layer 3; Kq 128 in the hidden GEMMs"),
    _c(12, 16, 600, 33, why="wide layer 3, R = 1 with two jb passes; Kq 80 with a short last wave"),
    _c(130, 260, 128, 33, why="wide layer 3, R = 4; Kq 48 and 32"),
    _c(300, 400, 100, 9, why="Kq 64 and 48; three column slices of uneven width (34, 34, 32)"),
    _c(36, 776, 64, 10, why="Kq 112: the ring reloads all three slots and goes round again"),
    _c(21, 30, 38, 3, why="float64: B vectorised, A scalar in MM_L2 (n_mid % 4 == 2)"),
    _c(19, 50, 37, 7, why="odd everything: no vector path, R = 13"),
    _c(1, 3, 1, 2, why="one row, one hidden unit: seven waves with no K at all"),
    _c(70, 33, 64, 40, why="wide layer 3, R = 8 (RB 4)"),
    _c(40, 64, 768, 6, why="Kq 96: slot 2 of the ring reloads once"),
    _c(33, 24, 64, 12, aligned=False, why="mask buffer one element off 16 bytes: vec_masks off with n_mid % 4 == 0"),
    _c(100, 100, 128, 5, masks="none", dtypes=("float32",), why="float32 without masks (MK_NONE), xmap 2"),
    _c(19, 50, 37, 7, masks="none", dtypes=("float32",), why="float32 without masks, scalar paths"),
]


def case_id(c):
    return "%d-%d-%d-%d%s%s" % (c["B"], c["n_in"], c["n_mid"], c["n_out"], "-nomask" if c["masks"] == "none" else "",
                                "" if c["aligned"] else "-off1")


def case_launches(c, dtype):
    return launches(c["B"], c["n_in"], c["n_mid"], c["n_out"], dtype, c["masks"], c["aligned"])


def _plain(g):
    return g["name"] in ("layer1", "gW1", "gW2")


# Every value of the branch inventory: (label, dtypes it exists in, predicate over one launch signature)
BOTH, F32, F64 = ("float32", "float64"), ("float32",), ("float64",)
REQUIRED = [
    ("xmap 1", F32, lambda g: g["xmap"] == 1),
    ("xmap 2", F32, lambda g: g["xmap"] == 2),
    ("xmap 1 with a ragged edge", F32, lambda g: g["xmap"] == 1 and (g["ragged_m"] or g["ragged_n"])),
    ("xmap 2 with a ragged M edge", F32, lambda g: g["xmap"] == 2 and g["ragged_m"]),
    ("xmap 2 with a ragged N edge", F32, lambda g: g["xmap"] == 2 and g["ragged_n"]),
    ("xmap 2 on layer 1", F32, lambda g: g["xmap"] == 2 and g["name"] == "layer1"),
    ("xmap 2 on the W1 gradient", F32, lambda g: g["xmap"] == 2 and g["name"] == "gW1"),
    ("xmap 2 on the W2 gradient", F32, lambda g: g["xmap"] == 2 and g["name"] == "gW2"),
    ("16 tiles or more in dispatch order", F64, lambda g: _plain(g) and g["tiles"][0] * g["tiles"][1] >= 16),
] + [("Kq %d" % k, BOTH, (lambda k: lambda g: g["Kq"] == k)(k)) for k in (16, 32, 48, 64, 80, 96, 112, 128)] + [
    ("a wave with no K", BOTH, lambda g: g["empty_wave"]),
    ("a short last chunk (K % 16)", BOTH, lambda g: g["ragged_k"]),
    ("a full wave range beside a short one", BOTH, lambda g: len({c for c in g["chunks"] if c}) > 1),
    ("MM_L2 (AV, BV) = (1, 1)", BOTH, lambda g: g["epi"] == "L2" and g["av"] and g["bv"]),
    ("MM_L2 (AV, BV) = (0, 0)", BOTH, lambda g: g["epi"] == "L2" and not g["av"] and not g["bv"]),
    ("MM_L2 B vectorised, A scalar by an unaligned mask buffer", BOTH,
     lambda g: g["epi"] == "L2" and not g["av"] and g["bv"] and g["K"] % 4 == 0),
    ("MM_L2 B vectorised, A scalar by n_mid % 4 == 2", F64,
     lambda g: g["epi"] == "L2" and not g["av"] and g["bv"] and g["K"] % 4 == 2),
    ("MM_L2 without masks", F32, lambda g: g["epi"] == "L2" and g["mk"] == "none"),
    ("MM_GA1 without masks", F32, lambda g: g["epi"] == "GA1" and g["mk"] == "none"),
    ("MM_L3CE without masks", F32, lambda g: g["epi"] == "L3CE" and g["mk"] == "none"),
    ("plain GEMM vectorised", BOTH, lambda g: g["name"] == "layer1" and g["av"] and g["bv"]),
    ("plain GEMM scalar", BOTH, lambda g: g["name"] == "layer1" and not g["av"] and not g["bv"]),
    ("narrow layer 3", BOTH, lambda g: "l3" in g and g["l3"]["kind"] == "narrow"),
    ("wide layer 3", BOTH, lambda g: "l3" in g and g["l3"]["kind"] == "wide"),
    ("narrow layer 3, W3 in LDS", BOTH, lambda g: "l3" in g and g["l3"]["kind"] == "narrow" and g["l3"]["wl"]),
    ("narrow layer 3, W3 not in LDS", BOTH, lambda g: "l3" in g and g["l3"]["kind"] == "narrow" and not g["l3"]["wl"]),
    ("wide layer 3, W3 not in LDS", BOTH, lambda g: "l3" in g and g["l3"]["kind"] == "wide" and not g["l3"]["wl"]),
] + [("l3_backward RB %d" % rb, BOTH, (lambda rb: lambda g: "l3" in g and rb in g["l3"]["RB"])(rb))
     for rb in (2, 4, 8, 16)] + [
    ("l3_backward R <= 4", BOTH, lambda g: "l3" in g and min(g["l3"]["R"]) <= 4),
    ("l3_backward R = 1 with several jb passes", BOTH, lambda g: "l3" in g and g["l3"]["R"] == (1,) and g["l3"]["jb"] > 1),
    ("l3_backward R = 13", BOTH, lambda g: "l3" in g and 13 in g["l3"]["R"]),
    ("one column slice", BOTH, lambda g: "l3" in g and g["l3"]["kind"] == "narrow" and g["l3"]["slices"] == 1),
    ("eight column slices", BOTH, lambda g: "l3" in g and g["l3"]["slices"] == 8),
    ("column slices of uneven width", BOTH, lambda g: "l3" in g and len(set(g["l3"]["widths"])) > 1),
    ("logits of a narrow shape", BOTH, lambda g: g["name"] == "logits" and g["tiles"][1] == 1),
    ("logits of a wide shape", BOTH, lambda g: g["name"] == "logits" and g["tiles"][1] == 2),
]


def coverage():
    """{(label, dtype): [case ids that reach it]} over CASES."""
    hit = {(label, d): [] for label, dts, _ in REQUIRED for d in dts}
    for c in CASES:
        for d in c["dtypes"]:
            sigs = case_launches(c, d)
            for label, dts, pred in REQUIRED:
                if d in dts and any(pred(g) for g in sigs):
                    hit[(label, d)].append(case_id(c))
    return hit


# ---------------------------------------------------------------------------------- problems
def _round32(a):
    return a.astype(np.float32).astype(np.float64)


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def problem(i, dtype="float64"):
    """Inputs of CASES[i] in float64 (read-only, shared): X [B, n_in], y [B], the six parameters under their
    oracle names, masks [3, B, n_mid] (None without dropout).  Weights are drawn with standard deviation
    fan_in^-1/2 so that no layer saturates at any width; dtype 'float32': every value rounded to float32."""
    c = CASES[i]
    B, n_in, n_mid, n_out = c["B"], c["n_in"], c["n_mid"], c["n_out"]
    rs = np.random.RandomState(c["seed"])
    par = {}
    for k, s in om.mlp_param_shapes(n_in, n_mid, n_out).items():
        par[k] = rs.normal(0, s[1] ** -0.5, s) if len(s) == 2 else rs.normal(0, 0.3, s)
    X = rs.rand(B, n_in)
    y = rs.randint(0, n_out, B)
    masks = np.stack(om.dropout_masks(rs, B, n_mid, dtype=np.float64)) if c["masks"] == "vals" else None
    if dtype == "float32":
        X, par = _round32(X), {k: _round32(v) for k, v in par.items()}
        masks = _round32(masks) if masks is not None else None
    p = dict(X=X, y=y, masks=masks, **par)
    return _freeze(p)


def _par(p):
    return {k: p[k] for k in om.MLP_PARAM_NAMES}


# ---------------------------------------------------------------------------------- references
_G = dict(zip(om.MLP_PARAM_NAMES, GRADS))


def outputs(p, z_edit=None, gz_edit=None):
    """The eight compared outputs at the inputs ``p`` (a dict as ``problem`` returns): the six gradients, the
    mean cross-entropy and the logits.  Without edits this is oracle.models.mlp (grad, log_likelihood, _forward)
    itself; ``z_edit`` / ``gz_edit`` change the logits before the cross-entropy resp. its gradient before the
    backward pass, restating mlp.grad (oracle/models.py:254-275) from its own pieces."""
    m = om.mlp({"alpha": ALPHA}, p["X"].shape[1], p["/l1/b"].size, p["/l3/b"].size)
    par, X, y = _par(p), p["X"], p["y"]
    masks = list(p["masks"]) if p["masks"] is not None else None
    z, (a1, h1, a2, h2, d3) = m._forward(par, X, masks)
    if z_edit is None and gz_edit is None:
        g = m.grad(par, masks=masks, X_train=X, y_train=y)
        out = {_G[k]: g[k] for k in om.MLP_PARAM_NAMES}
        out["loss"] = float(m.log_likelihood(par, masks=masks, X_train=X, y_train=y))
        out["logits"] = z
        return out
    if z_edit is not None:
        z = z_edit(z.copy())
    m1, m2, m3 = masks if masks is not None else (1, 1, 1)
    B = z.shape[0]
    loss, logp = m._ce(z, y)
    gz = np.exp(logp)
    gz[np.arange(B), y] -= 1
    gz = gz / B
    if gz_edit is not None:
        gz, loss = gz_edit(gz, -logp[np.arange(B), y])
    ga2 = gz.dot(par['/l3/W']) * m3 * (a2 * m2 > 0) * m2
    ga1 = ga2.dot(par['/l2/W']) * (a1 * m1 > 0) * m1
    g = {'/l3/W': gz.T.dot(d3), '/l3/b': gz.sum(axis=0), '/l2/W': ga2.T.dot(h1), '/l2/b': ga2.sum(axis=0),
         '/l1/W': ga1.T.dot(X), '/l1/b': ga1.sum(axis=0)}
    out = {_G[k]: g[k] + 0.5 * ALPHA * par[k] for k in om.MLP_PARAM_NAMES}
    out["loss"] = float(loss)
    out["logits"] = z
    return out


@functools.lru_cache(maxsize=None)
def reference(i, dtype="float64"):
    """float64 reference outputs of case i on the inputs of ``dtype`` (computed once, read-only)."""
    return _freeze(outputs(problem(i, dtype)))


@functools.lru_cache(maxsize=None)
def bounds(i, dtype):
    """Per output, shaped like it: the absolute-value run times the summed contraction length times the unit
    roundoff of ``dtype``.  Forward: |X|·|W1|ᵀ + |b1| and so on through the masks (relu passes everything);
    the cross-entropy gradient (softmax + onehot)/B; backward and weight gradients with |·| operands, plus the
    prior term.  Contraction lengths (+ 1 per bias or prior addition): n_in + 1 to a1, + n_mid + 1 to a2,
    + n_mid + 1 to z, + n_out for the softmax, then n_mid per backward layer and B per batch sum.  The loss
    takes the mean over rows of the row's largest |z| bound, twice (z[y] and the log-sum-exp), plus 1."""
    p = problem(i, dtype)
    c = CASES[i]
    B, n_in, n_mid, n_out = c["B"], c["n_in"], c["n_mid"], c["n_out"]
    A = {k: np.abs(p[k]) for k in om.MLP_PARAM_NAMES}
    m1, m2, m3 = p["masks"] if p["masks"] is not None else (1.0, 1.0, 1.0)
    X = np.abs(p["X"])
    h1 = (X.dot(A['/l1/W'].T) + A['/l1/b']) * m1
    h2 = (h1.dot(A['/l2/W'].T) + A['/l2/b']) * m2
    d3 = h2 * m3
    z = d3.dot(A['/l3/W'].T) + A['/l3/b']
    ref = reference(i, dtype)
    e = np.exp(ref["logits"] - ref["logits"].max(axis=1, keepdims=True))
    gz = e / e.sum(axis=1, keepdims=True)
    gz[np.arange(B), p["y"]] += 1
    gz = gz / B
    ga2 = gz.dot(A['/l3/W']) * m3 * m2
    ga1 = ga2.dot(A['/l2/W']) * m1
    nz = (n_in + 1) + (n_mid + 1) + (n_mid + 1)
    ngz = nz + n_out
    u = UNIT[dtype]
    half = 0.5 * ALPHA
    out = {"logits": z * nz * u,
           "loss": float(np.mean(2 * z.max(axis=1) + 1)) * (ngz + B) * u,
           "gW3": (gz.T.dot(d3) + half * A['/l3/W']) * (ngz + B + 1) * u,
           "gb3": (gz.sum(axis=0) + half * A['/l3/b']) * (ngz + B + 1) * u,
           "gW2": (ga2.T.dot(h1) + half * A['/l2/W']) * (ngz + n_mid + B + 1) * u,
           "gb2": (ga2.sum(axis=0) + half * A['/l2/b']) * (ngz + n_mid + B + 1) * u,
           "gW1": (ga1.T.dot(X) + half * A['/l1/W']) * (ngz + 2 * n_mid + B + 1) * u,
           "gb1": (ga1.sum(axis=0) + half * A['/l1/b']) * (ngz + 2 * n_mid + B + 1) * u}
    return _freeze(out)


# Worst |device float32 − reference| / bound per case (the largest over the eight outputs and their elements),
# measured on an MI355X; the float32 tolerance is F32_MARGIN times this times the bound, and never more than
# F32_CAP of the output's largest entry.  tests/test_gpu_mlp_kernels.py prints the figure per output.
F32_RATIO = {
    "100-100-128-5": 2.638e-3, "8-520-256-3": 6.00e-4, "40-24-256-32": 4.828e-3, "33-20-1024-4": 3.59e-4,
    "12-16-600-33": 2.476e-3, "130-260-128-33": 3.186e-3, "300-400-100-9": 1.455e-3, "36-776-64-10": 1.453e-3,
    "21-30-38-3": 6.458e-3, "19-50-37-7": 8.623e-3, "1-3-1-2": 1.106e-1, "70-33-64-40": 1.871e-2,
    "40-64-768-6": 3.30e-4, "33-24-64-12-off1": 1.102e-2, "100-100-128-5-nomask": 2.191e-3,
    "19-50-37-7-nomask": 1.119e-2,
}


def tolerances(i, dtype, ref=None):
    """Allowed |device − reference| per output of case i (arrays shaped like the output, or scalars)."""
    ref = reference(i, dtype) if ref is None else ref
    big = {o: float(np.max(np.abs(ref[o]))) for o in OUTPUTS}
    if dtype == "float64":
        tol = {o: F64_GRAD * big[o] + 1e-300 for o in GRADS}
        tol["loss"] = F64_LOSS * max(1.0, abs(ref["loss"]))
        tol["logits"] = bounds(i, "float64")["logits"] + 1e-300
        return tol
    r = F32_RATIO[case_id(CASES[i])]
    b = bounds(i, "float32")
    return {o: np.minimum(F32_MARGIN * r * b[o], F32_CAP * big[o]) for o in OUTPUTS}


# ---------------------------------------------------------------------------------- mutations
MUTATIONS = ("row", "feature", "hidden", "class", "swap", "tileW1", "tileW2", "zrows")


def applies(i, mutation):
    c = CASES[i]
    if mutation == "swap":                                  # the one-row, one-unit case keeps all three elements
        m = problem(i, "float32")["masks"]
        return m is not None and not np.array_equal(m[0], m[1])
    if mutation == "tileW1":
        return -(-c["n_mid"] // 32) * -(-c["n_in"] // 32) >= 2
    if mutation == "tileW2":
        return c["n_mid"] > 32
    if mutation == "zrows":                                 # the fused launch's range, rows past the first 512 items
        return 16 < c["n_out"] <= 32 and min(c["B"], 32) > MM_NT // c["n_out"]
    return True


def _swap_tiles(G):
    """Tile (0, 0) of the 32 × 32 tiling exchanged with the last tile (clipped to the last tile's extent)."""
    G = G.copy()
    M, N = G.shape
    r0, c0 = (-(-M // 32) - 1) * 32, (-(-N // 32) - 1) * 32
    h, w = M - r0, N - c0
    a, b = G[:h, :w].copy(), G[r0:r0 + h, c0:c0 + w].copy()
    G[:h, :w], G[r0:r0 + h, c0:c0 + w] = b, a
    return G


def mutated(i, mutation):
    """The float64 outputs of case i (float32-rounded inputs) with one defect a kernel could have:
    'row'      the last batch row left out: its cross-entropy gradient and loss term zero, its logits b3 alone;
    'feature'  the last input feature zeroed;
    'hidden'   the last hidden unit dropped (column n_mid − 1 of all three masks zero);
    'class'    the last class's row of W3 zeroed (a lost column of the layer-3 tile);
    'swap'     masks m1 and m2 exchanged;
    'tileW1' / 'tileW2'  one 32 × 32 tile of that gradient exchanged with another (a misplaced xmap tile);
    'zrows'    the logits of rows r >= 512 // n_out of every 32-row block replaced by zeros (the fused launch
               whose publish / poll stops at its 512 threads)."""
    p = dict(problem(i, "float32"))
    c = CASES[i]
    if mutation == "row":
        def gz_edit(gz, rowloss):
            gz = gz.copy()
            gz[-1] = 0
            return gz, rowloss[:-1].sum() / c["B"]
        out = outputs(p, gz_edit=gz_edit)
        out["logits"] = out["logits"].copy()
        out["logits"][-1] = p["/l3/b"]
        return out
    if mutation == "feature":
        p["X"] = p["X"].copy()
        p["X"][:, -1] = 0
        return outputs(p)
    if mutation == "hidden":
        m = p["masks"].copy() if p["masks"] is not None else np.ones((3, c["B"], c["n_mid"]))
        m[:, :, -1] = 0
        p["masks"] = m
        return outputs(p)
    if mutation == "class":
        p["/l3/W"] = p["/l3/W"].copy()
        p["/l3/W"][-1] = 0
        return outputs(p)
    if mutation == "swap":
        p["masks"] = p["masks"][[1, 0, 2]]
        return outputs(p)
    if mutation in ("tileW1", "tileW2"):
        out = dict(reference(i, "float32"))
        k = "g" + mutation[4:]
        out[k] = _swap_tiles(out[k])
        return out
    assert mutation == "zrows"
    first = MM_NT // c["n_out"]

    def z_edit(z):
        z[np.arange(c["B"]) % 32 >= first] = 0
        return z
    return outputs(p, z_edit=z_edit)
