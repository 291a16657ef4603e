"""The MLP entry points' argument checks (csrc/hmcx_mlp_checks.h) on the CPU: a stand-alone C++ program, built
with the host compiler, runs every row of the table below and prints status and message; each must equal what the
entry point returned before the checks moved out of hmcx_ctx.hip (statuses and message bytes copied from there).

A row is (entry, case, statements that damage a valid argument block `a` (or, for the three positional entries, the
whole call), status, message).  The per-step arrays are heap blocks of exactly n_steps (3) or n_steps * C (6)
entries with the defect in the last one, and the program runs under the address and undefined-behaviour sanitizers
where the compiler can link them, so a scan that read past an array would fail the run."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "dropout_hamiltonian_montecarlo_amd", "csrc")
OK, EINVAL, EUNSUP = 0, -1, -4
DTYPE = "dtype must be HMCX_F32/HMCX_F64"
SIZES = "mlp: sizes must be >= 1"
LARGE = "mlp: layer too large"

# the seven struct-taking entries: (check function, message prefix, name of the batch-size field)
STRUCTS = {
    "sghmc": ("sghmc", "mlp sghmc: ", "B"), "leapfrog": ("leapfrog", "mlp leapfrog: ", "B"),
    "sgd": ("sgd", "mlp sgd: ", "B"), "sgld": ("sgld", "mlp sgld: ", "B"),
    "sgld_chains": ("sgld_chains", "mlp sgld chains: ", "B"), "hmc_chains": ("hmc_chains", "mlp hmc chains: ", "B"),
    "predictive": ("predictive", "mlp predictive: ", "N"),
}

ROWS = [
    # ---- hmcx_mlp_masks(dtype, B, n_mid, out) ----
    ("masks", "valid", "masks(HMCX_F64, 4, 8, P)", OK, ""),
    ("masks", "dtype", "masks(5, 4, 8, P)", EINVAL, DTYPE),
    ("masks", "sizes", "masks(HMCX_F32, 0, 8, P)", EINVAL, SIZES),
    ("masks", "large", "masks(HMCX_F32, 40000, 40000, P)", EUNSUP, LARGE),
    ("masks", "null out", "masks(HMCX_F32, 4, 8, nullptr)", EINVAL, "null pointer"),
    ("masks", "dtype wins over null out", "masks(-1, 4, 8, nullptr)", EINVAL, DTYPE),
    # ---- hmcx_mlp_grad(dtype, X, y, B, n_in, n_mid, n_out, par, grads) ----
    ("grad", "valid", "grad(HMCX_F32, P, Y, 4, 3, 8, 2, &PAR, &PAR)", OK, ""),
    ("grad", "dtype", "grad(2, P, Y, 4, 3, 8, 2, &PAR, &PAR)", EINVAL, DTYPE),
    ("grad", "sizes", "grad(HMCX_F32, P, Y, 4, 3, 8, 0, &PAR, &PAR)", EINVAL, SIZES),
    ("grad", "large", "grad(HMCX_F32, P, Y, 4, 50000, 50000, 2, &PAR, &PAR)", EUNSUP, LARGE),
    ("grad", "null X", "grad(HMCX_F32, nullptr, Y, 4, 3, 8, 2, &PAR, &PAR)", EINVAL, "null pointer"),
    ("grad", "null y", "grad(HMCX_F32, P, nullptr, 4, 3, 8, 2, &PAR, &PAR)", EINVAL, "null pointer"),
    ("grad", "hole in par", "grad(HMCX_F32, P, Y, 4, 3, 8, 2, &HOLE, &PAR)", EINVAL, "null pointer"),
    ("grad", "null grads", "grad(HMCX_F32, P, Y, 4, 3, 8, 2, &PAR, nullptr)", EINVAL, "null pointer"),
    # ---- hmcx_mlp_loss(dtype, X, y, B, n_in, n_mid, n_out, par, logits) ----
    ("loss", "valid with labels", "loss(HMCX_F64, P, Y, 4, 3, 8, 2, &PAR, nullptr)", OK, ""),
    ("loss", "valid with logits", "loss(HMCX_F64, P, nullptr, 4, 3, 8, 2, &PAR, P)", OK, ""),
    ("loss", "dtype", "loss(9, P, Y, 4, 3, 8, 2, &PAR, nullptr)", EINVAL, DTYPE),
    ("loss", "sizes", "loss(HMCX_F64, P, Y, 4, 0, 8, 2, &PAR, nullptr)", EINVAL, SIZES),
    ("loss", "large", "loss(HMCX_F64, P, Y, 4, 3, 50000, 2, &PAR, nullptr)", EUNSUP, LARGE),
    ("loss", "null X", "loss(HMCX_F64, nullptr, Y, 4, 3, 8, 2, &PAR, nullptr)", EINVAL, "null pointer"),
    ("loss", "null par", "loss(HMCX_F64, P, Y, 4, 3, 8, 2, nullptr, nullptr)", EINVAL, "null pointer"),
    ("loss", "neither labels nor logits", "loss(HMCX_F64, P, nullptr, 4, 3, 8, 2, &PAR, nullptr)", EINVAL,
     "mlp_loss: need labels or a logits output"),
    ("loss", "null X wins over no labels", "loss(HMCX_F64, nullptr, nullptr, 4, 3, 8, 2, &PAR, nullptr)", EINVAL,
     "null pointer"),
    # ---- hmcx_mlp_sghmc_run: the general messages carry no prefix, both modes compare against the noise constants
    ("sghmc", "n_steps 0", "a.n_steps = 0;", OK, ""),
    ("sghmc", "n_steps < 0 has no prefix", "a.n_steps = -1;", EINVAL, "n_steps < 0"),
    ("sghmc", "null X", "a.X = nullptr;", EINVAL, "mlp sghmc: null pointer"),
    ("sghmc", "null row0", "a.row0 = nullptr;", EINVAL, "mlp sghmc: null pointer"),
    ("sghmc", "null u_accept", "a.u_accept = nullptr;", EINVAL, "mlp sghmc: null pointer"),
    ("sghmc", "hole in par", "a.par.p[5] = nullptr;", EINVAL, "mlp sghmc: null pointer"),
    ("sghmc", "null out_loss", "a.out_loss = nullptr;", EINVAL, "mlp sghmc: null pointer"),
    ("sghmc", "bad noise_mode has no prefix", "a.noise_mode = 2;", EINVAL, "bad noise_mode"),
    ("sghmc", "bad mask_mode has no prefix (2 is no noise constant)", "a.mask_mode = HMCX_MLP_MASKS_PHILOX;", EINVAL,
     "bad mask_mode"),
    ("sghmc", "BUFFER noise without noise_off", "a.noise_mode = HMCX_NOISE_BUFFER; a.noise = PD;", EINVAL,
     "BUFFER noise mode needs noise and noise_off"),
    ("sghmc", "BUFFER masks without masks", "a.mask_mode = HMCX_NOISE_BUFFER; a.mask_off = b.off.data();", EINVAL,
     "BUFFER mask mode needs masks and mask_off"),
    ("sghmc", "both modes before either's buffers", "a.mask_mode = 7; a.noise_mode = HMCX_NOISE_BUFFER;", EINVAL,
     "bad mask_mode"),
    ("sghmc", "n_steps before null pointer", "a.n_steps = -2; a.eps = nullptr;", EINVAL, "n_steps < 0"),
    # ---- hmcx_mlp_hmc_leapfrog ----
    ("leapfrog", "n_iter < 0", "a.n_iter = -1;", EINVAL, "mlp leapfrog: n_iter < 0"),
    ("leapfrog", "null y", "a.y = nullptr;", EINVAL, "mlp leapfrog: null pointer"),
    ("leapfrog", "hole in g", "a.g.p[0] = nullptr;", EINVAL, "mlp leapfrog: null pointer"),
    ("leapfrog", "bad mask_mode", "a.mask_mode = 3;", EINVAL, "mlp leapfrog: bad mask_mode"),
    ("leapfrog", "FIXED without masks", "a.mask_mode = HMCX_MLP_MASKS_FIXED; a.masks = nullptr;", EINVAL,
     "mlp leapfrog: masks required for FIXED / PHILOX"),
    ("leapfrog", "PHILOX without masks", "a.mask_mode = HMCX_MLP_MASKS_PHILOX; a.masks = nullptr;", EINVAL,
     "mlp leapfrog: masks required for FIXED / PHILOX"),
    ("leapfrog", "NONE needs no masks", "a.mask_mode = HMCX_MLP_MASKS_NONE; a.masks = nullptr;", OK, ""),
    ("leapfrog", "order repeats", "a.order[5] = 0;", EINVAL, "mlp leapfrog: order must be a permutation of 0..5"),
    ("leapfrog", "order out of range", "a.order[5] = 6;", EINVAL, "mlp leapfrog: order must be a permutation of 0..5"),
    ("leapfrog", "mask_mode before order", "a.mask_mode = -1; a.order[0] = -1;", EINVAL, "mlp leapfrog: bad mask_mode"),
    # ---- hmcx_mlp_sgd_run ----
    ("sgd", "n_steps 0", "a.n_steps = 0;", OK, ""),
    ("sgd", "n_steps < 0", "a.n_steps = -1;", EINVAL, "mlp sgd: n_steps < 0"),
    ("sgd", "null row0", "a.row0 = nullptr;", EINVAL, "mlp sgd: null pointer"),
    ("sgd", "hole in mom", "a.mom.p[2] = nullptr;", EINVAL, "mlp sgd: null pointer"),
    ("sgd", "bad mask_mode", "a.mask_mode = 3;", EINVAL, "mlp sgd: bad mask_mode"),
    ("sgd", "FIXED without mask_off", "a.mask_off = nullptr;", EINVAL, "mlp sgd: FIXED masks need masks and mask_off"),
    ("sgd", "want_eval without out_eval_loss", "a.out_eval_loss = nullptr;", EINVAL,
     "mlp sgd: want_eval needs out_eval_loss"),
    ("sgd", "FIXED want_eval without eval_mask_off", "a.eval_mask_off = nullptr;", EINVAL,
     "mlp sgd: FIXED masks with want_eval need eval_mask_off"),
    ("sgd", "no want_eval needs neither", "a.want_eval = nullptr; a.out_eval_loss = nullptr; a.eval_mask_off = nullptr;",
     OK, ""),
    ("sgd", "negative row0 in the last step", "b.row0.back() = -1;", EINVAL, "mlp sgd: negative row0"),
    ("sgd", "negative mask_off is not rejected", "b.off.back() = -1;", OK, ""),
    ("sgd", "want_eval before the row0 scan", "b.row0[0] = -1; a.out_eval_loss = nullptr;", EINVAL,
     "mlp sgd: want_eval needs out_eval_loss"),
]


def _sgld_rows(entry, who):
    """The rows hmcx_mlp_sgld_run and hmcx_mlp_sgld_chains_run share."""
    return [
        (entry, "n_steps 0", "a.n_steps = 0;", OK, ""),
        (entry, "n_steps < 0", "a.n_steps = -1;", EINVAL, who + "n_steps < 0"),
        (entry, "2^31 parameters", "a.n_in = 46000; a.n_mid = 46000;", EUNSUP, who + "more than 2^31 - 1 parameters"),
        (entry, "variant", "a.variant = 2;", EINVAL, who + "variant must be 0 or 1"),
        (entry, "null eps", "a.eps = nullptr;", EINVAL, who + "null pointer"),
        (entry, "variant 1 without mom", "a.variant = 1; a.mom.p[3] = nullptr;", EINVAL, who + "null pointer"),
        (entry, "variant 0 needs no mom", "a.variant = 0; a.mom = hmcx_mlp_params{};", OK, ""),
        (entry, "bad noise_mode", "a.noise_mode = -1;", EINVAL, who + "bad noise_mode"),
        (entry, "BUFFER noise without noise", "a.noise = nullptr;", EINVAL,
         who + "BUFFER noise mode needs noise and noise_off"),
        (entry, "bad mask_mode", "a.mask_mode = 3;", EINVAL, who + "bad mask_mode"),
        (entry, "FIXED without masks", "a.masks = nullptr;", EINVAL, who + "FIXED masks need masks and mask_off"),
        (entry, "want_eval without out_eval_loss", "a.out_eval_loss = nullptr;", EINVAL,
         who + "want_eval needs out_eval_loss"),
        (entry, "FIXED want_eval without eval_mask_off", "a.eval_mask_off = nullptr;", EINVAL,
         who + "FIXED masks with want_eval need eval_mask_off"),
        (entry, "want_draw without draws", "a.draws.p[1] = nullptr;", EINVAL, who + "want_draw needs draws"),
        (entry, "order repeats", "a.order[0] = 1;", EINVAL, who + "order must be a permutation of 0..5"),
        (entry, "negative row0 in the last step", "b.row0.back() = -1;", EINVAL, who + "negative row0"),
        (entry, "negative noise_off in the last step", "b.off.back() = -1;", EINVAL, who + "negative noise_off"),
        (entry, "PHILOX noise does not read noise_off", "a.noise_mode = HMCX_NOISE_PHILOX; a.noise_off = nullptr;", OK, ""),
        (entry, "want_eval above 3 in the last step", "b.flags.back() = 4;", EINVAL, who + "want_eval holds bits 0 and 1"),
        (entry, "negative mask_off is not rejected", "b.moff.back() = -1;", OK, ""),
        (entry, "variant before null pointer", "a.variant = -1; a.eps = nullptr;", EINVAL, who + "variant must be 0 or 1"),
        (entry, "the scan goes step by step", "b.off[0] = -1; b.row0.back() = -1;", EINVAL, who + "negative noise_off"),
        (entry, "noise before masks", "a.noise_off = nullptr; a.mask_mode = 9;", EINVAL,
         who + "BUFFER noise mode needs noise and noise_off"),
    ]


def _chain_rows(entry, who):
    """The rows the two chain entries share."""
    return [
        (entry, "C 0", "a.C = 0;", EINVAL, who + "C must be 1 .. 64"),
        (entry, "C 65", "a.C = 65;", EINVAL, who + "C must be 1 .. 64"),
        (entry, "chain0 + C wraps", "a.chain0 = 0xffffffffu;", EINVAL, who + "chain0 + C wraps 2^32"),
        (entry, "chain0 + C reaches 2^32", "a.chain0 = 0xfffffffeu;", OK, ""),
        (entry, "step_base + n_steps wraps", "a.step_base = 0xfffffffeu;", EINVAL, who + "step_base + n_steps wraps 2^32"),
        (entry, "draw_stride below the flagged steps", "a.draw_stride = 2;", EINVAL,
         who + "draw_stride below the call's flagged steps"),
        (entry, "C before order", "a.C = 0; a.order[0] = 9;", EINVAL, who + "C must be 1 .. 64"),
        (entry, "wrap before the parameter limit", "a.chain0 = 0xffffffffu; a.n_in = 46000; a.n_mid = 46000;", EINVAL,
         who + "chain0 + C wraps 2^32"),
        (entry, "n_steps before C", "a.n_steps = -1; a.C = 0;", EINVAL, who + "n_steps < 0"),
    ]


ROWS += _sgld_rows("sgld", "mlp sgld: ") + [
    ("sgld", "no wrap check in the one-chain call", "a.step_base = 0xffffffffu;", OK, ""),
    ("sgld", "dtype wins over null X", "a.dtype = 3; a.X = nullptr;", EINVAL, DTYPE),
]
ROWS += _sgld_rows("sgld_chains", "mlp sgld chains: ") + _chain_rows("sgld_chains", "mlp sgld chains: ")
ROWS += _chain_rows("hmc_chains", "mlp hmc chains: ") + [
    ("hmc_chains", "n_steps 0", "a.n_steps = 0;", OK, ""),
    ("hmc_chains", "n_steps < 0", "a.n_steps = -1;", EINVAL, "mlp hmc chains: n_steps < 0"),
    ("hmc_chains", "2^31 parameters", "a.n_in = 46000; a.n_mid = 46000;", EUNSUP,
     "mlp hmc chains: more than 2^31 - 1 parameters"),
    ("hmc_chains", "null n_iter", "a.n_iter = nullptr;", EINVAL, "mlp hmc chains: null pointer"),
    ("hmc_chains", "null out_accepted", "a.out_accepted = nullptr;", EINVAL, "mlp hmc chains: null pointer"),
    ("hmc_chains", "bad noise_mode", "a.noise_mode = 2;", EINVAL, "mlp hmc chains: bad noise_mode"),
    ("hmc_chains", "BUFFER noise without noise_off", "a.noise_off = nullptr;", EINVAL,
     "mlp hmc chains: BUFFER noise mode needs noise and noise_off"),
    ("hmc_chains", "bad mask_mode", "a.mask_mode = -1;", EINVAL, "mlp hmc chains: bad mask_mode"),
    ("hmc_chains", "FIXED without mask_off", "a.mask_off = nullptr;", EINVAL,
     "mlp hmc chains: FIXED masks need masks and mask_off"),
    ("hmc_chains", "want_eval without out_eval_loss", "a.out_eval_loss = nullptr;", EINVAL,
     "mlp hmc chains: want_eval needs out_eval_loss"),
    ("hmc_chains", "want_draw without draws", "a.draws.p[4] = nullptr;", EINVAL, "mlp hmc chains: want_draw needs draws"),
    ("hmc_chains", "order out of range", "a.order[3] = -1;", EINVAL, "mlp hmc chains: order must be a permutation of 0..5"),
    ("hmc_chains", "n_iter < 0 in the last entry", "b.iters.back() = -1;", EINVAL, "mlp hmc chains: n_iter < 0"),
    ("hmc_chains", "n_iter wraps the forward number", "b.iters.back() = 357913941;", EINVAL,
     "mlp hmc chains: n_iter so large that the forward number wraps 2^32"),
    ("hmc_chains", "the largest n_iter", "b.iters.back() = 357913940;", OK, ""),
    ("hmc_chains", "negative noise_off in the last entry", "b.coff.back() = -1;", EINVAL,
     "mlp hmc chains: negative noise_off"),
    ("hmc_chains", "negative mask_off in the last entry", "b.cmoff.back() = -1;", EINVAL,
     "mlp hmc chains: negative mask_off"),
    ("hmc_chains", "PHILOX masks do not read mask_off", "a.mask_mode = HMCX_MLP_MASKS_PHILOX; a.mask_off = nullptr;", OK, ""),
    ("hmc_chains", "the scan before draw_stride", "b.iters.back() = -1; a.draw_stride = 0;", EINVAL,
     "mlp hmc chains: n_iter < 0"),
    # ---- hmcx_mlp_predictive (the context-free part) ----
    ("predictive", "S 0", "a.S = 0;", EINVAL, "mlp predictive: S and T must be >= 1"),
    ("predictive", "T 0", "a.T = 0;", EINVAL, "mlp predictive: S and T must be >= 1"),
    ("predictive", "too many draws", "a.S = 70000; a.T = 70000;", EUNSUP, "mlp predictive: too many draws"),
    ("predictive", "null X", "a.X = nullptr;", EINVAL, "mlp predictive: null pointer"),
    ("predictive", "hole in par", "a.par.p[0] = nullptr;", EINVAL, "mlp predictive: null pointer"),
    ("predictive", "bad mask_mode", "a.mask_mode = 3;", EINVAL, "mlp predictive: bad mask_mode"),
    ("predictive", "no dropout with T 2", "a.mask_mode = HMCX_MLP_MASKS_NONE;", EINVAL,
     "mlp predictive: without dropout every draw of a set is the same (T must be 1)"),
    ("predictive", "FIXED without masks", "a.mask_mode = HMCX_MLP_MASKS_FIXED; a.masks = nullptr;", EINVAL,
     "mlp predictive: FIXED masks required"),
    ("predictive", "slot0 + S*T wraps", "a.slot0 = 0xfffffffbu;", EINVAL, "mlp predictive: slot0 + S*T wraps 2^32"),
    ("predictive", "slot0 + S*T reaches 2^32", "a.slot0 = 0xfffffffau;", OK, ""),
    ("predictive", "lppd without labels", "a.y = nullptr;", EINVAL,
     "mlp predictive: lppd / draw_nll / draw_correct need labels"),
    ("predictive", "path 3", "a.path = 3;", EINVAL, "mlp predictive: path must be 0, 1 or 2"),
    ("predictive", "T before path", "a.mask_mode = HMCX_MLP_MASKS_NONE; a.path = -1;", EINVAL,
     "mlp predictive: without dropout every draw of a set is the same (T must be 1)"),
]
# every struct-taking entry: the valid block, null args and check_mlp's three messages
for _e, (_fn, _who, _bf) in STRUCTS.items():
    ROWS += [(_e, "valid", "", OK, ""), (_e, "null args", "%s(nullptr)" % _fn, EINVAL, "null args"),
             (_e, "dtype", "a.dtype = 2;", EINVAL, DTYPE), (_e, "sizes", "a.%s = 0;" % _bf, EINVAL, SIZES),
             (_e, "large", "a.n_mid = 50000;", EUNSUP, LARGE)]

# set_error calls between check_mlp and the end of hmcx_ctx.hip before the checks moved
SET_ERROR_CALLS_BEFORE = 94

PROGRAM_HEAD = r"""
#include "hmcx_mlp_checks.h"
#include <cstdio>
#include <vector>
using namespace hmcx::mlp_checks;

static void* const P = (void*)0x1000;                  // device pointers: compared with null, never read
static double* const PD = (double*)0x1000;
static int32_t* const Y = (int32_t*)0x1000;
static const hmcx_mlp_params PAR = {{P, P, P, P, P, P}};
static const hmcx_mlp_params HOLE = {{P, P, P, nullptr, P, P}};
enum { NS = 3, NC = 2 };

// the host arrays of a valid block, each exactly as long as the call may read
struct Bufs {
  std::vector<int64_t> row0 = std::vector<int64_t>(NS, 0), off = std::vector<int64_t>(NS, 0),
                       moff = std::vector<int64_t>(NS, 0), eoff = std::vector<int64_t>(2 * NS, 0),
                       coff = std::vector<int64_t>(NS * NC, 0), cmoff = std::vector<int64_t>(NS * NC, 0);
  std::vector<double> eps = std::vector<double>(NS, 1e-3), u = std::vector<double>(NS * NC, 0.5);
  std::vector<int32_t> iters = std::vector<int32_t>(NS * NC, 2);
  std::vector<uint8_t> flags = std::vector<uint8_t>(NS, 3), draw = std::vector<uint8_t>(NS, 1);
};
template <typename A> static void dims(A& a) { a.dtype = HMCX_F32; a.B = 4; a.n_in = 3; a.n_mid = 8; a.n_out = 2; }
template <typename A> static void order(A& a) { const int o[6] = {2, 0, 1, 5, 4, 3}; for (int i = 0; i < 6; ++i) a.order[i] = o[i]; }

static hmcx_mlp_sghmc_args valid_sghmc(Bufs& b) {
  hmcx_mlp_sghmc_args a{}; dims(a); order(a); a.n_steps = NS;
  a.X = P; a.y = Y; a.row0 = b.row0.data(); a.eps = b.eps.data(); a.n_iter = b.iters.data(); a.u_accept = b.u.data();
  a.noise_mode = HMCX_NOISE_PHILOX; a.mask_mode = HMCX_NOISE_PHILOX; a.par = PAR;
  a.out_A = PD; a.out_accepted = Y; a.out_loss = PD;
  return a;
}
static hmcx_mlp_leapfrog_args valid_leapfrog(Bufs&) {
  hmcx_mlp_leapfrog_args a{}; dims(a); order(a); a.n_iter = 2; a.X = P; a.y = Y; a.q = PAR; a.p = PAR; a.g = PAR;
  a.mask_mode = HMCX_MLP_MASKS_PHILOX; a.masks = P;
  return a;
}
static hmcx_mlp_sgd_args valid_sgd(Bufs& b) {
  hmcx_mlp_sgd_args a{}; dims(a); a.n_steps = NS; a.X = P; a.y = Y; a.row0 = b.row0.data();
  a.want_eval = b.draw.data(); a.mask_mode = HMCX_MLP_MASKS_FIXED; a.masks = P; a.mask_off = b.off.data();
  a.eval_mask_off = b.moff.data(); a.par = PAR; a.mom = PAR; a.out_eval_loss = PD;
  return a;
}
// BUFFER noise, FIXED masks, evaluations and draws: every optional array is read
template <typename A> static void sgld_fields(A& a, Bufs& b) {
  dims(a); order(a); a.n_steps = NS; a.variant = 1; a.X = P; a.y = Y; a.row0 = b.row0.data(); a.eps = b.eps.data();
  a.want_eval = b.flags.data(); a.noise_mode = HMCX_NOISE_BUFFER; a.noise = PD; a.noise_off = b.off.data();
  a.mask_mode = HMCX_MLP_MASKS_FIXED; a.masks = P; a.mask_off = b.moff.data(); a.eval_mask_off = b.eoff.data();
  a.par = PAR; a.mom = PAR; a.out_eval_loss = PD; a.want_draw = b.draw.data(); a.draws = PAR;
}
static hmcx_mlp_sgld_args valid_sgld(Bufs& b) { hmcx_mlp_sgld_args a{}; sgld_fields(a, b); return a; }
static hmcx_mlp_sgld_chains_args valid_sgld_chains(Bufs& b) {
  hmcx_mlp_sgld_chains_args a{}; sgld_fields(a, b); a.C = NC; a.draw_stride = NS;
  return a;
}
static hmcx_mlp_hmc_chains_args valid_hmc_chains(Bufs& b) {
  hmcx_mlp_hmc_chains_args a{}; dims(a); order(a); a.n_steps = NS; a.C = NC; a.X = P; a.y = Y; a.eps = b.eps.data();
  a.n_iter = b.iters.data(); a.u_accept = b.u.data(); a.noise_mode = HMCX_NOISE_BUFFER; a.noise = PD;
  a.noise_off = b.coff.data(); a.mask_mode = HMCX_MLP_MASKS_FIXED; a.masks = P; a.mask_off = b.cmoff.data();
  a.par = PAR; a.out_A = PD; a.out_accepted = Y; a.want_eval = b.draw.data(); a.out_eval_loss = PD;
  a.want_draw = b.draw.data(); a.draws = PAR; a.draw_stride = NS;
  return a;
}
static hmcx_mlp_predictive_args valid_predictive(Bufs&) {
  hmcx_mlp_predictive_args a{}; a.dtype = HMCX_F64; a.N = 4; a.n_in = 3; a.n_mid = 8; a.n_out = 2; a.S = 3; a.T = 2;
  a.mask_mode = HMCX_MLP_MASKS_PHILOX; a.X = P; a.y = Y; a.par = PAR; a.out_lppd = PD;
  return a;
}
static void report(int row, const MlpCheck& r) { std::printf("%d\t%d\t%s\n", row, r.status, r.msg.c_str()); }

int main() {
"""


def _program():
    body = []
    for i, (entry, _case, code, _st, _msg) in enumerate(ROWS):
        if entry not in STRUCTS or code.endswith("(nullptr)"):
            body.append("  report(%d, %s);" % (i, code))
        else:
            fn = STRUCTS[entry][0]
            body.append("  { Bufs b; auto a = valid_%s(b); %s report(%d, %s(&a)); }" % (entry, code, i, fn))
    return PROGRAM_HEAD + "\n".join(body) + "\n  return 0;\n}\n"


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("mlp_checks")
    src, exe = d / "checks.cpp", d / "checks"
    src.write_text(_program())
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(REPO, "include"), "-I", CSRC,
            str(src), "-o", str(exe)]
    # the sanitizers where their runtimes link (statically: nothing to preload); the plain program otherwise
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    # out-of-bounds reads and undefined behaviour are what the run looks for; the leak pass at exit needs ptrace
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    got = {}
    for line in r.stdout.splitlines():
        row, status, msg = line.split("\t")
        got[int(row)] = (int(status), msg)
    return got


def test_table_covers_every_entry_and_message():
    assert {r[0] for r in ROWS} == {"masks", "grad", "loss"} | set(STRUCTS)
    assert len(ROWS) >= SET_ERROR_CALLS_BEFORE
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS)
    for e in STRUCTS:
        assert (e, "valid", "", OK, "") in ROWS


def test_header_needs_no_hip():
    """Only include/hmcx.h and the standard library."""
    with open(os.path.join(CSRC, "hmcx_mlp_checks.h")) as fh:
        incs = [ln.split()[1] for ln in fh if ln.startswith("#include")]
    assert incs == ['"hmcx.h"', "<cstdint>", "<string>"]


def test_every_row_gives_the_status_and_message(results):
    assert sorted(results) == list(range(len(ROWS)))
    bad = [(ROWS[i][0], ROWS[i][1], results[i], (ROWS[i][3], ROWS[i][4]))
           for i in range(len(ROWS)) if results[i] != (ROWS[i][3], ROWS[i][4])]
    assert not bad, bad
