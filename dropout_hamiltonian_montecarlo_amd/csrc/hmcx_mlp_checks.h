// hmcx_mlp_checks.h — the argument checks of the dropout MLP's entry points as plain host C++: include/hmcx.h and
// the standard library, no HIP header and no hmcx_ctx, so a host compiler builds them into a test program.
// One function per rule, then one per entry point that calls the rules in the order the caller sees: the first
// failing rule's status and message are the call's.  `who` is the message prefix ("mlp sgld: ", ...); the rules that
// older calls share without one take "".  hmcx_ctx.hip turns a failed MlpCheck into set_error and launches nothing.
#pragma once
#include "hmcx.h"
#include <cstdint>
#include <string>

namespace hmcx::mlp_checks {
struct MlpCheck { int status = HMCX_OK; std::string msg; };
using Who = const std::string&;
inline MlpCheck fail(int status, Who who, const char* text) { return MlpCheck{status, who + text}; }
inline MlpCheck einval(Who who, const char* text) { return fail(HMCX_EINVAL, who, text); }
// return the first failed rule
#define HMCX_MLP_TRY(expr) do { MlpCheck r_ = (expr); if (r_.status != HMCX_OK) return r_; } while (0)

inline MlpCheck sizes(int dtype, int B, int n_in, int n_mid, int n_out) {
  if (dtype != HMCX_F32 && dtype != HMCX_F64) return einval("", "dtype must be HMCX_F32/HMCX_F64");
  if (B < 1 || n_in < 1 || n_mid < 1 || n_out < 1) return einval("", "mlp: sizes must be >= 1");
  if ((long long)B * n_mid * 3 > 0x7fffffffLL || (long long)n_mid * n_in > 0x7fffffffLL ||
      (long long)n_mid * n_mid > 0x7fffffffLL)
    return fail(HMCX_EUNSUPPORTED, "", "mlp: layer too large");
  return {};
}
inline bool params_ok(const hmcx_mlp_params* p) {
  return p && p->p[0] && p->p[1] && p->p[2] && p->p[3] && p->p[4] && p->p[5];
}
inline MlpCheck steps_nonneg(Who who, int n_steps) { return n_steps < 0 ? einval(who, "n_steps < 0") : MlpCheck{}; }
// the noise index of an element is a 32-bit Philox counter field: all six variables together stay below 2^31
inline MlpCheck param_limit(Who who, int n_in, int n_mid, int n_out) {
  if ((long long)n_mid * n_in + (long long)n_mid * n_mid + (long long)n_out * n_mid + 2LL * n_mid + n_out > 0x7fffffffLL)
    return fail(HMCX_EUNSUPPORTED, who, "more than 2^31 - 1 parameters");
  return {};
}
// the chain count, then the two Philox counters that must not wrap
inline MlpCheck chains_and_wraps(Who who, int C, uint32_t chain0, uint32_t step_base, int n_steps) {
  if (C < 1 || C > 64) return einval(who, "C must be 1 .. 64");
  if ((uint64_t)chain0 + (uint64_t)C > 0x100000000ULL) return einval(who, "chain0 + C wraps 2^32");
  if ((uint64_t)step_base + (uint64_t)n_steps > 0x100000000ULL) return einval(who, "step_base + n_steps wraps 2^32");
  return {};
}
inline MlpCheck noise_mode(Who who, int mode) {
  return mode != HMCX_NOISE_BUFFER && mode != HMCX_NOISE_PHILOX ? einval(who, "bad noise_mode") : MlpCheck{};
}
inline MlpCheck noise_buffers(Who who, int mode, const double* noise, const int64_t* noise_off) {
  const bool bad = mode == HMCX_NOISE_BUFFER && (!noise || !noise_off);
  return bad ? einval(who, "BUFFER noise mode needs noise and noise_off") : MlpCheck{};
}
inline MlpCheck mask_mode(Who who, int mode) {
  const bool ok = mode == HMCX_MLP_MASKS_NONE || mode == HMCX_MLP_MASKS_FIXED || mode == HMCX_MLP_MASKS_PHILOX;
  return ok ? MlpCheck{} : einval(who, "bad mask_mode");
}
inline MlpCheck mask_buffers(Who who, int mode, const void* masks, const int64_t* mask_off) {
  const bool bad = mode == HMCX_MLP_MASKS_FIXED && (!masks || !mask_off);
  return bad ? einval(who, "FIXED masks need masks and mask_off") : MlpCheck{};
}
// want_eval with its output and, where eval_off is part of the call (`has_eval_off`), its FIXED mask offsets
inline MlpCheck eval_outputs(Who who, const uint8_t* want_eval, const double* out_eval_loss, int mode,
                             const int64_t* eval_mask_off, bool has_eval_off) {
  if (want_eval && !out_eval_loss) return einval(who, "want_eval needs out_eval_loss");
  if (has_eval_off && want_eval && mode == HMCX_MLP_MASKS_FIXED && !eval_mask_off)
    return einval(who, "FIXED masks with want_eval need eval_mask_off");
  return {};
}
inline MlpCheck draw_outputs(Who who, const uint8_t* want_draw, const hmcx_mlp_params* draws) {
  return want_draw && !params_ok(draws) ? einval(who, "want_draw needs draws") : MlpCheck{};
}
inline MlpCheck order_permutation(Who who, const int* order) {
  int seen = 0;
  for (int i = 0; i < 6; ++i) {
    const int v = order[i];
    if (v < 0 || v > 5 || ((seen >> v) & 1)) return einval(who, "order must be a permutation of 0..5");
    seen |= 1 << v;
  }
  return {};
}
// the per-step arrays of the minibatch calls, step by step; noise_off and want_eval null: not scanned
inline MlpCheck step_scan(Who who, int n_steps, const int64_t* row0, const int64_t* noise_off, const uint8_t* want_eval) {
  for (int s = 0; s < n_steps; ++s) {
    if (row0[s] < 0) return einval(who, "negative row0");
    if (noise_off && noise_off[s] < 0) return einval(who, "negative noise_off");
    if (want_eval && want_eval[s] > 3) return einval(who, "want_eval holds bits 0 and 1");
  }
  return {};
}
// the per-(step, chain) arrays of the full-batch HMC call; noise_off and mask_off null: not scanned
inline MlpCheck chain_step_scan(Who who, int64_t n, const int32_t* n_iter, const int64_t* noise_off,
                                const int64_t* mask_off) {
  for (int64_t j = 0; j < n; ++j) {
    if (n_iter[j] < 0) return einval(who, "n_iter < 0");
    // the mask slot of the step's last forward, 0x80000000 + 6n + 3, stays below 2^32
    if ((int64_t)n_iter[j] > (0x7fffffffLL - 3) / 6) return einval(who, "n_iter so large that the forward number wraps 2^32");
    if (noise_off && noise_off[j] < 0) return einval(who, "negative noise_off");
    if (mask_off && mask_off[j] < 0) return einval(who, "negative mask_off");
  }
  return {};
}
inline MlpCheck draw_stride(Who who, int n_steps, const uint8_t* want_draw, int64_t stride) {
  int64_t n_draws = 0;
  for (int s = 0; s < n_steps; ++s)
    if (want_draw && want_draw[s]) ++n_draws;
  return n_draws > stride ? einval(who, "draw_stride below the call's flagged steps") : MlpCheck{};
}

// ---- the entry points: null args, sizes and n_steps first, as every struct-taking call has them ----
template <typename A>
MlpCheck head(const A* a, Who who) {
  if (!a) return einval("", "null args");
  HMCX_MLP_TRY(sizes(a->dtype, a->B, a->n_in, a->n_mid, a->n_out));
  return steps_nonneg(who, a->n_steps);
}
// noise and mask modes with their buffers, the evaluation and draw outputs, the order
template <typename A>
MlpCheck modes_outputs_order(const A* a, Who who, const int64_t* eval_mask_off, bool has_eval_off) {
  HMCX_MLP_TRY(noise_mode(who, a->noise_mode));
  HMCX_MLP_TRY(noise_buffers(who, a->noise_mode, a->noise, a->noise_off));
  HMCX_MLP_TRY(mask_mode(who, a->mask_mode));
  HMCX_MLP_TRY(mask_buffers(who, a->mask_mode, a->masks, a->mask_off));
  HMCX_MLP_TRY(eval_outputs(who, a->want_eval, a->out_eval_loss, a->mask_mode, eval_mask_off, has_eval_off));
  HMCX_MLP_TRY(draw_outputs(who, a->want_draw, &a->draws));
  return order_permutation(who, a->order);
}
inline MlpCheck masks(int dtype, int B, int n_mid, const void* out) {
  HMCX_MLP_TRY(sizes(dtype, B, 1, n_mid, 1));
  return out ? MlpCheck{} : einval("", "null pointer");
}
inline MlpCheck grad(int dtype, const void* X, const int32_t* y, int B, int n_in, int n_mid, int n_out,
                     const hmcx_mlp_params* par, const hmcx_mlp_params* grads) {
  HMCX_MLP_TRY(sizes(dtype, B, n_in, n_mid, n_out));
  return X && y && params_ok(par) && params_ok(grads) ? MlpCheck{} : einval("", "null pointer");
}
inline MlpCheck loss(int dtype, const void* X, const int32_t* y, int B, int n_in, int n_mid, int n_out,
                     const hmcx_mlp_params* par, const void* logits) {
  HMCX_MLP_TRY(sizes(dtype, B, n_in, n_mid, n_out));
  if (!X || !params_ok(par)) return einval("", "null pointer");
  return y || logits ? MlpCheck{} : einval("", "mlp_loss: need labels or a logits output");
}
// SGHMC takes the noise constants for both modes and checks both modes before either's buffers; its general
// messages carry no prefix
inline MlpCheck sghmc(const hmcx_mlp_sghmc_args* a) {
  HMCX_MLP_TRY(head(a, ""));
  if (!a->X || !a->y || !a->row0 || !a->eps || !a->n_iter || !a->u_accept || !params_ok(&a->par) || !a->out_A ||
      !a->out_accepted || !a->out_loss)
    return einval("", "mlp sghmc: null pointer");
  HMCX_MLP_TRY(noise_mode("", a->noise_mode));
  if (a->mask_mode != HMCX_NOISE_BUFFER && a->mask_mode != HMCX_NOISE_PHILOX) return einval("", "bad mask_mode");
  HMCX_MLP_TRY(noise_buffers("", a->noise_mode, a->noise, a->noise_off));
  if (a->mask_mode == HMCX_NOISE_BUFFER && (!a->masks || !a->mask_off))
    return einval("", "BUFFER mask mode needs masks and mask_off");
  return {};
}
inline MlpCheck leapfrog(const hmcx_mlp_leapfrog_args* a, Who who = "mlp leapfrog: ") {
  if (!a) return einval("", "null args");
  HMCX_MLP_TRY(sizes(a->dtype, a->B, a->n_in, a->n_mid, a->n_out));
  if (a->n_iter < 0) return einval(who, "n_iter < 0");
  if (!a->X || !a->y || !params_ok(&a->q) || !params_ok(&a->p) || !params_ok(&a->g)) return einval(who, "null pointer");
  HMCX_MLP_TRY(mask_mode(who, a->mask_mode));
  if (a->mask_mode != HMCX_MLP_MASKS_NONE && !a->masks) return einval(who, "masks required for FIXED / PHILOX");
  return order_permutation(who, a->order);
}
inline MlpCheck sgd(const hmcx_mlp_sgd_args* a, Who who = "mlp sgd: ") {
  HMCX_MLP_TRY(head(a, who));
  if (!a->X || !a->y || !a->row0 || !params_ok(&a->par) || !params_ok(&a->mom)) return einval(who, "null pointer");
  HMCX_MLP_TRY(mask_mode(who, a->mask_mode));
  HMCX_MLP_TRY(mask_buffers(who, a->mask_mode, a->masks, a->mask_off));
  HMCX_MLP_TRY(eval_outputs(who, a->want_eval, a->out_eval_loss, a->mask_mode, a->eval_mask_off, true));
  return step_scan(who, a->n_steps, a->row0, nullptr, nullptr);
}
// what hmcx_mlp_sgld_args and hmcx_mlp_sgld_chains_args share, from the variant to the order
template <typename A>
MlpCheck sgld_common(const A* a, Who who) {
  if (a->variant != 0 && a->variant != 1) return einval(who, "variant must be 0 or 1");
  if (!a->X || !a->y || !a->row0 || !a->eps || !params_ok(&a->par) || (a->variant == 1 && !params_ok(&a->mom)))
    return einval(who, "null pointer");
  HMCX_MLP_TRY(modes_outputs_order(a, who, a->eval_mask_off, true));
  return step_scan(who, a->n_steps, a->row0, a->noise_mode == HMCX_NOISE_BUFFER ? a->noise_off : nullptr, a->want_eval);
}
// the one-chain call has no wrap check
inline MlpCheck sgld(const hmcx_mlp_sgld_args* a, Who who = "mlp sgld: ") {
  HMCX_MLP_TRY(head(a, who));
  HMCX_MLP_TRY(param_limit(who, a->n_in, a->n_mid, a->n_out));
  return sgld_common(a, who);
}
inline MlpCheck sgld_chains(const hmcx_mlp_sgld_chains_args* a, Who who = "mlp sgld chains: ") {
  HMCX_MLP_TRY(head(a, who));
  HMCX_MLP_TRY(chains_and_wraps(who, a->C, a->chain0, a->step_base, a->n_steps));
  HMCX_MLP_TRY(param_limit(who, a->n_in, a->n_mid, a->n_out));
  HMCX_MLP_TRY(sgld_common(a, who));
  return draw_stride(who, a->n_steps, a->want_draw, a->draw_stride);
}
inline MlpCheck hmc_chains(const hmcx_mlp_hmc_chains_args* a, Who who = "mlp hmc chains: ") {
  HMCX_MLP_TRY(head(a, who));
  HMCX_MLP_TRY(chains_and_wraps(who, a->C, a->chain0, a->step_base, a->n_steps));
  HMCX_MLP_TRY(param_limit(who, a->n_in, a->n_mid, a->n_out));
  if (!a->X || !a->y || !a->eps || !a->n_iter || !a->u_accept || !params_ok(&a->par) || !a->out_A || !a->out_accepted)
    return einval(who, "null pointer");
  HMCX_MLP_TRY(modes_outputs_order(a, who, nullptr, false));
  HMCX_MLP_TRY(chain_step_scan(who, (int64_t)a->n_steps * a->C, a->n_iter,
                               a->noise_mode == HMCX_NOISE_BUFFER ? a->noise_off : nullptr,
                               a->mask_mode == HMCX_MLP_MASKS_FIXED ? a->mask_off : nullptr));
  return draw_stride(who, a->n_steps, a->want_draw, a->draw_stride);
}
// no evaluation outputs: the modes and their buffers one by one.  chain_step_scan's n_iter limit (6n + 3 below 2^31)
// is two forwards stricter than this call's last forward, 6n + 1
inline MlpCheck sghmc_chains(const hmcx_mlp_sghmc_chains_args* a, Who who = "mlp sghmc chains: ") {
  HMCX_MLP_TRY(head(a, who));
  HMCX_MLP_TRY(chains_and_wraps(who, a->C, a->chain0, a->step_base, a->n_steps));
  HMCX_MLP_TRY(param_limit(who, a->n_in, a->n_mid, a->n_out));
  if (!a->X || !a->y || !a->row0 || !a->eps || !a->n_iter || !a->u_accept || !params_ok(&a->par) || !a->out_A ||
      !a->out_accepted || !a->out_loss)
    return einval(who, "null pointer");
  HMCX_MLP_TRY(noise_mode(who, a->noise_mode));
  HMCX_MLP_TRY(noise_buffers(who, a->noise_mode, a->noise, a->noise_off));
  HMCX_MLP_TRY(mask_mode(who, a->mask_mode));
  HMCX_MLP_TRY(mask_buffers(who, a->mask_mode, a->masks, a->mask_off));
  HMCX_MLP_TRY(draw_outputs(who, a->want_draw, &a->draws));
  HMCX_MLP_TRY(order_permutation(who, a->order));
  HMCX_MLP_TRY(step_scan(who, a->n_steps, a->row0, nullptr, nullptr));
  HMCX_MLP_TRY(chain_step_scan(who, (int64_t)a->n_steps * a->C, a->n_iter,
                               a->noise_mode == HMCX_NOISE_BUFFER ? a->noise_off : nullptr,
                               a->mask_mode == HMCX_MLP_MASKS_FIXED ? a->mask_off : nullptr));
  return draw_stride(who, a->n_steps, a->want_draw, a->draw_stride);
}
// the context-free part of hmcx_mlp_predictive; the fused path's eligibility needs the context and follows it
inline MlpCheck predictive(const hmcx_mlp_predictive_args* a, Who who = "mlp predictive: ") {
  if (!a) return einval("", "null args");
  HMCX_MLP_TRY(sizes(a->dtype, a->N, a->n_in, a->n_mid, a->n_out));
  if (a->S < 1 || a->T < 1) return einval(who, "S and T must be >= 1");
  const long long D = (long long)a->S * a->T;
  if (D > 0x7fffffffLL || D * a->N > 0x7fffffffLL * 64) return fail(HMCX_EUNSUPPORTED, who, "too many draws");
  if (!a->X || !params_ok(&a->par)) return einval(who, "null pointer");
  HMCX_MLP_TRY(mask_mode(who, a->mask_mode));
  if (a->mask_mode == HMCX_MLP_MASKS_NONE && a->T != 1)
    return einval(who, "without dropout every draw of a set is the same (T must be 1)");
  if (a->mask_mode == HMCX_MLP_MASKS_FIXED && !a->masks) return einval(who, "FIXED masks required");
  if (a->mask_mode == HMCX_MLP_MASKS_PHILOX && (unsigned long long)a->slot0 + (unsigned long long)D > 0x100000000ULL)
    return einval(who, "slot0 + S*T wraps 2^32");
  if (!a->y && (a->out_lppd || a->out_draw_nll || a->out_draw_correct))
    return einval(who, "lppd / draw_nll / draw_correct need labels");
  if (a->path < 0 || a->path > 2) return einval(who, "path must be 0, 1 or 2");
  return {};
}
#undef HMCX_MLP_TRY
}  // namespace hmcx::mlp_checks
