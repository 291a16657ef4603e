// hmcx_xdrop.h — the Bernoulli(p) input-dropout mask of the linear models (sgd.py:61-62, softmax.py:91-100):
// one definition for sgd.fit_dropout's k_xdrop (hmcx_softmax.hip) and the posterior predictive
// (hmcx_lin_pred.hip), so both draw the same stream.
#pragma once
#include "hmcx_common.h"
#include "hmcx_internal.h"

namespace hmcx {

// Z[idx] of the mask drawn for (seed, chain, step): keep element idx (row·D + column) with probability p.
__host__ __device__ inline bool xdrop_keep(uint64_t seed, uint32_t chain, uint32_t step, uint32_t idx, double p) {
  return philox_uniform(seed, chain, step, SLOT_DROPX, idx) < p;
}

}  // namespace hmcx
