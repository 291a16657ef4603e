// hmcx_persist.h — launch plan of the persistent single-chain SGHMC kernel (hmcx_persist2.hip).
#pragma once
#include "hmcx_internal.h"

namespace hmcx {

// hmcx_persist2.hip: reduce-scatter / all-gather teams over tagged-granule hand-offs.
struct PersistPlan2 {
  bool ok;
  int Gr, Gf, Br, Bf, BfP, BFP, Ro, Fo;
  size_t lds;
  double cost;
};
PersistPlan2 plan_p2(int B, int D, int K, size_t tsize, int num_cus, size_t lds_max);
// Helper workgroups (HMCX_P2_HELP): the mode a launch of plan p runs in when `want` is asked for — `want`
// when 2·G workgroups fit the device at ONE per CU, else 0 (today's kernel path) — and the dynamic LDS of
// that launch: more than half of a CU's, so that a chain workgroup never shares a CU with a helper.
int p2_help_mode(const PersistPlan2& p, int K, int num_cus, size_t lds_max, int want, size_t* lds);
// Granule arena of one launch: offset and size of every region, in granules.
// With look-ahead (ahead): no helper regions but XQ; L1 is lane 1's copy of XA … XS, XV the verdict records.
struct P2Layout {
  long oXA, nXA, oXD, nXD, oXB, nXB, oXW, nXW, oXS, nXS, oXC, nXC, oXAh, nXAh, oXQ, nXQ, oXP, nXP, ngran;
  long oL1, nL1, oXV, nXV;
};
P2Layout p2_layout(const PersistPlan2& p, int K, int pad, int help, int ahead = 0);
// Look-ahead (HMCX_P2_AHEAD): 1 when `want` is 1 and a second chain lane fits (2·G workgroups at one per
// CU, a second X tile in LDS), else 0; *lds is then the launch's dynamic LDS.
int p2_ahead_mode(const PersistPlan2& p, int K, size_t tsize, int num_cus, size_t lds_max, int want, size_t* lds);
// The auto rule (hmcx_p2_ahead_rule, include/hmcx.h): window and thresholds.
constexpr int P2_AHEAD_WINDOW = 32, P2_AHEAD_MIN = 16;
constexpr double P2_AHEAD_OFF_ABOVE = 0.4, P2_AHEAD_ON_BELOW = 0.3;
template <typename T> int sghmc_p2_t(hmcx_ctx*, const hmcx_sampler_args*, const PersistPlan2&);

}  // namespace hmcx
