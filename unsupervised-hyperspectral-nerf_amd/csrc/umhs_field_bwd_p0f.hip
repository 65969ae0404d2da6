// Field backward, part 0 on the fp32 chain: launch_tf_p0f and the field_bwd_tf_kernel<0, ...> instances it can select.
#include "umhs_field_bwd.h"

template <int TBMAX, bool FU>
static int launch_tf_p0f_(const TfPart& pt, const TfLaunch& a, bool spec) {
  if (spec) {
    if constexpr (TBMAX <= 12) LAUNCH_K_(field_bwd_tf_kernel<0, true, TBMAX, FU>);
    return UMHS_ERR_UNSUPPORTED;
  }
  LAUNCH_K_(field_bwd_tf_kernel<0, false, TBMAX, FU>);
}
template <int TBMAX>
int launch_tf_p0f(const TfPart& pt, const TfLaunch& a, bool spec, bool fused) {
  return fused ? launch_tf_p0f_<TBMAX, true>(pt, a, spec) : launch_tf_p0f_<TBMAX, false>(pt, a, spec);
}
INSTANTIATE_(launch_tf_p0f, const TfPart&, const TfLaunch&, bool, bool);
