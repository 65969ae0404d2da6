// Field backward, part 0 on the bf16x3 chain: launch_tf_p0z and the zipped kernels (field_bwd_tfz0_kernel) it can select.
#include "umhs_field_bwd.h"

template <int TBMAX, bool FU>
static int launch_tf_p0z_(const TfPart& pt, const TfLaunch& a, bool spec) {
  if (spec) {
    if constexpr (TBMAX < 8 || (TBMAX == 8 && FU)) LAUNCH_K_(field_bwd_tfz0_kernel<true, TBMAX, FU>);
    return UMHS_ERR_UNSUPPORTED;
  }
  if constexpr (TBMAX < 16 || FU) LAUNCH_K_(field_bwd_tfz0_kernel<false, TBMAX, FU>);
  return UMHS_ERR_UNSUPPORTED;
}
template <int TBMAX>
int launch_tf_p0z(const TfPart& pt, const TfLaunch& a, bool spec, bool fused) {
  return fused ? launch_tf_p0z_<TBMAX, true>(pt, a, spec) : launch_tf_p0z_<TBMAX, false>(pt, a, spec);
}
INSTANTIATE_(launch_tf_p0z, const TfPart&, const TfLaunch&, bool, bool);
