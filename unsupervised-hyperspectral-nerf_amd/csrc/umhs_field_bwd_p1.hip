// Field backward, part 1: launch_tf_p1 and its kernels (zipped field_bwd_tfz1_kernel, fp32-chain field_bwd_tf_kernel<1, ...>).
#include "umhs_field_bwd.h"

template <int TBMAX>
int launch_tf_p1(const TfPart& pt, const TfLaunch& a, bool zipped) {  // (part 1 does not depend on the specular head)
  if (zipped) LAUNCH_K_(field_bwd_tfz1_kernel<TBMAX>);
  LAUNCH_K_(field_bwd_tf_kernel<1, false, TBMAX, false>);
}
INSTANTIATE_(launch_tf_p1, const TfPart&, const TfLaunch&, bool);
