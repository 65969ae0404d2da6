// The Adam update of libumhs_hip.so, written once: the device expression shared by the stand-alone kernels (umhs_adam.hip) and the
// epilogue of the hash grid's bucket reduce (umhs_hashgrid_part.h), and the host side's bias correction.
#pragma once
#include "umhs_common.h"

// One Adam update (torch.optim.Adam, no weight decay / amsgrad); one expression for the stand-alone kernels and for the
// epilogue of hg_reduce_kernel, so that the fused and the separate update give the same bits.
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, const float gk, const float lr_bc1, const float b1,
                                            const float b2, const float eps, const float sqrt_bc2) {
#pragma clang fp contract(off)  // the same rounding in every kernel this is inlined into (and torch's mul_/add_ sequence)
  m = m * b1 + gk * (1.0f - b1);
  v = v * b2 + gk * gk * (1.0f - b2);
  const float denom = sqrtf(v) / sqrt_bc2 + eps;
  p = p - lr_bc1 * (m / denom);
}

// The ``clamp_endmembers`` epilogue of the stand-alone kernels: torch's clamp_(0, 1), which keeps a NaN.  (fminf(fmaxf(p, 0), 1)
// returns the bound for a NaN: a parameter whose moments a non-finite gradient has poisoned would read 0 for ever and hide it.)
__device__ __forceinline__ float adam_clamp01(const float p) { return p < 0.0f ? 0.0f : (p > 1.0f ? 1.0f : p); }

// The step's bias correction as the two factors adam_update takes, in double precision on the host: one function for every entry
// point that launches an Adam update, so that the fused and the stand-alone step get the same two floats.
struct AdamBias {
  float lr_bc1, sqrt_bc2;
};
static inline AdamBias adam_bias(float lr, float beta1, float beta2, int64_t step) {
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  return AdamBias{(float)(lr / bc1), (float)sqrt(bc2)};
}
