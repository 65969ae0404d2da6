// The world affine of the mesh exports: the written xyz of a model-frame position, one rounded float32 operation per step
// (include/umhs_hip.h, umhs_mesh_vertices).  Shared by umhs_mesh.hip and umhs_simplify.hip so that both write the same bits.
#pragma once
#include "umhs_exact.h"

struct xf_world {
  int has;
  float a[12];  // [3,4] row-major
};

__host__ inline xf_world xf_world_from_host(const float* world_host12) {
  xf_world w;
  w.has = world_host12 ? 1 : 0;
  for (int k = 0; k < 12; ++k) w.a[k] = world_host12 ? world_host12[k] : 0.0f;
  return w;
}

// w = p, or with an affine  w_r = (((A[r][0] p_0) + (A[r][1] p_1)) + (A[r][2] p_2)) + A[r][3]
__device__ __forceinline__ void xf_world_apply(const xf_world& Wd, const float p[3], float w[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = p[k];
  if (Wd.has) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
      w[r] = xf_add(xf_add(xf_add(xf_mul(Wd.a[4 * r], p[0]), xf_mul(Wd.a[4 * r + 1], p[1])), xf_mul(Wd.a[4 * r + 2], p[2])),
                    Wd.a[4 * r + 3]);
  }
}
