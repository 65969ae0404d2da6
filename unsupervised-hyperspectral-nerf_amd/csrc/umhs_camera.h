// Camera and box geometry that the ray generators (umhs_data.hip) and the exporters (umhs_pointcloud.hip, umhs_mesh.hip) share: one
// body each, so projection, ray generation and the crop boxes are one model to the bit.  Every function is compiled with contraction
// off by a pragma of its own: one rounded float32 operation per step wherever it is inlined.
#pragma once
#include "umhs_common.h"

// component k of R^T e for a row-major 3x3 R (column k of R against e): a point or a direction taken into the frame of a camera or
// of an oriented box.  The association is part of the definition.
__device__ __forceinline__ float cam_rt_row(const float* R, int k, float e0, float e1, float e2) {
#pragma clang fp contract(off)
  return (R[k] * e0 + R[3 + k] * e1) + R[6 + k] * e2;
}

// The forward OpenCV radial / tangential model at the image-plane point (x, y), y DOWN; k = (k1, k2, k3, k4, p1, p2), nerfstudio's
// order:   r = x^2 + y^2,  d = 1 + r(k1 + r(k2 + r(k3 + r k4)))
//          xd = d x + 2 p1 x y + p2 (r + 2 x^2),   yd = d y + 2 p2 x y + p1 (r + 2 y^2)
// r and d come back too: the Newton step below builds its Jacobian from them.
struct cam_distorted {
  float x, y, r, d;
};
__device__ __forceinline__ cam_distorted distort_opencv(float x, float y, const float k[6]) {
#pragma clang fp contract(off)
  const float k1 = k[0], k2 = k[1], k3 = k[2], k4 = k[3], p1 = k[4], p2 = k[5];
  cam_distorted o;
  o.r = x * x + y * y;
  o.d = 1.0f + o.r * (k1 + o.r * (k2 + o.r * (k3 + o.r * k4)));
  o.x = o.d * x + 2.0f * p1 * x * y + p2 * (o.r + 2.0f * x * x);
  o.y = o.d * y + 2.0f * p2 * x * y + p1 * (o.r + 2.0f * y * y);
  return o;
}

// camera_utils.radial_and_tangential_undistort  [upstream-recalled]: a fixed 10 Newton steps on the residual of the model above,
//   fx = xd(x, y) - xd,   fy = yd(x, y) - yd,
// with the analytic Jacobian; a step is divided by the 2x2 determinant only where |det| > 1e-3 and is zero otherwise.
// (xd, yd) is the distorted image-plane point in OpenCV's frame (y DOWN).  With k = 0 every step is an exact zero, so the point comes
// back bit for bit.
__device__ __forceinline__ void undistort_opencv(float xd, float yd, const float k[6], float& xo, float& yo) {
#pragma clang fp contract(off)
  const float k1 = k[0], k2 = k[1], k3 = k[2], k4 = k[3], p1 = k[4], p2 = k[5];
  float x = xd, y = yd;
  for (int it = 0; it < 10; ++it) {
    const cam_distorted f = distort_opencv(x, y, k);
    const float r = f.r, d = f.d;
    const float fx = f.x - xd, fy = f.y - yd;
    const float d_r = k1 + r * (2.0f * k2 + r * (3.0f * k3 + r * 4.0f * k4));
    const float d_x = 2.0f * x * d_r, d_y = 2.0f * y * d_r;
    const float fx_x = d + d_x * x + 2.0f * p1 * y + 6.0f * p2 * x;
    const float fx_y = d_y * x + 2.0f * p1 * x + 2.0f * p2 * y;
    const float fy_x = d_x * y + 2.0f * p2 * y + 2.0f * p1 * x;
    const float fy_y = d + d_y * y + 2.0f * p2 * x + 6.0f * p1 * y;
    const float den = fy_x * fx_y - fx_x * fy_y;
    const float xn = fx * fy_y - fy * fx_y, yn = fy * fx_x - fx * fy_x;
    const bool ok = fabsf(den) > 1e-3f;
    x = x + (ok ? xn / den : 0.0f);
    y = y + (ok ? yn / den : 0.0f);
  }
  xo = x, yo = y;
}

// the three image-plane points of a ray of camera c, undistorted in place; dist [n,6] = (k1, k2, k3, k4, p1, p2) per camera.  A camera
// whose six parameters are all zero skips the solve (which would be an exact no-op), so its rays carry the undistorted kernel's bits.
__device__ __forceinline__ void undistort_plane_points(const float* __restrict__ dist, int64_t c, float px[3], float py[3]) {
  float kd[6];
  bool any = false;
#pragma unroll
  for (int i = 0; i < 6; ++i) kd[i] = dist[6 * c + i], any = any || (kd[i] != 0.0f);
  if (any) {
#pragma unroll
    for (int s = 0; s < 3; ++s) undistort_opencv(px[s], py[s], kd, px[s], py[s]);
  }
}
