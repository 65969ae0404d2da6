// pixel sampler / ray generator / ground-truth gather for gfx950.
// Replaces what UMHSDataManager.next_train (umhs_datamanager.py:95-108) reaches in nerfstudio==1.1.5 with
// --images-on-gpu: PixelSampler.sample (indices (camera, y, x) -> rows of the cached image stacks) and RayGenerator ->
// Cameras.generate_rays (perspective; raygen_kernel without lens distortion, raygen_distorted_kernel with the OpenCV radial /
// tangential model that COLMAP's OPENCV cameras carry).  nerfstudio's source is not available offline; the arithmetic below
// restates its published behaviour (oracle/torch_ref.py generate_rays / gather_pixels; the undistortion is
// camera_utils.radial_and_tangential_undistort  [upstream-recalled], restated in tests/raygen_f64.py).  All kernels are HBM-bound:
// ray generation moves 24 B in + 28 B out per ray (the distorted one adds ~2 k flops of Newton steps per ray, still far below the
// roofline's ridge), the gather one (B+3)-float row per ray from a stack of n*H*W rows.
#include "umhs_common.h"

// indices [R,3] int64 (camera, y, x); c2w [n,3,4]; intr [n,4] = (fx, fy, cx, cy)
__global__ __launch_bounds__(256) void raygen_kernel(const int64_t* __restrict__ indices, const float* __restrict__ c2w,
                                                     const float* __restrict__ intr, int64_t n_rays, int64_t n_cams,
                                                     float* __restrict__ origins, float* __restrict__ directions,
                                                     float* __restrict__ pixel_area, float* __restrict__ dir_norm) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  int64_t c = indices[3 * r];
  c = c < 0 ? 0 : (c >= n_cams ? n_cams - 1 : c);  // indices are validated on the host; never read out of bounds
  const float y = (float)indices[3 * r + 1] + 0.5f, x = (float)indices[3 * r + 2] + 0.5f;  // pixel centres
  const float fx = intr[4 * c], fy = intr[4 * c + 1], cx = intr[4 * c + 2], cy = intr[4 * c + 3];
  const float* M = c2w + 12 * c;
  // three directions: the pixel, its +x and its +y neighbour (pixel_area = |d - dx| * |d - dy|)
  const float px[3] = {(x - cx) / fx, (x - cx + 1.0f) / fx, (x - cx) / fx};
  const float py[3] = {-(y - cy) / fy, -(y - cy) / fy, -(y - cy + 1.0f) / fy};
  float d[3][3], nrm0 = 0.0f;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    float v[3], sq = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = (px[s] * M[4 * k] + py[s] * M[4 * k + 1]) + (-1.0f) * M[4 * k + 2];
      // the squares are accumulated as torch.linalg.vector_norm accumulates them on the CPU the oracle runs on -- v0 * v0, then one
      // fused multiply-add per further component -- so that directions and directions_norm carry the oracle's bits (the plain
      // float32 sum was one unit in the last place off in ~11 % of the components)
      sq = k == 0 ? v[k] * v[k] : fmaf(v[k], v[k], sq);
    }
    const float nrm = fmaxf(sqrtf(sq), 1.1920928955078125e-07f);
    if (s == 0) nrm0 = nrm;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[s][k] = v[k] / nrm;
  }
  float dx = 0.0f, dy = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a = d[0][k] - d[1][k], b = d[0][k] - d[2][k];
    dx += a * a, dy += b * b;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) origins[3 * r + k] = M[4 * k + 3], directions[3 * r + k] = d[0][k];
  if (pixel_area) pixel_area[r] = sqrtf(dx) * sqrtf(dy);
  if (dir_norm) dir_norm[r] = nrm0;
}

extern "C" int umhs_raygen(const int64_t* indices, const float* c2w, const float* intrinsics, int64_t n_rays,
                           int64_t n_cams, float* origins, float* directions, float* pixel_area, float* directions_norm,
                           umhs_stream_t stream) {
  if (n_rays == 0) return UMHS_OK;
  if (n_rays < 0 || n_cams < 1 || !indices || !c2w || !intrinsics || !origins || !directions) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(raygen_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream), indices, c2w,
                     intrinsics, n_rays, n_cams, origins, directions, pixel_area, directions_norm);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// camera_utils.radial_and_tangential_undistort  [upstream-recalled]: a fixed 10 Newton steps on the residual of the OpenCV model
//   r = x^2 + y^2,  d = 1 + r(k1 + r(k2 + r(k3 + r k4)))
//   fx = d x + 2 p1 x y + p2 (r + 2 x^2) - xd,   fy = d y + 2 p2 x y + p1 (r + 2 y^2) - yd
// with the analytic Jacobian; a step is divided by the 2x2 determinant only where |det| > 1e-3 and is zero otherwise.
// (xd, yd) is the distorted image-plane point in OpenCV's frame (y DOWN); k = (k1, k2, k3, k4, p1, p2), nerfstudio's order.
// With k = 0 every step is an exact zero, so the point comes back bit for bit.
__device__ __forceinline__ void undistort_opencv(float xd, float yd, const float k[6], float& xo, float& yo) {
#pragma clang fp contract(off)
  const float k1 = k[0], k2 = k[1], k3 = k[2], k4 = k[3], p1 = k[4], p2 = k[5];
  float x = xd, y = yd;
  for (int it = 0; it < 10; ++it) {
    const float r = x * x + y * y;
    const float d = 1.0f + r * (k1 + r * (k2 + r * (k3 + r * k4)));
    const float fx = d * x + 2.0f * p1 * x * y + p2 * (r + 2.0f * x * x) - xd;
    const float fy = d * y + 2.0f * p2 * x * y + p1 * (r + 2.0f * y * y) - yd;
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

// raygen_kernel with lens distortion: dist [n,6] = (k1, k2, k3, k4, p1, p2) per camera.  The pixel, its +x and its +y neighbour are
// each undistorted in OpenCV image-plane coordinates ((x-cx)/fx, (y-cy)/fy), y down, and y is negated afterwards (camera y is up);
// everything after that is raygen_kernel's arithmetic.  A camera whose six parameters are all zero skips the solve (which would be an
// exact no-op), so its rays carry the bits raygen_kernel gives.
__global__ __launch_bounds__(256) void raygen_distorted_kernel(const int64_t* __restrict__ indices, const float* __restrict__ c2w,
                                                               const float* __restrict__ intr, const float* __restrict__ dist,
                                                               int64_t n_rays, int64_t n_cams, float* __restrict__ origins,
                                                               float* __restrict__ directions, float* __restrict__ pixel_area,
                                                               float* __restrict__ dir_norm) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rays) return;
  int64_t c = indices[3 * r];
  c = c < 0 ? 0 : (c >= n_cams ? n_cams - 1 : c);  // indices are validated on the host; never read out of bounds
  const float y = (float)indices[3 * r + 1] + 0.5f, x = (float)indices[3 * r + 2] + 0.5f;  // pixel centres
  const float fx = intr[4 * c], fy = intr[4 * c + 1], cx = intr[4 * c + 2], cy = intr[4 * c + 3];
  const float* M = c2w + 12 * c;
  float kd[6];
  bool any = false;
#pragma unroll
  for (int i = 0; i < 6; ++i) kd[i] = dist[6 * c + i], any = any || (kd[i] != 0.0f);
  // three image-plane points, y down: the pixel, its +x and its +y neighbour (pixel_area = |d - dx| * |d - dy|)
  float px[3] = {(x - cx) / fx, (x - cx + 1.0f) / fx, (x - cx) / fx};
  float py[3] = {(y - cy) / fy, (y - cy) / fy, (y - cy + 1.0f) / fy};
  if (any) {
#pragma unroll
    for (int s = 0; s < 3; ++s) undistort_opencv(px[s], py[s], kd, px[s], py[s]);
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) py[s] = -py[s];
  float d[3][3], nrm0 = 0.0f;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    float v[3], sq = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[k] = (px[s] * M[4 * k] + py[s] * M[4 * k + 1]) + (-1.0f) * M[4 * k + 2];
      sq = k == 0 ? v[k] * v[k] : fmaf(v[k], v[k], sq);  // (torch.linalg.vector_norm's order and roundings: see raygen_kernel)
    }
    const float nrm = fmaxf(sqrtf(sq), 1.1920928955078125e-07f);
    if (s == 0) nrm0 = nrm;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[s][k] = v[k] / nrm;
  }
  float dx = 0.0f, dy = 0.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a = d[0][k] - d[1][k], b = d[0][k] - d[2][k];
    dx += a * a, dy += b * b;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) origins[3 * r + k] = M[4 * k + 3], directions[3 * r + k] = d[0][k];
  if (pixel_area) pixel_area[r] = sqrtf(dx) * sqrtf(dy);
  if (dir_norm) dir_norm[r] = nrm0;
}

extern "C" int umhs_raygen_distorted(const int64_t* indices, const float* c2w, const float* intrinsics, const float* distortion,
                                     int64_t n_rays, int64_t n_cams, float* origins, float* directions, float* pixel_area,
                                     float* directions_norm, umhs_stream_t stream) {
  if (n_rays == 0) return UMHS_OK;
  if (n_rays < 0 || n_cams < 1 || !indices || !c2w || !intrinsics || !distortion || !origins || !directions) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(raygen_distorted_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream), indices, c2w,
                     intrinsics, distortion, n_rays, n_cams, origins, directions, pixel_area, directions_norm);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// out[r, :] = stack[c, y, x, :]  (stack [n,H,W,K] fp32, or uint8 scaled by 1/255 as nerfstudio's get_image_float32 does)
template <typename SRC>
__global__ __launch_bounds__(256) void pixel_gather_kernel(const int64_t* __restrict__ indices, const SRC* __restrict__ stack,
                                                           int64_t n, int64_t H, int64_t W, int K, int64_t n_rays,
                                                           float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rays * K) return;
  const int64_t r = i / K;
  const int k = (int)(i - r * K);
  int64_t c = indices[3 * r], y = indices[3 * r + 1], x = indices[3 * r + 2];
  c = c < 0 ? 0 : (c >= n ? n - 1 : c), y = y < 0 ? 0 : (y >= H ? H - 1 : y), x = x < 0 ? 0 : (x >= W ? W - 1 : x);
  const SRC v = stack[((c * H + y) * W + x) * K + k];
  if constexpr (sizeof(SRC) == 1)
    out[i] = (float)v / 255.0f;
  else
    out[i] = v;
}

extern "C" int umhs_pixel_gather(const int64_t* indices, const void* stack, int src_is_u8, int64_t n_images, int64_t height,
                                 int64_t width, int n_channels, int64_t n_rays, float* out, umhs_stream_t stream) {
  if (n_rays == 0) return UMHS_OK;
  if (n_rays < 0 || n_images < 1 || height < 1 || width < 1 || n_channels < 1 || !indices || !stack || !out) return UMHS_ERR_ARG;
  const int64_t total = n_rays * n_channels;
  if ((total + 255) / 256 > 0x7fffffffLL) return UMHS_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (src_is_u8)
    hipLaunchKernelGGL(pixel_gather_kernel<uint8_t>, grid, dim3(256), 0, umhs_s(stream), indices, (const uint8_t*)stack,
                       n_images, height, width, n_channels, n_rays, out);
  else
    hipLaunchKernelGGL(pixel_gather_kernel<float>, grid, dim3(256), 0, umhs_s(stream), indices, (const float*)stack, n_images,
                       height, width, n_channels, n_rays, out);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}

// indices[r] = (long)(u[r] * (n, H, W))  -- PixelSampler.sample_method; u from torch.rand so the stream of draws is torch's
__global__ __launch_bounds__(256) void pixel_indices_kernel(const float* __restrict__ u, int64_t n_rays, float n, float H,
                                                            float W, int64_t* __restrict__ indices) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * n_rays) return;
  const int k = (int)(i % 3);
  indices[i] = (int64_t)(u[i] * (k == 0 ? n : (k == 1 ? H : W)));
}

extern "C" int umhs_pixel_indices(const float* uniform, int64_t n_rays, int64_t n_images, int64_t height, int64_t width,
                                  int64_t* indices, umhs_stream_t stream) {
  if (n_rays == 0) return UMHS_OK;
  if (n_rays < 0 || n_images < 1 || height < 1 || width < 1 || !uniform || !indices) return UMHS_ERR_ARG;
  hipLaunchKernelGGL(pixel_indices_kernel, dim3((unsigned)((3 * n_rays + 255) / 256)), dim3(256), 0, umhs_s(stream), uniform,
                     n_rays, (float)n_images, (float)height, (float)width, indices);
  UMHS_CHECK_LAUNCH();
  return UMHS_OK;
}
